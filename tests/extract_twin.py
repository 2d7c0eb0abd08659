"""Numpy twin of kmp_lp_extract_subgraphs (rule: include/kaminpar_lp.h).

Given labels L (n entries, values < k) on a CSR graph:
  nodes    all vertex ids ordered by (L[u], u); node_off[b] (k + 1 entries) is
           the start of block b in nodes; mapping[u] = (position of u in
           nodes) - node_off[L[u]]: the rank of u among its block's vertices in
           ascending id
  sub-row  of the vertex at position i, u = nodes[i]: the arcs (u, v) of u's
           row with L[v] == L[u], in their original adjacency order, stored as
           mapping[v] and the arc's weight; self-arcs and parallel arcs stay
  packed   sub_xadj (n + 1, u64) = exclusive prefix sum of the internal degrees
           in nodes order; arc_off[b] = sub_xadj[node_off[b]]; block b's CSR is
           the slice [node_off[b], node_off[b + 1]] of sub_xadj rebased by
           arc_off[b]; weights are carried only when the graph has them.

Written row by row on purpose: it shares no code and no vectorised trick with
the kernels it referees."""

import numpy as np


def extract(xadj, adjncy, k, part, vwgt=None, adjwgt=None):
    """Returns a dict with mapping, nodes, node_off, arc_off, sub_xadj and
    blocks: one (xadj, adjncy, vwgt | None, adjwgt | None) tuple per block."""
    xadj = np.asarray(xadj, dtype=np.int64)
    adjncy = np.asarray(adjncy, dtype=np.int64)
    part = np.asarray(part, dtype=np.int64)
    n = len(xadj) - 1
    assert len(part) == n and (n == 0 or (part.min() >= 0 and part.max() < k))

    nodes = np.array(sorted(range(n), key=lambda u: (int(part[u]), u)), dtype=np.int64)
    node_off = np.zeros(k + 1, dtype=np.int64)
    for u in range(n):
        node_off[part[u] + 1] += 1
    node_off = np.cumsum(node_off)
    mapping = np.zeros(n, dtype=np.int64)
    for i, u in enumerate(nodes):
        mapping[u] = i - node_off[part[u]]

    sub_xadj = np.zeros(n + 1, dtype=np.int64)
    sub_adj, sub_w = [], []
    for i, u in enumerate(nodes):
        for e in range(xadj[u], xadj[u + 1]):
            v = adjncy[e]
            if part[v] == part[u]:
                sub_adj.append(mapping[v])
                sub_w.append(1 if adjwgt is None else int(adjwgt[e]))
        sub_xadj[i + 1] = len(sub_adj)
    sub_adj = np.array(sub_adj, dtype=np.uint32)
    sub_w = np.array(sub_w, dtype=np.int32)
    arc_off = sub_xadj[node_off]

    blocks = []
    for b in range(k):
        lo, hi = node_off[b], node_off[b + 1]
        a0, a1 = arc_off[b], arc_off[b + 1]
        blocks.append((
            (sub_xadj[lo:hi + 1] - a0).astype(np.uint32),
            sub_adj[a0:a1],
            None if vwgt is None else np.asarray(vwgt, dtype=np.int32)[nodes[lo:hi]],
            None if adjwgt is None else sub_w[a0:a1],
        ))
    return {
        "mapping": mapping.astype(np.uint32),
        "nodes": nodes.astype(np.uint32),
        "node_off": node_off.astype(np.uint32),
        "arc_off": arc_off.astype(np.uint64),
        "sub_xadj": sub_xadj.astype(np.uint64),
        "blocks": blocks,
    }


def extract_graph(g, k, part):
    """extract() on a kaminpar_amd.Graph, with the weights it carries."""
    return extract(g.xadj, g.adjncy, k, part, vwgt=g.vwgt, adjwgt=g.adjwgt)
