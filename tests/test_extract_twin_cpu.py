"""The numpy twin of the block subgraph extraction (tests/extract_twin.py)
against a hand-computed case and against invariants of the rule on R-MAT. No
GPU: test_extract_gpu.py pins kmp_lp_extract_subgraphs to this twin."""

import numpy as np

import kaminpar_amd as ka
import extract_twin as et


def test_hand_computed_case():
    """7 vertices, 3 blocks, block 1 empty; weights on vertices and arcs.
    Undirected edges (weight): 0-1 (5), 0-2 (3), 0-4 (2), 1-3 (4), 1-5 (1),
    2-4 (6), 3-6 (7), 5-6 (8), 2-3 (9). Cut edges: 0-1, 2-3."""
    rows = [
        [(1, 5), (2, 3), (4, 2)],
        [(0, 5), (3, 4), (5, 1)],
        [(0, 3), (4, 6), (3, 9)],
        [(1, 4), (6, 7), (2, 9)],
        [(0, 2), (2, 6)],
        [(1, 1), (6, 8)],
        [(3, 7), (5, 8)],
    ]
    xadj = np.cumsum([0] + [len(r) for r in rows])
    adjncy = np.array([v for r in rows for v, _ in r])
    adjwgt = np.array([w for r in rows for _, w in r], dtype=np.int32)
    vwgt = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.int32)
    part = np.array([2, 0, 2, 0, 2, 0, 0])

    r = et.extract(xadj, adjncy, 3, part, vwgt=vwgt, adjwgt=adjwgt)
    assert r["nodes"].tolist() == [1, 3, 5, 6, 0, 2, 4]
    assert r["node_off"].tolist() == [0, 4, 4, 7]
    assert r["mapping"].tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert r["sub_xadj"].tolist() == [0, 2, 4, 6, 8, 10, 12, 14]
    assert r["arc_off"].tolist() == [0, 8, 8, 14]
    expected = [
        ([0, 2, 4, 6, 8], [1, 2, 0, 3, 0, 3, 1, 2], [2, 4, 6, 7], [4, 1, 4, 7, 1, 8, 7, 8]),
        ([0], [], [], []),
        ([0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [1, 3, 5], [3, 2, 3, 6, 2, 6]),
    ]
    for (x, a, vw, aw), (ex, ea, evw, eaw) in zip(r["blocks"], expected):
        assert x.tolist() == ex
        assert a.tolist() == ea
        assert vw.tolist() == evw
        assert aw.tolist() == eaw

    # without weights nothing is carried
    r0 = et.extract(xadj, adjncy, 3, part)
    assert all(vw is None and aw is None for _, _, vw, aw in r0["blocks"])
    assert [b[1].tolist() for b in r0["blocks"]] == [e[1] for e in expected]


def _arcs(x, a, w=None):
    src = np.repeat(np.arange(len(x) - 1), np.diff(x.astype(np.int64)))
    ww = np.ones(len(a), dtype=np.int64) if w is None else w.astype(np.int64)
    return sorted(zip(src.tolist(), a.tolist(), ww.tolist()))


def test_rmat_invariants():
    g = ka.Graph.rmat(10, 8, seed=7)
    k = 16
    part = ka.random_partition(g.n, k, seed=3)
    r = et.extract_graph(g, k, part)
    xadj = np.asarray(g.xadj, dtype=np.int64)
    adjncy = np.asarray(g.adjncy, dtype=np.int64)
    src = np.repeat(np.arange(g.n), np.diff(xadj))
    cut_arcs = int((part[src] != part[adjncy]).sum())

    assert (np.bincount(part, minlength=k) == np.diff(r["node_off"].astype(np.int64))).all()
    total = 0
    for b, (x, a, vw, aw) in enumerate(r["blocks"]):
        assert vw is None and aw is None  # unit-weight input
        assert len(x) - 1 == int((part == b).sum())
        assert len(a) == 0 or a.max() < len(x) - 1
        fwd = _arcs(x, a)
        assert fwd == sorted((v, u, w) for u, v, w in fwd), f"block {b} is not symmetric"
        total += len(a)
    assert total == g.m - cut_arcs
    # unit weights: (sum(adjwgt) - sum(sub_adjwgt)) / 2 is the edge cut
    assert (g.m - total) % 2 == 0 and (g.m - total) // 2 == g.edge_cut(part)


def test_weighted_cut_identity():
    import rebalance_cases as rc

    g, vwgt, adjwgt = rc.weighted_rgg()
    k = 16
    part = rc.skewed(g.n, k, seed=3)
    r = et.extract_graph(g, k, part)
    sub = sum(int(aw.astype(np.int64).sum()) for _, _, _, aw in r["blocks"])
    assert (int(adjwgt.astype(np.int64).sum()) - sub) // 2 == g.edge_cut(part)
    for _, (x, a, vw, aw) in enumerate(r["blocks"]):
        fwd = _arcs(x, a, aw)
        assert fwd == sorted((v, u, w) for u, v, w in fwd)
    got_vw = np.concatenate([vw for _, _, vw, _ in r["blocks"]])
    assert (got_vw == vwgt[r["nodes"]]).all()


def test_k1_reproduces_the_graph():
    g = ka.Graph.rmat(10, 8, seed=7)
    r = et.extract_graph(g, 1, np.zeros(g.n, dtype=np.uint32))
    x, a, vw, aw = r["blocks"][0]
    assert (r["nodes"] == np.arange(g.n)).all() and (r["mapping"] == np.arange(g.n)).all()
    assert (x == np.asarray(g.xadj)).all()
    assert (a == np.asarray(g.adjncy)).all()
    assert vw is None and aw is None
    assert r["arc_off"].tolist() == [0, g.m]
