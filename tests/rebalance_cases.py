"""Inputs shared by test_rebalance_twin_cpu.py and test_rebalance_gpu.py: the
GPU file pins kmp_lp_rebalance to the twin on these, the CPU file proves that
the twin reaches feasibility on them within the same max_passes (so a GPU
assertion of feasibility cannot hide a stall)."""

import os

import numpy as np

import kaminpar_amd as ka

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    def __init__(self, g, k, caps, part0, vwgt=None, adjwgt=None, max_passes=16,
                 feasible=True):
        self.g, self.k, self.caps, self.part0 = g, k, caps, part0
        self.vwgt, self.adjwgt = vwgt, adjwgt
        self.max_passes, self.feasible = max_passes, feasible


def caps_of(g, k, eps=0.03):
    return np.full(k, g.max_block_weight(k, eps), dtype=np.int64)


def skewed(n, k, seed=5):
    """Random, with a third of the vertices forced into block 0."""
    part0 = ka.random_partition(n, k, seed=seed)
    part0[::3] = 0
    return part0


def rmat_case(scale, k, start):
    g = ka.Graph.rmat(scale, 8, seed=7)
    part0 = skewed(g.n, k) if start == "skewed" else np.zeros(g.n, dtype=np.uint32)
    return Case(g, k, caps_of(g, k), part0)


RMAT = [(scale, k, start) for scale in (10, 12) for k in (2, 16, 256, 512)
        for start in ("skewed", "block0")]


def tier_graph():
    """Ring of 6000 vertices plus five spokes of degree exactly 16, 17, 2048,
    2049 and 3000 (both sides of each tier boundary, and a hub)."""
    ring = 6000
    degs = [16, 17, 2048, 2049, 3000]
    n = ring + len(degs)
    adj = [[(v - 1) % ring, (v + 1) % ring] for v in range(ring)] + [[] for _ in degs]
    for i, d in enumerate(degs):
        s = ring + i
        for j in range(d):
            v = (j * 2 + i * 7) % ring if d <= ring // 2 else j
            adj[s].append(v)
            adj[v].append(s)
    xadj = np.zeros(n + 1, dtype=np.uint32)
    xadj[1:] = np.cumsum([len(a) for a in adj])
    adjncy = np.array([v for a in adj for v in a], dtype=np.uint32)
    g = ka.Graph.from_csr(xadj, adjncy)
    assert np.diff(np.asarray(g.xadj, dtype=np.int64))[ring:].tolist() == degs
    return g


def tiers_case():
    """The five spokes and a third of the ring sit in the overloaded block."""
    g = tier_graph()
    k = 4
    part0 = skewed(g.n, k, seed=11)
    part0[6000:] = 0
    return Case(g, k, caps_of(g, k), part0)


def weighted_rgg():
    g0 = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    xadj = np.asarray(g0.xadj, dtype=np.uint32).copy()
    adjncy = np.asarray(g0.adjncy, dtype=np.uint32).copy()
    rng = np.random.RandomState(17)
    vwgt = rng.randint(1, 10, size=g0.n).astype(np.int32)
    src = np.repeat(np.arange(g0.n, dtype=np.int64), np.diff(xadj.astype(np.int64)))
    lo = np.minimum(src, adjncy.astype(np.int64))
    hi = np.maximum(src, adjncy.astype(np.int64))
    adjwgt = (((lo * 1000003 + hi * 7919) % 9) + 1).astype(np.int32)  # symmetric, 1..9
    return ka.Graph.from_csr(xadj, adjncy, vwgt, adjwgt), vwgt, adjwgt


def weighted_case(k):
    g, vwgt, adjwgt = weighted_rgg()
    return Case(g, k, caps_of(g, k), skewed(g.n, k, seed=3), vwgt=vwgt, adjwgt=adjwgt)


def odd_n_case():
    g = ka.Graph.rgg2d(1000 + 37, 8.0, seed=3)
    assert g.n % 64 != 0
    return Case(g, 8, caps_of(g, 8), skewed(g.n, 8, seed=3))


def isolated_case():
    """37 isolated vertices in a block that is over its cap."""
    g0 = ka.Graph.rgg2d(1003, 8.0, seed=4)
    xadj = np.concatenate([np.asarray(g0.xadj, dtype=np.uint32),
                           np.full(37, g0.m, dtype=np.uint32)])
    g = ka.Graph.from_csr(xadj, np.asarray(g0.adjncy, dtype=np.uint32).copy())
    assert g.n == 1040 and (np.diff(xadj.astype(np.int64))[-37:] == 0).all()
    k = 4
    part0 = ka.random_partition(g.n, k, seed=3)
    part0[-37:] = 0
    part0[:400] = 0  # over by more than the vertices with a positive key
    caps = caps_of(g, k)
    assert np.bincount(part0, minlength=k)[0] > caps[0]
    return Case(g, k, caps, part0)


def multigraph_case():
    g0 = ka.Graph.rgg2d(500, 8.0, seed=5)
    x0 = np.asarray(g0.xadj, dtype=np.int64)
    a0 = np.asarray(g0.adjncy, dtype=np.uint32)
    src = np.repeat(np.arange(g0.n), np.diff(x0))
    und = [(u, v) for u, v in zip(src.tolist(), a0.tolist()) if u < v]
    adj = [[] for _ in range(g0.n)]
    for i, (u, v) in enumerate(und):
        for _ in range(1 + i % 3):  # multiplicity 1..3
            adj[u].append(v)
            adj[v].append(u)
    xadj = np.zeros(g0.n + 1, dtype=np.uint32)
    xadj[1:] = np.cumsum([len(a) for a in adj])
    adjncy = np.array([v for a in adj for v in a], dtype=np.uint32)
    g = ka.Graph.from_csr(xadj, adjncy)
    return Case(g, 4, caps_of(g, 4), skewed(g.n, 4, seed=3))


def unmeetable_case():
    """Sum of the caps below the total weight: the call has to stall."""
    g = ka.Graph.rmat(10, 8, seed=7)
    k = 8
    caps = np.full(k, g.total_node_weight // k - 3, dtype=np.int64)
    return Case(g, k, caps, skewed(g.n, k), feasible=False)


def one_pass_case():
    """Everything in block 0 at k = 16 needs several passes: cut off at one."""
    g = ka.Graph.rmat(10, 8, seed=7)
    k = 16
    return Case(g, k, caps_of(g, k), np.zeros(g.n, dtype=np.uint32), max_passes=1,
                feasible=False)


OTHER = {
    "tiers": tiers_case,
    "weighted_k4": lambda: weighted_case(4),
    "weighted_k16": lambda: weighted_case(16),
    "odd_n": odd_n_case,
    "isolated": isolated_case,
    "multigraph": multigraph_case,
    "unmeetable": unmeetable_case,
    "one_pass": one_pass_case,
}

# eng.jet(..., balancer=1) against rebalance_twin.jet
JET = [(scale, k, temp) for scale in (10, 12) for k in (8, 16, 256) for temp in (0.25, 0.75)]
