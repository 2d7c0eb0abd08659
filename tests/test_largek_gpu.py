"""LP refinement and balancing above k = 2048 (hash gain tiers): bit parity
with the CPU oracle in labels, cut, moves and arcs_scanned.

Every comparison also asserts moves > 0, so an early exit cannot pass for
parity. Without the large-k path every call here at k > 2048 raises."""

import functools

import numpy as np
import pytest

import kaminpar_amd as ka
from helpers import oracle_balance, oracle_refine

pytestmark = pytest.mark.gpu

KMP_LP_MAX_K = 1 << 24  # include/kaminpar_lp.h


def _caps(g, k, eps=0.10):
    return np.full(k, g.max_block_weight(k, eps), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    return ka.Graph.rmat(scale, 8, seed=3)


def _same(got, want):
    """(cut, part, stats) of the engine against the oracle's."""
    cut, part, st = got
    ocut, opart, ost = want
    assert int(ost[1]) > 0, "the oracle moved nothing: the case tests nothing"
    assert cut == ocut
    assert np.array_equal(part, opart)
    assert int(st.moves) == int(ost[1])
    assert int(st.arcs_scanned) == int(ost[0])


# ------------------------------------------------------ 1. refine, R-MAT
@pytest.mark.parametrize("k", [2049, 4096, 8000])
def test_refine_parity_rmat(oracle, k):
    """rmat15 has vertices in all four degree tiers; at k >= 4096 its hub
    (degree 3958) sees more than 2048 distinct blocks."""
    g = _rmat(15)
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    assert (deg <= 16).any() and ((deg > 16) & (deg <= 512)).any()
    assert ((deg > 512) & (deg <= 1536)).any() and (deg > 1536).any()
    part0 = ka.random_partition(g.n, k, seed=8)
    mbw = _caps(g, k)
    got = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
    _same(got, oracle_refine(oracle, g, k, mbw, part0, seed=5, iters=5))


# ------------------------------------------- 2. above the u16 label range
def test_refine_parity_above_u16(oracle):
    """k = 70001: the gathers must read the u32 labels, not the u16 shadow."""
    g = _rmat(17)
    k = 70001
    part0 = ka.random_partition(g.n, k, seed=8)
    mbw = _caps(g, k)
    got = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
    _same(got, oracle_refine(oracle, g, k, mbw, part0, seed=5, iters=5))
    assert (got[1] >= 65536).any()


# --------------------------------------------- 3. tier boundaries, full tables
TIER_RING = 6000
TIER_DEGS = [16, 17, 512, 513, 1536, 1537, 3000]


@functools.lru_cache(maxsize=None)
def _tier_graph():
    """Ring of 6000 vertices plus seven spokes of degree exactly 16, 17, 512,
    513, 1536, 1537 and 3000: both sides of each tier boundary, and a pooled
    region. Spoke i is joined to the consecutive ring vertices 7 i, 7 i + 1,
    ..., fewer than 4096 of them, so that under the start partition u mod 4096
    every neighbour of a spoke lies in a different block."""
    ring = TIER_RING
    n = ring + len(TIER_DEGS)
    adj = [[(v - 1) % ring, (v + 1) % ring] for v in range(ring)] + [[] for _ in TIER_DEGS]
    for i, d in enumerate(TIER_DEGS):
        s = ring + i
        for j in range(d):
            v = 7 * i + j
            adj[s].append(v)
            adj[v].append(s)
    xadj = np.zeros(n + 1, dtype=np.uint32)
    xadj[1:] = np.cumsum([len(a) for a in adj])
    adjncy = np.array([v for a in adj for v in a], dtype=np.uint32)
    g = ka.Graph.from_csr(xadj, adjncy)
    assert np.diff(np.asarray(g.xadj, dtype=np.int64))[ring:].tolist() == TIER_DEGS
    return g


def test_tier_boundaries_full_tables(oracle):
    """512 distinct keys in the 1024-slot hash, 1536 in the 4096-slot hash and
    3000 in a pooled region. Start partition u mod k; caps of 8 (blocks start
    at weight 1 or 2), except that the seven home blocks of the spoke centres
    are closed at cap 1. With open home blocks the ring neighbours join their
    spoke first and four of the seven centres stay; with closed ones the
    oracle moves every centre, asserted below."""
    g = _tier_graph()
    k = 4096
    part0 = (np.arange(g.n) % k).astype(np.uint32)
    adjncy = np.asarray(g.adjncy)
    xadj = np.asarray(g.xadj, dtype=np.int64)
    for i, d in enumerate(TIER_DEGS):
        s = TIER_RING + i
        assert len(set(part0[adjncy[xadj[s]:xadj[s + 1]]].tolist())) == d
    mbw = np.full(k, 8, dtype=np.int64)
    mbw[part0[TIER_RING:]] = 1
    want = oracle_refine(oracle, g, k, mbw, part0, seed=5, iters=5)
    assert (want[1][TIER_RING:] != part0[TIER_RING:]).all()
    got = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
    _same(got, want)


# ------------------------------------------------------------ 4. weighted
@functools.lru_cache(maxsize=None)
def _weighted_graph():
    """Seeded random graph with vertex weights 1..9 and symmetric edge weights
    1..9, plus a weighted hub of degree 2500 (the pooled tier) and one of
    degree 700 (the workgroup tier)."""
    rng = np.random.default_rng(0)
    n = 12000
    src = rng.integers(0, n, 150000)
    dst = rng.integers(0, n, 150000)
    hubs = [(0, rng.choice(np.arange(1, n), 2500, replace=False)),
            (1, rng.choice(np.arange(2, n), 700, replace=False))]
    src = np.concatenate([src] + [np.full(len(v), h) for h, v in hubs])
    dst = np.concatenate([dst] + [v for _, v in hubs])
    mask = src != dst
    pairs = np.unique(
        np.stack([np.concatenate([src[mask], dst[mask]]),
                  np.concatenate([dst[mask], src[mask]])], 1), axis=0)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    xadj = np.zeros(n + 1, np.uint32)
    np.add.at(xadj, pairs[:, 0] + 1, 1)
    xadj = np.cumsum(xadj).astype(np.uint32)
    adjncy = pairs[:, 1].astype(np.uint32)
    vwgt = rng.integers(1, 10, n).astype(np.int32)
    lo = np.minimum(pairs[:, 0], pairs[:, 1]).astype(np.int64)
    hi = np.maximum(pairs[:, 0], pairs[:, 1]).astype(np.int64)
    adjwgt = (((lo * 1000003 + hi * 7919) % 9) + 1).astype(np.int32)
    return ka.Graph.from_csr(xadj, adjncy, vwgt, adjwgt), vwgt, adjwgt


def test_refine_parity_weighted(oracle):
    g, vwgt, adjwgt = _weighted_graph()
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    assert deg.max() > 1536 and ((deg > 512) & (deg <= 1536)).any()
    k = 3000
    part0 = ka.random_partition(g.n, k, seed=8)
    mbw = _caps(g, k)
    got = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
    _same(got, oracle_refine(oracle, g, k, mbw, part0, seed=5, iters=5, vwgt=vwgt,
                             adjwgt=adjwgt))


# ------------------------------------------------------------- 5. balance
@pytest.mark.parametrize("start", ["block0", "random"])
def test_balance_parity(oracle, start):
    """Mode 1 (overloaded vertices lose stay, per-chunk fallback target). The
    graph has isolated vertices, so the host pre-pass runs as well."""
    g = _rmat(15)
    k = 4096
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    assert (deg == 0).any()
    if start == "block0":
        part0 = np.zeros(g.n, dtype=np.uint32)
        mbw = _caps(g, k)
    else:
        part0 = ka.random_partition(g.n, k, seed=8)
        mbw = np.full(k, g.max_block_weight(k, 0.0), dtype=np.int64)
    w0 = np.bincount(part0, minlength=k)
    assert (w0 > mbw).any(), "the start partition must violate the caps"
    got = ka.LpEngine(g).balance(k, mbw, part0, seed=5, iters=5)
    _same(got, oracle_balance(oracle, g, k, mbw, part0, seed=5, iters=5))


# ------------------------------------------------------ 6. resident forms
def test_resident_refine(oracle):
    g = _rmat(15)
    k = 4096
    part0 = ka.random_partition(g.n, k, seed=8)
    mbw = _caps(g, k)
    cut, part, st = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
    assert st.moves > 0
    eng = ka.LpEngine(g)
    eng.set_labels(k, part0)
    rcut, rpart, rst = eng.refine(k, mbw, None, seed=5, iters=5)
    assert rpart is None
    assert rcut == cut and rst.moves == st.moves
    assert np.array_equal(eng.get_labels(), part)


@functools.lru_cache(maxsize=None)
def _deep_gpu():
    from kaminpar_amd.partition import partition_deep

    return partition_deep(_rmat(15), 4096)


def test_resident_partition_deep():
    from kaminpar_amd.partition import partition_deep

    cut, part, sizes = _deep_gpu()
    rcut, rpart, rsizes = partition_deep(_rmat(15), 4096, resident=True)
    assert rcut == cut and rsizes == sizes
    assert np.array_equal(rpart, part)


# ------------------------------------------------------------ 7. pipelines
def test_partition_deep_matches_oracle(oracle):
    from oracle_pipeline import oracle_partition_deep

    g = _rmat(15)
    k = 4096
    cut, part, sizes = _deep_gpu()
    ocut, opart, osizes = oracle_partition_deep(oracle, g, k)
    assert cut == ocut and sizes == osizes
    assert np.array_equal(part, opart)
    w = np.bincount(part, minlength=k)
    assert w.max() <= g.max_block_weight(k, 0.03)
    assert (w > 0).all()


def test_partition_deep_native_matches_python():
    cut, part, _ = _deep_gpu()
    ncut, npart = _rmat(15).partition_deep_native(4096)
    assert ncut == cut
    assert np.array_equal(npart, part)


def test_partition_matches_oracle(oracle):
    """Equality only: the basic driver's result is not feasible at k close to
    n (its coarsening / initial-partition rule, not LP)."""
    from kaminpar_amd.partition import partition
    from oracle_pipeline import oracle_partition

    g = _rmat(15)
    cut, part, sizes = partition(g, 4096)
    ocut, opart, osizes = oracle_partition(oracle, g, 4096)
    assert cut == ocut and sizes == osizes
    assert np.array_equal(part, opart)


# ------------------------------------------------- 8. limits and refusals
def test_limits_and_refusals(oracle):
    g = ka.Graph.rmat(12, 8, seed=7)
    eng = ka.LpEngine(g)
    k = KMP_LP_MAX_K + 1
    with pytest.raises(RuntimeError):
        eng.refine(k, np.full(k, g.n, np.int64), np.zeros(g.n, np.uint32))
    k = 4096
    part0 = ka.random_partition(g.n, k, seed=5)
    with pytest.raises(RuntimeError):
        eng.underload(k, _caps(g, k), np.zeros(k, np.int64), part0)
    bad = part0.copy()
    bad[17] = k  # a label that is not below k
    with pytest.raises(RuntimeError):
        eng.refine(k, _caps(g, k), bad)
    with pytest.raises(RuntimeError):
        eng.balance(k, _caps(g, k), bad)
    # the engine still works after the rejections
    k = 16
    part0 = ka.random_partition(g.n, k, seed=5)
    mbw = _caps(g, k, 0.03)
    got = eng.refine(k, mbw, part0, seed=1, iters=5)
    _same(got, oracle_refine(oracle, g, k, mbw, part0, seed=1, iters=5))


# ------------------------------------------- 9. engine reuse across paths
def test_engine_reuse_across_paths():
    """k = 4096 (hash tiers), 16 (v2 commit), 1024 (dense legacy), 4096 again
    on one engine: per-k buffers and the hash pool must be left clean."""
    g = _rmat(15)
    eng = ka.LpEngine(g)
    for k in (4096, 16, 1024, 4096):
        part0 = ka.random_partition(g.n, k, seed=8)
        mbw = _caps(g, k)
        cut, part, st = eng.refine(k, mbw, part0, seed=5, iters=5)
        fcut, fpart, fst = ka.LpEngine(g).refine(k, mbw, part0, seed=5, iters=5)
        assert st.moves > 0
        assert cut == fcut and st.moves == fst.moves
        assert st.arcs_scanned == fst.arcs_scanned
        assert np.array_equal(part, fpart)
