"""Engines built on the device from edge lists (kmp_lp_create_from_edges,
LpEngine.from_edges / from_edge_index, partition_edges, get_labels(out=)).
The device CSR is fetched with download_graph() and compared bit for bit with
the numpy twin (tests/edges_twin.py) and with the hand-computed cases
(tests/edges_cases.py); the stats are compared with the twin's."""

import ctypes
import functools

import numpy as np
import pytest

# torch bundles its own HIP runtime; it must initialize BEFORE any engine in
# this process creates a context with the system runtime (see
# test_extract_gpu.py).
import torch

if torch.cuda.is_available():
    torch.zeros(1, device="cuda:0")

import edges_cases as ec
import kaminpar_amd as ka
from edges_twin import STAT_FIELDS, edges_to_csr
from helpers import oracle_refine
from kaminpar_amd.partition import partition, partition_deep, partition_edges

pytestmark = pytest.mark.gpu

HOWS = ("host", "tensor64", "tensor32")


def build(src, dst, n=None, weights=None, combine="max", how="host", vwgt=None):
    """(engine, EdgesStats) through host pointers or GPU tensors."""
    if how == "host":
        return ka.LpEngine.from_edges(src, dst, n=n, weights=weights, vwgt=vwgt,
                                      combine=combine, return_stats=True)
    dt = torch.int64 if how == "tensor64" else torch.int32
    dev = lambda a, t: None if a is None else torch.as_tensor(
        np.asarray(a).astype(np.int64), device="cuda:0").to(t).contiguous()
    return ka.LpEngine.from_edges(
        dev(src, dt), dev(dst, dt), n=n, weights=dev(weights, torch.int32),
        vwgt=dev(vwgt, torch.int32), combine=combine, return_stats=True)


def csr_of(eng):
    g = eng.download_graph()
    aw = g.adjwgt
    return (np.asarray(g.xadj).astype(np.int64), np.asarray(g.adjncy).copy(),
            None if aw is None else np.asarray(aw).copy())


def same_as(eng, stats, want):
    """Engine and stats against a twin result (n, xadj, adjncy, adjwgt, stats)."""
    n, xadj, adjncy, adjwgt, wstats = want
    for name in STAT_FIELDS:
        assert int(getattr(stats, name)) == wstats[name], name
    assert eng.n == n and eng.m == len(adjncy)
    got = csr_of(eng)
    assert np.array_equal(got[0], xadj)
    assert np.array_equal(got[1], adjncy)
    if adjwgt is None or len(adjwgt) == 0:  # a host graph keeps no empty array
        assert got[2] is None or len(got[2]) == 0
    else:
        assert np.array_equal(got[2], adjwgt)


# ------------------------------------------------ hand-computed cases
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_hand_cases(name, how):
    src, dst, n, weights, combine, want = ec.case_arrays(name)
    eng, stats = build(src, dst, n, weights, combine, how)
    wn, wxadj, wadj, wwgt, wloops = want
    got = csr_of(eng)
    assert eng.n == wn and got[0].tolist() == wxadj and got[1].tolist() == wadj
    if wwgt is not None:
        assert got[2].tolist() == wwgt
    else:
        assert got[2] is None
    assert stats.self_loops == wloops and stats.pairs == len(src)
    same_as(eng, stats, edges_to_csr(src, dst, n, weights, combine))


def test_uint32_host_ids_and_edge_index():
    src, dst, n, weights, combine, _ = ec.case_arrays("weights_sum", np.uint32)
    want = edges_to_csr(src, dst, n, weights, combine)
    same_as(*build(src, dst, n, weights, combine), want)
    ei = np.stack([src, dst])
    same_as(*ka.LpEngine.from_edge_index(ei, n=n, weights=weights, combine=combine,
                                         return_stats=True), want)
    tei = torch.as_tensor(ei.astype(np.int64), device="cuda:0")
    tw = torch.as_tensor(weights, device="cuda:0")
    same_as(*ka.LpEngine.from_edge_index(tei, n=n, weights=tw, combine=combine,
                                         return_stats=True), want)
    # an odd number of pairs: row 1 of the tensor is not 16-byte aligned
    ei3 = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int32)
    t3 = torch.as_tensor(ei3, device="cuda:0")
    same_as(*ka.LpEngine.from_edge_index(t3, return_stats=True),
            edges_to_csr(ei3[0], ei3[1]))


def test_empty_list_is_all_isolated():
    none = np.zeros(0, dtype=np.int64)
    for how in HOWS:
        eng, stats = build(none, none, 5, how=how)
        same_as(eng, stats, edges_to_csr(none, none, 5))
        assert stats.isolated == 5 and stats.max_degree == 0 and eng.m == 0
    nc, clus, _ = eng.cluster(2, seed=1, iters=3)
    ref = ka.LpEngine(ka.Graph.from_csr(np.zeros(6, np.uint32), np.zeros(0, np.uint32)))
    nc2, clus2, _ = ref.cluster(2, seed=1, iters=3)
    assert nc == nc2 and np.array_equal(clus, clus2)


def test_single_vertex():
    none = np.zeros(0, dtype=np.int64)
    same_as(*build(none, none, 1), edges_to_csr(none, none, 1))
    loop = np.zeros(3, dtype=np.int64)
    for how in HOWS:
        eng, stats = build(loop, loop, None, how=how)
        same_as(eng, stats, edges_to_csr(loop, loop))
        assert eng.n == 1 and eng.m == 0 and stats.self_loops == 3


# ------------------------------------------------ long runs, hubs, widths
@pytest.mark.parametrize("how", ("host", "tensor64"))
def test_long_run_of_duplicates(how):
    """One edge 5000 times: the run is longer than any workgroup tile."""
    src, dst, w = ec.long_run()
    eng, stats = build(src, dst, 2, w, "max", how)
    assert csr_of(eng)[2].tolist() == [5000, 5000]
    same_as(eng, stats, edges_to_csr(src, dst, 2, w, "max"))
    eng, stats = build(src, dst, 2, w, "sum", how)
    assert csr_of(eng)[2].tolist() == [12502500, 12502500]
    same_as(eng, stats, edges_to_csr(src, dst, 2, w, "sum"))
    assert stats.merged_arcs == 2 * 5000 - 2


def test_long_run_overflows():
    src, dst, _ = ec.long_run()
    big = np.full(5000, (1 << 31) // 2500, dtype=np.int32)
    with pytest.raises(RuntimeError):
        build(src, dst, 2, big, "sum")
    eng, _ = build(src, dst, 2, big, "max")
    assert csr_of(eng)[2].tolist() == [(1 << 31) // 2500] * 2
    # the largest sum that fits, and one more
    fit = np.array([(1 << 31) - 2, 1], dtype=np.int32)
    eng, _ = build([0, 1], [1, 0], 2, fit, "sum")
    assert csr_of(eng)[2].tolist() == [ec.I32_MAX] * 2
    with pytest.raises(RuntimeError):
        build([0, 1, 0], [1, 0, 1], 2, np.array([(1 << 31) - 2, 1, 1], np.int32), "sum")


@pytest.mark.parametrize("how", ("host", "tensor32"))
def test_hub_and_empty_rows(how):
    src, dst, n = ec.hub_graph()
    p = np.random.default_rng(4).permutation(len(src))
    eng, stats = build(src[p], dst[p], n, how=how)
    same_as(eng, stats, edges_to_csr(src, dst, n))
    deg = np.diff(csr_of(eng)[0])
    assert deg[0] == 0 and deg[1] == 3000 and deg[2] == 16 and deg[3] == 17
    assert np.flatnonzero(deg[:100] > 0).tolist() == [1, 2, 3, 5, 8, 79]
    assert (deg[3100:] == 0).all() and stats.max_degree == 3000


@pytest.mark.parametrize("n", (1023, 1024, 1025))
def test_key_width_boundaries(n):
    rng = np.random.default_rng(n)
    src = rng.integers(0, n, 4000)
    dst = rng.integers(0, n, 4000)
    src[7], dst[7] = n - 1, 0
    src[8], dst[8] = n - 2, n - 1
    w = rng.integers(1, 8, 4000).astype(np.int32)
    same_as(*build(src, dst, n), edges_to_csr(src, dst, n))
    same_as(*build(src, dst, None, w, "sum", "tensor64"), edges_to_csr(src, dst, None, w, "sum"))
    with pytest.raises(RuntimeError):
        build(src, dst, n - 1)


# ------------------------------------------------ R-MAT round trip
@functools.lru_cache(maxsize=None)
def rmat14():
    """(graph, rows sorted CSR, shuffled messy list, twin result)."""
    g = ka.Graph.rmat(14, 8, seed=3)
    xadj = np.asarray(g.xadj).astype(np.int64)
    adjncy = np.asarray(g.adjncy).copy()
    rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(xadj))
    order = np.lexsort((adjncy, rows))
    sorted_adj = adjncy[order]
    up = rows < adjncy
    src, dst = rows[up].copy(), adjncy[up].astype(np.int64)
    third = np.arange(len(src)) % 3 == 0
    src[third], dst[third] = dst[third], src[third].copy()
    rng = np.random.default_rng(14)
    dup = rng.integers(0, len(src), len(src) // 10)
    loops = rng.integers(0, g.n, 50)
    src = np.concatenate([src, src[dup], loops])
    dst = np.concatenate([dst, dst[dup], loops])
    p = rng.permutation(len(src))
    src, dst = src[p], dst[p]
    src.setflags(write=False)
    dst.setflags(write=False)
    return g, (xadj, sorted_adj), (src, dst), edges_to_csr(src, dst, g.n)


@pytest.mark.parametrize("how", HOWS)
def test_rmat_round_trip(how):
    g, (xadj, sorted_adj), (src, dst), want = rmat14()
    eng, stats = build(src, dst, g.n, how=how)
    same_as(eng, stats, want)
    got = csr_of(eng)
    assert np.array_equal(got[0], xadj) and np.array_equal(got[1], sorted_adj)
    assert got[2] is None and stats.self_loops == 50
    assert stats.merged_arcs == 2 * (len(src) - 50) - g.m


def test_second_shuffle_gives_the_same_engine():
    g, _, (src, dst), want = rmat14()
    p = np.random.default_rng(99).permutation(len(src))
    flip = np.random.default_rng(98).random(len(src)) < 0.5
    s2 = np.where(flip, dst[p], src[p])
    d2 = np.where(flip, src[p], dst[p])
    a, b = build(src, dst, g.n)[0], build(s2, d2, g.n, how="tensor64")[0]
    for x, y in zip(csr_of(a), csr_of(b)):
        assert (x is None and y is None) or np.array_equal(x, y)
    same_as(b, b.edges_stats, want)


def test_inputs_are_not_modified():
    g, _, (src, dst), _ = rmat14()
    rng = np.random.default_rng(3)
    w = rng.integers(1, 8, len(src)).astype(np.int32)
    vw = rng.integers(1, 4, g.n).astype(np.int32)
    s0, d0, w0, v0 = src.copy(), dst.copy(), w.copy(), vw.copy()
    ka.LpEngine.from_edges(s0, d0, n=g.n, weights=w0, vwgt=v0, combine="sum")
    assert np.array_equal(s0, src) and np.array_equal(d0, dst)
    assert np.array_equal(w0, w) and np.array_equal(v0, vw)
    ts, td = torch.as_tensor(src.copy(), device="cuda:0"), torch.as_tensor(dst.copy(), device="cuda:0")
    tw, tv = torch.as_tensor(w, device="cuda:0"), torch.as_tensor(vw, device="cuda:0")
    eng = ka.LpEngine.from_edges(ts, td, n=g.n, weights=tw, vwgt=tv, combine="sum")
    assert np.array_equal(ts.cpu().numpy(), src) and np.array_equal(td.cpu().numpy(), dst)
    assert np.array_equal(tw.cpu().numpy(), w) and np.array_equal(tv.cpu().numpy(), vw)
    assert np.array_equal(np.asarray(eng.download_graph().vwgt), vw)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("combine", ("max", "sum"))
def test_random_weights(combine, how):
    g, _, (src, dst), _ = rmat14()
    w = np.random.default_rng(21).integers(1, 8, len(src)).astype(np.int32)
    same_as(*build(src, dst, g.n, w, combine, how), edges_to_csr(src, dst, g.n, w, combine))


# ------------------------------------------------ errors
# every error through every entry, except the id 2^32 as a 32-bit tensor,
# where it does not exist
ERROR_RUNS = [(name, how) for name in sorted(ec.ERRORS) for how in HOWS
              if not (name == "id_2_pow_32" and how == "tensor32")]


@pytest.mark.parametrize("name,how", ERROR_RUNS)
def test_errors(name, how):
    src, dst, n, weights, combine = ec.error_arrays(name)
    with pytest.raises(RuntimeError):
        build(src, dst, n, weights, combine, how)
    # the next valid build in the same process succeeds
    s, d, n2, w2, c2, _ = ec.case_arrays("weights_sum")
    same_as(*build(s, d, n2, w2, c2, how), edges_to_csr(s, d, n2, w2, c2))


def test_too_many_pairs():
    """2 * pairs >= 2^32 is refused before anything is read."""
    one = np.zeros(4, dtype=np.uint32)
    h = ka._lib.kmp_lp_create_from_edges(5, 1 << 31, one.ctypes.data, one.ctypes.data,
                                         None, None, 0, None)
    assert not h
    assert not ka._lib.kmp_lp_create_from_edges(5, 4, one.ctypes.data, one.ctypes.data,
                                                None, None, 1 << 9, None)  # unknown flag
    # vwgt without n: its length would have to be the inferred n
    vw = np.ones(4, dtype=np.int32)
    assert not ka._lib.kmp_lp_create_from_edges(0, 4, one.ctypes.data, one.ctypes.data,
                                                None, vw.ctypes.data, 0, None)
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(one, one, vwgt=vw)


def test_argument_errors():
    a = np.array([0, 1], dtype=np.int64)
    t = torch.as_tensor(a, device="cuda:0")
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(a, t, n=3)  # host and device mixed
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(t, t, n=3, weights=np.array([1, 1], np.int32))
    wide = torch.zeros((2, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(wide[:, 0], wide[:, 1], n=3)  # not contiguous
    with pytest.raises(ValueError):
        ka.LpEngine.from_edge_index(wide[:, :2])  # not contiguous
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(t.cpu(), t.cpu(), n=3)  # tensors must be on the GPU
    with pytest.raises(ValueError):
        ka.LpEngine.from_edges(a, a, n=3, combine="min")


# ------------------------------------------------ downstream state
@functools.lru_cache(maxsize=None)
def hub_case():
    src, dst, n = ec.hub_graph()
    rng = np.random.default_rng(31)
    src = np.concatenate([src, rng.integers(100, 3100, 6000)])
    dst = np.concatenate([dst, rng.integers(100, 3100, 6000)])
    w = rng.integers(1, 8, len(src)).astype(np.int32)
    return src, dst, n, w, edges_to_csr(src, dst, n, w, "max")


def engines_pair(how="tensor64"):
    src, dst, n, w, want = hub_case()
    a, _ = build(src, dst, n, w, "max", how)
    g = ka.Graph.from_csr(want[1], want[2], None, want[3])
    return a, ka.LpEngine(g), g, want


def lp_stats(st):
    return (st.arcs_scanned, st.moves, st.num_clusters, st.edge_cut)


def test_downstream_cluster_and_contract():
    a, b, g, want = engines_pair()
    assert want[4]["isolated"] > 0 and want[4]["max_degree"] >= 3000
    ra, rb = a.cluster(40, seed=2, iters=3), b.cluster(40, seed=2, iters=3)
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1])
    assert lp_stats(ra[2]) == lp_stats(rb[2])
    ca, ma = a.contract_engine(ra[1])
    cb, mb = b.contract_engine(rb[1])
    assert np.array_equal(ma, mb) and ca.n == cb.n and ca.m == cb.m
    ga, gb = ca.download_graph(), cb.download_graph()
    for name in ("xadj", "adjncy", "adjwgt", "vwgt"):
        assert np.array_equal(getattr(ga, name), getattr(gb, name)), name
    # and the resident form, from the clustering the engine holds
    ca2, _ = a.contract_engine(None, download_mapping=False)
    assert np.array_equal(ca2.download_graph().adjwgt, gb.adjwgt)


def test_downstream_refine_and_jet(oracle):
    a, b, g, want = engines_pair("host")
    k = 8
    caps = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    part0 = ka.random_partition(g.n, k, seed=5)
    ra, rb = a.refine(k, caps, part0, seed=3, iters=3), b.refine(k, caps, part0, seed=3, iters=3)
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and lp_stats(ra[2]) == lp_stats(rb[2])
    ocut, opart, _ = oracle_refine(oracle, g, k, caps, part0, seed=3, iters=3,
                                   adjwgt=np.ascontiguousarray(want[3]))
    assert ocut == ra[0] and np.array_equal(opart, ra[1])
    ja = a.jet(k, caps, ra[1], seed=3, balancer=1, max_fruitless=3)
    jb = b.jet(k, caps, rb[1], seed=3, balancer=1, max_fruitless=3)
    assert ja[0] == jb[0] and np.array_equal(ja[1], jb[1])
    assert ja[0] == g.edge_cut(ja[1])


def test_rearrange_degree_buckets():
    a, b, g, _ = engines_pair()
    _, host_perm = g.rearrange_degree_buckets()
    assert np.array_equal(a.rearrange_degree_buckets(), host_perm)


def test_vertex_weights():
    src, dst, n, w, want = hub_case()
    vw = np.random.default_rng(8).integers(1, 5, n).astype(np.int32)
    g = ka.Graph.from_csr(want[1], want[2], vw, want[3])
    b = ka.LpEngine(g)
    for how in ("host", "tensor32"):
        a, _ = build(src, dst, n, w, "max", how, vwgt=vw)
        assert np.array_equal(a.download_graph().vwgt, vw)
        ra, rb = a.cluster(60, seed=1, iters=2), b.cluster(60, seed=1, iters=2)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1])


# ------------------------------------------------ drivers
def test_partition_edges_without_download():
    g, _, (src, dst), want = rmat14()
    tg = ka.Graph.from_csr(want[1], want[2])
    ref = partition(tg, 16, fm=False, resident=True)
    facade = []
    ts, td = torch.as_tensor(src.copy(), device="cuda:0"), torch.as_tensor(dst.copy(), device="cuda:0")
    got = partition_edges(ts, td, 16, n=g.n, fm=False, resident=True, facade_out=facade)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert len(got[2]) > 1 and facade[0].downloaded is False
    assert facade[0].max_block_weight(16, 0.03) == tg.max_block_weight(16, 0.03)
    assert facade[0].total_node_weight == tg.total_node_weight


def test_partition_edges_with_fm_downloads_once():
    g, _, (src, dst), want = rmat14()
    tg = ka.Graph.from_csr(want[1], want[2])
    ref = partition(tg, 16)
    facade = []
    got = partition_edges(src, dst, 16, n=g.n, facade_out=facade)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert facade[0].downloaded is True


def test_partition_edges_deep():
    g, _, (src, dst), want = rmat14()
    tg = ka.Graph.from_csr(want[1], want[2])
    ref = partition_deep(tg, 16)
    got = partition_edges(src, dst, 16, n=g.n, deep=True)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


def test_get_labels_on_device():
    a, _, g, _ = engines_pair()
    with pytest.raises(RuntimeError):
        a.get_labels(out=torch.zeros(a.n, dtype=torch.int32, device="cuda:0"))
    k = 8
    caps = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    a.refine(k, caps, ka.random_partition(g.n, k, seed=5), seed=3, iters=2)
    before = ka.label_traffic_bytes()
    out = torch.full((a.n,), -1, dtype=torch.int32, device="cuda:0")
    assert a.get_labels(out=out) is out
    assert ka.label_traffic_bytes() == before
    assert np.array_equal(out.cpu().numpy().astype(np.uint32), a.get_labels())
    with pytest.raises(ValueError):
        a.get_labels(out=torch.zeros(a.n + 1, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        a.get_labels(out=torch.zeros(a.n, dtype=torch.float32, device="cuda:0"))
