"""Resident labels: partitions, clusterings and mappings that stay on the device
between the stages of the multilevel chain (kmp_lp_set_labels / get_labels /
project, the NULL forms of refine / jet / rebalance / cluster / contract_engine,
and resident=True of the Python pipelines). Everything is compared EXACTLY with
the host forms, which are the yardstick: the projection with numpy's
coarse_part[mapping], a resident call with the same call on host arrays on a
second engine, a resident pipeline with the host pipeline."""

import os

import numpy as np
import pytest

# torch bundles its own HIP runtime; it must initialize BEFORE any engine in
# this process creates a context with the system runtime (see
# test_extract_gpu.py).
import torch as _torch

if _torch.cuda.is_available():
    _torch.zeros(1, device="cuda:0")

import kaminpar_amd as ka
import rebalance_cases as rc
from kaminpar_amd.partition import level_cluster_weight, partition, partition_deep
from test_extract_gpu import same_graph

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def coarse_labels(c_n, k):
    return ((np.arange(c_n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7))
            % np.uint64(k)).astype(np.uint32)


def coarse_caps(coarse, k):
    """Uniform caps of the coarse graph at 3 % imbalance (any caps would do: the
    refiners only have to produce some state of their own)."""
    hg = coarse.download_graph()
    return np.full(k, hg.max_block_weight(k, 0.03), dtype=np.int64)


def contract_host(g, k=16, mcw=None):
    """(fine engine, coarse engine, mapping) through the host forms."""
    eng = ka.LpEngine(g)
    if mcw is None:
        mcw = level_cluster_weight(g.total_node_weight, g.n, k, 0.03)
    _, clus, _ = eng.cluster(mcw, seed=1)
    coarse, mapping = eng.contract_engine(clus)
    return eng, coarse, mapping


def same_stats(a, b):
    """Every stats field that is not a time."""
    assert type(a) is type(b)
    for name, _ in a._fields_:
        if not name.endswith("_ns"):
            assert getattr(a, name) == getattr(b, name), name


def ring(n):
    xadj = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    v = np.arange(n, dtype=np.int64)
    adjncy = np.stack([(v - 1) % n, (v + 1) % n], axis=1).reshape(-1).astype(np.uint32)
    return ka.Graph.from_csr(xadj, adjncy)


# ------------------------------------------------------------ 1. projection
_PAIRS = {}


def rmat_pair(scale):
    """One contraction per scale, shared: the tests only replace label state."""
    if scale not in _PAIRS:
        _PAIRS[scale] = contract_host(ka.Graph.rmat(scale, 8, seed=7))
    return _PAIRS[scale]


def produce(coarse, k, how):
    """Puts a partition on the coarse engine the given way; returns it."""
    coarse.set_labels(k, coarse_labels(coarse.n, k))
    if how == "set_labels":
        return coarse_labels(coarse.n, k)
    caps = coarse_caps(coarse, k)
    if how == "refine":
        coarse.refine(k, caps, None, seed=1, iters=2)
    elif how == "jet0":
        coarse.jet(k, caps, None, seed=1, coarse_level=1, balancer=0, max_fruitless=3)
    elif how == "jet1":
        coarse.jet(k, caps, None, seed=1, coarse_level=1, balancer=1, max_fruitless=3)
    else:
        raise AssertionError(how)
    return coarse.get_labels()


def check_projection(fine, coarse, mapping, k, how="set_labels"):
    cpart = produce(coarse, k, how)
    assert cpart.max() < k
    fine.project_from(coarse)
    assert (fine.get_labels() == cpart[mapping]).all()
    # the coarse state is untouched
    assert (coarse.get_labels() == cpart).all()


@pytest.mark.parametrize("how", ["set_labels", "refine", "jet0", "jet1"])
@pytest.mark.parametrize("k", [2, 16, 256, 257, 2048])
@pytest.mark.parametrize("scale", [10, 12])
def test_projection_rmat(scale, k, how):
    """k = 256 is the last u8 shadow, 257 the first u16 one; the refiners leave
    the shadows the gather may read, set_labels does not."""
    fine, coarse, mapping = rmat_pair(scale)
    check_projection(fine, coarse, mapping, k, how)


@pytest.mark.parametrize("how", ["set_labels", "refine", "jet1"])
def test_projection_odd_n(how):
    c = rc.odd_n_case()
    assert c.g.n == 1037
    fine, coarse, mapping = contract_host(c.g, c.k)
    check_projection(fine, coarse, mapping, c.k, how)


@pytest.mark.parametrize("how", ["set_labels", "refine", "jet0"])
def test_projection_weighted(how):
    g, _, _ = rc.weighted_rgg()
    fine, coarse, mapping = contract_host(g, 4)
    check_projection(fine, coarse, mapping, 4, how)


def test_projection_tiny_coarse_graph():
    """Fewer than 64 coarse vertices: the gather table is below one wavefront."""
    fine = ka.LpEngine(ring(200))
    while True:  # a ring shrinks slowly: contract until the table is that small
        _, clus, _ = fine.cluster(64, seed=1)
        coarse, mapping = fine.contract_engine(clus)
        assert 0 < coarse.n < fine.n
        if coarse.n < 64:
            break
        fine = coarse
    for k in (2, 16):
        check_projection(fine, coarse, mapping, k)
        check_projection(fine, coarse, mapping, k, "refine")


def test_projection_second_trip():
    """2^22 vertices: the grid is capped at 2048 workgroups of 256 lanes with
    four vertices each, so the grid-stride loop takes a second trip."""
    g = ka.Graph.rmat(22, 1)
    assert g.n == 1 << 22 and g.n > 2048 * 256 * 4
    eng = ka.LpEngine(g)
    clus = (np.arange(g.n, dtype=np.uint32) & ~np.uint32(1)).astype(np.uint32)
    coarse, mapping = eng.contract_engine(clus)
    assert coarse.n == g.n // 2
    assert (mapping == np.arange(g.n, dtype=np.uint32) >> 1).all()
    cpart = coarse_labels(coarse.n, 16)
    coarse.set_labels(16, cpart)
    eng.project_from(coarse)
    assert (eng.get_labels() == cpart[mapping]).all()


def test_projection_chain_of_two():
    """Project twice without a refiner in between: the middle engine's shadows
    are stale then, and must not be read."""
    fine, mid, map0 = contract_host(ka.Graph.rmat(12, 8, seed=7))
    mid.cluster(level_cluster_weight(fine.n, mid.n, 16, 0.03), seed=2, download=False)
    coarse, map1 = mid.contract_engine(None)
    k = 16
    # leave shadows of another partition on the middle engine first
    mid.set_labels(k, coarse_labels(mid.n, k)[::-1].copy())
    mid.refine(k, coarse_caps(mid, k), None, seed=1, iters=1)
    cpart = coarse_labels(coarse.n, k)
    coarse.set_labels(k, cpart)
    mid.project_from(coarse)
    fine.project_from(mid)
    assert (fine.get_labels() == cpart[map1][map0]).all()


# ---------------------------------------------------- 2. resident == host
def cases():
    return {
        "rmat12_k16": lambda: rc.rmat_case(12, 16, "skewed"),
        "rmat12_k300": lambda: rc.rmat_case(12, 300, "skewed"),
        "weighted_k4": lambda: rc.weighted_case(4),
        "isolated": rc.isolated_case,
        "tiers": rc.tiers_case,
    }


CASES = sorted(cases())


def both_forms(c, call):
    """call(engine, partition) on host arrays and, on a second engine, on the
    resident partition. Returns (host result, resident result, resident
    labels)."""
    host = call(ka.LpEngine(c.g), c.part0)
    eng = ka.LpEngine(c.g)
    eng.set_labels(c.k, c.part0)
    res = call(eng, None)
    return host, res, eng.get_labels()


def check_both_forms(c, call):
    (hcut, hpart, hst), (rcut, rpart, rst), labels = both_forms(c, call)
    assert rpart is None
    assert (labels == hpart).all()
    assert rcut == hcut == c.g.edge_cut(hpart)
    same_stats(hst, rst)


@pytest.mark.parametrize("name", CASES)
def test_refine_resident_equals_host(name):
    """k = 16 and 4 run the v2 commit, k = 300 the legacy one."""
    c = cases()[name]()
    check_both_forms(c, lambda e, p: e.refine(c.k, c.caps, p, seed=3, iters=3))


@pytest.mark.parametrize("balancer", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_jet_resident_equals_host(name, balancer):
    """isolated: Jet's balancer 0 reads the isolated vertices' labels."""
    c = cases()[name]()
    check_both_forms(c, lambda e, p: e.jet(c.k, c.caps, p, seed=3, balancer=balancer,
                                           max_fruitless=4))


@pytest.mark.parametrize("name", CASES)
def test_rebalance_resident_equals_host(name):
    c = cases()[name]()
    check_both_forms(c, lambda e, p: e.rebalance(c.k, c.caps, p))


# ------------------------------------------------------------- 3. chaining
@pytest.mark.parametrize("name", ["rmat12_k16", "isolated", "weighted_k4"])
def test_chain_resident_equals_host(name):
    c = cases()[name]()
    h = ka.LpEngine(c.g)
    _, part, _ = h.refine(c.k, c.caps, c.part0, seed=2, iters=2)
    _, part, _ = h.jet(c.k, c.caps, part, seed=2, balancer=1, max_fruitless=3)
    hcut, part, _ = h.rebalance(c.k, c.caps, part)
    r = ka.LpEngine(c.g)
    r.set_labels(c.k, c.part0)
    r.refine(c.k, c.caps, None, seed=2, iters=2)
    r.jet(c.k, c.caps, None, seed=2, balancer=1, max_fruitless=3)
    rcut, none, _ = r.rebalance(c.k, c.caps, None)
    assert none is None and rcut == hcut
    assert (r.get_labels() == part).all()


def test_host_form_leaves_result_resident():
    c = rc.rmat_case(12, 16, "skewed")
    eng = ka.LpEngine(c.g)
    for call in (lambda p: eng.refine(c.k, c.caps, p, seed=1, iters=2),
                 lambda p: eng.jet(c.k, c.caps, p, seed=1, max_fruitless=2),
                 lambda p: eng.rebalance(c.k, c.caps, p)):
        _, part, _ = call(c.part0)
        assert (eng.get_labels() == part).all()
    # and a resident call continues from it
    cut, _, _ = eng.refine(c.k, c.caps, None, seed=1, iters=1)
    assert cut == c.g.edge_cut(eng.get_labels())


# -------------------------------------------------- 4. resident coarsening
def coarsen_both(g, k):
    mcw = level_cluster_weight(g.total_node_weight, g.n, k, 0.03)
    a = ka.LpEngine(g)
    nca, clus, _ = a.cluster(mcw, seed=1)
    ca, mapa = a.contract_engine(clus)
    b = ka.LpEngine(g)
    ncb, none, _ = b.cluster(mcw, seed=1, download=False)
    assert none is None and ncb == nca
    assert (b.get_labels() == clus).all()
    cb, mapb = b.contract_engine(None)
    assert (mapa == mapb).all()
    cb2, nomap = b.contract_engine(None, download_mapping=False)
    assert nomap is None and cb2.n == ca.n
    ga, gb = ca.download_graph(), cb.download_graph()
    same_graph(ga, gb)
    same_graph(ga, cb2.download_graph())
    # the clusterer uses the child's isolated list, their weights and max_deg
    mcw2 = level_cluster_weight(g.total_node_weight, ca.n, k, 0.03)
    ra, rb = ca.cluster(mcw2, seed=5), cb.cluster(mcw2, seed=5)
    assert ra[0] == rb[0] and (ra[1] == rb[1]).all()
    same_stats(ra[2], rb[2])
    return ca, cb, ga


@pytest.mark.parametrize("name", ["rmat12", "weighted_rgg"])
def test_resident_coarsening(name):
    g = ka.Graph.rmat(12, 8, seed=7) if name == "rmat12" else rc.weighted_rgg()[0]
    coarsen_both(g, 16)


def test_resident_coarsening_isolated_vertices():
    """The coarse graph keeps isolated vertices; balance and Jet's balancer 0
    move them, from the list the device scan produced."""
    c = rc.isolated_case()
    ca, cb, cg = coarsen_both(c.g, c.k)
    deg = np.diff(np.asarray(cg.xadj, dtype=np.int64))
    iso = np.flatnonzero(deg == 0)
    assert len(iso) > 0
    k = c.k
    caps = np.full(k, cg.max_block_weight(k, 0.03), dtype=np.int64)
    part0 = ka.random_partition(cg.n, k, seed=3)
    part0[iso] = 0
    part0[: cg.n // 2] = 0
    w = cg.vwgt.astype(np.int64)
    assert np.bincount(part0, weights=w, minlength=k)[0] > caps[0]
    for call in (lambda e: e.balance(k, caps, part0, seed=2, iters=3),
                 lambda e: e.jet(k, caps, part0, seed=2, balancer=0, max_fruitless=3)):
        xa, xb = call(ca), call(cb)
        assert xa[0] == xb[0] and (xa[1] == xb[1]).all()
        same_stats(xa[2], xb[2])
    # the balancer's isolated pre-pass did run: it moved isolated vertices
    assert (ca.balance(k, caps, part0, seed=2, iters=3)[1][iso] != 0).any()


# ------------------------------------------------------------- 5. refusals
def small():
    c = rc.rmat_case(10, 16, "skewed")
    return c, ka.LpEngine(c.g)


def test_refuse_refine_on_fresh_engine():
    c, eng = small()
    with pytest.raises(RuntimeError):
        eng.refine(c.k, c.caps, None)
    with pytest.raises(RuntimeError):
        eng.get_labels()
    cut, part, _ = eng.refine(c.k, c.caps, c.part0)
    assert cut == c.g.edge_cut(part)


def test_refuse_refine_on_clustering():
    c, eng = small()
    eng.cluster(8, seed=1, download=False)
    with pytest.raises(RuntimeError):
        eng.refine(c.k, c.caps, None)
    eng.set_labels(c.k, c.part0)
    cut, _, _ = eng.refine(c.k, c.caps, None)
    assert cut == c.g.edge_cut(eng.get_labels())


def test_refuse_contract_on_partition():
    c, eng = small()
    eng.refine(c.k, c.caps, c.part0)
    with pytest.raises(RuntimeError):
        eng.contract_engine(None)
    eng.cluster(8, seed=1, download=False)
    coarse, mapping = eng.contract_engine(None)
    assert 0 < coarse.n < eng.n and mapping.max() == coarse.n - 1


def test_refuse_label_out_of_range():
    c, eng = small()
    eng.set_labels(c.k, c.part0)
    bad = (c.part0 % 4).astype(np.uint32)
    bad[-1] = 4
    with pytest.raises(RuntimeError):
        eng.set_labels(4, bad)
    with pytest.raises(RuntimeError):  # nothing was uploaded, nothing is held
        eng.get_labels()
    eng.set_labels(5, bad)
    assert (eng.get_labels() == bad).all()


def test_refuse_smaller_k_than_resident():
    c, eng = small()
    eng.set_labels(16, c.part0)
    caps8 = rc.caps_of(c.g, 8)
    with pytest.raises(RuntimeError):
        eng.jet(8, caps8, None)
    with pytest.raises(RuntimeError):  # a failed call leaves no resident state
        eng.jet(16, c.caps, None)
    eng.set_labels(8, (c.part0 % 8).astype(np.uint32))
    cut, _, _ = eng.jet(16, c.caps, None, max_fruitless=2)  # a larger k is fine
    assert cut == c.g.edge_cut(eng.get_labels())


def test_refuse_project_onto_other_engine():
    c, eng = small()
    _, clus, _ = eng.cluster(8, seed=1)
    coarse, mapping = eng.contract_engine(clus)
    cpart = coarse_labels(coarse.n, 16)
    coarse.set_labels(16, cpart)
    other = ka.LpEngine(c.g)  # same graph, same n, another engine
    with pytest.raises(RuntimeError):
        other.project_from(coarse)
    with pytest.raises(RuntimeError):  # never a child
        coarse.project_from(eng)
    with pytest.raises(RuntimeError):
        other.get_labels()
    eng.project_from(coarse)
    assert (eng.get_labels() == cpart[mapping]).all()


def test_refuse_project_without_coarse_labels():
    c, eng = small()
    _, clus, _ = eng.cluster(8, seed=1)
    coarse, mapping = eng.contract_engine(clus)
    with pytest.raises(RuntimeError):
        eng.project_from(coarse)
    coarse.cluster(8, seed=1, download=False)  # a clustering is no partition
    with pytest.raises(RuntimeError):
        eng.project_from(coarse)
    cpart = coarse_labels(coarse.n, 4)
    coarse.set_labels(4, cpart)
    eng.project_from(coarse)
    assert (eng.get_labels() == cpart[mapping]).all()


def test_refuse_rebalance_after_balance():
    c, eng = small()
    _, part, _ = eng.balance(c.k, c.caps, c.part0)
    with pytest.raises(RuntimeError):
        eng.rebalance(c.k, c.caps, None)
    cut, part2, st = eng.rebalance(c.k, c.caps, part)
    assert cut == c.g.edge_cut(part2)


# ------------------------------------------------------------ 6. pipelines
def pipeline_graph(name):
    if name == "rmat14":
        return ka.Graph.rmat(14, 8, seed=7), 16
    return ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis")), 4


def same_result(a, b):
    assert a[0] == b[0]
    assert (a[1] == b[1]).all()
    assert list(a[2]) == list(b[2])


@pytest.mark.parametrize("fm", [None, False])
@pytest.mark.parametrize("jet", [False, dict(balancer=1)], ids=["lp", "jet"])
@pytest.mark.parametrize("name", ["rmat14", "rgg2d"])
def test_partition_resident_equals_host(name, jet, fm):
    g, k = pipeline_graph(name)
    same_result(partition(g, k, jet=jet, fm=fm, resident=True),
                partition(g, k, jet=jet, fm=fm))


@pytest.mark.parametrize("fm", [None, False])
@pytest.mark.parametrize("jet", [False, dict(balancer=1)], ids=["lp", "jet"])
@pytest.mark.parametrize("name", ["rmat14", "rgg2d"])
def test_partition_deep_resident_equals_host(name, jet, fm):
    g, k = pipeline_graph(name)
    same_result(partition_deep(g, k, jet=jet, fm=fm, resident=True),
                partition_deep(g, k, jet=jet, fm=fm))


@pytest.mark.parametrize("fm", [None, False])
@pytest.mark.parametrize("jet", [False, dict(balancer=1)], ids=["lp", "jet"])
@pytest.mark.parametrize("name", ["rmat14", "rgg2d"])
def test_partition_deep_gpu_split_resident_equals_host(name, jet, fm):
    g, k = pipeline_graph(name)
    kw = dict(jet=jet, fm=fm, gpu_split=True, gpu_split_min_n=256)
    same_result(partition_deep(g, k, resident=True, **kw), partition_deep(g, k, **kw))


# -------------------------------------------------------------- 7. traffic
def test_label_traffic():
    """Resident: one upload on the coarsest level and one download at the end,
    and nothing else of size n (no xadj / vwgt for the isolated scan either).
    Host: per level the clustering down and up, the mapping down, and two
    refiners up and down."""
    g = ka.Graph.rmat(14, 8, seed=7)
    kw = dict(fm=False, jet=dict(balancer=1))
    t0 = ka.label_traffic_bytes()
    cut_r, part_r, sizes = partition(g, 16, resident=True, **kw)
    t1 = ka.label_traffic_bytes()
    cut_h, part_h, sizes_h = partition(g, 16, resident=False, **kw)
    t2 = ka.label_traffic_bytes()
    assert len(sizes) > 2 and list(sizes) == list(sizes_h)
    assert t1 - t0 == 4 * (sizes[0] + sizes[-1])
    assert t2 - t1 >= 28 * sum(sizes[:-1])
    assert cut_r == cut_h and (part_r == part_h).all()
