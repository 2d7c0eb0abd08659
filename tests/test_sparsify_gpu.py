"""Threshold edge sparsification of coarse graphs on the device
(kmp_contract_engine_sparsified, LpEngine.contract_engine(sparsify=...), the
`sparsify` option of the Python and C drivers and of the shim). Every
comparison is bit-exact: the pass against the numpy twin
(tests/sparsify_twin.py) in xadj, adjncy, adjwgt and the stats, the engines
made from it against the CPU oracle on the twin's graph, the drivers against
the CPU mirror (tests/sparsify_mirror.py) and against each other."""

import ctypes
import functools
import json
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
import sparsify_mirror as sm
from helpers import oracle_cluster, oracle_refine
from kaminpar_amd.partition import level_cluster_weight, partition, partition_deep
from sparsify_twin import fmix64, sparsify
from test_largek_gpu import _weighted_graph

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HALF = dict(density_target_factor=0.5, edge_target_factor=0.5, laziness_factor=1)
# keeps a tenth: on weights 1..9 only part of the nines, so rows run empty
TENTH = dict(density_target_factor=0.1, edge_target_factor=0.1, laziness_factor=1)
STAT_FIELDS = ("applied", "m_before", "m_after", "target", "threshold", "larger",
               "equal", "include")


def arrays(g):
    """(xadj, adjncy, adjwgt, vwgt) of a host graph as owned arrays."""
    aw, vw = g.adjwgt, g.vwgt
    return (np.asarray(g.xadj).copy(), np.asarray(g.adjncy).copy(),
            np.ones(g.m, np.int32) if aw is None else np.asarray(aw).copy(),
            np.ones(g.n, np.int32) if vw is None else np.asarray(vw).copy())


def same_as_twin(eng, want, vwgt):
    """A sparsified engine against the twin's (xadj, adjncy, adjwgt, stats)."""
    xadj, adjncy, adjwgt, stats = want
    st = eng.sparsify_stats
    for name in STAT_FIELDS:
        assert int(getattr(st, name)) == int(stats[name]), name
    assert eng.m == stats["m_after"] == len(adjncy)
    got = arrays(eng.download_graph())
    assert np.array_equal(got[0], xadj)
    assert np.array_equal(got[1], adjncy)
    assert np.array_equal(got[2], adjwgt)
    assert np.array_equal(got[3], vwgt)


def through_identity(g, params, seed):
    """Sparsifies g itself: under the identity clustering the contraction
    returns g (rows sorted), and old_* = c_*. Returns (fine engine, sparsified
    engine, twin result, vwgt)."""
    eng = ka.LpEngine(g)
    clus = np.arange(g.n, dtype=np.uint32)
    plain, _ = eng.contract_engine(clus)
    xadj, adjncy, adjwgt, vwgt = arrays(plain.download_graph())
    assert len(xadj) == g.n + 1 and len(adjncy) == g.m
    want = sparsify(xadj, adjncy, adjwgt, g.n, g.m, params, seed)
    got, mapping = eng.contract_engine(clus, sparsify=params, seed=seed)
    assert np.array_equal(mapping, clus)
    same_as_twin(got, want, vwgt)
    return eng, got, want, vwgt


def pair_hash(xadj, adjncy):
    """A symmetric 64-bit hash per arc."""
    src = np.repeat(np.arange(len(xadj) - 1, dtype=np.uint64),
                    np.diff(np.asarray(xadj, dtype=np.int64)))
    dst = np.asarray(adjncy, dtype=np.uint64)
    return fmix64((np.minimum(src, dst) << np.uint64(32)) | np.maximum(src, dst))


def reweighted(kind):
    """The topology of test_largek_gpu._weighted_graph under other weights."""
    g, vwgt, adjwgt = _weighted_graph()
    xadj, adjncy = np.asarray(g.xadj).copy(), np.asarray(g.adjncy).copy()
    h = pair_hash(xadj, adjncy)
    if kind == "small":      # 1..9: massive ties at T
        w = adjwgt
    elif kind == "equal":    # T = 7, larger = 0: the dice decide everything
        w = np.full(g.m, 7, np.int32)
    elif kind == "wide":     # every radix digit matters
        w = (1 + h % np.uint64(2**31 - 1)).astype(np.int32)
    elif kind == "topbyte":  # the last three passes see one digit
        w = ((1 + h % np.uint64(127)) << np.uint64(24)).astype(np.int32)
    else:
        raise AssertionError(kind)
    assert w.min() >= 1
    return ka.Graph.from_csr(xadj, adjncy, vwgt, w)


# ------------------------------------------------ 1. the pass, any graph
@pytest.mark.parametrize("kind", ["small", "equal", "wide", "topbyte"])
def test_pass_weighted_graph(kind):
    """12 000 vertices, hubs of degree 2500 and 700: all three row tiers."""
    g = reweighted(kind)
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    assert deg.max() > 2048 and ((deg > 16) & (deg <= 2048)).any() and (deg <= 16).any()
    _, got, want, _ = through_identity(g, HALF, seed=11)
    st = want[3]
    assert st["applied"] == 1
    if kind in ("small", "equal", "topbyte"):
        assert 0 < st["include"] < st["equal"]
    if kind == "equal":
        assert st["threshold"] == 7 and st["larger"] == 0


def test_pass_empties_rows():
    g = reweighted("small")
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    _, _, want, _ = through_identity(g, TENTH, seed=11)
    st = want[3]
    assert st["applied"] == 1 and st["threshold"] == 9 and 0 < st["include"] < st["equal"]
    assert (np.diff(want[0].astype(np.int64)) == 0).sum() > (deg == 0).sum()


def test_pass_tier_boundaries():
    """Rows of degree 16, 17, 2048, 2049 and 3000, weights 1..3."""
    g0 = rc.tier_graph()
    xadj, adjncy = np.asarray(g0.xadj).copy(), np.asarray(g0.adjncy).copy()
    w = (1 + pair_hash(xadj, adjncy) % np.uint64(3)).astype(np.int32)
    g = ka.Graph.from_csr(xadj, adjncy, None, w)
    _, _, want, _ = through_identity(g, HALF, seed=3)
    st = want[3]
    assert st["applied"] == 1 and 0 < st["include"] < st["equal"]


def test_pass_odd_n_and_empty_rows():
    """n = 1000 is no multiple of 64; 37 rows are empty before the pass."""
    g0 = ka.Graph.rgg2d(963, 8.0, seed=4)
    xadj = np.concatenate([np.asarray(g0.xadj, dtype=np.uint32),
                           np.full(37, g0.m, dtype=np.uint32)])
    g = ka.Graph.from_csr(xadj, np.asarray(g0.adjncy, dtype=np.uint32).copy())
    assert g.n == 1000
    _, _, want, _ = through_identity(g, HALF, seed=5)
    st = want[3]
    assert st["applied"] == 1 and 0 < st["include"] < st["equal"]


def test_flag_byte_form_gives_the_same_graph(monkeypatch):
    """KMP_SPARSIFY_FLAGS, the measurement switch: count stores a byte per arc
    and fill reads it instead of evaluating the rule again. All three tiers."""
    monkeypatch.setenv("KMP_SPARSIFY_FLAGS", "1")
    _, _, want, _ = through_identity(reweighted("small"), TENTH, seed=11)
    assert want[3]["applied"] == 1 and 0 < want[3]["include"] < want[3]["equal"]
    through_identity(reweighted("wide"), HALF, seed=11)


def zero_arc_engine(g):
    tiny = dict(HALF, edge_target_factor=1e-9)
    return through_identity(g, tiny, seed=1)


def test_pass_target_below_two():
    fine, got, want, _ = zero_arc_engine(reweighted("small"))
    assert want[3]["applied"] == 1 and want[3]["target"] < 2
    assert got.m == 0 and got.n == fine.n
    assert not np.asarray(got.download_graph().xadj).any()


# ------------------------------------------------- 2. the contraction path
@functools.lru_cache(maxsize=None)
def rmat16():
    return ka.Graph.rmat(16, 8, seed=42)


def contract_both(params, seed=9):
    """rmat16 clustered for k = 16, contracted through the host and the
    resident form. Returns (fine, coarse, mapping) of either."""
    g = rmat16()
    mcw = level_cluster_weight(g.total_node_weight, g.n, 16, 0.03)
    host = ka.LpEngine(g)
    _, clus, _ = host.cluster(mcw, seed=1)
    hc, hmap = host.contract_engine(clus, sparsify=params, seed=seed)
    res = ka.LpEngine(g)
    res.cluster(mcw, seed=1, download=False)
    rcoarse, rmap = res.contract_engine(None, download_mapping=False, sparsify=params,
                                        seed=seed)
    assert rmap is None
    return (host, hc, hmap), (res, rcoarse, None), clus


def same_engine_graph(a, b):
    ga, gb = arrays(a.download_graph()), arrays(b.download_graph())
    assert a.n == b.n and a.m == b.m
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)


def test_contraction_defaults_do_not_trigger():
    (host, hc, hmap), (_, rcoarse, _), clus = contract_both(True)
    plain, pmap = host.contract_engine(clus)
    assert hc.sparsify_stats.applied == 0 and rcoarse.sparsify_stats.applied == 0
    assert hc.sparsify_stats.m_after == hc.sparsify_stats.m_before == plain.m
    assert np.array_equal(hmap, pmap)
    same_engine_graph(hc, plain)
    same_engine_graph(rcoarse, plain)


def test_contraction_laziness_two_equals_twin():
    params = dict(laziness_factor=2)
    (host, hc, hmap), (_, rcoarse, _), clus = contract_both(params)
    plain, pmap = host.contract_engine(clus)
    assert np.array_equal(hmap, pmap)
    xadj, adjncy, adjwgt, vwgt = arrays(plain.download_graph())
    g = rmat16()
    want = sparsify(xadj, adjncy, adjwgt, g.n, g.m, params, 9)
    assert want[3]["applied"] == 1 and want[3]["m_after"] < plain.m
    same_as_twin(hc, want, vwgt)
    same_as_twin(rcoarse, want, vwgt)


# ------------------------------------------------------- 3. derived state
def twin_graph(want, vwgt):
    return ka.Graph.from_csr(want[0], want[1], vwgt, want[2])


def check_derived(oracle, fine, coarse, mapping, want, vwgt, k=16):
    """cluster, refine and the projection of a sparsified engine against the
    oracle on the twin's graph."""
    tg = twin_graph(want, vwgt)
    mcw = max(1, int(vwgt.sum()) // 64)
    nc, clus, _ = coarse.cluster(mcw, seed=3)
    onc, oclus, _ = oracle_cluster(oracle, tg, mcw, seed=3, vwgt=vwgt, adjwgt=want[2])
    assert nc == onc and np.array_equal(clus, oclus)
    caps = np.full(k, tg.max_block_weight(k, 0.03), dtype=np.int64)
    part0 = ka.random_partition(coarse.n, k, seed=4)
    cut, part, _ = coarse.refine(k, caps, part0, seed=2)
    ocut, opart, _ = oracle_refine(oracle, tg, k, caps, part0, seed=2, vwgt=vwgt,
                                   adjwgt=want[2])
    assert cut == ocut and np.array_equal(part, opart)
    fine.project_from(coarse)
    assert np.array_equal(fine.get_labels(), part[mapping])


def test_derived_state_with_new_isolated_vertices(oracle):
    g = reweighted("small")
    fine, got, want, vwgt = through_identity(g, TENTH, seed=11)
    before = np.diff(np.asarray(g.xadj, dtype=np.int64)) == 0
    after = np.diff(want[0].astype(np.int64)) == 0
    assert (after & ~before).sum() > 0
    check_derived(oracle, fine, got, np.arange(g.n), want, vwgt)


def test_derived_state_after_contraction(oracle):
    params = dict(laziness_factor=2)
    (host, hc, hmap), _, clus = contract_both(params)
    plain, _ = host.contract_engine(clus)
    xadj, adjncy, adjwgt, vwgt = arrays(plain.download_graph())
    g = rmat16()
    want = sparsify(xadj, adjncy, adjwgt, g.n, g.m, params, 9)
    assert ((np.diff(want[0].astype(np.int64)) == 0)
            & (np.diff(xadj.astype(np.int64)) > 0)).sum() > 0
    check_derived(oracle, host, hc, hmap, want, vwgt)


def test_zero_arc_engine_runs(oracle):
    g = reweighted("small")
    fine, got, want, vwgt = zero_arc_engine(g)
    check_derived(oracle, fine, got, np.arange(g.n), want, vwgt)
    again, mapping = got.contract_engine(np.arange(got.n, dtype=np.uint32), sparsify=HALF)
    assert again.n == got.n and again.m == 0 and again.sparsify_stats.applied == 0


# -------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("bad", [
    dict(density_target_factor=0), dict(edge_target_factor=-1),
    dict(laziness_factor=float("nan")), dict(laziness_factor=0.5),
    dict(edge_target_factor=float("inf"))])
def test_invalid_params_raise_and_engine_survives(bad):
    g = ka.Graph.rmat(10, 8, seed=7)
    eng = ka.LpEngine(g)
    clus = np.arange(g.n, dtype=np.uint32)
    with pytest.raises(RuntimeError):
        eng.contract_engine(clus, sparsify=bad)
    coarse, _ = eng.contract_engine(clus, sparsify=HALF, seed=2)
    assert coarse.sparsify_stats.applied == 1


# --------------------------------------------------------------- 5. drivers
LAZY1 = dict(laziness_factor=1)
DEEP_KW = dict(split_c=2000)  # the mid-split schedule: coarse levels take splits


@functools.lru_cache(maxsize=None)
def rmat(scale):
    return ka.Graph.rmat(scale, 8, seed=42)


_MIRROR = {}


def mirror(oracle, scale, deep):
    """The CPU mirror's result, computed once and left unchanged."""
    if (scale, deep) not in _MIRROR:
        run = sm.mirror_partition_deep if deep else sm.mirror_partition
        cut, part, levels, stats = run(oracle, rmat(scale), 16, LAZY1, seed=1,
                                       **(DEEP_KW if deep else {}))
        part.setflags(write=False)
        _MIRROR[scale, deep] = (cut, part, levels, stats)
    return _MIRROR[scale, deep]


def same_level_stats(got, want):
    assert got["level_arcs"] == want["level_arcs"]
    assert len(got["sparsify"]) == len(want["sparsify"])
    for a, b in zip(got["sparsify"], want["sparsify"]):
        for name in STAT_FIELDS:
            assert a[name] == b[name], name


def checksum(part):
    return int(np.bitwise_xor.reduce(
        np.asarray(part, np.uint64) * np.arange(1, len(part) + 1, dtype=np.uint64)))


@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
@pytest.mark.parametrize("scale", [14, 16])
def test_drivers_equal_the_mirror(oracle, scale, deep):
    g = rmat(scale)
    cut, part, levels, stats = mirror(oracle, scale, deep)
    assert sum(s["applied"] for s in stats["sparsify"]) >= 1
    drv = partition_deep if deep else partition
    kw = DEEP_KW if deep else {}
    for resident in (False, True):
        got_stats = {}
        got = drv(g, 16, seed=1, sparsify=LAZY1, resident=resident, stats=got_stats, **kw)
        assert got[0] == cut == g.edge_cut(got[1])
        assert np.array_equal(got[1], part) and got[2] == levels
        same_level_stats(got_stats, stats)
    with open(os.path.join(GOLDEN, "sparsify_expected.json")) as f:
        want = json.load(f)[f"rmat{scale}_s42_k16_lazy1"]["partition_deep" if deep else
                                                           "partition"]
    assert (cut, levels, stats["level_arcs"]) == (want["cut"], want["levels"],
                                                  want["level_arcs"])
    assert checksum(part) == want["part_checksum"]


@pytest.mark.parametrize("jet", [False, dict(balancer=1)], ids=["lp", "jet"])
@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
@pytest.mark.parametrize("scale", [14, 16])
def test_c_twins_equal_python(scale, deep, jet):
    g = rmat(scale)
    stats = {}
    if deep:
        cut, part, levels = partition_deep(g, 16, seed=1, sparsify=LAZY1, jet=jet,
                                           stats=stats, **DEEP_KW)
        ncut, npart, st = g.partition_deep_native(16, seed=1, sparsify=LAZY1, jet=jet,
                                                  return_stats=True, **DEEP_KW)
    else:
        cut, part, levels = partition(g, 16, seed=1, sparsify=LAZY1, jet=jet, stats=stats)
        ncut, npart, st = g.partition_native(16, seed=1, sparsify=LAZY1, jet=jet,
                                             return_stats=True)
    assert ncut == cut == g.edge_cut(npart) and np.array_equal(npart, part)
    assert st.levels == levels and st.arcs == stats["level_arcs"]
    applied = [s for s in stats["sparsify"] if s["applied"]]
    assert st.sparsified_levels == len(applied) >= 1
    assert st.sparsify_arcs_dropped == sum(s["m_before"] - s["m_after"] for s in applied)
    assert st.sparsify_ns > 0


@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
@pytest.mark.parametrize("scale", [14, 16])
def test_off_and_defaults_reproduce_the_goldens(scale, deep):
    name = "pipeline_deep_expected.json" if deep else "pipeline_expected.json"
    with open(os.path.join(GOLDEN, name)) as f:
        want = json.load(f)[f"rmat{scale}_s42_k16"]
    g = rmat(scale)
    drv = partition_deep if deep else partition
    nat = g.partition_deep_native if deep else g.partition_native
    for opt in (False, True):
        stats = {}
        cut, part, levels = drv(g, 16, seed=1, sparsify=opt, stats=stats)
        assert (cut, levels, checksum(part)) == (want["cut"], want["levels"],
                                                 want["part_checksum"])
        assert stats["sparsify"] == [None] * (len(levels) - 1) or not any(
            s["applied"] for s in stats["sparsify"])
        ncut, npart, st = nat(16, seed=1, sparsify=opt, return_stats=True)
        assert ncut == cut and np.array_equal(npart, part)
        assert st.arcs == stats["level_arcs"] and st.sparsified_levels == 0


def walshaw():
    with open(os.path.join(GOLDEN, "walshaw_data.json")) as f:
        d = json.load(f)
    return ka.Graph.from_csr(np.array(d["xadj"], np.uint32), np.array(d["adjncy"], np.uint32))


@pytest.mark.parametrize("name", ["rmat14", "walshaw"])
def test_shim_setter_reaches_the_driver(name):
    """The shim against kmp_partition_deep_ex. On rmat14 the default late-split
    schedule takes no split on a coarse level and the option leaves the result
    as it is; on the walshaw mesh it changes it, asserted below, so the setter
    is seen to reach the driver."""
    g, k = (rmat(14) if name == "rmat14" else walshaw()), 16
    xadj = np.ascontiguousarray(g.xadj, dtype=np.uint32)
    adjncy = np.ascontiguousarray(g.adjncy, dtype=np.uint32)
    want_cut, want_part = g.partition_deep_native(k, seed=1, sparsify=LAZY1)
    plain_cut, plain_part = g.partition_deep_native(k, seed=1)
    if name == "walshaw":
        assert not np.array_equal(want_part, plain_part)
    lib, u32p = ka._lib, ka._u32p
    shm = lib.kaminpar_amd_create(1)
    try:
        lib.kaminpar_amd_reseed(shm, 1)
        lib.kaminpar_amd_copy_graph(shm, g.n, u32p(xadj), u32p(adjncy), None, None)
        lib.kaminpar_amd_set_k(shm, k)
        lib.kaminpar_amd_set_uniform_max_block_weights(shm, 0.03)
        part = np.zeros(g.n, dtype=np.uint32)
        params = ka.sparsify_params(LAZY1)
        lib.kaminpar_amd_set_sparsification(shm, 1, ctypes.byref(params))
        assert lib.kaminpar_amd_compute_partition(shm, u32p(part)) == want_cut
        assert np.array_equal(part, want_part)
        lib.kaminpar_amd_set_sparsification(shm, 0, None)
        assert lib.kaminpar_amd_compute_partition(shm, u32p(part)) == plain_cut
        assert np.array_equal(part, plain_part)
        params.laziness_factor = 0.5
        lib.kaminpar_amd_set_sparsification(shm, 1, ctypes.byref(params))
        assert lib.kaminpar_amd_compute_partition(shm, u32p(part)) == -1
        lib.kaminpar_amd_set_sparsification(shm, 1, None)  # the defaults: valid
        assert lib.kaminpar_amd_compute_partition(shm, u32p(part)) >= 0
    finally:
        lib.kaminpar_amd_free(shm)


def test_driver_refuses_invalid_params():
    g = rmat(14)
    with pytest.raises(RuntimeError):
        partition(g, 16, sparsify=dict(laziness_factor=0.5))
    with pytest.raises(RuntimeError):
        g.partition_native(16, sparsify=dict(edge_target_factor=-1))
    assert partition(g, 16, seed=1)[0] > 0
