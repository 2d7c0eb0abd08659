"""The C pipeline drivers with options (kmp_partition_ex / kmp_partition_deep_ex,
Graph.partition_native / partition_deep_native with keywords) and the shim's
"jet" preset. The yardstick is the Python driver of the same configuration
(kaminpar_amd.partition.partition / partition_deep): partition, cut and level
sizes must be EQUAL, for Jet with either balancer, with and without the CPU FM,
with host and with resident labels. Nothing here is larger than R-MAT scale 14;
a Python reference is computed once per configuration and shared."""

import ctypes
import json
import os
import subprocess

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
from kaminpar_amd import _lib, _u32p
from kaminpar_amd.partition import level_cluster_weight, partition, partition_deep

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

JET_LP = dict(balancer=0, balance_iters=2)
JET_SEL = dict(balancer=1)

_GRAPHS = {}
_PY = {}


def graph(name):
    """(graph, k): walshaw takes the mesh arm and the eager coarsest split,
    rmat14 the heavy-tail arm and late splits, wrgg has vertex and edge
    weights."""
    if name not in _GRAPHS:
        if name == "walshaw_k16":
            d = json.load(open(os.path.join(GOLDEN, "walshaw_data.json")))
            g = ka.Graph.from_csr(np.array(d["xadj"], np.uint32),
                                  np.array(d["adjncy"], np.uint32))
            _GRAPHS[name] = (g, 16)
        elif name == "rmat14_s42_k16":
            _GRAPHS[name] = (ka.Graph.rmat(14, 8, 42), 16)
        else:
            _GRAPHS[name] = (rc.weighted_rgg()[0], 4)
    return _GRAPHS[name]


def py_driver(deep):
    return partition_deep if deep else partition


def native(g, deep):
    return g.partition_deep_native if deep else g.partition_native


def py_ref(deep, name, jet, fm):
    """(cut, part, levels) of the Python driver, once per configuration."""
    key = (deep, name, json.dumps(jet, sort_keys=True), fm)
    if key not in _PY:
        g, k = graph(name)
        cut, part, levels = py_driver(deep)(g, k, seed=1, jet=jet, fm=fm)
        part.setflags(write=False)
        _PY[key] = (cut, part, list(levels))
    return _PY[key]


def block_weights(g, k, part):
    vw = g.vwgt
    vw = np.ones(g.n, np.int64) if vw is None else vw.astype(np.int64)
    return np.bincount(part, weights=vw, minlength=k).astype(np.int64)


def ex_fn(deep):
    return _lib.kmp_partition_deep_ex if deep else _lib.kmp_partition_ex


def call_ex(g, k, deep, opts, seed=1, eps=0.03):
    """The _ex driver through ctypes alone: (rc, part, stats)."""
    part = np.zeros(g.n, dtype=np.uint32)
    stats = ka.PipelineStats()
    cut = ex_fn(deep)(g._h, k, eps, seed,
                      None if opts is None else ctypes.byref(opts), _u32p(part),
                      ctypes.byref(stats))
    return cut, part, stats


# ------------------------------------------------------------- 1. defaults
@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
@pytest.mark.parametrize("name", ["walshaw_k16", "rmat14_s42_k16", "wrgg_k4"])
def test_defaults_equal_the_old_entry_points(name, deep):
    g, k = graph(name)
    old = np.zeros(g.n, dtype=np.uint32)
    if deep:
        old_cut = _lib.kmp_partition_deep(g._h, k, 0.03, 1, 5, 0, 0, 0, 0, _u32p(old))
    else:
        old_cut = _lib.kmp_partition(g._h, k, 0.03, 1, 5, 0, 0, 0, _u32p(old))
    assert old_cut >= 0
    py_cut, py_part, py_levels = py_ref(deep, name, False, None)
    for opts in (None, _lib.kmp_pipeline_opts_default()):
        cut, part, stats = call_ex(g, k, deep, opts)
        assert cut == old_cut == py_cut
        assert np.array_equal(part, old) and np.array_equal(part, py_part)
        assert stats.levels == py_levels and stats.levels[0] == g.n
        assert stats.jet_iterations == 0 and stats.jet_moves == 0
        assert stats.total_ns > 0
    if name != "wrgg_k4":
        gold = "pipeline_deep_expected.json" if deep else "pipeline_expected.json"
        exp = json.load(open(os.path.join(GOLDEN, gold)))[name]
        assert exp["k"] == k and cut == exp["cut"]
    # the keyword-less Python wrappers still return a pair
    out = native(g, deep)(k)
    assert len(out) == 2 and out[0] == old_cut and np.array_equal(out[1], old)


# --------------------------------------------- 2. parity with the Python drivers
_MATRIX = [("rmat14_s42_k16", jet, fm)
           for jet in (JET_LP, JET_SEL) for fm in (False, True)]
_MATRIX += [(name, JET_SEL, False) for name in ("walshaw_k16", "wrgg_k4")]


@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
@pytest.mark.parametrize(
    "name,jet,fm", _MATRIX,
    ids=[f"{n.split('_')[0]}-b{j['balancer']}-fm{int(f)}" for n, j, f in _MATRIX])
def test_parity_with_the_python_driver(name, jet, fm, deep):
    g, k = graph(name)
    py_cut, py_part, py_levels = py_ref(deep, name, jet, fm)
    for resident in (False, True):
        cut, part, stats = native(g, deep)(
            k, seed=1, jet=jet, fm=fm, resident=resident, return_stats=True)
        assert np.array_equal(part, py_part), (resident, cut, py_cut)
        assert cut == py_cut == g.edge_cut(part)
        assert stats.levels == py_levels
        assert stats.jet_iterations > 0


# ------------------------------------------------------- 3. Jet actually ran
def test_jet_changes_the_result():
    name = "rmat14_s42_k16"
    g, k = graph(name)
    cut, part, stats = g.partition_native(k, jet=JET_SEL, fm=False, return_stats=True)
    lp_cut, lp_part = g.partition_native(k, jet=False, fm=False)
    assert stats.jet_iterations > 0 and stats.jet_moves > 0
    assert not np.array_equal(part, lp_part)
    assert cut != lp_cut
    assert block_weights(g, k, part).max() <= g.max_block_weight(k, 0.03)
    assert block_weights(g, k, lp_part).max() <= g.max_block_weight(k, 0.03)


# ------------------------------------------ 4. one parameter set per level kind
def py_partition_jet_levels(g, k, fine, coarse, seed=1, iters=5):
    """partition(jet=..., fm=False) written out with LpEngine calls, with one
    set of Jet overrides for level 0 and one for the levels above. Returns
    (cut, part, Jet iterations per level, finest first)."""
    mbw = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    engines, mappings = [ka.LpEngine(g)], []
    while engines[-1].n > max(512, 2 * k):
        mcw = level_cluster_weight(g.total_node_weight, engines[-1].n, k, 0.03)
        _, clus, _ = engines[-1].cluster(mcw, seed=seed + len(mappings), iters=iters)
        coarse_eng, mapping = engines[-1].contract_engine(clus)
        if coarse_eng.n > 0.95 * engines[-1].n:
            break
        engines.append(coarse_eng)
        mappings.append(mapping)
    part = engines[-1].download_graph().initial_partition_native(k, int(mbw[0]))
    its = {}
    for level in range(len(engines) - 1, -1, -1):
        _, part, _ = engines[level].refine(k, mbw, part, seed=seed, iters=iters)
        cut, part, jst = engines[level].jet(
            k, mbw, part, seed=seed, coarse_level=level,
            **(fine if level == 0 else coarse))
        its[level] = int(jst.iterations)
        if level > 0:
            part = part[mappings[level - 1]]
    return cut, part, [its[lv] for lv in range(len(engines))]


@pytest.mark.parametrize("name", ["walshaw_k16", "rmat14_s42_k16"])
def test_fine_and_coarse_parameters_are_separate(name):
    """max_iterations = 1 in jet_fine alone against the same in both sets. The
    run with the override on level 0 only equals the written-out Python
    reference, and the stats tell the two runs apart on both graphs. The
    partitions differ on the mesh, where Jet improves the coarse levels. On the
    R-MAT graph they do not: its coarse levels run Jet to the fruitless limit
    (12 iterations each, three times the moves of the one-iteration run)
    without ever beating the state LP handed them, so every coarse level
    returns its input either way -- there only the stats can differ."""
    g, k = graph(name)
    fine_only = ka.pipeline_opts(jet=JET_SEL, fm=False)
    fine_only.jet_fine.max_iterations = 1
    both = ka.pipeline_opts(jet=dict(JET_SEL, max_iterations=1), fm=False)
    cut_f, part_f, st_f = call_ex(g, k, False, fine_only)
    cut_b, part_b, st_b = call_ex(g, k, False, both)
    assert cut_f >= 0 and cut_b >= 0

    ref_cut, ref_part, ref_its = py_partition_jet_levels(
        g, k, dict(JET_SEL, max_iterations=1), JET_SEL)
    assert len(ref_its) >= 2 and ref_its[0] == 1 and min(ref_its[1:]) > 1
    assert cut_f == ref_cut and np.array_equal(part_f, ref_part)
    assert st_f.levels == st_b.levels and len(st_f.levels) == len(ref_its)
    assert st_f.jet_iterations == sum(ref_its)
    assert st_b.jet_iterations == len(ref_its)  # one iteration on every level
    assert st_f.jet_moves > st_b.jet_moves
    if name == "walshaw_k16":
        assert not np.array_equal(part_f, part_b)


# ------------------------------------------------------------ 5. resident
@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
def test_resident_moves_fewer_label_bytes(deep):
    name = "rmat14_s42_k16"
    g, k = graph(name)
    _, host_part, host = native(g, deep)(
        k, jet=JET_SEL, fm=False, resident=False, return_stats=True)
    _, res_part, res = native(g, deep)(
        k, jet=JET_SEL, fm=False, resident=True, return_stats=True)
    assert np.array_equal(host_part, res_part)
    assert 0 < res.label_traffic_bytes < host.label_traffic_bytes
    # the same calls as the Python driver makes: the same bytes
    for resident, stats in ((False, host), (True, res)):
        before = ka.label_traffic_bytes()
        py_driver(deep)(g, k, seed=1, jet=JET_SEL, fm=False, resident=resident)
        assert ka.label_traffic_bytes() - before == stats.label_traffic_bytes


# --------------------------------------------------------- 6. engine reuse
@pytest.mark.parametrize("deep", [False, True], ids=["basic", "deep"])
def test_engine_reuse(deep):
    name = "rmat14_s42_k16"
    g, k = graph(name)
    mbw = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    eng = ka.LpEngine(g)
    for resident in (False, True):
        cut0, part0 = native(g, deep)(k, jet=JET_SEL, fm=False, resident=resident)
        for _ in range(2):
            cut, part = native(g, deep)(k, jet=JET_SEL, fm=False,
                                        resident=resident, engine=eng)
            assert cut == cut0 and np.array_equal(part, part0)
    # still alive, and in no state that changes a later call
    assert _lib.kmp_lp_n(eng._h) == g.n
    start = ka.random_partition(g.n, k, seed=5)
    cut_a, part_a, _ = eng.refine(k, mbw, start, seed=3)
    cut_b, part_b, _ = ka.LpEngine(g).refine(k, mbw, start, seed=3)
    assert cut_a == cut_b and np.array_equal(part_a, part_b)


# ------------------------------------------------------------ 7. refusals
def test_refusals_leave_everything_usable():
    name = "rmat14_s42_k16"
    g, k = graph(name)
    other = ka.Graph.rmat(10, 8, 3)
    eng = ka.LpEngine(g)
    other_eng = ka.LpEngine(other)
    good_cut, good_part = g.partition_native(k, jet=JET_SEL, fm=False)

    def bad(mutate, k_=k):
        opts = _lib.kmp_pipeline_opts_default()
        opts.engine = eng._h
        mutate(opts)
        for deep in (False, True):
            cut, _, _ = call_ex(g, k_, deep, opts)
            assert cut == -1
        # the caller's engine and the process still work
        cut, part = g.partition_native(k, jet=JET_SEL, fm=False, engine=eng)
        assert cut == good_cut and np.array_equal(part, good_part)

    def set_(field, value):
        return lambda o: setattr(o, field, value)

    bad(set_("fm", 2))
    bad(set_("fm", -2))
    bad(set_("jet", 2))
    bad(set_("resident", -1))
    bad(set_("jet", 1), k_=4096)

    def no_stop(o):
        o.jet = 1
        o.jet_fine.max_iterations = 0
        o.jet_fine.max_fruitless = 0
    bad(no_stop)

    def coarse_rounds(o):
        o.jet = 1
        o.jet_coarse.num_rounds = 0
    bad(coarse_rounds)
    bad(set_("engine", other_eng._h))

    with pytest.raises(RuntimeError):
        g.partition_native(k, engine=other_eng)
    with pytest.raises(RuntimeError):
        g.partition_deep_native(4096, jet=True)
    for deep in (False, True):
        with pytest.raises(TypeError):
            native(g, deep)(k, jet=dict(balancr=1))


# ---------------------------------------------------------------- 8. shim
class Shim:
    def __init__(self, g, k, eps=0.03, seed=1):
        self.g = g
        self.xadj = np.ascontiguousarray(g.xadj, dtype=np.uint32)
        self.adjncy = np.ascontiguousarray(g.adjncy, dtype=np.uint32)
        self.h = _lib.kaminpar_amd_create(1)
        _lib.kaminpar_amd_reseed(self.h, seed)
        _lib.kaminpar_amd_copy_graph(self.h, g.n, _u32p(self.xadj),
                                     _u32p(self.adjncy), None, None)
        _lib.kaminpar_amd_set_k(self.h, k)
        _lib.kaminpar_amd_set_uniform_max_block_weights(self.h, eps)

    def preset(self, name):
        return _lib.kaminpar_amd_set_preset(self.h, name)

    def compute(self):
        part = np.zeros(self.g.n, dtype=np.uint32)
        return _lib.kaminpar_amd_compute_partition(self.h, _u32p(part)), part

    def __del__(self):
        _lib.kaminpar_amd_free(self.h)


def test_shim_preset():
    """On the mesh graph, because there the two presets give different
    partitions with the CPU FM on, which the shim cannot switch off
    (profiles/jet/pipeline_balancer_goldens.json: 1262 against 1255; on rmat14
    both end at 60021)."""
    name = "walshaw_k16"
    g, k = graph(name)
    plain_cut, plain_part = Shim(g, k).compute()
    assert plain_cut >= 0

    opts = _lib.kmp_pipeline_opts_default()
    opts.jet = 1
    opts.jet_fine.balancer = ka.JET_BALANCER_SELECT
    opts.jet_coarse.balancer = ka.JET_BALANCER_SELECT
    opts.fm = -1
    opts.resident = 1
    jet_cut, jet_part, _ = call_ex(g, k, True, opts)
    assert jet_cut >= 0 and not np.array_equal(jet_part, plain_part)

    shm = Shim(g, k)
    assert shm.preset(b"jet") == 0
    cut, part = shm.compute()
    assert cut == jet_cut and np.array_equal(part, jet_part)
    assert shm.preset(b"default") == 0
    cut, part = shm.compute()
    assert cut == plain_cut and np.array_equal(part, plain_part)
    # an unknown name changes nothing: still "default", then still "jet"
    assert shm.preset(b"nope") == -1 and shm.preset(None) == -1
    cut, part = shm.compute()
    assert cut == plain_cut and np.array_equal(part, plain_part)
    assert shm.preset(b"jet") == 0 and shm.preset(b"Jet") == -1
    cut, part = shm.compute()
    assert cut == jet_cut and np.array_equal(part, jet_part)
    # no silent fall-back above Jet's k limit
    _lib.kaminpar_amd_set_k(shm.h, 4096)
    cut, _ = shm.compute()
    assert cut == -1
    _lib.kaminpar_amd_set_k(shm.h, k)
    cut, part = shm.compute()
    assert cut == jet_cut and np.array_equal(part, jet_part)


# ------------------------------------------------------------ 9. C caller
def fnv1a64(part):
    h = 0xCBF29CE484222325
    for byte in np.ascontiguousarray(part, dtype="<u4").tobytes():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_caller(tmp_path):
    """tools/c_pipeline_check.c, compiled as C11 against libkaminpar_lp.so, run
    once as a child process: its three lines equal what the Python drivers
    compute."""
    src = os.path.join(REPO, "tools", "c_pipeline_check.c")
    lib_dir = os.path.join(REPO, "kaminpar_amd")
    exe = str(tmp_path / "c_pipeline_check")
    subprocess.run(
        ["gcc", "-std=c11", "-O1", "-Wall", "-Werror", src, "-o", exe,
         f"-L{lib_dir}", "-lkaminpar_lp", f"-Wl,-rpath,{lib_dir}"],
        check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr

    g, k = graph("rmat14_s42_k16")
    d_cut, d_part, _ = py_ref(True, "rmat14_s42_k16", False, None)
    j_cut, j_part, _ = partition_deep(g, k, seed=1, jet=JET_SEL, resident=True)
    want = [f"default {d_cut} {fnv1a64(d_part):016x}",
            f"jet {j_cut} {fnv1a64(j_part):016x}",
            f"preset {j_cut} {fnv1a64(j_part):016x}"]
    assert r.stdout.splitlines() == want
