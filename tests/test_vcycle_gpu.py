"""V-cycles on the GPU: the device pieces (restriction, resident communities,
labels_from_communities, resident_cut), one cycle against the CPU mirror
(vcycle_mirror.py) bit for bit, and the drivers' `vcycles` option in Python, C
and the shim. Nothing here is larger than R-MAT scale 14; inputs and mirror
results are computed once and shared."""

import ctypes
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
from helpers import oracle_cluster_comm
from kaminpar_amd import _lib, _u32p
from kaminpar_amd.partition import (level_cluster_weight, partition,
                                    partition_deep, vcycle)
from vcycle_mirror import mirror_vcycle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

# three iterations per level: the LP balancer's sweeps are what makes a Jet
# call slow at this size, and five cycles per case go through them
JET_LP = dict(balancer=0, balance_iters=2, max_iterations=3)
JET_LP_DEFAULT = dict(balancer=0, balance_iters=2)  # the default iteration rule
JET_SEL = dict(balancer=1)

_GRAPHS = {}
_INPUT = {}
_MIRROR = {}
_STEPWISE = {}


def graph(name):
    """(graph, k) as in test_cpipeline_gpu.py: a mesh, a heavy-tailed graph and
    one with vertex and edge weights."""
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


def input_partition(name):
    """The basic pipeline's result (LP only, no FM): what the cycles improve."""
    if name not in _INPUT:
        g, k = graph(name)
        cut, part, _ = partition(g, k, seed=1, fm=False)
        part.setflags(write=False)
        _INPUT[name] = (cut, part)
    return _INPUT[name]


def mirror(oracle, name, jet, fm):
    key = (name, json.dumps(jet, sort_keys=True), fm)
    if key not in _MIRROR:
        g, k = graph(name)
        res = mirror_vcycle(oracle, g, k, input_partition(name)[1], seed=1,
                            jet=jet, fm=fm)
        res[1].setflags(write=False)
        _MIRROR[key] = res
    return _MIRROR[key]


def caps(g, k):
    return np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)


RING, ISOLATED = 120, 389


def with_isolated():
    """A ring, then isolated vertices with consecutive ids. They are the
    majority, so LP shrinks the graph by less than half and the clusterer goes
    on to its isolated-vertex chain."""
    ring = RING
    n = ring + ISOLATED
    xadj = np.zeros(n + 1, dtype=np.uint32)
    xadj[1:ring + 1] = 2 * np.arange(1, ring + 1)
    xadj[ring + 1:] = 2 * ring
    u = np.arange(ring)
    adjncy = np.stack([(u - 1) % ring, (u + 1) % ring], axis=1).reshape(-1)
    return ka.Graph.from_csr(xadj, adjncy.astype(np.uint32))


def clustered(g, part, k, seed=1, resident=False):
    """An engine of g clustered under `part` as communities, its contraction
    and the mapping: (engine, coarse engine, mapping, clustering)."""
    eng = ka.LpEngine(g)
    mcw = level_cluster_weight(g.total_node_weight, g.n, k, 0.03)
    if resident:
        eng.set_labels(k, part)
        eng.set_communities_resident()
    else:
        eng.set_communities(part)
    _, clus, _ = eng.cluster(mcw, seed=seed, iters=5)
    coarse, mapping = eng.contract_engine(clus)
    return eng, coarse, mapping, clus


# ------------------------------------------------------------- 1. restrict
def _restrict_case(g, k):
    part = ka.random_partition(g.n, k, seed=3)
    eng, coarse, mapping, _ = clustered(g, part, k)
    want = np.zeros(coarse.n, dtype=np.uint32)
    want[mapping] = part
    assert np.array_equal(want[mapping], part)  # the clustering respects it
    eng.restrict_to(coarse)
    assert np.array_equal(coarse.get_labels(), want)
    # the restricted partition is a resident partition like any other: cut and
    # feasibility without a download, and a resident refine equals the host
    # form of a fresh engine on the same labels
    mbw = caps(g, k)
    hg = coarse.download_graph()
    cut0, feas0 = coarse.resident_cut(k, mbw)
    vw = hg.vwgt
    bw = np.bincount(want, weights=vw, minlength=k)
    assert cut0 == hg.edge_cut(want) and feas0 == bool((bw <= mbw).all())
    cut, none, _ = coarse.refine(k, mbw, None, seed=1, iters=3)
    assert none is None
    fcut, fpart, _ = ka.LpEngine(hg).refine(k, mbw, want, seed=1, iters=3)
    assert cut == fcut and np.array_equal(coarse.get_labels(), fpart)


@pytest.mark.parametrize("k", [2, 16, 256, 257, 2048, 4096])
def test_restrict_equals_numpy(k):
    _restrict_case(ka.Graph.rmat(12, 8, seed=7), k)


@pytest.mark.parametrize("which", ["odd-n", "isolated"])
def test_restrict_on_awkward_graphs(which):
    g = rc.odd_n_case().g if which == "odd-n" else with_isolated()
    assert g.n % 64 != 0
    _restrict_case(g, 8)


# ------------------------------------------------------------ 2. refusals
def test_refusals_leave_the_engines_usable(capfd):
    g, k = ka.Graph.rmat(12, 8, seed=7), 16
    part = ka.random_partition(g.n, k, seed=3)
    mbw = caps(g, k)
    eng, coarse, mapping, clus = clustered(g, part, k)
    want = np.zeros(coarse.n, dtype=np.uint32)
    want[mapping] = part

    # no communities
    eng.set_communities(None)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        eng.restrict_to(coarse)
    assert "no communities" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        eng.labels_from_communities()

    # a coarse engine of another parent
    other = ka.LpEngine(g)
    other.set_communities(part)
    with pytest.raises(RuntimeError):
        other.restrict_to(coarse)
    assert "not contracted from" in capfd.readouterr().err

    # communities the clustering does not respect: count reported, nothing held
    wrong = (clus % k).astype(np.uint32)  # constant on clusters ...
    wrong[::2] = (wrong[::2] + 1) % k     # ... then broken on every other vertex
    probe = np.zeros(coarse.n, dtype=np.uint32)
    probe[mapping] = wrong
    bad = int((probe[mapping] != wrong).sum())
    assert bad > 0
    eng.set_communities(wrong)
    with pytest.raises(RuntimeError):
        eng.restrict_to(coarse)
    err = capfd.readouterr().err
    assert "fine vertices share a coarse vertex" in err
    # the count depends on which writer won a slot; it is positive and at most
    # the vertices of clusters with mixed values
    reported = int(err.split("restrict: ")[1].split()[0])
    mixed = np.zeros(coarse.n, dtype=bool)
    mixed[mapping[probe[mapping] != wrong]] = True
    assert 0 < reported <= int(mixed[mapping].sum())
    with pytest.raises(RuntimeError):
        coarse.get_labels()  # holds nothing
    with pytest.raises(RuntimeError):
        coarse.refine(k, mbw, None)

    # set_communities_resident needs a partition: not nothing, not a clustering
    fresh = ka.LpEngine(g)
    with pytest.raises(RuntimeError):
        fresh.set_communities_resident()
    with pytest.raises(RuntimeError):
        eng.set_communities_resident()  # holds the clustering
    assert "no resident partition" in capfd.readouterr().err

    # everything still works
    eng.set_communities(part)
    eng.restrict_to(coarse)
    assert np.array_equal(coarse.get_labels(), want)
    cut, out, _ = fresh.refine(k, mbw, part, seed=1, iters=2)
    assert cut == g.edge_cut(out)


# ------------------------------------ 3. resident against host communities
@pytest.mark.parametrize("which", ["rmat12", "isolated"])
def test_resident_communities_equal_host_communities(oracle, which):
    if which == "rmat12":
        g, k = ka.Graph.rmat(12, 8, seed=7), 16
        part = ka.random_partition(g.n, k, seed=3)
    else:
        g, k = with_isolated(), 4
        part = ka.random_partition(g.n, k, seed=3)
        # consecutive isolated vertices in different blocks, and runs in one
        pattern = np.array([0, 1, 1, 2, 3, 3, 3, 0, 1], dtype=np.uint32)
        part[RING:] = np.resize(pattern, ISOLATED)
    mcw = max(4, level_cluster_weight(g.total_node_weight, g.n, k, 0.03))

    host = ka.LpEngine(g)
    host.set_communities(part)
    nc_h, clus_h, _ = host.cluster(mcw, seed=2, iters=5)

    res = ka.LpEngine(g)
    res.set_labels(k, part)
    before = ka.label_traffic_bytes()
    res.set_communities_resident()
    assert ka.label_traffic_bytes() == before
    assert np.array_equal(res.get_labels(), part)  # the labels stay
    nc_r, clus_r, _ = res.cluster(mcw, seed=2, iters=5)
    assert nc_r == nc_h and np.array_equal(clus_r, clus_h)

    nc_o, clus_o, _ = oracle_cluster_comm(oracle, g, mcw, part, seed=2, iters=5)
    assert nc_o == nc_h and np.array_equal(clus_o, clus_h)
    assert np.array_equal(part[clus_h], part)  # no cluster spans two blocks
    if which == "isolated":
        # the chain of the isolated vertices (unit weights, mcw >= 2): a
        # vertex pairs with the pending one iff they share a block
        pending, pairs = None, []
        for u in range(RING, g.n):
            if pending is not None and part[pending] == part[u]:
                pairs.append((pending, u))
                pending = None
            else:
                pending = u
        assert len(pairs) > ISOLATED // 9
        assert all(clus_h[a] == clus_h[b] for a, b in pairs)
        assert len(np.unique(clus_h[RING:])) == ISOLATED - len(pairs)

    # the partition comes back after the clustering overwrote it
    res.labels_from_communities()
    assert np.array_equal(res.get_labels(), part)
    mbw = caps(g, k)
    bw = np.bincount(part, minlength=k)
    assert res.resident_cut(k, mbw) == (g.edge_cut(part), bool((bw <= mbw).all()))
    # the cut alone needs no caps; feasibility without caps is refused
    assert _lib.kmp_lp_resident_cut(res._h, k, None, None) == g.edge_cut(part)
    assert _lib.kmp_lp_resident_cut(res._h, k, None, ctypes.byref(ctypes.c_int32())) == -1
    cut, _, _ = res.refine(k, mbw, None, seed=1, iters=2)
    fcut, fpart, _ = ka.LpEngine(g).refine(k, mbw, part, seed=1, iters=2)
    assert cut == fcut and np.array_equal(res.get_labels(), fpart)


# --------------------------------------------- 4. a cycle against the mirror
# every refiner with FM off and on, on every graph; the two small graphs run
# Jet with LP sweeps at its default iteration rule, rmat14 with the cap above
_MATRIX = [("rmat14_s42_k16", jet, fm)
           for jet in (False, JET_LP, JET_SEL) for fm in (False, True)]
_MATRIX += [(name, jet, fm) for name in ("walshaw_k16", "wrgg_k4")
            for jet in (False, JET_LP_DEFAULT, JET_SEL) for fm in (False, True)]


def _jet_id(jet):
    if not jet:
        return "lp"
    return f"jet-b{jet['balancer']}" + ("" if "max_iterations" in jet or jet["balancer"] else "d")


@pytest.mark.parametrize(
    "name,jet,fm", _MATRIX,
    ids=[f"{n.split('_')[0]}-{_jet_id(j)}-fm{int(f)}" for n, j, f in _MATRIX])
def test_cycle_equals_the_mirror(oracle, name, jet, fm):
    g, k = graph(name)
    cut_in, part_in = input_partition(name)
    m_cut, m_part, m_sizes, m_acc = mirror(oracle, name, jet, fm)
    print(name, _jet_id(jet), fm, "cut", cut_in, "->", m_cut, m_sizes, m_acc)
    assert m_cut <= cut_in
    eng = ka.LpEngine(g)
    for resident in (False, True):
        before = ka.label_traffic_bytes()
        cut, part, sizes, acc = vcycle(g, k, part_in, seed=1, jet=jet, fm=fm,
                                       resident=resident, engine=eng)
        moved = ka.label_traffic_bytes() - before
        assert (cut, sizes, acc) == (m_cut, m_sizes, m_acc)
        assert np.array_equal(part, m_part) and cut == g.edge_cut(part)
        if resident and not fm:
            assert moved == 8 * g.n  # one set_labels, one get_labels
    # the input resident on the engine, the result left there
    eng.set_labels(k, part_in)
    before = ka.label_traffic_bytes()
    cut, none, sizes, acc = vcycle(g, k, None, seed=1, jet=jet, fm=fm,
                                   resident=True, engine=eng, download=False)
    if not fm:
        assert ka.label_traffic_bytes() == before
    assert none is None and (cut, sizes, acc) == (m_cut, m_sizes, m_acc)
    assert np.array_equal(eng.get_labels(), m_part)
    assert eng.resident_cut(k, caps(g, k)) == (m_cut, True)
    # the C twin
    for resident in (False, True):
        ncut, npart, st = g.vcycle_native(k, part_in, seed=1, jet=jet, fm=fm,
                                          resident=resident, engine=eng)
        assert ncut == m_cut and np.array_equal(npart, m_part)
        assert st.levels == m_sizes and st.cycle_cuts == [m_cut]
        assert (st.vcycles_run, st.vcycles_accepted) == (1, int(m_acc))
        if resident and not fm:
            assert st.label_traffic_bytes == 8 * g.n


def test_cycle_without_refiners_returns_its_input():
    g, k = graph("rmat14_s42_k16")
    cut_in, part_in = input_partition("rmat14_s42_k16")
    for resident in (False, True):
        cut, part, sizes, acc = vcycle(g, k, part_in, seed=1, iters=0, jet=False,
                                       fm=False, resident=resident)
        assert acc and cut == cut_in and np.array_equal(part, part_in)
        assert sizes[0] == g.n


def test_cycle_refuses_bad_input():
    g, k = graph("wrgg_k4")
    _, part_in = input_partition("wrgg_k4")
    with pytest.raises(ValueError):
        vcycle(g, k, None)  # a resident input needs resident=True
    with pytest.raises(ValueError):
        vcycle(g, k, None, resident=True)  # ... and the engine that holds it
    with pytest.raises(ValueError):
        vcycle(g, k, part_in[:-1])
    with pytest.raises(ValueError):
        vcycle(g, k, part_in + 1)  # a label equal to k
    with pytest.raises(RuntimeError):
        vcycle(g, k, None, resident=True, engine=ka.LpEngine(g))  # holds nothing
    # k above Jet's limit is refused only with Jet
    g14, _ = graph("rmat14_s42_k16")
    big = ka.random_partition(g14.n, 4096, seed=1)
    with pytest.raises(RuntimeError):
        vcycle(g14, 4096, big, jet=True, stop_n=16384)
    cut, part, _, acc = vcycle(g14, 4096, big, resident=True, fm=False)
    assert acc and cut == g14.edge_cut(part) <= g14.edge_cut(big)


# --------------------------------------------------------------- 5. drivers
@pytest.mark.parametrize("deep,vcycles", [(False, 2), (True, 1)],
                         ids=["basic-2", "deep-1"])
@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_drivers_run_cycles_on_their_result(deep, vcycles, resident):
    name = "rmat14_s42_k16"
    g, k = graph(name)
    drv = partition_deep if deep else partition
    kw = dict(seed=1, jet=JET_SEL, fm=False)
    if deep not in _STEPWISE:  # the driver, then the cycles one by one
        cut, part, levels = drv(g, k, **kw)
        cuts = []
        for c in range(vcycles):
            cut, part, _, _ = vcycle(g, k, part, seed=1 + c, jet=JET_SEL, fm=False)
            cuts.append(cut)
        part.setflags(write=False)
        _STEPWISE[deep] = (cut, part, levels, cuts)
    cut, part, levels, cuts = _STEPWISE[deep]
    got = drv(g, k, vcycles=vcycles, resident=resident, **kw)
    assert got[0] == cut and np.array_equal(got[1], part) and got[2] == levels
    nat = g.partition_deep_native if deep else g.partition_native
    ncut, npart, st = nat(k, vcycles=vcycles, resident=resident,
                          return_stats=True, **kw)
    assert ncut == cut and np.array_equal(npart, part) and st.levels == levels
    assert st.vcycles_run == vcycles and st.cycle_cuts == cuts
    assert 0 <= st.vcycles_accepted <= vcycles and st.vcycle_ns > 0
    if not resident:  # without the option nothing of it shows
        _, _, st0 = nat(k, return_stats=True, **kw)
        assert (st0.vcycles_run, st0.vcycles_accepted, st0.vcycle_ns) == (0, 0, 0)


def test_shim_setter_reaches_the_driver():
    name = "walshaw_k16"
    g, k = graph(name)
    xadj = np.ascontiguousarray(g.xadj, dtype=np.uint32)
    adjncy = np.ascontiguousarray(g.adjncy, dtype=np.uint32)
    want_cut, want_part = g.partition_deep_native(k, seed=1, vcycles=1)
    plain_cut, plain_part = g.partition_deep_native(k, seed=1)
    shm = _lib.kaminpar_amd_create(1)
    try:
        _lib.kaminpar_amd_reseed(shm, 1)
        _lib.kaminpar_amd_copy_graph(shm, g.n, _u32p(xadj), _u32p(adjncy), None, None)
        _lib.kaminpar_amd_set_k(shm, k)
        _lib.kaminpar_amd_set_uniform_max_block_weights(shm, 0.03)
        part = np.zeros(g.n, dtype=np.uint32)
        _lib.kaminpar_amd_set_vcycles(shm, 1)
        assert _lib.kaminpar_amd_compute_partition(shm, _u32p(part)) == want_cut
        assert np.array_equal(part, want_part)
        _lib.kaminpar_amd_set_vcycles(shm, 0)
        assert _lib.kaminpar_amd_compute_partition(shm, _u32p(part)) == plain_cut
        assert np.array_equal(part, plain_part)
        _lib.kaminpar_amd_set_vcycles(shm, -1)
        assert _lib.kaminpar_amd_compute_partition(shm, _u32p(part)) == -1
    finally:
        _lib.kaminpar_amd_free(shm)


# -------------------------------------------------------------- 6. no leaks
def test_a_cycle_leaves_the_engine_as_new():
    name = "rmat14_s42_k16"
    g, k = graph(name)
    _, part_in = input_partition(name)
    mbw = caps(g, k)
    mcw = level_cluster_weight(g.total_node_weight, g.n, k, 0.03)
    used = ka.LpEngine(g)
    first = vcycle(g, k, part_in, seed=1, jet=JET_SEL, fm=False, resident=True,
                   engine=used)
    fresh = ka.LpEngine(g)
    nc_u, clus_u, _ = used.cluster(mcw, seed=1, iters=5)
    nc_f, clus_f, _ = fresh.cluster(mcw, seed=1, iters=5)
    assert nc_u == nc_f and np.array_equal(clus_u, clus_f)  # no communities left
    cut_u, out_u, _ = used.refine(k, mbw, part_in, seed=1, iters=5)
    cut_f, out_f, _ = fresh.refine(k, mbw, part_in, seed=1, iters=5)
    assert cut_u == cut_f and np.array_equal(out_u, out_f)
    second = vcycle(g, k, part_in, seed=1, jet=JET_SEL, fm=False, resident=True,
                    engine=used)
    third = vcycle(g, k, part_in, seed=1, jet=JET_SEL, fm=False, resident=True)
    for other in (second, third):
        assert other[0] == first[0] and np.array_equal(other[1], first[1])
        assert other[2:] == first[2:]
