"""GPU selection rebalancer (kmp_lp_rebalance / LpEngine.rebalance, and Jet's
balancer=1) against its numpy twin (tests/rebalance_twin.py): labels, cut,
passes, selected, moves and arcs must be BIT-IDENTICAL. Covers the three
degree tiers of the score kernels, the u8 and u16 label shadows, weighted
graphs, the fallback for isolated vertices, stalls, the Jet loop with this
rebalancer as its step 4, and the pipelines' jet=dict(balancer=1) switch.
test_rebalance_twin_cpu.py proves that the twin ends feasible on the same
inputs."""

import json
import os

import numpy as np
import pytest

# torch bundles its own HIP runtime; it must initialize BEFORE any engine in
# this process creates a context with the system runtime (same SONAME: the
# engine then binds torch's already-loaded runtime). Engine-first leaves
# torch.cuda unable to see the GPU.
import torch as _torch

if _torch.cuda.is_available():
    _torch.zeros(1, device="cuda:0")

import kaminpar_amd as ka
import jet_twin
import rebalance_cases as rc
import rebalance_twin as rt

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_against_twin(oracle, c, eng=None):
    """Runs both sides on a rebalance_cases.Case and compares bit-exactly."""
    eng = eng or ka.LpEngine(c.g)
    cut, part, st = eng.rebalance(c.k, c.caps, c.part0, max_passes=c.max_passes)
    tpart, tst = rt.rebalance(c.g, c.k, c.caps, c.part0, max_passes=c.max_passes,
                              vwgt=c.vwgt, adjwgt=c.adjwgt)
    print(f"rebalance gpu/twin passes {st.passes}/{tst['passes']} selected "
          f"{st.selected}/{tst['selected']} moves {st.moves}/{tst['moves']} arcs "
          f"{st.arcs_scanned}/{tst['arcs']} feasible {st.feasible}/{tst['feasible']}")
    assert (part == tpart).all(), f"{(part != tpart).sum()} labels differ"
    assert st.passes == tst["passes"]
    assert st.selected == tst["selected"]
    assert st.moves == tst["moves"]
    assert st.arcs_scanned == tst["arcs"]
    assert bool(st.feasible) == tst["feasible"] == c.feasible
    adjwgt32 = None if c.adjwgt is None else np.ascontiguousarray(c.adjwgt, dtype=np.int32)
    assert cut == st.edge_cut == jet_twin.edge_cut(oracle, c.g, tpart, adjwgt32)
    return cut, part, st


# ------------------------------------------------- 1. against the twin
@pytest.mark.parametrize("scale,k,start", rc.RMAT)
def test_rmat(oracle, scale, k, start):
    """k <= 256 gathers the u8 shadow, k = 512 the u16 one; R-MAT rows fill
    the subgroup and the wavefront tier."""
    _, _, st = check_against_twin(oracle, rc.rmat_case(scale, k, start))
    assert st.moves > 0


def test_degree_tiers(oracle):
    """Spokes of degree 16, 17, 2048, 2049 and 3000 inside the overloaded
    block: both sides of each tier boundary."""
    check_against_twin(oracle, rc.tiers_case())


@pytest.mark.parametrize("k", [4, 16])
def test_weighted(oracle, k):
    c = rc.weighted_case(k)
    cut, part, _ = check_against_twin(oracle, c)
    assert cut == c.g.edge_cut(part)
    assert (np.bincount(part, weights=c.vwgt, minlength=k) <= c.caps).all()


def test_n_not_a_multiple_of_64(oracle):
    check_against_twin(oracle, rc.odd_n_case())


def test_isolated_vertices_in_an_overloaded_block(oracle):
    _, part, _ = check_against_twin(oracle, rc.isolated_case())
    assert (part[-37:] != 0).any()  # the fallback moved isolated vertices


def test_multigraph_parallel_arcs(oracle):
    check_against_twin(oracle, rc.multigraph_case())


def test_caps_that_cannot_be_met_stall(oracle):
    c = rc.unmeetable_case()
    assert c.caps.sum() < c.g.total_node_weight
    _, part, st = check_against_twin(oracle, c)
    assert st.feasible == 0 and st.passes < c.max_passes
    # nothing was pushed over its cap on the way
    w0 = np.bincount(c.part0, minlength=c.k)
    w1 = np.bincount(part, minlength=c.k)
    assert (w1 <= np.maximum(w0, c.caps)).all()


def test_max_passes_cuts_off(oracle):
    _, _, st = check_against_twin(oracle, rc.one_pass_case())
    assert st.passes == 1 and st.feasible == 0 and st.moves > 0


# ------------------------------------------------- 2. invariants and state
def test_feasible_input_is_untouched():
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 16
    part0 = ka.random_partition(g.n, k, seed=5)
    caps = np.full(k, np.bincount(part0, minlength=k).max(), dtype=np.int64)
    cut, part, st = ka.LpEngine(g).rebalance(k, caps, part0)
    assert (part == part0).all()
    assert cut == g.edge_cut(part0) == st.edge_cut
    assert (st.passes, st.selected, st.moves, st.arcs_scanned, st.feasible) == (0, 0, 0, 0, 1)


def test_bad_arguments_are_rejected():
    g = ka.Graph.rmat(10, 8, seed=7)
    eng = ka.LpEngine(g)
    part0 = ka.random_partition(g.n, 4, seed=5)
    with pytest.raises(RuntimeError):
        eng.rebalance(4, rc.caps_of(g, 4), part0, max_passes=0)
    bad = part0.copy()
    bad[17] = 4  # a label that is not below k
    with pytest.raises(RuntimeError):
        eng.rebalance(4, rc.caps_of(g, 4), bad)
    with pytest.raises(RuntimeError):
        eng.rebalance(4096, rc.caps_of(g, 4096), ka.random_partition(g.n, 4096, seed=5))
    with pytest.raises(ValueError):
        eng.rebalance(4, rc.caps_of(g, 8), part0)
    for over in (dict(balancer=2), dict(balancer=-1), dict(balancer=1, balance_passes=0)):
        with pytest.raises(RuntimeError):
            eng.jet(4, rc.caps_of(g, 4), part0, max_iterations=2, **over)
    # the engine still works after the rejections
    _, part, st = eng.rebalance(4, rc.caps_of(g, 4), rc.skewed(g.n, 4))
    assert st.feasible == 1 and (np.bincount(part, minlength=4) <= rc.caps_of(g, 4)).all()


def test_defaults_did_not_move():
    jp = ka._lib.kmp_jet_params_default(0)
    assert (jp.balancer, jp.balance_passes, jp.balance_iters) == (ka.JET_BALANCER_LP, 16, 2)
    assert (ka.JET_BALANCER_LP, ka.JET_BALANCER_SELECT) == (0, 1)


def test_two_identical_calls_agree():
    c = rc.rmat_case(12, 16, "block0")
    eng = ka.LpEngine(c.g)
    cut, part, st = eng.rebalance(c.k, c.caps, c.part0)
    cut2, part2, st2 = eng.rebalance(c.k, c.caps, c.part0)
    assert cut2 == cut and (part2 == part).all()
    assert (st2.passes, st2.selected, st2.moves, st2.arcs_scanned, st2.feasible) == \
           (st.passes, st.selected, st.moves, st.arcs_scanned, st.feasible)


def test_no_state_leaks_between_calls():
    """refine -> rebalance -> jet -> cluster on one engine equals the same
    calls on fresh engines."""
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 16
    mbw = rc.caps_of(g, k)
    part0 = ka.random_partition(g.n, k, seed=5)
    mcw = int(g.total_node_weight // 128)

    def run(engine_for):
        c1, p1, _ = engine_for().refine(k, mbw, part0, seed=1, iters=5)
        skew = p1.copy()
        skew[::3] = 0
        c2, p2, _ = engine_for().rebalance(k, mbw, skew)
        c3, p3, _ = engine_for().jet(k, mbw, p2, seed=1, max_iterations=4, balancer=1)
        c4, p4, _ = engine_for().jet(k, mbw, p2, seed=1, max_iterations=4)
        nc, clus, _ = engine_for().cluster(mcw, seed=1, iters=5)
        return (c1, c2, c3, c4, nc), (p1, p2, p3, p4, clus)

    shared = ka.LpEngine(g)
    a_s, a_p = run(lambda: shared)
    b_s, b_p = run(lambda: ka.LpEngine(g))
    assert a_s == b_s
    for x, y in zip(a_p, b_p):
        assert (x == y).all()


# ------------------------------------------------- 3. Jet with balancer=1
@pytest.mark.parametrize("scale,k,temp", rc.JET)
def test_jet_with_the_selection_rebalancer(oracle, scale, k, temp):
    g = ka.Graph.rmat(scale, 8, seed=7)
    caps = rc.caps_of(g, k)
    part0 = ka.random_partition(g.n, k, seed=5)
    p = dict(num_rounds=1, max_iterations=8, max_fruitless=12, fruitless_threshold=0.999,
             initial_gain_temp=temp, final_gain_temp=temp)
    # balance_iters and the seed are ignored by balancer=1
    cut, part, st = ka.LpEngine(g).jet(k, caps, part0, seed=9, balancer=ka.JET_BALANCER_SELECT,
                                       balance_passes=16, balance_iters=3, **p)
    tcut, tpart, tst = rt.jet(oracle, g, k, caps, part0, balance_passes=16, **p)
    print(f"jet gpu cut {cut} twin {tcut} iterations {st.iterations}/{tst['iterations']} "
          f"balancer {st.balancer_calls}/{tst['balancer_calls']} "
          f"moves {st.balancer_moves}/{tst['balancer_moves']}")
    assert cut == tcut == st.edge_cut
    assert (part == tpart).all(), f"{(part != tpart).sum()} labels differ"
    assert st.iterations == tst["iterations"]
    assert st.balancer_calls == tst["balancer_calls"] >= 1
    assert st.jet_moves == tst["jet_moves"]
    assert st.balancer_moves == tst["balancer_moves"]
    assert (np.bincount(part, minlength=k) <= caps).all()


# ------------------------------------------------------------- 4. pipeline
def pipeline_graph(name):
    if name.startswith("walshaw"):
        d = json.load(open(os.path.join(GOLDEN, "walshaw_data.json")))
        return ka.Graph.from_csr(np.array(d["xadj"], np.uint32), np.array(d["adjncy"], np.uint32))
    return ka.Graph.rmat(int(name.split("_")[0][4:]), 8, 42)


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("name", ["walshaw_k16", "rmat14_s42_k16"])
def test_pipeline_with_the_selection_rebalancer(name, deep):
    from kaminpar_amd.partition import partition, partition_deep

    g = pipeline_graph(name)
    k = json.load(open(os.path.join(GOLDEN, "pipeline_expected.json")))[name]["k"]
    fn = partition_deep if deep else partition
    cut, part, levels = fn(g, k, seed=1, jet=dict(balancer=1))
    assert cut == g.edge_cut(part)
    assert (np.bincount(part, minlength=k) <= g.max_block_weight(k, 0.03)).all()
    cut2, part2, levels2 = fn(g, k, seed=1, jet=dict(balancer=1))
    assert cut2 == cut and (part2 == part).all() and levels2 == levels
