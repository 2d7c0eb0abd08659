"""GPU Jet refiner (kmp_lp_jet / LpEngine.jet) against its numpy twin
(tests/jet_twin.py): labels, cut, iterations, balancer calls and move counts
must be BIT-IDENTICAL. Covers the three degree tiers (16-lane subgroups,
wavefront, workgroup), the u8 and u16 label shadows, weighted graphs, the
rebalance step (v1 commit, isolated pre-pass), rounds with rollback, and the
pipelines' jet=True switch."""

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
from helpers import oracle_refine

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def params(**over):
    p = dict(num_rounds=1, max_iterations=8, max_fruitless=12, fruitless_threshold=0.999,
             initial_gain_temp=0.25, final_gain_temp=0.25, balance_iters=1)
    p.update(over)
    return p


def check_against_twin(oracle, g, k, mbw, part0, seed=1, vwgt=None, adjwgt=None, **p):
    """Runs both sides with explicit parameters and compares bit-exactly."""
    eng = ka.LpEngine(g)
    cut, part, st = eng.jet(k, mbw, part0, seed=seed, **p)
    tcut, tpart, tst = jet_twin.jet(oracle, g, k, mbw, part0, seed=seed, vwgt=vwgt,
                                    adjwgt=adjwgt, **p)
    print(f"jet gpu cut {cut} twin {tcut} iterations {st.iterations}/{tst['iterations']} "
          f"balancer {st.balancer_calls}/{tst['balancer_calls']} "
          f"moves {st.jet_moves}/{tst['jet_moves']} rollbacks {tst['rollbacks']}")
    assert cut == tcut
    assert st.iterations == tst["iterations"]
    assert st.balancer_calls == tst["balancer_calls"]
    assert st.jet_moves == tst["jet_moves"]
    assert st.balancer_moves == tst["balancer_moves"]
    assert (part == tpart).all(), f"{(part != tpart).sum()} labels differ"
    assert st.edge_cut == cut
    return cut, part, st, tst


def caps(g, k, eps=0.03):
    return np.full(k, g.max_block_weight(k, eps), dtype=np.int64)


# ---------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("scale,k", [(10, 2), (10, 16), (10, 256), (12, 2), (12, 16),
                                     (12, 256), (12, 512)])
def test_kernels_alone(oracle, scale, k):
    """Caps at the total weight: the balancer never runs; one iteration."""
    g = ka.Graph.rmat(scale, 8, seed=7)
    mbw = np.full(k, g.total_node_weight, dtype=np.int64)
    part0 = ka.random_partition(g.n, k, seed=5)
    cut, part, st, _ = check_against_twin(
        oracle, g, k, mbw, part0, **params(max_iterations=1, initial_gain_temp=0.75,
                                           final_gain_temp=0.75))
    assert st.balancer_calls == 0 and st.iterations == 1 and st.jet_moves > 0
    assert cut < g.edge_cut(part0)  # so the returned labels are the iteration's


# -------------------------------------------------------------- 2. full loop
@pytest.mark.parametrize("balance_iters", [1, 2])
@pytest.mark.parametrize("temp", [0.25, 0.75])
@pytest.mark.parametrize("scale,k", [(10, 8), (12, 16), (12, 256), (14, 16)])
def test_full_loop(oracle, scale, k, temp, balance_iters):
    g = ka.Graph.rmat(scale, 8, seed=7)
    part0 = ka.random_partition(g.n, k, seed=5)
    _, _, st, _ = check_against_twin(
        oracle, g, k, caps(g, k), part0, seed=3,
        **params(initial_gain_temp=temp, final_gain_temp=temp, balance_iters=balance_iters))
    assert st.balancer_calls >= 1  # the rebalance step is part of what is pinned


def test_two_rounds_with_rollback(oracle):
    """0.75 -> 0.25 over two rounds; the first round ends on a state that is
    not the best, so it is rolled back before the second starts."""
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 16
    mbw = caps(g, k)
    _, part0, _ = oracle_refine(oracle, g, k, mbw, ka.random_partition(g.n, k, seed=5),
                                seed=1, iters=5)
    _, _, st, tst = check_against_twin(
        oracle, g, k, mbw, part0, seed=2,
        **params(num_rounds=2, max_iterations=4, initial_gain_temp=0.75, final_gain_temp=0.25))
    assert st.iterations == 8
    assert tst["rollbacks"] >= 1


def test_full_loop_k512_legacy_commit(oracle):
    """k > 256: u16 shadow in find, and the balance sweeps commit through the
    sort-based path."""
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 512
    _, _, st, _ = check_against_twin(oracle, g, k, caps(g, k),
                                     ka.random_partition(g.n, k, seed=5), seed=4,
                                     **params(max_iterations=4, initial_gain_temp=0.75,
                                              final_gain_temp=0.75))
    assert st.balancer_calls >= 1


# ---------------------------------------------------------- 3. degree tiers
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
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    assert deg[ring:].tolist() == degs
    return g


@pytest.mark.parametrize("temp", [0.25, 0.75])
def test_degree_tiers(oracle, temp):
    g = tier_graph()
    k = 4
    check_against_twin(oracle, g, k, caps(g, k), ka.random_partition(g.n, k, seed=11), seed=1,
                       **params(initial_gain_temp=temp, final_gain_temp=temp))


# ---------------------------------------------------------------- 4. weights
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


@pytest.mark.parametrize("k", [4, 16])
def test_weighted(oracle, k):
    g, vwgt, adjwgt = weighted_rgg()
    cut, part, _, _ = check_against_twin(
        oracle, g, k, caps(g, k), ka.random_partition(g.n, k, seed=3), seed=5, vwgt=vwgt,
        adjwgt=adjwgt, **params(initial_gain_temp=0.75, final_gain_temp=0.75))
    assert cut == g.edge_cut(part)


# --------------------------------------------------------- 5. awkward shapes
def test_n_not_a_multiple_of_64(oracle):
    g = ka.Graph.rgg2d(1000 + 37, 8.0, seed=3)
    assert g.n % 64 != 0
    k = 8
    check_against_twin(oracle, g, k, caps(g, k), ka.random_partition(g.n, k, seed=3), seed=1,
                       **params())


def test_isolated_vertices_in_an_overloaded_block(oracle):
    """37 isolated vertices sit in a block that is over its cap, so the
    balancer's isolated pre-pass runs inside the Jet loop."""
    g0 = ka.Graph.rgg2d(1003, 8.0, seed=4)
    xadj = np.concatenate([np.asarray(g0.xadj, dtype=np.uint32),
                           np.full(37, g0.m, dtype=np.uint32)])
    g = ka.Graph.from_csr(xadj, np.asarray(g0.adjncy, dtype=np.uint32).copy())
    assert g.n == 1040 and (np.diff(xadj.astype(np.int64))[-37:] == 0).all()
    k = 4
    mbw = caps(g, k)
    part0 = ka.random_partition(g.n, k, seed=3)
    part0[-37:] = 0
    part0[:60] = 0  # block 0 is over its cap by about the isolated vertices
    assert np.bincount(part0, minlength=k)[0] > mbw[0]
    _, part, st, _ = check_against_twin(oracle, g, k, mbw, part0, seed=1,
                                        **params(balance_iters=2))
    assert st.balancer_calls >= 1
    assert (part[-37:] != 0).any()  # the pre-pass moved isolated vertices
    assert (np.bincount(part, minlength=k) <= mbw).all()


def test_multigraph_parallel_arcs(oracle):
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
    k = 4
    check_against_twin(oracle, g, k, caps(g, k), ka.random_partition(g.n, k, seed=3), seed=1,
                       **params(initial_gain_temp=0.75, final_gain_temp=0.75))


# ------------------------------------------------- 6. invariants and state
def test_invariants_and_determinism():
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 16
    mbw = caps(g, k)
    eng = ka.LpEngine(g)
    lp_cut, part0, _ = eng.refine(k, mbw, ka.random_partition(g.n, k, seed=5), seed=1, iters=5)
    cut, part, st = eng.jet(k, mbw, part0, seed=1, **params())
    assert cut == g.edge_cut(part) == st.edge_cut
    assert (np.bincount(part, minlength=k) <= mbw).all()
    assert cut <= lp_cut
    cut2, part2, st2 = eng.jet(k, mbw, part0, seed=1, **params())
    assert cut2 == cut and (part2 == part).all()
    assert (st2.iterations, st2.balancer_calls, st2.jet_moves, st2.balancer_moves,
            st2.arcs_scanned) == (st.iterations, st.balancer_calls, st.jet_moves,
                                  st.balancer_moves, st.arcs_scanned)


def test_no_state_leaks_between_calls():
    """refine -> jet -> refine -> cluster on one engine equals the same calls
    on fresh engines (jet reallocates nothing the other modes rely on, and
    captured sweep graphs are rebuilt)."""
    g = ka.Graph.rmat(12, 8, seed=7)
    k = 16
    mbw = caps(g, k)
    part0 = ka.random_partition(g.n, k, seed=5)
    mcw = int(g.total_node_weight // 128)

    def run(engine_for):
        c1, p1, _ = engine_for().refine(k, mbw, part0, seed=1, iters=5)
        c2, p2, _ = engine_for().jet(k, mbw, p1, seed=1, **params(max_iterations=4))
        c3, p3, _ = engine_for().refine(k, mbw, p2, seed=2, iters=5)
        nc, clus, _ = engine_for().cluster(mcw, seed=1, iters=5)
        return (c1, c2, c3, nc), (p1, p2, p3, clus)

    shared = ka.LpEngine(g)
    a_s, a_p = run(lambda: shared)
    b_s, b_p = run(lambda: ka.LpEngine(g))
    assert a_s == b_s
    for x, y in zip(a_p, b_p):
        assert (x == y).all()


def test_infeasible_input_ends_feasible(oracle):
    g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    k = 4
    mbw = caps(g, k)
    part0 = np.zeros(g.n, dtype=np.uint32)  # everything in block 0
    _, part, st, _ = check_against_twin(oracle, g, k, mbw, part0, seed=1,
                                        **params(max_fruitless=0, balance_iters=2))
    assert st.balancer_calls >= 1
    assert (np.bincount(part, minlength=k) <= mbw).all()


def test_bad_parameters_are_rejected():
    g = ka.Graph.rmat(10, 8, seed=7)
    eng = ka.LpEngine(g)
    part0 = ka.random_partition(g.n, 4, seed=5)
    with pytest.raises(RuntimeError):
        eng.jet(4, caps(g, 4), part0, **params(max_iterations=0, max_fruitless=0))
    with pytest.raises(RuntimeError):
        eng.jet(4, caps(g, 4), part0, **params(balance_iters=0))
    with pytest.raises(TypeError):
        eng.jet(4, caps(g, 4), part0, temperature=0.5)
    bad = part0.copy()
    bad[17] = 4  # a label that is not below k
    with pytest.raises(RuntimeError):
        eng.jet(4, caps(g, 4), bad, **params())
    k = 4096
    with pytest.raises(RuntimeError):
        eng.jet(k, caps(g, k), ka.random_partition(g.n, k, seed=5), **params())


# ------------------------------------------------------------- 7. quality
@pytest.mark.parametrize("k", [4, 16])
def test_quality_rgg2d(oracle, k):
    """Jet from the 5-sweep LP result, run to its own stopping rule (the one
    test beyond 8 iterations). Twin on the CPU: LP 530 -> Jet 352 (k=4) and
    LP 1747 -> Jet 601 (k=16); test_jet_twin_cpu.py pins those figures."""
    g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    mbw = caps(g, k)
    eng = ka.LpEngine(g)
    lp_cut, part0, _ = eng.refine(k, mbw, ka.random_partition(g.n, k, seed=3), seed=1, iters=5)
    cut, part, st, _ = check_against_twin(
        oracle, g, k, mbw, part0, seed=1, **params(max_iterations=0, max_fruitless=12))
    print(f"rgg2d k={k}: LP {lp_cut} -> Jet {cut} in {st.iterations} iterations")
    assert cut < lp_cut
    assert (np.bincount(part, minlength=k) <= mbw).all()


# ------------------------------------------------------------- 8. pipeline
def pipeline_graph(name):
    if name.startswith("walshaw"):
        d = json.load(open(os.path.join(GOLDEN, "walshaw_data.json")))
        return ka.Graph.from_csr(np.array(d["xadj"], np.uint32), np.array(d["adjncy"], np.uint32))
    return ka.Graph.rmat(int(name.split("_")[0][4:]), 8, 42)


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("name", ["walshaw_k16", "rmat14_s42_k16"])
def test_pipeline_with_jet(name, deep):
    from kaminpar_amd.partition import partition, partition_deep

    g = pipeline_graph(name)
    k = json.load(open(os.path.join(GOLDEN, "pipeline_expected.json")))[name]["k"]
    fn = partition_deep if deep else partition
    cut, part, levels = fn(g, k, seed=1, jet=True)
    assert cut == g.edge_cut(part)
    assert (np.bincount(part, minlength=k) <= g.max_block_weight(k, 0.03)).all()
    cut2, part2, levels2 = fn(g, k, seed=1, jet=True)
    assert cut2 == cut and (part2 == part).all() and levels2 == levels
