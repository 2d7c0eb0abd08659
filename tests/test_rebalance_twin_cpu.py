"""The numpy twin of the selection rebalancer (tests/rebalance_twin.py)
against hand-computed cases and its own invariants.

The GPU path (kmp_lp_rebalance) is pinned bit-exactly to the twin in
test_rebalance_gpu.py; this file pins the twin itself, without a GPU, and
proves that it reaches feasibility on every input the GPU file uses."""

import os

import numpy as np
import pytest

import kaminpar_amd as ka
import jet_twin
import rebalance_cases as rc
import rebalance_twin as rt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M = 1 << 20


def graph_from_edges(n, edges, vwgt=None):
    adj = [[] for _ in range(n)]
    for u, v in edges:
        adj[u].append(v)
        adj[v].append(u)
    xadj = np.zeros(n + 1, dtype=np.uint32)
    xadj[1:] = np.cumsum([len(a) for a in adj])
    adjncy = np.array([v for a in adj for v in a], dtype=np.uint32)
    if vwgt is None:
        return ka.Graph.from_csr(xadj, adjncy)
    return ka.Graph.from_csr(xadj, adjncy, np.asarray(vwgt, dtype=np.int32),
                             np.ones(len(adjncy), dtype=np.int32))


def run(g, k, caps, labels, max_passes=16, vwgt=None):
    out, st = rt.rebalance(g, k, np.array(caps, dtype=np.int64),
                           np.array(labels, dtype=np.uint32), max_passes=max_passes, vwgt=vwgt)
    return out.tolist(), st


def splitmix64_int(x):
    mask = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & mask
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
    return x ^ (x >> 31)


# ------------------------------------------------------------------ the key
def test_key_values():
    """gain > 0: gain * w; gain = 0: 0; gain < 0: gain / w, truncated, all with
    20 fractional bits; positive products saturate at 2^31 - 1."""
    assert rt.relative_key(3, 4) == 12 * M
    assert rt.relative_key(0, 5) == 0
    assert rt.relative_key(-3, 2) == -((3 * M) // 2) == -1572864
    assert rt.relative_key(-1, 3) == -349525  # 1048576 / 3 = 349525.33
    assert rt.relative_key(-7, 1) == -7 * M
    assert rt.relative_key(1 << 30, 4) == ((1 << 31) - 1) * M
    # the packed sort key of the kernels needs (-2^51 - 1, 2^51)
    assert rt.relative_key(-(1 << 31), 1) == -(1 << 51)
    assert rt.relative_key((1 << 31) - 1, 9) < (1 << 51)


def test_splitmix64_matches_the_scalar_definition():
    xs = np.array([0, 1, 17, (3 << 32) | 12345, (1 << 64) - 1], dtype=np.uint64)
    assert rt.splitmix64(xs).tolist() == [splitmix64_int(int(x)) for x in xs]


# ------------------------------------------------------------- hand cases
def test_path_key_order_decides_and_prefix_stops():
    """Path 0-..-5, blocks 0 0 0 0 1 1, caps 3: block 0 is over by 1, block 1
    has room 1. Vertex 3 touches block 1 (conn 1, own 1: gain 0, key 0).
    Vertices 0, 1, 2 see only block 0 and fall back to block 1 (the only room)
    with gain -own: keys -1, -2, -2 (x 2^20). Order 3, 0, 1, 2; the exclusive
    prefix 0, 1, 2, 3 is below the overload 1 for vertex 3 alone."""
    g = graph_from_edges(6, [(i, i + 1) for i in range(5)])
    n, src, dst, w, vw = jet_twin._arrays(g, None, None)
    labels = np.array([0, 0, 0, 0, 1, 1], dtype=np.uint32)
    caps = np.array([3, 3], dtype=np.int64)
    cand, to, key, arcs = rt.score(n, src, dst, w, vw, 2, labels,
                                   jet_twin.block_weights(labels, vw, 2), caps, 0)
    assert cand.tolist() == [True, True, True, True, False, False]
    assert to[:4].tolist() == [1, 1, 1, 1]
    assert key[:4].tolist() == [-M, -2 * M, -2 * M, 0]
    assert arcs == 1 + 2 + 2 + 2
    out, st = run(g, 2, caps, labels)
    assert out == [0, 0, 0, 1, 1, 1]
    assert st == {"passes": 1, "selected": 1, "moves": 1, "arcs": 7, "feasible": True}


def test_two_cliques_best_relative_gain_leaves_first():
    """Two K4 joined by 3-4, blocks 0 0 0 0 0 1 1 1 (vertex 4 on the wrong
    side), caps 4: block 0 is over by 1. Vertex 4: conn[1] 3, own 1, gain +2,
    key 2 * 2^20. Vertex 3: own 4 (three mates and 4), nothing adjacent in
    block 1, fallback, key -4 * 2^20; vertices 0..2: own 3, key -3 * 2^20.
    Vertex 4 goes home, nobody else."""
    k4 = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    g = graph_from_edges(8, k4 + [(a + 4, b + 4) for a, b in k4] + [(3, 4)])
    out, st = run(g, 2, [4, 4], [0, 0, 0, 0, 0, 1, 1, 1])
    assert out == [0, 0, 0, 0, 1, 1, 1, 1]
    assert (st["passes"], st["selected"], st["moves"], st["feasible"]) == (1, 1, 1, True)
    assert st["arcs"] == 3 + 3 + 3 + 4 + 4


def test_heavy_vertex_is_skipped_then_the_call_stalls():
    """Path 0-1-2, weights 2 5 1, blocks 0 0 1, caps 4. Block 0 weighs 7 (over
    3), block 1 has room 3. Vertex 1 (weight 5) fits nowhere: adjacent block 1,
    the fallback block and t* all lack room, so it is no candidate. Vertex 0
    (weight 2) has no adjacent target and falls back to block 1: gain -1, key
    -(2^20 / 2). It moves. Pass 1: block 0 weighs 5 (over 1), room 1 in block
    1, vertex 1 still fits nowhere: no candidate, stalled, infeasible."""
    vwgt = np.array([2, 5, 1], dtype=np.int32)
    g = graph_from_edges(3, [(0, 1), (1, 2)], vwgt=vwgt)
    n, src, dst, w, vw = jet_twin._arrays(g, vwgt, None)
    labels = np.array([0, 0, 1], dtype=np.uint32)
    caps = np.array([4, 4], dtype=np.int64)
    cand, to, key, _ = rt.score(n, src, dst, w, vw, 2, labels,
                                jet_twin.block_weights(labels, vw, 2), caps, 0)
    assert cand.tolist() == [True, False, False]
    assert to[0] == 1 and key[0] == -(M // 2)
    out, st = run(g, 2, caps, labels, vwgt=vwgt)
    assert out == [1, 0, 1]
    assert st == {"passes": 2, "selected": 1, "moves": 1, "arcs": 3 + 2, "feasible": False}


def test_admission_rejects_the_tail_and_the_next_pass_retargets():
    """Edges 0-2 and 1-2; 3, 4, 5 isolated. Blocks 0 0 1 0 0 2, caps 2 2 6:
    block 0 is over by 2, room 1 in block 1 and 5 in block 2. Vertices 0 and 1
    both target block 1 (gain +1, key 2^20) and are the selected prefix (the
    isolated 3 and 4 have key 0). Block 1 admits vertex 0 (prefix 1 <= 1) and
    rejects vertex 1 (2 > 1). Pass 1: block 1 is full, so vertex 1 falls back
    to block 2 (key 0, lowest id among three zeros) and covers the overload."""
    g = graph_from_edges(6, [(0, 2), (1, 2)])
    caps = [2, 2, 6]
    labels = [0, 0, 1, 0, 0, 2]
    out, st = run(g, 3, caps, labels, max_passes=1)
    assert out == [1, 0, 1, 0, 0, 2]
    assert st == {"passes": 1, "selected": 2, "moves": 1, "arcs": 2, "feasible": False}
    out, st = run(g, 3, caps, labels)
    assert out == [1, 2, 1, 0, 0, 2]
    assert st == {"passes": 2, "selected": 3, "moves": 2, "arcs": 3, "feasible": True}


def test_isolated_vertices_take_the_fallback():
    """Edge 2-3; 0 and 1 isolated in block 0, caps 1 3: one of them has to go,
    both have key 0, the lower id leaves."""
    g = graph_from_edges(4, [(2, 3)])
    out, st = run(g, 2, [1, 3], [0, 0, 1, 1])
    assert out == [1, 0, 1, 1]
    assert st == {"passes": 1, "selected": 1, "moves": 1, "arcs": 0, "feasible": True}


@pytest.mark.parametrize("p", [0, 3])
def test_fallback_is_proportional_to_room(p):
    """40 isolated vertices in block 0, rooms 3 and 5 in blocks 1 and 2:
    cum = 0 3 8, so r = splitmix64((p << 32) | u) mod 8 picks block 1 iff
    r < 3. Vertices 40.. are the ballast of blocks 1 and 2."""
    n = 40 + 2 + 2
    g = graph_from_edges(n, [(40, 41), (42, 43)])
    _, src, dst, w, vw = jet_twin._arrays(g, None, None)
    labels = np.array([0] * 40 + [1, 1, 2, 2], dtype=np.uint32)
    caps = np.array([10, 5, 7], dtype=np.int64)
    cand, to, key, _ = rt.score(n, src, dst, w, vw, 3, labels,
                                jet_twin.block_weights(labels, vw, 3), caps, p)
    want = [1 if splitmix64_int((p << 32) | u) % 8 < 3 else 2 for u in range(40)]
    assert cand[:40].all() and not cand[40:].any()
    assert to[:40].tolist() == want
    assert len(set(want)) == 2
    assert (key[:40] == 0).all()


# -------------------------------------------------------------- properties
def property_graphs():
    yield ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis")), 4
    yield ka.Graph.rmat(10, 8, seed=7), 16
    yield ka.Graph.rmat(12, 8, seed=7), 16


def test_pass_invariants():
    """Pass by pass: the total overload never grows, no target ends above its
    cap, and vertices outside the source blocks never move."""
    for g, k in property_graphs():
        n, src, dst, w, vw = jet_twin._arrays(g, None, None)
        caps = rc.caps_of(g, k)
        for labels in (rc.skewed(g.n, k), np.zeros(g.n, dtype=np.uint32)):
            for p in range(16):
                W = jet_twin.block_weights(labels, vw, k)
                out, sources, sel, adm, _ = rt.rebalance_pass(n, src, dst, w, vw, k, labels,
                                                              caps, p)
                if not sources:
                    break
                W2 = jet_twin.block_weights(out, vw, k)
                assert np.maximum(W2 - caps, 0).sum() <= np.maximum(W - caps, 0).sum()
                was_ok = W <= caps
                assert (W2[was_ok] <= caps[was_ok]).all()
                assert (W2[~was_ok] <= W[~was_ok]).all()
                moved = out != labels
                assert (W[labels[moved]] > caps[labels[moved]]).all()
                assert moved.sum() == adm <= sel
                labels = out
            assert (jet_twin.block_weights(labels, vw, k) <= caps).all()


def test_feasible_input_is_a_no_op():
    for g, k in property_graphs():
        part0 = ka.random_partition(g.n, k, seed=5)
        caps = np.full(k, np.bincount(part0, minlength=k).max(), dtype=np.int64)
        out, st = rt.rebalance(g, k, caps, part0)
        assert (out == part0).all()
        assert st == {"passes": 0, "selected": 0, "moves": 0, "arcs": 0, "feasible": True}


# ------------------------------------- the inputs of test_rebalance_gpu.py
def check_case(c):
    out, st = rt.rebalance(c.g, c.k, c.caps, c.part0, max_passes=c.max_passes, vwgt=c.vwgt,
                           adjwgt=c.adjwgt)
    print(f"passes {st['passes']} selected {st['selected']} moves {st['moves']} "
          f"feasible {st['feasible']}")
    assert st["feasible"] == c.feasible
    assert st["passes"] <= c.max_passes
    assert st["moves"] > 0
    return out, st


@pytest.mark.parametrize("scale,k,start", rc.RMAT)
def test_twin_reaches_feasibility_rmat(scale, k, start):
    check_case(rc.rmat_case(scale, k, start))


@pytest.mark.parametrize("name", sorted(rc.OTHER))
def test_twin_on_the_other_gpu_inputs(name):
    c = rc.OTHER[name]()
    out, st = check_case(c)
    if name == "isolated":
        assert (out[-37:] != 0).any()  # the fallback moved isolated vertices
    if name == "one_pass":
        assert st["passes"] == 1
    if name == "unmeetable":
        assert c.caps.sum() < c.g.total_node_weight


@pytest.mark.parametrize("scale,k,temp", rc.JET)
def test_jet_with_the_twin_as_its_rebalance_step(oracle, scale, k, temp):
    """The reference for eng.jet(..., balancer=1): the rebalance step runs and
    the result is feasible."""
    g = ka.Graph.rmat(scale, 8, seed=7)
    caps = rc.caps_of(g, k)
    cut, part, st = rt.jet(oracle, g, k, caps, ka.random_partition(g.n, k, seed=5),
                           max_iterations=8, initial_gain_temp=temp, final_gain_temp=temp)
    assert st["balancer_calls"] >= 1
    assert (np.bincount(part, minlength=k) <= caps).all()
    assert cut == jet_twin.edge_cut(oracle, g, part)
