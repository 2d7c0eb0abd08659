"""The numpy Jet twin (tests/jet_twin.py) against hand-computed cases.

The GPU refiner (kmp_lp_jet) is pinned bit-exactly to the twin in
test_jet_gpu.py; this file pins the twin itself, without a GPU."""

import os

import numpy as np
import pytest

import kaminpar_amd as ka
import jet_twin
from helpers import oracle_refine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def graph_from_edges(n, edges):
    adj = [[] for _ in range(n)]
    for u, v in edges:
        adj[u].append(v)
        adj[v].append(u)
    xadj = np.zeros(n + 1, dtype=np.uint32)
    xadj[1:] = np.cumsum([len(a) for a in adj])
    adjncy = np.array([v for a in adj for v in a], dtype=np.uint32)
    return ka.Graph.from_csr(xadj, adjncy)


def one_iteration(g, k, labels, t):
    n, src, dst, w, _ = jet_twin._arrays(g, None, None)
    lock = np.zeros(n, dtype=bool)
    lab = np.asarray(labels, dtype=np.uint32)
    cand, nxt, gain = jet_twin.find(n, src, dst, w, k, lab, lock, t)
    out, new_lock, _, moved = jet_twin.jet_iteration(n, src, dst, w, k, lab, lock, t)
    return cand, nxt, gain, out, new_lock, moved


def test_path_swap_is_rejected_by_the_afterburner(oracle):
    """Path 0-..-7, blocks 0 0 0 1 0 1 1 1. Vertices 3 and 4 both want to
    swap sides (gain 2 each: own 0, two neighbours across). Vertices 2 and 5
    have gain 0, which is not > -floor(0.25 * 1) = 0. The afterburner ranks 3
    ahead of 4 (equal gain, lower id): 3 sees 2 and 4 in its target block
    (+2) and moves; 4 assumes 3 already sits in block 0 (its own block: -1)
    against 5 in its target (+1), total 0, and is rejected."""
    g = graph_from_edges(8, [(i, i + 1) for i in range(7)])
    labels = [0, 0, 0, 1, 0, 1, 1, 1]
    assert jet_twin.edge_cut(oracle, g, np.array(labels, dtype=np.uint32)) == 3
    cand, nxt, gain, out, lock, moved = one_iteration(g, 2, labels, 0.25)
    assert cand.tolist() == [False, False, False, True, True, False, False, False]
    assert nxt.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert gain.tolist() == [0, 0, 0, 2, 2, 0, 0, 0]
    assert lock.tolist() == [False, False, False, True, False, False, False, False]
    assert out.tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert moved == 1
    assert jet_twin.edge_cut(oracle, g, out) == 1


def test_two_cliques(oracle):
    """Two K4 joined by the edge 3-4, vertex 3 on the wrong side: own 1,
    connectivity 3 to block 0, gain 2. Its clique mates have own 2, other 1,
    gain -1, which is not > -floor(0.75 * 2) = -1, so even the coarse
    temperature keeps them in place; 4..7 have no neighbour in another block
    (3 still carries block 1 in the snapshot). One move, cut 3 -> 1."""
    k4 = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    edges = k4 + [(a + 4, b + 4) for a, b in k4] + [(3, 4)]
    g = graph_from_edges(8, edges)
    labels = [0, 0, 0, 1, 1, 1, 1, 1]
    assert jet_twin.edge_cut(oracle, g, np.array(labels, dtype=np.uint32)) == 3
    for t in (0.25, 0.75):
        cand, nxt, gain, out, lock, moved = one_iteration(g, 2, labels, t)
        assert cand.tolist() == [False, False, False, True, False, False, False, False]
        assert nxt.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
        assert gain[3] == 2
        assert lock.tolist() == [False, False, False, True, False, False, False, False]
        assert out.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
        assert jet_twin.edge_cut(oracle, g, out) == 1


def test_tie_goes_to_the_lowest_block_id():
    """Vertex 0 (block 2) has one neighbour in block 1 (listed first) and one
    in block 0: equal connectivity, the smaller id wins."""
    g = graph_from_edges(3, [(0, 1), (0, 2)])
    cand, nxt, gain, _, _, _ = one_iteration(g, 3, [2, 1, 0], 0.25)
    assert cand[0] and nxt[0] == 0 and gain[0] == 1


@pytest.mark.parametrize("other,expect", [(2, {0.0: False, 0.25: False, 0.75: True}),
                                          (1, {0.0: False, 0.25: False, 0.75: False}),
                                          (4, {0.0: True, 0.25: True, 0.75: True})])
def test_temperature_rule_with_own_three(other, expect):
    """Vertex 0 has own connectivity 3 and `other` arcs into block 1. The move
    is kept iff gain > -floor(t * 3): thresholds 0, 0 and -2 at t = 0, 0.25
    and 0.75, so gain -1 passes only at 0.75 and gain -2 never does."""
    edges = [(0, v) for v in range(1, 4 + other)]
    g = graph_from_edges(4 + other, edges)
    labels = [0, 0, 0, 0] + [1] * other
    for t, want in expect.items():
        cand, nxt, gain, _, _, _ = one_iteration(g, 2, labels, t)
        assert bool(cand[0]) == want, (t, other)
        if want:
            assert nxt[0] == 1 and gain[0] == other - 3


def test_locked_vertices_are_not_candidates():
    g = graph_from_edges(8, [(i, i + 1) for i in range(7)])
    n, src, dst, w, _ = jet_twin._arrays(g, None, None)
    lab = np.array([0, 0, 0, 1, 0, 1, 1, 1], dtype=np.uint32)
    lock = np.zeros(n, dtype=bool)
    lock[3] = True
    cand, nxt, _ = jet_twin.find(n, src, dst, w, 2, lab, lock, 0.25)
    assert not cand[3] and nxt[3] == 1 and cand[4]


@pytest.mark.parametrize("k", [4, 16])
def test_invariants_rgg2d(oracle, k):
    g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    mbw = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    _, part0, _ = oracle_refine(oracle, g, k, mbw, ka.random_partition(g.n, k, seed=3),
                                seed=1, iters=5)
    assert (np.bincount(part0, minlength=k) <= mbw).all()
    cut0 = g.edge_cut(part0)
    runs = [jet_twin.jet(oracle, g, k, mbw, part0, seed=1, max_iterations=8,
                         initial_gain_temp=0.25, final_gain_temp=0.25)
            for _ in range(2)]
    cut, part, stats = runs[0]
    assert (np.bincount(part, minlength=k) <= mbw).all()
    assert cut == g.edge_cut(part)
    assert cut <= cut0
    assert stats["iterations"] == 8
    assert cut == runs[1][0] and (part == runs[1][1]).all() and stats == runs[1][2]


@pytest.mark.parametrize("k,lp_cut,jet_cut", [(4, 530, 352), (16, 1747, 601)])
def test_quality_rgg2d_pinned(oracle, k, lp_cut, jet_cut):
    """Jet run to its own stopping rule (12 fruitless iterations, t = 0.25,
    one balance sweep) from the 5-sweep LP result: the figures the GPU
    quality test reproduces. Pinned from this twin; they only move if the
    twin, the oracle's balancer or the LP schedule changes."""
    g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    mbw = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    c0, part0, _ = oracle_refine(oracle, g, k, mbw, ka.random_partition(g.n, k, seed=3),
                                 seed=1, iters=5)
    cut, part, _ = jet_twin.jet(oracle, g, k, mbw, part0, seed=1, max_iterations=0,
                                max_fruitless=12, initial_gain_temp=0.25,
                                final_gain_temp=0.25, balance_iters=1)
    assert (c0, cut) == (lp_cut, jet_cut)
    assert (np.bincount(part, minlength=k) <= mbw).all()


def test_infeasible_input_ends_feasible(oracle):
    g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
    k = 4
    mbw = np.full(k, g.max_block_weight(k, 0.03), dtype=np.int64)
    part0 = np.zeros(g.n, dtype=np.uint32)  # everything in block 0
    cut, part, stats = jet_twin.jet(oracle, g, k, mbw, part0, seed=1, max_iterations=8,
                                    max_fruitless=0, balance_iters=2)
    assert stats["balancer_calls"] >= 1
    assert (np.bincount(part, minlength=k) <= mbw).all()
    assert cut == g.edge_cut(part)
