"""The numpy twin of the threshold edge sparsification (tests/sparsify_twin.py)
against hand-computed cases and against invariants of the rule on seeded random
weighted graphs. No GPU: test_sparsify_gpu.py pins
kmp_contract_engine_sparsified to this twin."""

import numpy as np
import pytest

import sparsify_twin as st

MASK = (1 << 64) - 1


def py_dice(u, v, seed):
    """The dice in Python integers, written independently of the twin."""
    x = (((max(u, v) << 32) | min(u, v)) + seed) & MASK
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & MASK
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & MASK
    x ^= x >> 33
    return x & 0xFFFFFFFF


def csr(n, edges):
    """Sorted-row CSR of undirected weighted edges (u, v, w)."""
    rows = [[] for _ in range(n)]
    for u, v, w in edges:
        rows[u].append((v, w))
        rows[v].append((u, w))
    rows = [sorted(r) for r in rows]
    xadj = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    adjncy = np.array([v for r in rows for v, _ in r], dtype=np.uint32)
    adjwgt = np.array([w for r in rows for _, w in r], dtype=np.int32)
    return xadj, adjncy, adjwgt


SIX = [(0, 1, 1), (0, 2, 2), (1, 2, 3), (2, 3, 4), (3, 4, 5), (4, 5, 6), (3, 5, 7)]


def test_distinct_weights_only_the_threshold_decides():
    """14 arcs; 0.43 * 14 = 6.02, so target = 6. The 9th smallest arc weight
    is T = 5: four arcs are heavier, the two of weight 5 are both included
    (include = equal = 2), and edges 3-4, 4-5, 3-5 stay."""
    xadj, adjncy, adjwgt = csr(6, SIX)
    p = dict(density_target_factor=1.0, edge_target_factor=0.43, laziness_factor=1)
    x2, a2, w2, s = st.sparsify(xadj, adjncy, adjwgt, 6, 14, p, seed=123)
    assert s == dict(applied=1, m_before=14, m_after=6, target=6, threshold=5,
                     larger=4, equal=2, include=2)
    assert x2.tolist() == [0, 0, 0, 0, 2, 4, 6]
    assert a2.tolist() == [4, 5, 3, 5, 3, 4]
    assert w2.tolist() == [5, 7, 5, 6, 7, 6]


@pytest.mark.parametrize("seed", [0, 1, 2**63 + 5])
def test_equal_weights_the_dice_decide_everything(seed):
    edges = [(u, v, 3) for u in range(12) for v in range(u + 1, 12)]
    xadj, adjncy, adjwgt = csr(12, edges)
    m = len(adjncy)
    assert m == 132
    p = dict(density_target_factor=0.5, edge_target_factor=0.5, laziness_factor=1)
    x2, a2, w2, s = st.sparsify(xadj, adjncy, adjwgt, 12, m, p, seed=seed)
    assert (s["threshold"], s["larger"], s["equal"], s["target"]) == (3, 0, 132, 66)
    assert s["include"] == 66
    want_rows = [[v for v in range(12) if v != u
                  and py_dice(u, v, seed) * 132 < 66 << 32] for u in range(12)]
    assert x2.tolist() == np.cumsum([0] + [len(r) for r in want_rows]).tolist()
    assert a2.tolist() == [v for r in want_rows for v in r]
    assert (w2 == 3).all() and s["m_after"] == len(a2)
    assert 0 < len(a2) < m  # the dice did run


def test_target_below_two_drops_every_arc():
    xadj, adjncy, adjwgt = csr(6, SIX)
    p = dict(density_target_factor=1.0, edge_target_factor=0.1, laziness_factor=1)
    x2, a2, w2, s = st.sparsify(xadj, adjncy, adjwgt, 6, 14, p, seed=0)
    assert s == dict(applied=1, m_before=14, m_after=0, target=1, threshold=0,
                     larger=0, equal=0, include=0)
    assert x2.tolist() == [0] * 7 and len(a2) == 0 and len(w2) == 0


def test_not_triggered_returns_the_input():
    """Defaults: target is 6 or 7, and 14 arcs are no more than 4 times that."""
    xadj, adjncy, adjwgt = csr(6, SIX)
    x2, a2, w2, s = st.sparsify(xadj, adjncy, adjwgt, 6, 14, None, seed=0)
    assert x2 is xadj and a2 is adjncy and w2 is adjwgt
    assert s["applied"] == 0 and s["m_after"] == s["m_before"] == 14
    # lazy enough and the same graph is left alone at target = 6 too
    p = dict(density_target_factor=1.0, edge_target_factor=0.43, laziness_factor=2.5)
    assert st.sparsify(xadj, adjncy, adjwgt, 6, 14, p)[0] is xadj


def test_target_follows_the_reference():
    p = dict(st.DEFAULT_PARAMS)
    assert p == dict(density_target_factor=0.5, edge_target_factor=0.5, laziness_factor=4.0)
    # the edge rule binds / the density rule binds / the cap at old_m
    assert st.sparsify_target(1000, 8000, 900, p) == 3600
    assert st.sparsify_target(1000, 8000, 100, p) == 400
    big = dict(p, edge_target_factor=3.0, density_target_factor=3.0)
    assert st.sparsify_target(1000, 8000, 900, big) == 8000


def random_graph(seed, n=300, m=4000, wmax=5):
    rng = np.random.default_rng(seed)
    pairs = {(min(a, b), max(a, b)) for a, b in rng.integers(0, n, (m, 2)) if a != b}
    return csr(n, [(u, v, int(rng.integers(1, wmax + 1))) for u, v in sorted(pairs)])


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("factor", [0.5, 0.2, 0.05])
def test_properties_on_random_graphs(seed, factor):
    xadj, adjncy, adjwgt = random_graph(seed)
    n, m = len(xadj) - 1, len(adjncy)
    p = dict(density_target_factor=factor, edge_target_factor=factor, laziness_factor=1)
    x2, a2, w2, s = st.sparsify(xadj, adjncy, adjwgt, n, m, p, seed=seed)
    assert s["applied"] == 1 and s["m_after"] == len(a2) == x2[-1]
    T = s["threshold"]
    arcs = lambda x, a, w: {(u, int(a[e]), int(w[e]))
                            for u in range(n) for e in range(x[u], x[u + 1])}
    before, after = arcs(xadj, adjncy, adjwgt), arcs(x2, a2, w2)
    assert len(before) == m and len(after) == len(a2)  # rows hold no duplicates
    assert after <= before
    assert all((v, u, w) in after for u, v, w in after)  # symmetric
    assert {a for a in before if a[2] > T} <= after
    assert not {a for a in after if a[2] < T}
    # per-row order is preserved: rows were sorted and still are
    for u in range(n):
        row = a2[x2[u]:x2[u + 1]]
        assert (np.diff(row.astype(np.int64)) > 0).all()
    # the count is near the target: within the ties that the dice decide
    assert s["larger"] <= s["m_after"] <= s["larger"] + s["equal"]
    assert s["larger"] < s["target"] <= s["larger"] + s["equal"]
