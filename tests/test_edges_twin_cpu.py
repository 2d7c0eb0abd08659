"""The numpy twin of kmp_lp_create_from_edges (tests/edges_twin.py) against
hand-computed cases (tests/edges_cases.py). No GPU."""

import numpy as np
import pytest

import edges_cases as ec
import kaminpar_amd as ka
from edges_twin import edges_to_csr


def check(got, want, pairs):
    n, xadj, adjncy, adjwgt, stats = got
    wn, wxadj, wadj, wwgt, wloops = want
    assert n == wn
    assert xadj.tolist() == wxadj
    assert adjncy.tolist() == wadj
    assert (adjwgt is None) == (wwgt is None)
    if wwgt is not None:
        assert adjwgt.tolist() == wwgt
    deg = np.diff(np.array(wxadj))
    assert stats == {
        "pairs": pairs, "self_loops": wloops, "arcs": len(wadj),
        "merged_arcs": 2 * (pairs - wloops) - len(wadj), "n": wn,
        "isolated": int((deg == 0).sum()), "max_degree": int(deg.max()),
    }


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_hand_cases(name):
    src, dst, n, weights, combine, want = ec.case_arrays(name)
    check(edges_to_csr(src, dst, n, weights, combine), want, len(src))


def test_triangle_forms_agree():
    got = [edges_to_csr(*ec.case_arrays(name)[:5])
           for name in ("triangle_one_direction", "triangle_both_directions",
                        "triangle_with_repeats")]
    for g in got[1:]:
        assert np.array_equal(g[1], got[0][1]) and np.array_equal(g[2], got[0][2])
    # what separates them is only the count of merged arcs
    assert [g[4]["merged_arcs"] for g in got] == [0, 6, 8]


def test_max_is_idempotent_for_both_directions():
    src, dst, n, w, _, _ = ec.case_arrays("weights_max")
    one = edges_to_csr(src, dst, n, w, "max")
    both = edges_to_csr(np.concatenate([src, dst]), np.concatenate([dst, src]), n,
                        np.concatenate([w, w]), "max")
    assert np.array_equal(one[3], both[3])
    twice = edges_to_csr(np.concatenate([src, dst]), np.concatenate([dst, src]), n,
                         np.concatenate([w, w]), "sum")
    assert np.array_equal(twice[3], 2 * edges_to_csr(src, dst, n, w, "sum")[3])


def test_long_run():
    src, dst, w = ec.long_run()
    assert edges_to_csr(src, dst, 2, w, "max")[3].tolist() == [5000, 5000]
    assert edges_to_csr(src, dst, 2, w, "sum")[3].tolist() == [12502500, 12502500]
    big = np.full(5000, (1 << 31) // 2500, dtype=np.int32)
    assert edges_to_csr(src, dst, 2, big, "max")[3].tolist() == [(1 << 31) // 2500] * 2
    with pytest.raises(ValueError):
        edges_to_csr(src, dst, 2, big, "sum")


@pytest.mark.parametrize("name", sorted(ec.ERRORS))
def test_errors(name):
    src, dst, n, weights, combine = ec.error_arrays(name)
    with pytest.raises(ValueError):
        edges_to_csr(src, dst, n, weights, combine)


def test_sum_overflow_list_is_valid_under_max():
    src, dst, n, weights, _ = ec.error_arrays("sum_overflow")
    assert edges_to_csr(src, dst, n, weights, "max")[3].tolist() == [1 << 30, 1 << 30, 5, 5]


def test_too_many_pairs():
    """2 * pairs >= 2^32 is refused before anything pair-sized is touched."""
    many = np.broadcast_to(np.zeros(1, dtype=np.uint32), (1 << 31,))
    with pytest.raises(ValueError):
        edges_to_csr(many, many, 5)


def test_permutation_invariance():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 300, 4000)
    dst = rng.integers(0, 300, 4000)
    w = rng.integers(1, 8, 4000).astype(np.int32)
    for combine in ("max", "sum"):
        base = edges_to_csr(src, dst, 300, w, combine)
        for seed in (1, 2):
            p = np.random.default_rng(seed).permutation(4000)
            flip = np.random.default_rng(seed + 10).random(4000) < 0.5
            s2 = np.where(flip, dst[p], src[p])
            d2 = np.where(flip, src[p], dst[p])
            again = edges_to_csr(s2, d2, 300, w[p], combine)
            assert again[0] == base[0] and again[4] == base[4]
            for a, b in zip(again[1:4], base[1:4]):
                assert np.array_equal(a, b)


def test_hub_graph_shape():
    src, dst, n = ec.hub_graph()
    _, xadj, adjncy, _, stats = edges_to_csr(src, dst, n)
    deg = np.diff(xadj)
    assert deg[0] == 0 and deg[1] == 3000 and deg[2] == 16 and deg[3] == 17
    nonempty = np.flatnonzero(deg[:100] > 0).tolist()
    assert nonempty == [1, 2, 3, 5, 8, 79]  # gaps of 1, 2 and 70 empty rows
    assert (deg[3100:] == 0).all() and stats["max_degree"] == 3000


def test_graph_from_csr_accepts_the_twin():
    rng = np.random.default_rng(9)
    src = rng.integers(0, 200, 1500)
    dst = rng.integers(0, 200, 1500)
    w = rng.integers(1, 8, 1500).astype(np.int32)
    n, xadj, adjncy, adjwgt, stats = edges_to_csr(src, dst, 200, w, "sum")
    g = ka.Graph.from_csr(xadj, adjncy, None, adjwgt)
    assert g.n == n and g.m == stats["arcs"]
    assert np.array_equal(g.xadj, xadj) and np.array_equal(g.adjncy, adjncy)
    assert np.array_equal(g.adjwgt, adjwgt)
    # symmetric: the arc (v, u) exists with the same weight
    rows = np.repeat(np.arange(n), np.diff(xadj))
    fwd = {(int(r), int(c)): int(x) for r, c, x in zip(rows, adjncy, adjwgt)}
    assert all(fwd[(c, r)] == x for (r, c), x in fwd.items())
    n2, xadj2, adjncy2, none, _ = edges_to_csr(src, dst, 200)
    g2 = ka.Graph.from_csr(xadj2, adjncy2)
    assert none is None and g2.adjwgt is None and g2.m == len(adjncy2)


def test_facade_max_block_weight_matches_the_library():
    """EdgesGraph.max_block_weight against kmp_max_block_weight, bit for bit."""
    from kaminpar_amd.partition import EdgesGraph

    class Engine:
        n, m = 1, 0

    for total in (1, 7, 1000, 12345677, ec.I32_MAX):
        g = ka.Graph.from_csr(np.zeros(2, np.uint32), np.zeros(0, np.uint32),
                              np.array([total], np.int32))
        assert g.total_node_weight == total
        f = EdgesGraph(Engine(), total)
        assert f.downloaded is False
        for k in (1, 2, 3, 7, 16, 1000):
            for eps in (0.0, 0.03, 0.1, 1 / 3):
                assert f.max_block_weight(k, eps) == g.max_block_weight(k, eps)
