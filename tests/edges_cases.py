"""Hand-computed cases of the edge-list rule (include/kaminpar_lp.h, "engines
from edge lists"), shared by the twin's CPU tests and the GPU tests. Every
expected CSR below was worked out by hand from the rule, not produced by the
twin or the device."""

import numpy as np

I32_MAX = (1 << 31) - 1

# name -> (src, dst, n or None, weights or None, combine,
#          expected (n, xadj, adjncy, adjwgt or None, self_loops))
TRIANGLE = (3, [0, 2, 4, 6], [1, 2, 0, 2, 0, 1], None, 0)
CASES = {
    "triangle_one_direction": (
        [0, 1, 2], [1, 2, 0], 3, None, "max", TRIANGLE),
    "triangle_both_directions": (
        [0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2], 3, None, "max", TRIANGLE),
    "triangle_with_repeats": (
        [0, 0, 1, 2, 0, 1, 0], [1, 1, 2, 0, 2, 0, 1], 3, None, "max", TRIANGLE),
    # (0,1) carries 3, 5 (given as (1,0)) and 2; (1,2) carries 4
    "weights_max": (
        [0, 1, 0, 1], [1, 0, 1, 2], 3, [3, 5, 2, 4], "max",
        (3, [0, 1, 3, 4], [1, 0, 2, 1], [5, 5, 4, 4], 0)),
    "weights_sum": (
        [0, 1, 0, 1], [1, 0, 1, 2], 3, [3, 5, 2, 4], "sum",
        (3, [0, 1, 3, 4], [1, 0, 2, 1], [10, 10, 4, 4], 0)),
    "self_loops_only": (
        [0, 2, 2], [0, 2, 2], 3, None, "max",
        (3, [0, 0, 0, 0], [], None, 3)),
    "self_loops_only_inferred_n": (
        [0, 2, 2], [0, 2, 2], None, None, "max",
        (3, [0, 0, 0, 0], [], None, 3)),
    # isolated: 0, the run 3 4 5, and n - 1 = 7
    "isolated_ends_and_run": (
        [2, 6], [1, 2], 8, None, "max",
        (8, [0, 0, 1, 3, 3, 3, 3, 4, 4], [2, 1, 6, 2], None, 0)),
    "inferred_n": (
        [5, 1], [1, 3], None, None, "max",
        (6, [0, 0, 2, 2, 3, 3, 4], [3, 5, 1, 1], None, 0)),
    "loop_among_edges_weighted": (
        [1, 1, 0], [1, 0, 1], 2, [9, 2, 7], "sum",
        (2, [0, 1, 2], [1, 0], [9, 9], 1)),
}

# name -> (src, dst, n or None, weights or None, combine, id dtype)
ERRORS = {
    "id_equals_n": ([0, 3], [1, 2], 3, None, "max", np.uint32),
    "id_above_n_64": ([0, 1], [1, 7], 3, None, "max", np.int64),
    "negative_id": ([0, -1], [1, 2], 3, None, "max", np.int64),
    "negative_id_inferred_n": ([0, -1], [1, 2], None, None, "max", np.int64),
    "negative_id_32": ([0, 2], [1, -2], 3, None, "max", np.int32),
    "id_2_pow_32": ([0, 1 << 32], [1, 2], None, None, "max", np.int64),
    "weight_zero": ([0, 1], [1, 2], 3, [4, 0], "max", np.uint32),
    "weight_negative": ([0, 1], [1, 2], 3, [-2, 4], "sum", np.uint32),
    # 2^30 + 2^30 = 2^31 > 2^31 - 1 (the same list is valid under "max")
    "sum_overflow": ([0, 1, 1], [1, 0, 2], 3, [1 << 30, 1 << 30, 5], "sum", np.uint32),
    "no_n_no_pairs": ([], [], None, None, "max", np.uint32),
}


def case_arrays(name, dtype=np.int64):
    src, dst, n, weights, combine, want = CASES[name]
    return (np.array(src, dtype=dtype), np.array(dst, dtype=dtype), n,
            None if weights is None else np.array(weights, dtype=np.int32), combine, want)


def error_arrays(name):
    src, dst, n, weights, combine, dtype = ERRORS[name]
    return (np.array(src, dtype=dtype), np.array(dst, dtype=dtype), n,
            None if weights is None else np.array(weights, dtype=np.int32), combine)


def long_run(count=5000):
    """One edge (0, 1) repeated `count` times in mixed orientation with the
    weights 1 .. count: a run of duplicates longer than a workgroup tile.
    Max gives count, sum count * (count + 1) / 2."""
    i = np.arange(count)
    flip = (i % 3) == 1
    src = np.where(flip, 1, 0).astype(np.int64)
    dst = np.where(flip, 0, 1).astype(np.int64)
    return src, dst, (i + 1).astype(np.int32)


def hub_graph():
    """n = 3200: row 0 empty; a hub (vertex 1) of degree 3000 over the
    vertices 100 .. 3099; vertex 2 of degree 16 and vertex 3 of degree 17 next
    to it; then gaps of 1, 2 and 70 empty rows between non-empty ones (4 |
    5 | 6 7 | 8 | 9 .. 78 | 79), and an empty tail 3100 .. 3199. Returns
    (src, dst, n), one direction per edge."""
    src = [np.full(3000, 1), np.full(16, 2), np.full(17, 3)]
    dst = [np.arange(100, 3100), np.arange(100, 116), np.arange(200, 217)]
    # 5, 8 and 79 get one edge each into the hub's range; 4, 6, 7, 9..78 stay
    # empty: gaps of 1 (4), 2 (6, 7) and 70 (9 .. 78) rows
    src.append(np.array([5, 8, 79]))
    dst.append(np.array([300, 301, 302]))
    return (np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64), 3200)
