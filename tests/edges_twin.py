"""Numpy twin of kmp_lp_create_from_edges (rule: include/kaminpar_lp.h,
"engines from edge lists"): an unsorted, possibly repeated, possibly
one-directional list of pairs becomes the canonical CSR of the undirected
simple graph. A restatement of the rule with lexsort, run heads, reduceat and
bincount; it shares nothing with the device code."""

import numpy as np

STAT_FIELDS = ("pairs", "self_loops", "arcs", "merged_arcs", "n", "isolated",
               "max_degree")


def edges_to_csr(src, dst, n=None, weights=None, combine="max"):
    """Returns (n, xadj, adjncy, adjwgt or None, stats); raises ValueError
    where the device call returns NULL."""
    if combine not in ("max", "sum"):
        raise ValueError("combine")
    pairs = len(src)
    if len(dst) != pairs:
        raise ValueError("src and dst differ in length")
    if 2 * pairs >= 1 << 32:  # before anything pair-sized is touched
        raise ValueError("2 * pairs must stay below 2^32")
    src = np.asarray(src).astype(np.int64).ravel()
    dst = np.asarray(dst).astype(np.int64).ravel()
    if not n:
        if pairs == 0:
            raise ValueError("n = 0 and no pairs")
        n = None
    if pairs and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= 1 << 32):
        raise ValueError("an id is negative or >= 2^32")
    if n is None:
        n = int(max(src.max(), dst.max())) + 1
        if n >= 1 << 32:
            raise ValueError("inferred n does not fit 32 bits")
    elif pairs and max(src.max(), dst.max()) >= n:
        raise ValueError("an id is not below n")
    w = None
    if weights is not None:
        w = np.asarray(weights).astype(np.int64).ravel()
        if len(w) != pairs:
            raise ValueError("weights differ in length")
        if pairs and w.min() <= 0:
            raise ValueError("a weight is <= 0")

    keep = src != dst
    self_loops = int(pairs - keep.sum())
    u, v = src[keep], dst[keep]
    row = np.concatenate([u, v])
    col = np.concatenate([v, u])
    order = np.lexsort((col, row))  # by row, then by col
    row, col = row[order], col[order]
    head = np.ones(len(row), dtype=bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    starts = np.flatnonzero(head)
    adjncy = col[starts].astype(np.uint32)
    rows = row[starts]
    adjwgt = None
    if w is not None and pairs > 0:
        ww = np.concatenate([w[keep], w[keep]])[order]
        if len(starts):
            red = np.maximum.reduceat(ww, starts) if combine == "max" else np.add.reduceat(ww, starts)
        else:
            red = np.zeros(0, dtype=np.int64)
        if len(red) and red.max() > (1 << 31) - 1:
            raise ValueError("a sum exceeds 2^31 - 1")
        adjwgt = red.astype(np.int32)
    deg = np.bincount(rows, minlength=n).astype(np.int64)
    xadj = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=xadj[1:])
    arcs = len(adjncy)
    stats = {
        "pairs": pairs,
        "self_loops": self_loops,
        "arcs": arcs,
        "merged_arcs": 2 * (pairs - self_loops) - arcs,
        "n": n,
        "isolated": int((deg == 0).sum()),
        "max_degree": int(deg.max()) if n else 0,
    }
    return n, xadj, adjncy, adjwgt, stats
