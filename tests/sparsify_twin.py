"""numpy twin of the threshold edge sparsification of a coarse graph
(kmp_contract_engine_sparsified; rule in include/kaminpar_lp.h). Exact in
integers, so the device result equals this one bit for bit."""

import numpy as np

DEFAULT_PARAMS = dict(density_target_factor=0.5, edge_target_factor=0.5,
                      laziness_factor=4.0)

_U64 = np.uint64


def fmix64(x):
    """The 64-bit Murmur3 finalizer on a uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=_U64).copy()
    x ^= x >> _U64(33)
    x *= _U64(0xFF51AFD7ED558CCD)
    x ^= x >> _U64(33)
    x *= _U64(0xC4CEB9FE1A85EC53)
    x ^= x >> _U64(33)
    return x


def dice(u, v, seed):
    """h(u, v): the low 32 bits of fmix64(((max << 32) | min) + seed)."""
    u = np.asarray(u, dtype=_U64)
    v = np.asarray(v, dtype=_U64)
    key = (np.maximum(u, v) << _U64(32)) | np.minimum(u, v)
    with np.errstate(over="ignore"):
        return fmix64(key + _U64(int(seed) & 0xFFFFFFFFFFFFFFFF)) & _U64(0xFFFFFFFF)


def sparsify_target(old_n, old_m, c_n, params):
    want = min(params["edge_target_factor"] * old_m,
               params["density_target_factor"] * old_m / old_n * c_n)
    return int(want) if want < old_m else int(old_m)


def sparsify(xadj, adjncy, adjwgt, old_n, old_m, params=None, seed=0):
    """Returns (xadj, adjncy, adjwgt, stats). Not triggered: the input arrays
    themselves come back. stats: applied, m_before, m_after, target,
    threshold, larger, equal, include."""
    p = dict(DEFAULT_PARAMS)
    p.update(params or {})
    c_n, c_m = len(xadj) - 1, len(adjncy)
    stats = dict(applied=0, m_before=c_m, m_after=c_m, target=0, threshold=0,
                 larger=0, equal=0, include=0)
    if c_m == 0:
        return xadj, adjncy, adjwgt, stats
    target = sparsify_target(old_n, old_m, c_n, p)
    stats["target"] = target
    if not (float(c_m) > p["laziness_factor"] * float(target)) or c_m <= target:
        return xadj, adjncy, adjwgt, stats
    stats["applied"] = 1
    w = np.asarray(adjwgt, dtype=np.int64)
    if target < 2:
        keep = np.zeros(c_m, dtype=bool)
    else:
        T = int(np.partition(w, c_m - target)[c_m - target])
        larger = int((w > T).sum())
        equal = int((w == T).sum())
        include = target - larger
        src = np.repeat(np.arange(c_n, dtype=np.uint64),
                        np.diff(np.asarray(xadj, dtype=np.int64)))
        h = dice(src, adjncy, seed)
        keep = (w > T) | ((w == T) & (h * _U64(equal) < _U64(include << 32)))
        stats.update(threshold=T, larger=larger, equal=equal, include=include)
    rows = np.repeat(np.arange(c_n), np.diff(np.asarray(xadj, dtype=np.int64)))
    new_xadj = np.zeros(c_n + 1, dtype=np.asarray(xadj).dtype)
    new_xadj[1:] = np.cumsum(np.bincount(rows[keep], minlength=c_n))
    stats["m_after"] = int(keep.sum())
    return (new_xadj, np.asarray(adjncy)[keep].copy(), np.asarray(adjwgt)[keep].copy(),
            stats)
