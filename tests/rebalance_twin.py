"""CPU twin of the GPU selection rebalancer (kmp_lp_rebalance).

A from-scratch numpy restatement of the rule in include/kaminpar_lp.h: the
reference's OverloadBalancer (refinement/balancer/overload_balancer.cc:162-271,
ordered by refinement/balancer/relative_gain.h) as fixed-shape passes over a
snapshot -- score, order, prefix-select, order, prefix-admit, apply. Every
pass is a pure function of (labels, block weights, caps, pass index), all in
integers, so the GPU path is pinned to this file bit-exactly (labels, cut,
passes, selected, moves, arcs).

jet() is jet_twin.jet with this rebalancer as its step 4 (balancer == 1).
"""

import numpy as np

import jet_twin
from jet_twin import block_weights, edge_cut, jet_iteration, round_temperature

KEY_SHIFT = 20
KEY_CAP = (1 << 31) - 1


def splitmix64(x):
    """lp_common.h's splitmix64 on a uint64 array."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def relative_key(gain, w):
    """Fixed-point compute_relative_gain: gain * w for positive gains (capped),
    gain / w otherwise; 20 fractional bits, truncating division."""
    gain = np.asarray(gain, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    pos = np.minimum(gain * w, KEY_CAP) << KEY_SHIFT
    neg = -(((-gain) << KEY_SHIFT) // np.maximum(w, 1))  # -gain >= 0: floor = trunc
    return np.where(gain > 0, pos, neg)


def tables(W, caps):
    over = W - caps
    room = caps - W
    cum = np.cumsum(np.maximum(room, 0))
    return over, room, cum, int(cum[-1]), int(np.argmax(room))  # first maximum


def score(n, src, dst, w, vw, k, labels, W, caps, p):
    """Returns (cand, to, key, arcs): candidate mask, target, key per vertex
    and the arcs of the scored vertices."""
    lab = labels.astype(np.int64)
    over, room, cum, R, tstar = tables(W, caps)
    scored = (over[lab] > 0) & (vw >= 1)
    arcs = int(scored[src].sum())
    rows = np.arange(n)
    conn = np.bincount(src * k + lab[dst], weights=w,
                       minlength=n * k).astype(np.int64).reshape(n, k)
    own = conn[rows, lab]
    elig = room[None, :] >= vw[:, None]
    elig[rows, lab] = False
    conn_e = np.where(elig, conn, 0)
    to1 = conn_e.argmax(axis=1)  # first maximum: ties go to the smallest id
    best = conn_e[rows, to1]
    adjacent = best > 0

    to = np.full(n, -1, dtype=np.int64)
    if R > 0:
        r = splitmix64((np.uint64(p) << np.uint64(32)) | rows.astype(np.uint64)) % np.uint64(R)
        b = np.searchsorted(cum, r.astype(np.int64), side="right")  # first cum[b] > r
        to = np.where(room[b] >= vw, b, to)
    to = np.where((to < 0) & (room[tstar] >= vw), tstar, to)
    to = np.where(adjacent, to1, to)

    cand = scored & (to >= 0)
    gain = np.where(adjacent, best, 0) - own
    return cand, to, relative_key(gain, vw), arcs


def segment_prefix(seg, wt):
    """Inclusive prefix sums of wt within runs of equal seg."""
    cs = np.cumsum(wt)
    start = np.r_[True, seg[1:] != seg[:-1]]
    base = np.maximum.accumulate(np.where(start, cs - wt, 0))
    return cs - base


def rebalance_pass(n, src, dst, w, vw, k, labels, caps, p):
    """One pass. Returns (labels, sources, selected, moves, arcs); sources is
    False iff no block was over its cap (the pass did not run)."""
    lab = labels.astype(np.int64)
    W = block_weights(labels, vw, k)
    over, room, _, _, _ = tables(W, caps)
    if not (over > 0).any():
        return labels, False, 0, 0, 0
    cand, to, key, arcs = score(n, src, dst, w, vw, k, labels, W, caps, p)
    ids = np.flatnonzero(cand)
    if len(ids) == 0:
        return labels, True, 0, 0, arcs
    # select: (block, key desc, id asc), exclusive prefix below the overload
    order = ids[np.lexsort((ids, -key[ids], lab[ids]))]
    blk = lab[order]
    excl = segment_prefix(blk, vw[order]) - vw[order]
    sel = order[excl < over[blk]]
    # admit: (target, key desc, id asc), inclusive prefix within the room
    order = sel[np.lexsort((sel, -key[sel], to[sel]))]
    tgt = to[order]
    incl = segment_prefix(tgt, vw[order])
    adm = order[incl <= room[tgt]]
    out = labels.copy()
    out[adm] = to[adm].astype(labels.dtype)
    return out, True, len(sel), len(adm), arcs


def rebalance_arrays(n, src, dst, w, vw, k, caps, labels, max_passes):
    stats = {"passes": 0, "selected": 0, "moves": 0, "arcs": 0}
    for p in range(max_passes):
        labels, sources, sel, adm, arcs = rebalance_pass(n, src, dst, w, vw, k, labels, caps, p)
        if not sources:
            break
        stats["passes"] += 1
        stats["selected"] += sel
        stats["moves"] += adm
        stats["arcs"] += arcs
        if adm == 0:  # stalled
            break
    stats["feasible"] = bool((block_weights(labels, vw, k) <= caps).all())
    return labels, stats


def rebalance(g, k, max_block_weights, partition, max_passes=16, vwgt=None, adjwgt=None):
    """Returns (partition, stats dict: passes, selected, moves, arcs, feasible)."""
    n, src, dst, w, vw = jet_twin._arrays(g, vwgt, adjwgt)
    caps = np.ascontiguousarray(max_block_weights, dtype=np.int64)
    labels = np.ascontiguousarray(partition, dtype=np.uint32).copy()
    return rebalance_arrays(n, src, dst, w, vw, k, caps, labels, max_passes)


def jet(oracle, g, k, max_block_weights, partition, vwgt=None, adjwgt=None, num_rounds=1,
        max_iterations=0, max_fruitless=12, fruitless_threshold=0.999,
        initial_gain_temp=0.25, final_gain_temp=0.25, balance_passes=16):
    """jet_twin.jet with the selection rebalancer as its rebalance step.
    Returns (cut, partition, stats dict)."""
    n, src, dst, w, vw = jet_twin._arrays(g, vwgt, adjwgt)
    caps = np.ascontiguousarray(max_block_weights, dtype=np.int64)
    adjwgt32 = None if adjwgt is None else np.ascontiguousarray(adjwgt, dtype=np.int32)

    labels = np.ascontiguousarray(partition, dtype=np.uint32).copy()
    lock = np.zeros(n, dtype=bool)
    best = labels.copy()
    best_cut = edge_cut(oracle, g, labels, adjwgt32)
    best_f = bool((block_weights(labels, vw, k) <= caps).all())
    stats = {"iterations": 0, "balancer_calls": 0, "jet_moves": 0,
             "balancer_moves": 0, "rollbacks": 0, "feasible_iterations": 0}

    for r in range(num_rounds):
        t = round_temperature(r, num_rounds, initial_gain_temp, final_gain_temp)
        iters = 0
        fruitless = 0
        cur_is_best = True
        while True:
            labels, lock, _, moved = jet_iteration(n, src, dst, w, k, labels, lock, t)
            stats["jet_moves"] += moved
            if (block_weights(labels, vw, k) > caps).any():
                labels, rst = rebalance_arrays(n, src, dst, w, vw, k, caps, labels,
                                               balance_passes)
                stats["balancer_calls"] += 1
                stats["balancer_moves"] += rst["moves"]
            c = edge_cut(oracle, g, labels, adjwgt32)
            f = bool((block_weights(labels, vw, k) <= caps).all())
            iters += 1
            stats["iterations"] += 1
            stats["feasible_iterations"] += int(f)

            gained = f and not best_f
            fruitless += 1
            if gained or (f == best_f and
                          float(best_cut - c) > (1.0 - fruitless_threshold) * float(best_cut)):
                fruitless = 0
            if gained or (f == best_f and c <= best_cut):
                best = labels.copy()
                cur_is_best = True
            else:
                cur_is_best = False
            if gained:
                best_cut = c
                best_f = True
            elif f == best_f:
                best_cut = min(best_cut, c)
            if (max_iterations and iters == max_iterations) or \
               (max_fruitless and fruitless == max_fruitless):
                break
        if not cur_is_best:
            labels = best.copy()
            stats["rollbacks"] += 1
    return best_cut, best, stats
