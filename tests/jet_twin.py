"""CPU twin of the GPU Jet refiner (kmp_lp_jet).

A from-scratch numpy restatement of the synchronous Jet schedule
(kaminpar-shm/refinement/jet/jet_refiner.cc:94-234 in terms of this engine):
find -> afterburner filter -> execute -> rebalance -> score, with the
best-snapshot / fruitless bookkeeping done in plain double arithmetic.
Rebalancing is the engine's deterministic overload-balancer mode (the oracle's
kmp_oracle_lp_balance), not the reference's priority-queue OverloadBalancer.

Every step is a pure function of a snapshot, so the GPU path is pinned to this
file bit-exactly (labels, cut, iterations, balancer_calls).
"""

import ctypes
import math

import numpy as np

from helpers import i32p, oracle_balance, u32p


def _arrays(g, vwgt, adjwgt):
    xadj = np.ascontiguousarray(g.xadj, dtype=np.int64)
    adjncy = np.ascontiguousarray(g.adjncy, dtype=np.int64)
    n = len(xadj) - 1
    deg = xadj[1:] - xadj[:-1]
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    w = (np.ones(len(adjncy), dtype=np.int64) if adjwgt is None
         else np.asarray(adjwgt, dtype=np.int64))
    vw = (np.ones(n, dtype=np.int64) if vwgt is None
          else np.asarray(vwgt, dtype=np.int64))
    return n, src, adjncy, w, vw


def edge_cut(oracle, g, labels, adjwgt=None):
    """The oracle's edge cut (metrics.cc:37-59 semantics)."""
    oracle.kmp_oracle_edge_cut.restype = ctypes.c_int64
    xadj = np.ascontiguousarray(g.xadj, dtype=np.uint32)
    adjncy = np.ascontiguousarray(g.adjncy, dtype=np.uint32)
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    return int(oracle.kmp_oracle_edge_cut(
        ctypes.c_uint32(g.n), ctypes.c_uint64(g.m), u32p(xadj), u32p(adjncy),
        i32p(adjwgt) if adjwgt is not None else None, u32p(lab)))


def block_weights(labels, vw, k):
    return np.bincount(labels, weights=vw, minlength=k).astype(np.int64)


def find(n, src, dst, w, k, labels, lock, t):
    """Step 1. Returns (cand, nxt, gain): candidate mask, next block, gain."""
    lab = labels.astype(np.int64)
    conn = np.bincount(src * k + lab[dst], weights=w,
                       minlength=n * k).astype(np.int64).reshape(n, k)
    rows = np.arange(n)
    own = conn[rows, lab].copy()
    conn[rows, lab] = 0  # edge weights >= 1: adjacent blocks have conn >= 1
    to = conn.argmax(axis=1)  # first maximum: ties go to the smallest id
    best = conn[rows, to]
    gain = best - own
    # floor(t * own) with the product in double, compared as integers
    thr = -np.floor(np.float64(t) * own.astype(np.float64)).astype(np.int64)
    cand = (~lock) & (best > 0) & (gain > thr)
    nxt = np.where(cand, to, lab)
    gain = np.where(cand, gain, 0)
    return cand, nxt, gain


def afterburner(n, src, dst, w, labels, cand, nxt, gain):
    """Step 2. Returns the new lock array (True = the move is executed)."""
    lab = labels.astype(np.int64)
    ahead = cand[dst] & ((gain[dst] > gain[src])
                         | ((gain[dst] == gain[src]) & (dst < src)))
    assumed = np.where(ahead, nxt[dst], lab[dst])
    contrib = (np.where(assumed == nxt[src], w, 0)
               - np.where(assumed == lab[src], w, 0))
    contrib = np.where(cand[src], contrib, 0)
    total = np.bincount(src, weights=contrib, minlength=n).astype(np.int64)
    return cand & (total > 0)


def jet_iteration(n, src, dst, w, k, labels, lock, t):
    """Steps 1-3 on a snapshot. Returns (labels, lock, nxt, moves)."""
    cand, nxt, gain = find(n, src, dst, w, k, labels, lock, t)
    new_lock = afterburner(n, src, dst, w, labels, cand, nxt, gain)
    out = np.where(new_lock, nxt, labels.astype(np.int64)).astype(np.uint32)
    return out, new_lock, nxt, int(new_lock.sum())


def round_temperature(r, num_rounds, t0, t1):
    if num_rounds > 1:
        return t0 + (r / (num_rounds - 1)) * (t1 - t0)
    return (t0 + t1) / 2.0


def jet(oracle, g, k, max_block_weights, partition, seed=1, vwgt=None,
        adjwgt=None, num_rounds=1, max_iterations=0, max_fruitless=12,
        fruitless_threshold=0.999, initial_gain_temp=0.25,
        final_gain_temp=0.25, balance_iters=1):
    """Returns (cut, partition, stats dict)."""
    n, src, dst, w, vw = _arrays(g, vwgt, adjwgt)
    caps = np.ascontiguousarray(max_block_weights, dtype=np.int64)
    vwgt32 = None if vwgt is None else np.ascontiguousarray(vwgt, dtype=np.int32)
    adjwgt32 = None if adjwgt is None else np.ascontiguousarray(adjwgt, dtype=np.int32)

    labels = np.ascontiguousarray(partition, dtype=np.uint32).copy()
    lock = np.zeros(n, dtype=bool)
    best = labels.copy()
    best_cut = edge_cut(oracle, g, labels, adjwgt32)
    best_f = bool((block_weights(labels, vw, k) <= caps).all())
    stats = {"iterations": 0, "balancer_calls": 0, "jet_moves": 0,
             "balancer_moves": 0, "rollbacks": 0}
    git = 0  # global iteration counter across rounds (balancer seed offset)

    for r in range(num_rounds):
        t = round_temperature(r, num_rounds, initial_gain_temp, final_gain_temp)
        iters = 0
        fruitless = 0
        cur_is_best = True
        while True:
            labels, lock, _, moved = jet_iteration(n, src, dst, w, k, labels, lock, t)
            stats["jet_moves"] += moved
            if (block_weights(labels, vw, k) > caps).any():
                _, labels, bst = oracle_balance(
                    oracle, g, k, caps, labels, seed=seed + git,
                    iters=balance_iters, vwgt=vwgt32, adjwgt=adjwgt32)
                stats["balancer_calls"] += 1
                stats["balancer_moves"] += int(bst[1])
            c = edge_cut(oracle, g, labels, adjwgt32)
            f = bool((block_weights(labels, vw, k) <= caps).all())
            git += 1
            iters += 1
            stats["iterations"] += 1

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
