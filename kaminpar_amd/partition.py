"""Multilevel k-way partitioning pipeline (BASELINE config 3).

Mirrors the reference's multilevel scheme (coarsen -> initial partition ->
uncoarsen+refine, kaminpar-shm/partitioning/): GPU LP clustering + GPU
contraction per level, CPU initial partitioning on the coarsest graph, GPU
LP refinement at every level.

Initial partitioning restates the reference's recipe in simplified form
(kaminpar-shm/initial_partitioning/): recursive bisection where each
bisection is greedy graph growing (initial_ggg_bipartitioner.cc) polished by
two-way FM (initial_two_way_fm_refiner.cc: best-prefix rollback, 100
fruitless moves, 5 passes), followed by a gain-aware overload balancer
(refinement/balancer/overload_balancer.cc in spirit). It is NOT claimed
bit-parity with the reference's initial-partitioner pool (which races many
repetitions); quality is validated end-to-end against the compiled
reference's full pipeline within a band (tests/golden/ref_golden_partition.json).

Cluster-weight rule per level: the reference's EPSILON_BLOCK_WEIGHT formula
(coarsening/max_cluster_weights.h:18-46) capped by its BLOCK_WEIGHT rule
with multiplier 1/12 (presets.cc: initial_partitioning.coarsening
.cluster_weight_limit = BLOCK_WEIGHT, multiplier = 1/12) so coarse vertices
stay small enough relative to the block capacity for a feasible initial
assignment -- without the cap, deep coarsening produces vertices weighing
~25% of a block, which makes balanced bin-packing infeasible.
"""

import os

import numpy as np

from . import LpEngine


def _subgraph_csr(xadj, adjncy, adjwgt, nodes, loc):
    """Extract local CSR of the induced subgraph (local vertex ids)."""
    rows_j = []
    rows_w = []
    sub_xadj = np.zeros(len(nodes) + 1, dtype=np.int64)
    for i, u in enumerate(nodes):
        e0, e1 = int(xadj[u]), int(xadj[u + 1])
        j = loc[adjncy[e0:e1]]
        sel = j >= 0
        rows_j.append(j[sel])
        if adjwgt is not None:
            rows_w.append(adjwgt[e0:e1][sel].astype(np.int64))
        sub_xadj[i + 1] = sub_xadj[i] + int(sel.sum())
    sub_adj = np.concatenate(rows_j) if rows_j else np.zeros(0, np.int64)
    if adjwgt is not None:
        sub_w = np.concatenate(rows_w) if rows_w else np.zeros(0, np.int64)
    else:
        sub_w = np.ones(len(sub_adj), dtype=np.int64)
    return sub_xadj, sub_adj, sub_w


def _fm_refine_bisection(sub_xadj, sub_adj, sub_w, vw, side, cap1, cap2,
                         max_passes=5, max_fruitless=100):
    """Two-way FM with best-prefix rollback on a bisection (side=True is
    part 1). Restates initial_two_way_fm_refiner.cc's schedule in simplified
    form: repeated passes, each greedily moving the best-gain movable vertex
    (ties: smallest id), locking it, tracking the best prefix."""
    n = len(side)
    w1 = int(vw[side].sum())
    w2 = int(vw.sum()) - w1
    for _ in range(max_passes):
        # gains from scratch: external - internal connection
        gains = np.zeros(n, dtype=np.int64)
        for i in range(n):
            e0, e1 = int(sub_xadj[i]), int(sub_xadj[i + 1])
            nb = sub_adj[e0:e1]
            w = sub_w[e0:e1]
            cross = side[nb] != side[i]
            gains[i] = int(w[cross].sum()) - int(w[~cross].sum())
        locked = np.zeros(n, dtype=bool)
        moves = []
        cum = best = 0
        best_len = 0
        fruitless = 0
        wa, wb = w1, w2
        while fruitless < max_fruitless:
            feas = (~locked) & (
                (side & (wb + vw <= cap2)) | (~side & (wa + vw <= cap1))
            )
            if not feas.any():
                break
            masked = np.where(feas, gains, np.iinfo(np.int64).min)
            i = int(np.argmax(masked))  # first occurrence = smallest id
            cum += int(gains[i])
            old = bool(side[i])
            e0, e1 = int(sub_xadj[i]), int(sub_xadj[i + 1])
            nb = sub_adj[e0:e1]
            w = sub_w[e0:e1]
            upd = ~locked[nb]
            same = side[nb[upd]] == old
            delta = np.where(same, 2 * w[upd], -2 * w[upd])
            np.add.at(gains, nb[upd], delta)
            gains[i] = -gains[i]
            side[i] = not old
            locked[i] = True
            if old:
                wa -= int(vw[i]); wb += int(vw[i])
            else:
                wa += int(vw[i]); wb -= int(vw[i])
            moves.append(i)
            if cum > best:
                best = cum
                best_len = len(moves)
                fruitless = 0
            else:
                fruitless += 1
        # rollback past the best prefix
        for i in moves[best_len:]:
            side[i] = not side[i]
        w1 = int(vw[side].sum())
        w2 = int(vw.sum()) - w1
        if best <= 0:
            break
    return side


def _greedy_grow(sub_xadj, sub_adj, sub_w, vw, target1, cap1, seed_rank=0):
    """Greedy graph growing: grow part 1 from a high-degree seed (the
    seed_rank-th vertex in descending-degree order -- repetitions use
    different seeds, like the reference's bipartitioner pool), absorbing
    the frontier vertex with the highest connection (ties: smallest id)."""
    n = len(vw)
    deg = np.diff(sub_xadj)
    order = np.lexsort((np.arange(n), -deg))
    seed_idx = int(order[seed_rank % n])

    side = np.zeros(n, dtype=bool)
    gain = np.full(n, -1, dtype=np.int64)  # -1 not frontier, -2 blocked/in
    w1 = 0

    def add(i):
        nonlocal w1
        side[i] = True
        w1 += int(vw[i])
        gain[i] = -2
        e0, e1 = int(sub_xadj[i]), int(sub_xadj[i + 1])
        j = sub_adj[e0:e1]
        keep = ~side[j] & (gain[j] != -2)
        j2 = j[keep]
        if len(j2) == 0:
            return
        gain[j2[gain[j2] < 0]] = 0
        np.add.at(gain, j2, sub_w[e0:e1][keep])

    add(seed_idx)
    while w1 < target1:
        cand = np.flatnonzero(gain >= 0)
        if len(cand) == 0:
            rest = np.flatnonzero(~side & (gain != -2))
            if len(rest) == 0:
                break
            nxt = int(rest[0])  # disconnected: smallest id outside
        else:
            best = cand[gain[cand] == gain[cand].max()]
            nxt = int(best[0])
        if w1 + int(vw[nxt]) > cap1:
            gain[nxt] = -2
            continue
        add(nxt)
    return side


def _balance(xadj, adjncy, adjwgt, vwgt, part, k, cap):
    """Gain-aware overload balancer: while a block exceeds cap, move the
    best vertex out of the most overloaded block -- preferring the
    max-gain feasible move, else any move that strictly lowers the
    overloaded block below the target's new weight (monotone, terminates)."""
    n = len(part)
    vw = vwgt if vwgt is not None else np.ones(n, dtype=np.int64)
    bw = np.zeros(k, dtype=np.int64)
    np.add.at(bw, part, vw)
    guard = 8 * (k + 16)
    while bw.max() > cap and guard > 0:
        guard -= 1
        b = int(np.argmax(bw))
        vs = np.flatnonzero(part == b)
        best_feas = None   # (gain, -weight, v, t)
        best_force = None  # (new_target_weight, v, t)
        for v in vs:
            e0, e1 = int(xadj[v]), int(xadj[v + 1])
            nb = part[adjncy[e0:e1]]
            w = adjwgt[e0:e1] if adjwgt is not None else np.ones(e1 - e0, np.int64)
            conn = np.zeros(k, dtype=np.int64)
            np.add.at(conn, nb, w)
            internal = int(conn[b])
            for t in range(k):
                if t == b:
                    continue
                nw = int(bw[t]) + int(vw[v])
                g = int(conn[t]) - internal
                if nw <= cap:
                    key = (g, -int(vw[v]), -v, t)
                    if best_feas is None or key > best_feas[:4]:
                        best_feas = (g, -int(vw[v]), -v, t, v)
                elif nw < int(bw[b]):
                    key = (-nw, g, -v)
                    if best_force is None or key > best_force[:3]:
                        best_force = (-nw, g, -v, t, v)
        if best_feas is not None:
            t, v = best_feas[3], best_feas[4]
        elif best_force is not None:
            t, v = best_force[3], best_force[4]
        else:
            break
        part[v] = t
        bw[b] -= int(vw[v])
        bw[t] += int(vw[v])
    return part


def initial_partition(g, k, max_block_weight, seed=1, reps=8):
    """Recursive bisection into k blocks on the (small) coarsest graph:
    per bisection, `reps` greedy-graph-growing attempts from different
    high-degree seeds, each polished by two-way FM, best cut kept
    (restates the reference's bipartitioner-pool repetition idea,
    initial_partitioning with min_num_non_adaptive_repetitions=5); then a
    k-way overload balancer."""
    xadj = np.asarray(g.xadj).astype(np.int64)
    adjncy = np.asarray(g.adjncy).astype(np.int64)
    from . import _lib

    vwgt = None
    vw_p = _lib.kmp_graph_vwgt(g._h)
    if vw_p:
        vwgt = np.ctypeslib.as_array(vw_p, shape=(g.n,)).astype(np.int64)
    adjwgt = None
    aw_p = _lib.kmp_graph_adjwgt(g._h)
    if aw_p:
        adjwgt = np.ctypeslib.as_array(aw_p, shape=(g.m,)).astype(np.int64)
    vwgt_all = vwgt if vwgt is not None else np.ones(g.n, dtype=np.int64)

    part = np.zeros(g.n, dtype=np.uint32)
    loc = np.full(g.n, -1, dtype=np.int64)

    def rec(nodes, k_lo, k_hi):
        if len(nodes) == 0:
            return
        if k_hi - k_lo == 1:
            part[nodes] = k_lo
            return
        k1 = (k_hi - k_lo + 1) // 2
        k2 = (k_hi - k_lo) - k1
        total = int(vwgt_all[nodes].sum())
        target1 = total * k1 // (k1 + k2)
        cap1 = k1 * max_block_weight
        cap2 = k2 * max_block_weight

        loc[nodes] = np.arange(len(nodes))
        sub_xadj, sub_adj, sub_w = _subgraph_csr(xadj, adjncy, adjwgt, nodes, loc)
        loc[nodes] = -1
        vw = vwgt_all[nodes]

        def bisection_cut(s):
            u = np.repeat(np.arange(len(nodes)), np.diff(sub_xadj))
            return int(sub_w[s[u] != s[sub_adj]].sum())

        best_side = None
        best_cut = None
        for rep in range(reps):
            side = _greedy_grow(sub_xadj, sub_adj, sub_w, vw, target1, cap1,
                                seed_rank=rep)
            side = _fm_refine_bisection(sub_xadj, sub_adj, sub_w, vw, side,
                                        cap1, cap2)
            c = bisection_cut(side)
            if best_cut is None or c < best_cut:
                best_cut = c
                best_side = side
        rec(nodes[best_side], k_lo, k_lo + k1)
        rec(nodes[~best_side], k_lo + k1, k_hi)

    rec(np.arange(g.n), 0, k)
    part = _balance(xadj, adjncy, adjwgt, vwgt, part, k, max_block_weight)
    return part


def level_cluster_weight(total_w, n, k, eps, contraction_limit=2000):
    """Per-level max cluster weight: the reference's EPSILON_BLOCK_WEIGHT
    formula (max_cluster_weights.h:18-46) capped by the BLOCK_WEIGHT rule
    with the reference's IP multiplier 1/12 (presets.cc)."""
    shrink = min(max(n // contraction_limit, 2), k)
    eps_rule = int(eps * total_w / shrink)
    block_rule = total_w // (12 * k)
    return max(1, min(eps_rule, block_rule) if block_rule > 0 else eps_rule)


def _level_stats(stats, engines):
    """Fills the drivers' `stats` out-parameter from the bottom-up chain."""
    if stats is None:
        return
    stats["level_arcs"] = [int(e.m) for e in engines]
    stats["sparsify"] = [
        None if e.sparsify_stats is None else e.sparsify_stats.as_dict()
        for e in engines[1:]]


def partition(g, k, eps=0.03, seed=1, iters=5, contraction_limit=2000,
              stop_n=512, engine=None, return_arcs=False, jet=False, fm=None,
              resident=False, vcycles=0, sparsify=False, stats=None):
    """Full multilevel partition on the GPU engine.

    `engine` reuses an existing LpEngine for the fine graph (keeps the
    fine CSR resident in HBM across repeated runs, e.g. in bench.py).
    Returns (cut, partition, level_sizes); with return_arcs also the LP
    arcs scanned and phase-A kernel nanoseconds summed over all levels.

    `jet=True` runs the GPU Jet refiner (LpEngine.jet, reference defaults:
    gain temperature 0.75 on coarse levels, 0.25 on the finest) after LP at
    every level and before the optional FM; a dict instead of True passes
    parameter overrides (e.g. {"balance_iters": 2}). `fm` overrides the size
    rule for the per-level CPU FM (None: on up to 2^21 fine vertices).

    `resident=True` keeps every label-shaped array on the device between the
    stages: clusterings and mappings never reach the host, the partition is
    uploaded once on the coarsest engine (LpEngine.set_labels), refined in
    place, projected level to level on the device (LpEngine.project_from) and
    downloaded once at the end; only the CPU FM, where it runs, brackets itself
    with get_labels / set_labels. Same result as resident=False.

    `vcycles=N` runs N V-cycles (vcycle()) on the result, with this call's
    jet / fm / resident and the level-0 engine reused: cycle c has seed
    seed + c and starts from the output of cycle c - 1. The returned cut and
    partition are the last cycle's; the level sizes stay those of the
    bottom-up pass.

    `sparsify=True`, or a dict of overrides of kaminpar_amd.sparsify_params(),
    runs the threshold edge sparsification of the coarse graph after every
    contraction of the bottom-up pass (LpEngine.contract_engine(sparsify=...,
    seed=seed + level)); the sparsified graph is what the deeper levels are
    built from. Coarse-level cuts (LP's, Jet's) then refer to the sparsified
    graphs; the level-0 cut that is returned is exact as before. The chains of
    the V-cycles coarsen without it (a cycle compares true level-0 cuts, so
    `vcycles=N` together with `sparsify` is allowed). Off by default.

    `stats`, a dict, receives "level_arcs" (arcs of every level's engine,
    [0] = g.m) and "sparsify" (one dict of kmp_sparsify_stats_t fields per
    contraction that was kept, or None where the pass is off)."""
    if vcycles < 0:
        raise ValueError("vcycles must be >= 0")
    total_w = g.total_node_weight
    mbw_val = g.max_block_weight(k, eps)
    mbw = np.full(k, mbw_val, dtype=np.int64)

    # ---- coarsen (GPU, device-resident chain: the coarse CSR is handed
    # engine-to-engine in HBM; only the mapping comes back to the host) ----
    sizes = [g.n]
    mappings = []
    engines = [engine if engine is not None else LpEngine(g)]
    arcs_total = 0
    ns_total = 0
    while sizes[-1] > max(stop_n, 2 * k):
        cur_n = sizes[-1]
        mcw = level_cluster_weight(total_w, cur_n, k, eps, contraction_limit)
        if resident:
            nc, clus, cst = engines[-1].cluster(mcw, seed=seed + len(mappings),
                                                iters=iters, download=False)
        else:
            nc, clus, cst = engines[-1].cluster(mcw, seed=seed + len(mappings), iters=iters)
        arcs_total += cst.arcs_scanned
        ns_total += cst.phase_a_ns
        if resident:
            coarse_eng, mapping = engines[-1].contract_engine(
                None, download_mapping=False, sparsify=sparsify,
                seed=seed + len(mappings))
        else:
            coarse_eng, mapping = engines[-1].contract_engine(
                clus, sparsify=sparsify, seed=seed + len(mappings))
        if coarse_eng.n > 0.95 * cur_n:
            del coarse_eng
            break
        engines.append(coarse_eng)
        mappings.append(mapping)
        sizes.append(coarse_eng.n)
    _level_stats(stats, engines)

    # ---- initial partition (CPU, coarsest downloaded from HBM; the C++
    # implementation, bit-identical to initial_partition() below) ----
    coarsest = engines[-1].download_graph() if len(engines) > 1 else g
    part = coarsest.initial_partition_native(k, mbw_val)

    # ---- uncoarsen: refine at every level (GPU), plus per-level k-way
    # boundary FM on small graphs (<= ~2M fine vertices; same recipe as
    # partition_deep) ----
    cut = None
    fm_on = g.n <= (1 << 21) if fm is None else bool(fm)
    if resident:
        engines[-1].set_labels(k, part)
        part = None  # on the device until a host step needs it
    for level in range(len(engines) - 1, -1, -1):
        cut, part, rst = engines[level].refine(k, mbw, part, seed=seed, iters=iters)
        arcs_total += rst.arcs_scanned
        ns_total += rst.phase_a_ns
        if jet:
            cut, part, _ = engines[level].jet(
                k, mbw, part, seed=seed, coarse_level=level,
                **(jet if isinstance(jet, dict) else {}))
        if fm_on:
            hg = g if level == 0 else engines[level].download_graph()
            if resident:
                part = engines[level].get_labels()
            part = hg.kway_fm(k, mbw, part)
            if level == 0:
                cut = g.edge_cut(part)
        if resident and level > 0:
            if part is not None:
                engines[level].set_labels(k, part)
                part = None
            engines[level - 1].project_from(engines[level])
        elif level > 0:
            part = part[mappings[level - 1]]
    if vcycles:
        eng0 = engines[0]
        del engines  # the cycles build their own chains
        cut, part = _run_vcycles(g, k, part, eng0, vcycles, eps, seed, iters,
                                 contraction_limit, stop_n, jet, fm, resident)
    elif resident and part is None:
        part = engines[0].get_labels()
    levels = sizes
    if return_arcs:
        return cut, part, levels, int(arcs_total), int(ns_total)
    return cut, part, levels


def vcycle_accept(feasible_in, cut_in, feasible_out, cut_out):
    """The V-cycle's accept rule: a result that differs from its input in
    feasibility is taken iff it is the feasible one; otherwise iff its cut is
    not above the input's."""
    if bool(feasible_in) != bool(feasible_out):
        return bool(feasible_out)
    return cut_out <= cut_in


def _host_cut_feasible(g, part, mbw):
    vw = g.vwgt
    bw = np.bincount(part, weights=vw, minlength=len(mbw))
    return int(g.edge_cut(part)), bool((bw <= mbw).all())


def vcycle(g, k, partition, eps=0.03, seed=1, iters=5, contraction_limit=2000,
           stop_n=512, engine=None, jet=False, fm=None, resident=False,
           download=True):
    """One V-cycle: multilevel refinement of an existing k-way partition.

    Coarsens as partition() does, with the level's partition as the
    clusterer's communities, so no cluster crosses a block boundary and every
    coarse level carries the partition exactly (its cut and block weights are
    the input's); there is no initial partitioning. Uncoarsens as partition()
    does: per level LP refinement, Jet if `jet`, the CPU FM if `fm` says so
    (None: up to 2^21 fine vertices), projection. The result is accepted
    (vcycle_accept) or the input comes back unchanged. Caps are
    max_block_weight(k, eps) for every block.

    `partition` is a host array, or None for the resident partition of
    `engine`. `resident=True` keeps everything label-shaped on the device
    (set_communities_resident / restrict_to / project_from /
    labels_from_communities): a host input costs one set_labels and an
    accepted result one get_labels; only the CPU FM brackets itself with
    copies. `download=False` (resident only) leaves the returned partition on
    the level-0 engine and returns None in its place. Same result as
    resident=False. Jet's limit k <= 2048 applies only with `jet`.

    The level-0 engine's communities are cleared on the way out, so a reused
    engine clusters afterwards as a fresh one does.

    Returns (cut, partition, level_sizes, accepted)."""
    if partition is None and not resident:
        raise ValueError("vcycle(): partition=None needs resident=True")
    if partition is None and engine is None:
        raise ValueError("vcycle(): partition=None needs the engine that holds it")
    if not download and not resident:
        raise ValueError("vcycle(): download=False needs resident=True")
    total_w = g.total_node_weight
    mbw_val = g.max_block_weight(k, eps)
    mbw = np.full(k, mbw_val, dtype=np.int64)
    part_in = None
    if partition is not None:
        part_in = np.ascontiguousarray(partition, dtype=np.uint32)
        if len(part_in) != g.n:
            raise ValueError("vcycle(): need n labels")
        if g.n and int(part_in.max()) >= k:
            raise ValueError("vcycle(): a label is not below k")
    eng0 = engine if engine is not None else LpEngine(g)
    try:
        return _vcycle_body(g, k, part_in, mbw, total_w, eps, seed, iters,
                            contraction_limit, stop_n, eng0, jet, fm, resident,
                            download)
    finally:
        eng0.set_communities(None)


def _vcycle_body(g, k, part_in, mbw, total_w, eps, seed, iters,
                 contraction_limit, stop_n, eng0, jet, fm, resident, download):
    # ---- the input: on the level-0 engine (resident) or on the host ----
    if resident:
        if part_in is not None:
            eng0.set_labels(k, part_in)
        cut_in, feas_in = eng0.resident_cut(k, mbw)
        # kept for the whole cycle: a rejected result is replaced by it
        eng0.set_communities_resident()
        part = None
    else:
        cut_in, feas_in = _host_cut_feasible(g, part_in, mbw)
        part = part_in.copy()

    # ---- coarsen: partition()'s loop with the partition as communities ----
    sizes = [g.n]
    mappings = []
    engines = [eng0]
    while sizes[-1] > max(stop_n, 2 * k):
        cur_n = sizes[-1]
        cur = engines[-1]
        mcw = level_cluster_weight(total_w, cur_n, k, eps, contraction_limit)
        if resident:
            if len(engines) > 1:
                cur.set_communities_resident()
            cur.cluster(mcw, seed=seed + len(mappings), iters=iters,
                        download=False)
            coarse_eng, mapping = cur.contract_engine(
                None, download_mapping=False)
        else:
            cur.set_communities(part)
            _, clus, _ = cur.cluster(mcw, seed=seed + len(mappings),
                                     iters=iters)
            coarse_eng, mapping = cur.contract_engine(clus)
        if coarse_eng.n > 0.95 * cur_n:
            del coarse_eng
            if resident:  # the clustering overwrote this level's partition
                cur.labels_from_communities()
            break
        if resident:
            cur.restrict_to(coarse_eng)
        else:
            coarse_part = np.zeros(coarse_eng.n, dtype=np.uint32)
            coarse_part[mapping] = part
            bad = int((coarse_part[mapping] != part).sum())
            if bad:
                raise RuntimeError(
                    f"vcycle(): {bad} fine vertices share a coarse vertex "
                    "with a vertex of another block")
            part = coarse_part
        engines.append(coarse_eng)
        mappings.append(mapping)
        sizes.append(coarse_eng.n)

    # ---- uncoarsen: partition()'s loop, from the restricted partition ----
    cut = cut_in
    fm_on = g.n <= (1 << 21) if fm is None else bool(fm)
    for level in range(len(engines) - 1, -1, -1):
        cut, part, _ = engines[level].refine(k, mbw, part, seed=seed,
                                             iters=iters)
        if jet:
            cut, part, _ = engines[level].jet(
                k, mbw, part, seed=seed, coarse_level=level,
                **(jet if isinstance(jet, dict) else {}))
        if fm_on:
            hg = g if level == 0 else engines[level].download_graph()
            if resident:
                part = engines[level].get_labels()
            part = hg.kway_fm(k, mbw, part)
        if resident and level > 0:
            if part is not None:
                engines[level].set_labels(k, part)
                part = None
            engines[level - 1].project_from(engines[level])
        elif level > 0:
            part = part[mappings[level - 1]]

    # ---- accept, or hand the input back ----
    if part is None:
        cut, feas = eng0.resident_cut(k, mbw)
    else:
        cut, feas = _host_cut_feasible(g, part, mbw)
    accepted = vcycle_accept(feas_in, cut_in, feas, cut)
    if not accepted:
        cut = cut_in
        if resident:  # level 0 still has the input as its communities
            eng0.labels_from_communities()
            part = None
            if download and part_in is not None:
                part = part_in.copy()
        else:
            part = part_in.copy()
    if resident and download and part is None:
        part = eng0.get_labels()
    elif resident and not download and part is not None:
        eng0.set_labels(k, part)  # the level-0 FM left it on the host
        part = None
    return cut, part, sizes, accepted


def _run_vcycles(g, k, part, eng0, vcycles, eps, seed, iters,
                 contraction_limit, stop_n, jet, fm, resident):
    """The drivers' `vcycles` option: cycle c runs with seed + c on the
    output of cycle c - 1, on the driver's level-0 engine. `part` is the
    driver's result, None where it is resident on eng0. Returns (cut, part)."""
    cut = None
    for c in range(vcycles):
        last = c == vcycles - 1
        cut, part, _, _ = vcycle(
            g, k, part, eps=eps, seed=seed + c, iters=iters,
            contraction_limit=contraction_limit, stop_n=stop_n, engine=eng0,
            jet=jet, fm=fm, resident=resident,
            download=last or not resident)
    return cut, part


def _group_caps(groups, k, mbw_val):
    caps = np.zeros(k, dtype=np.int64)
    for b, w in groups:
        caps[b] = w * mbw_val
    return caps


def _pick_bisector(hg, nodes):
    """Deterministic dispatch of the host bisectors (keep in sync with the C
    twin kmp_extend_partition): pinned O(n^2) bisector <= 128 vertices; above
    that by degree variance (CV^2 >= 1): heavy-tailed subgraphs use flat FM
    (O(n^2) to 4096, then lazy-PQ -- HEM collapses hubs), low-variance
    (geometric/mesh-like) subgraphs use the HEM multilevel bisector, where
    flat FM gets lost (measured: rgg2d k=2 at 2.5x the reference with flat vs
    1.0x with HEM)."""
    ns = len(nodes)
    if ns <= 128:
        return hg.bisect_subset
    xadj = np.asarray(hg.xadj)
    d = (xadj[nodes.astype(np.int64) + 1]
         - xadj[nodes.astype(np.int64)]).astype(object)
    s = int(np.sum(d))
    sq = int(np.sum(d * d))
    heavy_tail = ns * sq >= 2 * s * s
    if heavy_tail:
        return hg.bisect_subset if ns <= 4096 else hg.bisect_subset_fast
    return hg.bisect_subset_ml


def _bisect_whole(sg, target1, cap1, cap2, reps=8):
    """Host bisection of ALL vertices of sg under the dispatch rule above.
    Returns the boolean side array (True = first half)."""
    nodes = np.arange(sg.n, dtype=np.uint32)
    return _pick_bisector(sg, nodes)(nodes, target1, cap1, cap2, reps=reps)


def bisect_engine(eng, total_w, target1, cap1, cap2, eps, seed=1, iters=5,
                  contraction_limit=2000, stop_n=512, reps=8, jet=False,
                  resident=False):
    """Multilevel bisection of the graph the engine holds, on the device:
    coarsen as partition() does (LP clustering + contraction, cluster-weight
    rule for k = 2) down to max(stop_n, 4) vertices or until a level shrinks
    by less than 5%, bisect the downloaded coarsest graph with the host
    bisectors, then refine (and optionally Jet) with caps [cap1, cap2] at
    every level on the way up. A level whose projected bisection is over a
    cap goes through the selection rebalancer first.

    total_w is the weight of the engine's graph, target1 the wanted weight of
    the first half. `resident` as in partition(). Returns the boolean side array (True = first half, the
    convention of Graph.bisect_subset)."""
    caps = np.array([cap1, cap2], dtype=np.int64)
    sizes = [eng.n]
    engines = [eng]
    mappings = []
    while sizes[-1] > max(stop_n, 4):
        cur_n = sizes[-1]
        mcw = level_cluster_weight(total_w, cur_n, 2, eps, contraction_limit)
        _, clus, _ = engines[-1].cluster(mcw, seed=seed + len(mappings),
                                         iters=iters, download=not resident)
        if resident:
            coarse_eng, mapping = engines[-1].contract_engine(
                None, download_mapping=False)
        else:
            coarse_eng, mapping = engines[-1].contract_engine(clus)
        if coarse_eng.n > 0.95 * cur_n:
            del coarse_eng
            break
        engines.append(coarse_eng)
        mappings.append(mapping)
        sizes.append(coarse_eng.n)

    coarsest = engines[-1].download_graph()
    side = _bisect_whole(coarsest, target1, cap1, cap2, reps)
    part = np.where(side, 0, 1).astype(np.uint32)
    # block weights change only where a refiner moves vertices (projection
    # keeps them, and LP / Jet keep a feasible bisection feasible), so one
    # probe on the coarsest graph is enough; a rebalance that stalls on heavy
    # coarse vertices is tried again on the next finer level
    cw = coarsest.vwgt
    cw = (np.ones(coarsest.n, dtype=np.int64) if cw is None
          else cw.astype(np.int64))
    feasible = bool((np.bincount(part, weights=cw, minlength=2) <= caps).all())
    if resident:
        engines[-1].set_labels(2, part)
        for level in range(len(engines) - 1, -1, -1):
            if not feasible:
                _, _, bst = engines[level].rebalance(2, caps, None)
                feasible = bool(bst.feasible)
            engines[level].refine(2, caps, None, seed=seed, iters=iters)
            if jet:
                engines[level].jet(
                    2, caps, None, seed=seed, coarse_level=level,
                    **(jet if isinstance(jet, dict) else {}))
            if level > 0:
                engines[level - 1].project_from(engines[level])
        return engines[0].get_labels() == 0
    for level in range(len(engines) - 1, -1, -1):
        if not feasible:
            _, part, bst = engines[level].rebalance(2, caps, part)
            feasible = bool(bst.feasible)
        _, part, _ = engines[level].refine(2, caps, part, seed=seed,
                                           iters=iters)
        if jet:
            _, part, _ = engines[level].jet(
                2, caps, part, seed=seed, coarse_level=level,
                **(jet if isinstance(jet, dict) else {}))
        if level > 0:
            part = part[mappings[level - 1]]
    return part == 0


def _level_weights(vw, mappings, sizes):
    """Host vertex weights of every level of a coarsening chain, from the
    finest weights (None = unit) by summing over the mappings."""
    out = [np.ones(sizes[0], dtype=np.int64) if vw is None
           else np.asarray(vw, dtype=np.int64)]
    for lvl, mp in enumerate(mappings):
        out.append(np.bincount(mp, weights=out[-1],
                               minlength=sizes[lvl + 1]).astype(np.int64))
    return out


def _extend_partition_gpu(eng, vw, part, groups, mbw_val, k, split_c, reps,
                          force, min_n, eps, seed, iters, jet, resident=False):
    """_extend_partition on the level's engine, without the level's graph on
    the host: one extract_subgraphs per extension round; a block of at least
    min_n vertices becomes an engine of its own and goes through
    bisect_engine, a smaller one is downloaded alone and goes through the
    host bisector. vw holds the level's vertex weights (host). Blocks are
    bisected one at a time, in block order."""
    while True:
        num = len(groups)
        if num >= k:
            break
        if not force and eng.n < 2 * split_c * num:
            break
        subs = eng.extract_subgraphs(k, part)
        new_groups = []
        for b, w in groups:
            if w < 2:
                new_groups.append((b, w))
                continue
            k1 = (w + 1) // 2
            k2 = w - k1
            new_groups += [(b, k1), (b + k1, k2)]
            lo, hi = int(subs.node_offsets[b]), int(subs.node_offsets[b + 1])
            ns = hi - lo
            if ns == 0:
                continue
            nodes = subs.nodes[lo:hi]
            total = int(vw[nodes].sum())
            t1 = total * k1 // w
            cap1, cap2 = k1 * mbw_val, k2 * mbw_val
            if ns >= min_n:
                side = bisect_engine(subs.engine(b), total, t1, cap1, cap2,
                                     eps, seed=seed, iters=iters, reps=reps,
                                     jet=jet, resident=resident)
            else:
                side = _bisect_whole(subs.graph(b), t1, cap1, cap2,
                                     reps=reps)
            part[nodes[~side]] = b + k1
        del subs
        groups = new_groups
    return part, groups


def _extend_partition(hg, part, groups, mbw_val, k, split_c=256, reps=8,
                      force=False):
    """Split every splittable block group in half via FM-polished bisection
    of its induced subgraph (the shape of the reference's deep-multilevel
    partition extension, kaminpar-shm/partitioning/deep/deep_multilevel.cc:
    bipartition blocks while uncoarsening instead of full-k at the coarsest).
    groups is a list of (first_block_id, width); repeats until every block
    would drop below split_c vertices (or all widths are 1)."""
    from . import _lib

    vwp = _lib.kmp_graph_vwgt(hg._h)
    vw = (np.ctypeslib.as_array(vwp, shape=(hg.n,)).astype(np.int64)
          if vwp else np.ones(hg.n, np.int64))
    from concurrent.futures import ThreadPoolExecutor

    def _bisect_group(task):
        _b, _k1, nodes, t1, reps_eff, cap1, cap2 = task
        return _pick_bisector(hg, nodes)(nodes, t1, cap1, cap2, reps=reps_eff)

    while True:
        num = len(groups)
        if num >= k:
            break
        if not force and hg.n < 2 * split_c * num:
            break
        new_groups = []
        tasks = []
        for b, w in groups:
            if w < 2:
                new_groups.append((b, w))
                continue
            k1 = (w + 1) // 2
            k2 = w - k1
            nodes = np.flatnonzero(part == b).astype(np.uint32)
            if len(nodes) == 0:
                new_groups += [(b, k1), (b + k1, k2)]
                continue
            total = int(vw[nodes].sum())
            t1 = total * k1 // w
            ns = len(nodes)
            reps_eff = reps if ns <= 16384 else 4
            reps_eff = min(reps, reps_eff)
            tasks.append((b, k1, nodes, t1, reps_eff,
                          k1 * mbw_val, k2 * mbw_val))
            new_groups += [(b, k1), (b + k1, k2)]
        # groups are independent subproblems (disjoint part[] writes); the
        # ctypes bisector calls release the GIL, so a thread pool gives the
        # same per-group parallelism as the C twin's OpenMP loop, with
        # bit-identical results (sides applied serially afterwards)
        if len(tasks) > 1:
            with ThreadPoolExecutor(max_workers=os.cpu_count()) as ex:
                sides = list(ex.map(_bisect_group, tasks))
        else:
            sides = [_bisect_group(t) for t in tasks]
        for (b, k1, nodes, _t1, _r, _c1, _c2), side in zip(tasks, sides):
            part[nodes[~side]] = b + k1
        groups = new_groups
    return part, groups


def partition_deep(g, k, eps=0.03, seed=1, iters=5, contraction_limit=2000,
                   stop_n=512, split_c=None, reps=8, engine=None,
                   return_arcs=False, jet=False, fm=None, gpu_split=False,
                   gpu_split_min_n=4096, resident=False, vcycles=0,
                   sparsify=False, stats=None):
    """Progressive-k multilevel partition: coarsen as in partition(), then
    instead of full-k initial partitioning at the coarsest level, grow k by
    FM-polished block bisections DURING uncoarsening whenever every block
    still holds >= split_c vertices -- the shape of the reference's deep
    multilevel mode. LP refinement runs at every level with per-group block
    caps (width x uniform cap; unopened block ids get cap 0).

    `jet` and `fm` as in partition(): Jet runs after LP with the level's
    group caps, before the optional FM.

    `gpu_split=True` runs the extension step on the level's engine instead
    of the host (needs k <= 2048): the level's graph is not downloaded for
    it; every extension round extracts the block subgraphs on the device
    (LpEngine.extract_subgraphs), blocks of at least `gpu_split_min_n`
    vertices are bisected by bisect_engine (with `jet` passed through),
    smaller ones by the host bisector on their own downloaded subgraph, and
    an over-cap result goes through LpEngine.rebalance where the host path
    calls balance_partition. The default runs the host path unchanged.

    `resident=True` as in partition(): labels stay on the device between the
    stages (bisect_engine included). A level whose extension step runs
    brackets that step with get_labels / set_labels, as the CPU FM does; with
    `gpu_split` the mappings are still downloaded (the level weights need
    them). Same result as resident=False.

    `vcycles=N` as in partition(): N V-cycles on the result (uniform caps,
    every block being open by then).

    `sparsify` and `stats` as in partition(). bisect_engine and the gpu_split
    extension step coarsen their block subgraphs without sparsification.

    Returns (cut, partition, level_sizes)."""
    if vcycles < 0:
        raise ValueError("vcycles must be >= 0")
    if split_c is None:
        # fine-level structure formation is affordable (and valuable) up to
        # ~2M vertices; beyond that CPU bisection cost explodes while the
        # quality difference vanishes (measured at scale 26: one clustering
        # level already destroyed the structure fine splits would need), so
        # fall back to reference-like block sizes (~2x contraction limit)
        split_c = 262144 if g.n <= (1 << 21) else 2000
    # Split-schedule dispatch by degree variance of the FINE graph (same
    # CV^2 >= 1 statistic as the bisector dispatch): on heavy-tailed graphs
    # every clustering level destroys cut structure (measured: mid-level
    # splits cost 1.4-1.6x vs <=1.0x for finest-level splits on R-MAT), so
    # defer ALL splits to the finest affordable level by skipping the eager
    # coarsest-level split; on low-variance (mesh-like) graphs multilevel
    # structure transfers well and the eager coarsest split wins.
    xadj = np.asarray(g.xadj, dtype=np.int64)
    d = xadj[1:] - xadj[:-1]
    # exact integer sum-of-squares without the object-dtype blowup (an
    # object sum over 67M degrees measured ~1.3 s per partition): split the
    # int64 products into high/low 32-bit halves and recombine as Python
    # ints -- bit-exact, vectorized
    sq = d * d  # per-element fits int64 (deg < 2^31)
    ssum = (int((sq & 0xFFFFFFFF).sum(dtype=np.int64))
            + (int((sq >> 32).sum(dtype=np.int64)) << 32))
    heavy = g.n * ssum >= 2 * int(d.sum()) ** 2
    # split_c >= n is the explicit full-late quality mode: every split at
    # the finest level regardless of size (measured at scale 23: cut 0.44x
    # the reference's best seed, profiles/round1/quality_rmat23_k16_late_full.json)
    late_splits = heavy and (g.n <= (1 << 21) or split_c >= g.n)
    total_w = g.total_node_weight
    mbw_val = g.max_block_weight(k, eps)

    import os as _os
    import time as _time
    _tdbg = _os.environ.get("KMP_TIME") == "1"
    _tt = {"cluster": 0.0, "contract": 0.0, "extend": 0.0, "refine": 0.0,
           "download": 0.0, "fm": 0.0, "other": 0.0}
    _t0 = _time.perf_counter()
    sizes = [g.n]
    mappings = []
    engines = [engine if engine is not None else LpEngine(g)]
    arcs_total = 0
    ns_total = 0
    while sizes[-1] > max(stop_n, 2 * k):
        cur_n = sizes[-1]
        mcw = level_cluster_weight(total_w, cur_n, k, eps, contraction_limit)
        _tc = _time.perf_counter()
        nc, clus, cst = engines[-1].cluster(mcw, seed=seed + len(mappings),
                                           iters=iters, download=not resident)
        _tt["cluster"] += _time.perf_counter() - _tc
        arcs_total += cst.arcs_scanned
        ns_total += cst.phase_a_ns
        _tc = _time.perf_counter()
        if resident:
            coarse_eng, mapping = engines[-1].contract_engine(
                None, download_mapping=bool(gpu_split), sparsify=sparsify,
                seed=seed + len(mappings))
        else:
            coarse_eng, mapping = engines[-1].contract_engine(
                clus, sparsify=sparsify, seed=seed + len(mappings))
        _tt["contract"] += _time.perf_counter() - _tc
        if coarse_eng.n > 0.95 * cur_n:
            del coarse_eng
            break
        engines.append(coarse_eng)
        mappings.append(mapping)
        sizes.append(coarse_eng.n)
    _level_stats(stats, engines)

    part = np.zeros(sizes[-1], dtype=np.uint32)
    groups = [(0, k)]
    cut = None
    coarsest = len(engines) - 1
    level_vw = None  # host vertex weights per level (gpu_split only)
    for level in range(coarsest, -1, -1):
        # at the coarsest level split eagerly (down to ~32-vertex blocks,
        # like the reference's initial bipartition of the coarsest graph);
        # afterwards extend only when every block keeps >= split_c vertices
        sc = (min(split_c, 48) if level == coarsest and not late_splits
              else split_c)
        hg = None
        if len(groups) < k and (sizes[level] >= 2 * sc * len(groups)
                                or level == 0):
            if part is None:  # resident: the extension works on host arrays
                part = engines[level].get_labels()
            if gpu_split:
                _tc = _time.perf_counter()
                if level_vw is None:
                    level_vw = _level_weights(g.vwgt, mappings, sizes)
                part, groups = _extend_partition_gpu(
                    engines[level], level_vw[level], part, groups, mbw_val,
                    k, sc, reps, level == 0, gpu_split_min_n, eps, seed,
                    iters, jet, resident)
                if len(groups) == k:
                    bw = np.bincount(part, weights=level_vw[level],
                                     minlength=k)
                    if bw.max() > mbw_val:
                        _, part, _ = engines[level].rebalance(
                            k, np.full(k, mbw_val, dtype=np.int64), part)
                _tt["extend"] += _time.perf_counter() - _tc
            else:
                _tc = _time.perf_counter()
                hg = g if level == 0 else engines[level].download_graph()
                _tt["download"] += _time.perf_counter() - _tc
                _tc = _time.perf_counter()
                part, groups = _extend_partition(hg, part, groups, mbw_val,
                                                 k, sc, reps,
                                                 force=(level == 0))
                if len(groups) == k:
                    hg.balance_partition(k, mbw_val, part)
                _tt["extend"] += _time.perf_counter() - _tc
        caps = _group_caps(groups, k, mbw_val)
        _tc = _time.perf_counter()
        if resident and part is not None:
            engines[level].set_labels(k, part)
            part = None  # on the device until a host step needs it
        cut, part, rst = engines[level].refine(
            k, caps, part, seed=seed, iters=iters)
        _tt["refine"] += _time.perf_counter() - _tc
        arcs_total += rst.arcs_scanned
        ns_total += rst.phase_a_ns
        if jet:
            _tc = _time.perf_counter()
            cut, part, _ = engines[level].jet(
                k, caps, part, seed=seed, coarse_level=level,
                **(jet if isinstance(jet, dict) else {}))
            _tt["refine"] += _time.perf_counter() - _tc
        # per-level k-way boundary FM on small graphs (<= ~2M fine
        # vertices): recovers the bisection quality LP refinement alone
        # cannot on mesh-like graphs (classic multilevel FM recipe)
        if (g.n <= (1 << 21)) if fm is None else bool(fm):
            _tc = _time.perf_counter()
            if hg is None:
                hg = g if level == 0 else engines[level].download_graph()
            if resident:
                part = engines[level].get_labels()
            part = hg.kway_fm(k, caps, part)
            if level == 0:
                cut = g.edge_cut(part)
            _tt["fm"] += _time.perf_counter() - _tc
        if resident and level > 0:
            if part is not None:
                engines[level].set_labels(k, part)
                part = None
            engines[level - 1].project_from(engines[level])
        elif level > 0:
            part = part[mappings[level - 1]]
    if vcycles:
        eng0 = engines[0]
        del engines  # the cycles build their own chains
        cut, part = _run_vcycles(g, k, part, eng0, vcycles, eps, seed, iters,
                                 contraction_limit, stop_n, jet, fm, resident)
    elif resident and part is None:
        part = engines[0].get_labels()
    if _tdbg:
        _tt["other"] = (_time.perf_counter() - _t0) - sum(
            v for q, v in _tt.items() if q != "other")
        import sys as _sys
        print("[deep-timing] " + " ".join(f"{q}={v:.2f}s"
                                          for q, v in _tt.items()),
              file=_sys.stderr)
    if return_arcs:
        return cut, part, sizes, int(arcs_total), int(ns_total)
    return cut, part, sizes


class EdgesGraph:
    """What partition() / partition_deep() ask of their graph argument,
    answered from an engine built by LpEngine.from_edges(): n, m,
    total_node_weight and max_block_weight(k, eps) come from the engine and the
    caller's vertex weights, the last in the double arithmetic of
    kmp_max_block_weight. Anything else a driver asks for (kway_fm, edge_cut,
    xadj, initial_partition_native, ...) needs the host graph, which is
    downloaded from the engine once, on that first use; `downloaded` records
    that it happened."""

    def __init__(self, engine, total_node_weight):
        self.engine = engine
        self.n = engine.n
        self.m = engine.m
        self.total_node_weight = int(total_node_weight)
        self.downloaded = False
        self._host = None

    def max_block_weight(self, k, eps=0.03):
        import math

        pbw = float(math.ceil(float(self.total_node_weight) / float(k)))
        return int((1.0 + float(eps)) * pbw)

    def host(self):
        if self._host is None:
            self._host = self.engine.download_graph()
            self.downloaded = True
        return self._host

    @property
    def _h(self):
        # the host graph's handle, for the drivers' direct library calls
        return self.host()._h

    def __getattr__(self, name):
        # only reached for what the attributes above do not answer
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.host(), name)


def partition_edges(src, dst, k, n=None, weights=None, vwgt=None,
                    combine="max", deep=False, facade_out=None, **kw):
    """partition() (or with deep=True partition_deep()) of the graph given as
    an edge list, host arrays or GPU tensors as in LpEngine.from_edges(): the
    fine graph is built on the device and reaches the host only where a host
    step of the driver needs it (the CPU FM, the level-0 edge_cut that follows
    it, the host bisections of partition_deep, an initial partition without any
    coarsening). With fm=False, resident=True and at least one coarsened level
    it never does. `facade_out`, a list, receives the EdgesGraph the driver
    ran on (its `downloaded` tells whether the host graph was fetched). Other
    keywords go to the driver. Returns what the driver returns."""
    if "engine" in kw:
        raise TypeError("partition_edges() builds its own engine")
    eng = LpEngine.from_edges(src, dst, n=n, weights=weights, vwgt=vwgt,
                              combine=combine)
    if vwgt is None:
        total_w = eng.n
    elif LpEngine._is_tensor(vwgt):
        total_w = int(vwgt.sum().item())
    else:
        total_w = int(np.asarray(vwgt, dtype=np.int64).sum())
    facade = EdgesGraph(eng, total_w)
    if facade_out is not None:
        facade_out.append(facade)
    driver = partition_deep if deep else partition
    return driver(facade, k, engine=eng, **kw)
