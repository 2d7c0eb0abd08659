"""CPU mirror of kaminpar_amd.partition.vcycle (keep in sync): one V-cycle
written over the oracle's cluster-with-communities / contract / refine, the
numpy Jet twins and Graph.kway_fm, with the level schedule, seeds and cap
formulas of partition(). Every stage is bit-identical to its GPU counterpart
by the parity tests, so the GPU cycle must give exactly this partition, cut,
level list and accepted flag.

The mirror also checks what makes a V-cycle sound: no cluster spans two
blocks, and the partition restricted to a coarse level has the cut and the
block weights of the finer one."""

import numpy as np

import jet_twin
import rebalance_twin
from helpers import oracle_cluster_comm, oracle_refine
from kaminpar_amd.partition import level_cluster_weight, vcycle_accept
from oracle_pipeline import oracle_contract


def _weights(gr):
    from kaminpar_amd import _lib
    vw = _lib.kmp_graph_vwgt(gr._h)
    aw = _lib.kmp_graph_adjwgt(gr._h)
    v = np.ctypeslib.as_array(vw, shape=(gr.n,)) if vw else None
    a = np.ctypeslib.as_array(aw, shape=(gr.m,)) if aw else None
    return v, a


def _block_weights(vw, n, part, k):
    w = np.ones(n, dtype=np.int64) if vw is None else vw.astype(np.int64)
    return np.bincount(part, weights=w, minlength=k).astype(np.int64)


def _jet(oracle, gr, k, mbw, part, seed, level, jet, vw, aw):
    """LpEngine.jet(coarse_level=level, **jet) on the twins."""
    params = dict(jet) if isinstance(jet, dict) else {}
    temp = 0.75 if level != 0 else 0.25  # kmp_jet_params_default
    common = dict(
        num_rounds=params.get("num_rounds", 1),
        max_iterations=params.get("max_iterations", 0),
        max_fruitless=params.get("max_fruitless", 12),
        fruitless_threshold=params.get("fruitless_threshold", 0.999),
        initial_gain_temp=params.get("initial_gain_temp", temp),
        final_gain_temp=params.get("final_gain_temp", temp))
    if params.get("balancer", 0) == 1:
        cut, out, _ = rebalance_twin.jet(
            oracle, gr, k, mbw, part, vwgt=vw, adjwgt=aw,
            balance_passes=params.get("balance_passes", 16), **common)
    else:
        cut, out, _ = jet_twin.jet(
            oracle, gr, k, mbw, part, seed=seed, vwgt=vw, adjwgt=aw,
            balance_iters=params.get("balance_iters", 2), **common)
    return cut, out


def mirror_vcycle(oracle, g, k, partition, eps=0.03, seed=1, iters=5,
                  contraction_limit=2000, stop_n=512, jet=False, fm=None):
    """Returns (cut, partition, level_sizes, accepted)."""
    total_w = g.total_node_weight
    mbw = np.full(k, g.max_block_weight(k, eps), dtype=np.int64)
    part_in = np.ascontiguousarray(partition, dtype=np.uint32)
    vw0, aw0 = _weights(g)
    cut_in = jet_twin.edge_cut(oracle, g, part_in, aw0)
    feas_in = bool((_block_weights(vw0, g.n, part_in, k) <= mbw).all())

    graphs = [g]
    mappings = []
    part = part_in.copy()
    while graphs[-1].n > max(stop_n, 2 * k):
        cur = graphs[-1]
        mcw = level_cluster_weight(total_w, cur.n, k, eps, contraction_limit)
        vw, aw = _weights(cur)
        _, clus, _ = oracle_cluster_comm(oracle, cur, mcw, part,
                                         seed=seed + len(mappings),
                                         iters=iters, vwgt=vw, adjwgt=aw)
        # cluster ids are vertex ids: a cluster lies in its leader's block
        assert (part[clus] == part).all(), "a cluster spans two blocks"
        coarse, mapping = oracle_contract(oracle, cur, clus, vwgt=vw, adjwgt=aw)
        if coarse.n > 0.95 * cur.n:
            break
        coarse_part = np.zeros(coarse.n, dtype=np.uint32)
        coarse_part[mapping] = part
        assert (coarse_part[mapping] == part).all()
        cvw, caw = _weights(coarse)
        assert (jet_twin.edge_cut(oracle, coarse, coarse_part, caw)
                == jet_twin.edge_cut(oracle, cur, part, aw))
        assert (_block_weights(cvw, coarse.n, coarse_part, k)
                == _block_weights(vw, cur.n, part, k)).all()
        graphs.append(coarse)
        mappings.append(mapping)
        part = coarse_part

    fm_on = g.n <= (1 << 21) if fm is None else bool(fm)
    for level in range(len(graphs) - 1, -1, -1):
        gr = graphs[level]
        vw, aw = _weights(gr)
        _, part, _ = oracle_refine(oracle, gr, k, mbw, part, seed=seed,
                                   iters=iters, vwgt=vw, adjwgt=aw)
        if jet:
            _, part = _jet(oracle, gr, k, mbw, part, seed, level, jet, vw, aw)
        if fm_on:
            part = gr.kway_fm(k, mbw, part)
        if level > 0:
            part = part[mappings[level - 1]]

    cut = jet_twin.edge_cut(oracle, g, part, aw0)
    feas = bool((_block_weights(vw0, g.n, part, k) <= mbw).all())
    accepted = vcycle_accept(feas_in, cut_in, feas, cut)
    if not accepted:
        cut, part = cut_in, part_in.copy()
    return cut, part, [gr.n for gr in graphs], accepted


def mirror_vcycles(oracle, g, k, partition, cycles, seed=1, **kw):
    """The drivers' `vcycles` option: cycle c with seed + c on the output of
    cycle c - 1. Returns the list of (cut, partition, level_sizes, accepted)."""
    out = []
    part = partition
    for c in range(cycles):
        res = mirror_vcycle(oracle, g, k, part, seed=seed + c, **kw)
        out.append(res)
        part = res[1]
    return out
