"""CPU mirror of kaminpar_amd.partition.partition / partition_deep with the
`sparsify` option: the oracle pipelines of tests/oracle_pipeline.py with their
contraction wrapped by the numpy twin of the pass (tests/sparsify_twin.py),
seeded with seed + level as the drivers do. Every stage is bit-reproducible,
so cut, partition, level sizes and level arcs are what the GPU drivers must
produce."""

import numpy as np

import kaminpar_amd as ka
import oracle_pipeline as op
from sparsify_twin import sparsify


def _arrays(g):
    aw, vw = g.adjwgt, g.vwgt
    return (np.asarray(g.xadj).copy(), np.asarray(g.adjncy).copy(),
            None if aw is None else np.asarray(aw).copy(),
            None if vw is None else np.asarray(vw).copy())


def _mirror(pipeline, oracle, g, k, sparsify_opt, seed, **kw):
    """Returns (cut, part, sizes, stats) with stats as the drivers fill it:
    level_arcs and one twin stats dict (or None) per level that was kept."""
    params = None
    if ka.sparsify_on(sparsify_opt):
        params = {} if sparsify_opt is True else dict(sparsify_opt)
    records = []  # one per contraction, in call order = level order
    plain = op.oracle_contract

    def wrapped(oracle_, cur, clus, vwgt=None, adjwgt=None):
        coarse, mapping = plain(oracle_, cur, clus, vwgt=vwgt, adjwgt=adjwgt)
        if params is None:
            records.append((coarse.m, None))
            return coarse, mapping
        xadj, adjncy, aw, vw = _arrays(coarse)
        if aw is None:
            aw = np.ones(coarse.m, np.int32)
        x2, a2, w2, st = sparsify(xadj, adjncy, aw, cur.n, cur.m, params,
                                  seed + len(records))
        if st["applied"]:
            coarse = ka.Graph.from_csr(x2, a2, vw, w2)
        records.append((coarse.m, st))
        return coarse, mapping

    op.oracle_contract = wrapped
    try:
        cut, part, sizes = pipeline(oracle, g, k, seed=seed, **kw)
    finally:
        op.oracle_contract = plain
    kept = records[:len(sizes) - 1]  # a level that did not shrink is dropped
    stats = dict(level_arcs=[int(g.m)] + [int(m) for m, _ in kept],
                 sparsify=[st for _, st in kept])
    return cut, part, sizes, stats


def mirror_partition(oracle, g, k, sparsify=False, seed=1, **kw):
    return _mirror(op.oracle_partition, oracle, g, k, sparsify, seed, **kw)


def mirror_partition_deep(oracle, g, k, sparsify=False, seed=1, **kw):
    return _mirror(op.oracle_partition_deep, oracle, g, k, sparsify, seed, **kw)
