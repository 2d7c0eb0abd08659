"""GPU parity tests for the commit train of the LP refine path: round 1 of
the admission fixpoint on the full grid (k_hist_v2 / k_scatter_v2, unit node
weights), the later rounds in k_fixpoint_v2, the one-barrier k_scan_coop and
the small arrays that the train's own kernels clear between chunks instead
of memset nodes. Every comparison is exact -- the edge cut, the whole label
array and the move count -- against the CPU oracle.

The graphs follow the headline benchmark: R-MAT, edge factor 8, generator
seed 42, degree-bucket order, random_partition(seed=5), LP seed 1, 5 sweeps.
At eps 0.03 from a random partition most chunks need three or more
admission rounds and round 1 de-admits in nearly all of them."""

import functools

import numpy as np
import pytest

# torch's HIP runtime must initialize before any engine in this process
# (see test_gpu_parity.py)
import torch as _torch

if _torch.cuda.is_available():
    _torch.zeros(1, device="cuda:0")

import kaminpar_amd as ka
from helpers import oracle_balance, oracle_refine

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    g, _ = ka.Graph.rmat(scale, 8, seed=42).rearrange_degree_buckets()
    return g


def _uniform_caps(g, k, eps=0.03):
    return np.full(k, g.max_block_weight(k, eps), dtype=np.int64)


def _check(oracle, g, k, mbw, part0, vwgt=None, seed=1):
    ocut, opart, ostats = oracle_refine(oracle, g, k, mbw, part0, seed=seed, iters=5,
                                        vwgt=vwgt)
    assert ostats[1] > 0  # the oracle really moves vertices
    eng = ka.LpEngine(g)
    cut, part, stats = eng.refine(k, mbw, part0, seed=seed, iters=5)
    print(f"cut gpu={cut} oracle={ocut} moves gpu={stats.moves} oracle={ostats[1]} "
          f"labels differing={(part != opart).sum()}")
    assert cut == ocut, f"cut gpu={cut} oracle={ocut}"
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"
    assert stats.moves == ostats[1]
    return opart


def test_scan_small_many_rounds(oracle):
    """Scale 16, k = 16: 16 rows x 16 targets, the single-workgroup scan."""
    g = _rmat(16)
    k = 16
    _check(oracle, g, k, _uniform_caps(g, k), ka.random_partition(g.n, k, seed=5))


def test_scan_coop_k256(oracle):
    """Scale 18, k = 256: a chunk of 4096 positions is 64 rows, 16 384
    histogram entries, so the resident-grid scan runs; labels8 at its upper
    end."""
    g = _rmat(18)
    k = 256
    _check(oracle, g, k, _uniform_caps(g, k), ka.random_partition(g.n, k, seed=5))


def test_k2(oracle):
    """k = 2: at most two admission rounds."""
    g = _rmat(16)
    k = 2
    _check(oracle, g, k, _uniform_caps(g, k), ka.random_partition(g.n, k, seed=5))


def test_weighted_keeps_prefix_weight_path(oracle):
    """Random node weights 1..8: the cutoffs need the prefix weights that
    the fixpoint builds, so round 1 stays in k_fixpoint_v2."""
    g0 = _rmat(16)
    k = 16
    vwgt = np.random.default_rng(99).integers(1, 9, g0.n).astype(np.int32)
    g = ka.Graph.from_csr(np.asarray(g0.xadj).copy(), np.asarray(g0.adjncy).copy(), vwgt=vwgt)
    total = int(vwgt.sum())
    mbw = np.full(k, int(np.ceil(total / k) * 1.03) + 8, dtype=np.int64)
    _check(oracle, g, k, mbw, ka.random_partition(g.n, k, seed=5), vwgt=vwgt)


def test_per_block_caps(oracle):
    """Block 0's cap lies below its initial weight (capacity <= 0, round-1
    cutoff 0) and block 1 is never truncated (cap >= n)."""
    g = _rmat(16)
    k = 16
    part0 = ka.random_partition(g.n, k, seed=5)
    w0 = np.bincount(part0, minlength=k)
    mbw = _uniform_caps(g, k)
    mbw[0] = int(w0[0]) - 100
    mbw[1] = g.n
    assert mbw[0] > 0 and (mbw[2:] >= w0[2:]).all()
    opart = _check(oracle, g, k, mbw, part0)
    # admission control is really exercised: loose caps give another result
    _, loose, _ = oracle_refine(oracle, g, k, np.full(k, g.n, np.int64), part0, seed=1,
                                iters=5)
    assert not np.array_equal(opart, loose)


@pytest.mark.parametrize("scale", [16, 11], ids=["rmat16", "n2048-empty-chunks"])
def test_replay(oracle, scale):
    """refine_begin, then reset + run_sweeps(5) three times: the third run
    replays the captured sweep graphs. n = 2048 leaves chunks empty."""
    g = _rmat(scale)
    k = 16
    part0 = ka.random_partition(g.n, k, seed=5)
    mbw = _uniform_caps(g, k)
    ocut, opart, ostats = oracle_refine(oracle, g, k, mbw, part0, seed=1, iters=5)
    assert ostats[1] > 0

    eng = ka.LpEngine(g)
    eng.refine_begin(k, mbw, part0, seed=1)
    for _ in range(3):
        eng.reset()
        eng.run_sweeps(5)
        assert eng.get_stats().moves == ostats[1]
    cut, part, _ = eng.refine_end()
    assert cut == ocut
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"


def test_interleaved_modes(oracle):
    """refine (v2 train), balance (legacy path, its own memsets), refine with
    other caps, on one engine: stale list counters or departure arrays from
    one mode would show in the next."""
    g = _rmat(16)
    k = 16
    eng = ka.LpEngine(g)

    part0 = ka.random_partition(g.n, k, seed=5)
    mbw1 = _uniform_caps(g, k, 0.03)
    ocut, opart, ostats = oracle_refine(oracle, g, k, mbw1, part0, seed=1, iters=5)
    cut, part, stats = eng.refine(k, mbw1, part0, seed=1, iters=5)
    assert cut == ocut and np.array_equal(part, opart) and stats.moves == ostats[1]

    # tighter caps make the refined partition infeasible
    mbw2 = np.full(k, int(np.bincount(opart, minlength=k).max()) - 64, dtype=np.int64)
    ocut2, opart2, _ = oracle_balance(oracle, g, k, mbw2, opart, seed=2, iters=5)
    assert not np.array_equal(opart2, opart)
    cut2, part2, _ = eng.balance(k, mbw2, opart, seed=2, iters=5)
    assert cut2 == ocut2 and np.array_equal(part2, opart2)

    mbw3 = _uniform_caps(g, k, 0.10)
    mbw3[3] = int(np.bincount(opart2, minlength=k)[3])  # block 3 is full as it stands
    ocut3, opart3, ostats3 = oracle_refine(oracle, g, k, mbw3, opart2, seed=3, iters=5)
    assert ostats3[1] > 0
    cut3, part3, stats3 = eng.refine(k, mbw3, opart2, seed=3, iters=5)
    assert cut3 == ocut3
    assert np.array_equal(part3, opart3), f"{(part3 != opart3).sum()} labels differ"
    assert stats3.moves == ostats3[1]
