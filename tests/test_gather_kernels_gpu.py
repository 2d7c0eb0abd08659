"""GPU parity tests for the gather kernels of the LP refine path: k_phase_s
(several positions per 16-lane subgroup), k_phase_m (unrolled edge loop, next
entry prefetched), k_phase_l_acc (short slices, unrolled) and k_activate_v2
(movers batched per wave). Every comparison is exact -- the edge cut and the
whole label array -- against the CPU oracle.

The degree-boundary graph puts one hub on every degree at which the S/M/L
tiers, the unroll remainders or the slice remainders change path."""

import functools

import numpy as np
import pytest

# torch's HIP runtime must initialize before any engine in this process
# (see test_gpu_parity.py)
import torch as _torch

if _torch.cuda.is_available():
    _torch.zeros(1, device="cuda:0")

import kaminpar_amd as ka
from helpers import oracle_balance, oracle_refine, oracle_underload

pytestmark = pytest.mark.gpu

# refine-path L slice length at k <= 64 (kLSliceSmall in lp_hip.hip); larger
# k keeps the 8192-edge slice, whose boundaries are in the list as well
S = 1024

HUB_DEGREES = [
    0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 2047, 2048, 2049,
    S - 1, S, S + 1, 2 * S + 1, 8191, 8192, 8193, 20011,
]
N_TOTAL = 25003  # not a multiple of 16 or of 64


@functools.lru_cache(maxsize=None)
def _boundary_csr():
    """Hubs 0..H-1 with exactly the degrees above, wired to a shared pool of
    leaves (no hub-hub and no duplicate edges, so symmetrising keeps every
    hub degree exact). Returns (xadj, adjncy, adjwgt, vwgt)."""
    assert N_TOTAL % 16 != 0 and N_TOTAL % 64 != 0
    rng = np.random.default_rng(2024)
    H = len(HUB_DEGREES)
    leaves = np.arange(H, N_TOTAL, dtype=np.int64)
    src, dst = [], []
    for h, d in enumerate(HUB_DEGREES):
        pick = rng.choice(leaves, size=d, replace=False)
        src.append(np.full(d, h, np.int64))
        dst.append(pick)
    src = np.concatenate(src)
    dst = np.concatenate(dst)
    rows = np.concatenate([src, dst])
    cols = np.concatenate([dst, src])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    xadj = np.zeros(N_TOTAL + 1, np.int64)
    np.add.at(xadj, rows + 1, 1)
    xadj = np.cumsum(xadj).astype(np.uint32)
    adjncy = cols.astype(np.uint32)
    deg = np.diff(xadj.astype(np.int64))
    assert list(deg[:H]) == HUB_DEGREES
    # symmetric edge weights: a function of the undirected edge
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    adjwgt = ((lo * 31 + hi) % 7 + 1).astype(np.int32)
    vwgt = rng.integers(1, 9, N_TOTAL).astype(np.int32)
    return xadj, adjncy, adjwgt, vwgt


def _boundary_graph(weighted):
    xadj, adjncy, adjwgt, vwgt = _boundary_csr()
    if weighted:
        return (ka.Graph.from_csr(xadj.copy(), adjncy.copy(), vwgt=vwgt, adjwgt=adjwgt),
                vwgt, adjwgt)
    return ka.Graph.from_csr(xadj.copy(), adjncy.copy()), None, None


def _caps(vwgt, n, k, eps):
    total = int(vwgt.sum()) if vwgt is not None else n
    return np.full(k, int(np.ceil(total / k) * (1.0 + eps)) + 8, dtype=np.int64)


def _hub(d):
    return HUB_DEGREES.index(d)


# k = 2, 16, 256: v2 path, u8 shadow (S = 1024 at k <= 64, 8192 at 256);
# k = 1024: legacy path, u16 shadow
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("k", [2, 16, 256, 1024])
def test_degree_boundary_refine(oracle, k, weighted):
    g, vwgt, adjwgt = _boundary_graph(weighted)
    part0 = ka.random_partition(g.n, k, seed=11)
    mbw = _caps(vwgt, g.n, k, 0.10)
    ocut, opart, ostats = oracle_refine(oracle, g, k, mbw, part0, seed=4, iters=5,
                                        vwgt=vwgt, adjwgt=adjwgt)
    assert ostats[1] > 0  # the oracle really moves vertices

    eng = ka.LpEngine(g)
    cut, part, stats = eng.refine(k, mbw, part0, seed=4, iters=5)
    assert cut == ocut, f"cut gpu={cut} oracle={ocut}"
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"
    assert stats.moves == ostats[1]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_degree_boundary_balance(oracle, weighted):
    """Mode 1 and the fallback target in the S, M and L kernels."""
    g, vwgt, adjwgt = _boundary_graph(weighted)
    k = 16
    mbw = _caps(vwgt, g.n, k, 0.03)
    for part0 in (
        np.zeros(g.n, np.uint32),  # everything in one block: fallback targets
        np.where(np.arange(g.n) < g.n // 2, 0,
                 ka.random_partition(g.n, k, seed=2)).astype(np.uint32),
    ):
        ocut, opart, _ = oracle_balance(oracle, g, k, mbw, part0, seed=1, iters=5,
                                        vwgt=vwgt, adjwgt=adjwgt)
        eng = ka.LpEngine(g)
        cut, part, _ = eng.balance(k, mbw, part0, seed=1, iters=5)
        assert cut == ocut
        assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"
        assert not np.array_equal(opart, part0)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_degree_boundary_underload(oracle, weighted):
    """Mode 2 (per-block minimum weights) in the S, M and L kernels."""
    g, vwgt, adjwgt = _boundary_graph(weighted)
    k = 16
    vw = vwgt.astype(np.int64) if vwgt is not None else np.ones(g.n, np.int64)
    avg = int(vw.sum()) // k
    mbw = np.full(k, int(avg * 1.25) + 1, np.int64)
    mnw = np.full(k, int(avg * 0.75), np.int64)
    # drain blocks 0..3 below their minimum, keeping one seed vertex each
    part0 = ka.random_partition(g.n, k, seed=3)
    drained = part0 < 4
    part0[drained] = (4 + (np.arange(g.n)[drained] % (k - 4))).astype(np.uint32)
    H = len(HUB_DEGREES)
    for b in range(4):
        part0[H + b] = b
    bw0 = np.bincount(part0, weights=vw, minlength=k)
    assert (bw0[:4] < mnw[:4]).all()

    ocut, opart, ostats = oracle_underload(oracle, g, k, mbw, mnw, part0, seed=1,
                                           iters=5, vwgt=vwgt, adjwgt=adjwgt)
    eng = ka.LpEngine(g)
    cut, part, _ = eng.underload(k, mbw, mnw, part0, seed=1, iters=5)
    assert cut == ocut
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"


# position groups that run past pos_hi or past n
@pytest.mark.parametrize("n", [1, 3, 15, 17, 63, 65, 129])
def test_tail_shapes_path(oracle, n):
    src = np.arange(n - 1, dtype=np.int64)
    rows = np.concatenate([src, src + 1])
    cols = np.concatenate([src + 1, src])
    order = np.lexsort((cols, rows))
    xadj = np.zeros(n + 1, np.int64)
    np.add.at(xadj, rows + 1, 1)
    xadj = np.cumsum(xadj).astype(np.uint32)
    adjncy = cols[order].astype(np.uint32)
    g = ka.Graph.from_csr(xadj, adjncy)
    k = 2
    part0 = (np.arange(n) % 2).astype(np.uint32)
    mbw = np.full(k, n, np.int64)
    ocut, opart, _ = oracle_refine(oracle, g, k, mbw, part0, seed=2, iters=5)
    eng = ka.LpEngine(g)
    cut, part, _ = eng.refine(k, mbw, part0, seed=2, iters=5)
    assert cut == ocut
    assert np.array_equal(part, opart)


def test_activation_of_hub_neighbours(oracle):
    """A degree-17, a degree-300 and the largest hub sit alone in block 0
    with all their neighbours in block 1 and loose limits, so each of them
    moves in sweep 1 and its whole row must be re-activated. A neighbour
    that is missed, or a vertex that is wrongly activated, shows from sweep
    2 on.

    What the activation kernel sees here: a chunk of this graph is 448
    positions (7 units), so its grid is 2 workgroups = 8 waves and lane l of
    wave w takes list entry w + 8 * l. The oracle's sweep 1 moves more than
    8192 vertices over at most 64 chunks, i.e. on average at least 16
    admitted rows per wave (asserted below), nearly all of them leaves of
    degree 1-4. So each wave builds its degree prefix over many lanes and
    walks several concatenated small rows per trip; the degree-300 row
    spans more than one 256-edge trip of its wave, next to those small
    rows; and the largest hub (above the 4096-edge concatenation limit)
    goes through the hub ballot from whichever lane holds it."""
    g, _, _ = _boundary_graph(False)
    xadj, adjncy, _, _ = _boundary_csr()
    k = 4
    hubs = [_hub(17), _hub(300), _hub(max(HUB_DEGREES))]
    part0 = (1 + ka.random_partition(g.n, k - 1, seed=6)).astype(np.uint32)
    for h in hubs:
        part0[adjncy[xadj[h]:xadj[h + 1]]] = 1
    part0[hubs] = 0
    assert (part0 == 0).sum() == len(hubs)
    # loose limits, so every hub is admitted wherever it goes; block 0 alone
    # is full as it stands, or the leaves processed before their hub would
    # join it there and the hub would stay
    mbw = np.full(k, g.n, np.int64)
    mbw[0] = len(hubs)

    _, opart1, ostats1 = oracle_refine(oracle, g, k, mbw, part0, seed=9, iters=1)
    assert all(opart1[h] != 0 for h in hubs), [int(opart1[h]) for h in hubs]
    # enough movers that a wave holds many rows: 64 chunks x 8 waves x 16
    assert ostats1[1] >= 64 * 8 * 16, int(ostats1[1])
    ocut, opart, _ = oracle_refine(oracle, g, k, mbw, part0, seed=9, iters=5)
    assert not np.array_equal(opart, opart1)  # later sweeps still move vertices

    eng = ka.LpEngine(g)
    cut, part, _ = eng.refine(k, mbw, part0, seed=9, iters=5)
    assert cut == ocut
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"


def test_replay_on_boundary_graph(oracle):
    """refine_begin, then reset + run_sweeps(5) three times: the third run
    replays the captured sweep graphs and must equal the oracle."""
    g, _, _ = _boundary_graph(False)
    k = 16
    part0 = ka.random_partition(g.n, k, seed=13)
    mbw = _caps(None, g.n, k, 0.10)
    ocut, opart, ostats = oracle_refine(oracle, g, k, mbw, part0, seed=7, iters=5)

    eng = ka.LpEngine(g)
    eng.refine_begin(k, mbw, part0, seed=7)
    for _ in range(3):
        eng.reset()
        eng.run_sweeps(5)
        assert eng.get_stats().moves == ostats[1]
    cut, part, _ = eng.refine_end()
    assert cut == ocut
    assert np.array_equal(part, opart), f"{(part != opart).sum()} labels differ"
