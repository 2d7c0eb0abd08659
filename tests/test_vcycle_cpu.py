"""Host-only side of the V-cycle: the CPU mirror (vcycle_mirror.py) with its
cuts pinned, the accept rule over its truth table, and the `vcycles` option of
the C drivers, which is filled and refused without a GPU."""

import ctypes
import os

import numpy as np
import pytest

import kaminpar_amd as ka
from kaminpar_amd import _lib, _u32p
from kaminpar_amd.partition import vcycle_accept
from oracle_pipeline import oracle_partition
from vcycle_mirror import mirror_vcycles

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

JET_SEL = dict(balancer=1)


# Basic partition() (LP + FM, seed 1, k = 16, eps 0.03), then three cycles
# with Jet and the selection rebalancer, FM off, seeds 1, 2, 3.
_PINNED = {
    "rmat14": (87155, [61310, 59203, 58963]),
    "rgg2d": (279, [246, 239, 239]),
}


def _graph(name):
    if name == "rmat14":
        return ka.Graph.rmat(14, 8, seed=42)
    return ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))


@pytest.mark.parametrize("name", sorted(_PINNED))
def test_mirror_cuts_are_pinned(oracle, name):
    g, k = _graph(name), 16
    base_cut, cycle_cuts = _PINNED[name]
    cut0, part0, _ = oracle_partition(oracle, g, k, seed=1)
    assert cut0 == base_cut
    res = mirror_vcycles(oracle, g, k, part0, 3, seed=1, jet=JET_SEL, fm=False)
    cuts = [r[0] for r in res]
    print(name, cut0, cuts, [r[2] for r in res], [r[3] for r in res])
    assert cuts == cycle_cuts
    mbw = g.max_block_weight(k, 0.03)
    prev = cut0
    for cut, part, sizes, accepted in res:
        assert accepted and cut <= prev and cut == g.edge_cut(part)
        assert sizes[0] == g.n and all(a > b for a, b in zip(sizes, sizes[1:]))
        assert np.bincount(part, minlength=k).max() <= mbw  # unit weights
        prev = cut


def test_mirror_without_refiners_returns_its_input(oracle):
    g, k = ka.Graph.rmat(10, 8, seed=5), 4
    part0 = ka.random_partition(g.n, k, seed=3)
    (cut, part, sizes, accepted), = mirror_vcycles(
        oracle, g, k, part0, 1, iters=0, jet=False, fm=False, stop_n=64)
    assert accepted and cut == g.edge_cut(part0) and np.array_equal(part, part0)
    assert sizes[0] == g.n


@pytest.mark.parametrize("feas_in", [False, True])
@pytest.mark.parametrize("feas_out", [False, True])
@pytest.mark.parametrize("cut_in,cut_out", [(10, 9), (10, 10), (10, 11)])
def test_accept_rule(feas_in, feas_out, cut_in, cut_out):
    got = vcycle_accept(feas_in, cut_in, feas_out, cut_out)
    if feas_out and not feas_in:
        want = True  # feasibility won, whatever the cut
    elif feas_in and not feas_out:
        want = False  # feasibility lost, whatever the cut
    else:
        want = cut_out <= cut_in
    assert got is want


def test_vcycles_option():
    assert _lib.kmp_pipeline_opts_default().vcycles == 0
    assert ka.pipeline_opts().vcycles == 0
    o = ka.pipeline_opts(vcycles=2, resident=True)
    assert (o.vcycles, o.resident, o.jet, o.fm) == (2, 1, 0, -1)
    st = ka.PipelineStats()
    assert len(st.vcycle_cuts) == ka.KMP_PIPELINE_MAX_VCYCLES == 16
    st.vcycles_run = 2
    st.vcycle_cuts[0], st.vcycle_cuts[1] = 50, 40
    assert st.cycle_cuts == [50, 40]


@pytest.mark.parametrize("vcycles", [-1, 17])
def test_bad_vcycles_are_refused_on_the_host(vcycles, capfd):
    """-1 with one line on stderr before an engine exists, by both drivers
    and by kmp_vcycle_ex; the Python drivers raise before they start."""
    g = ka.Graph.rmat(8, 8, 1)
    opts = _lib.kmp_pipeline_opts_default()
    opts.vcycles = vcycles
    for fn in (_lib.kmp_partition_ex, _lib.kmp_partition_deep_ex, _lib.kmp_vcycle_ex):
        part = np.full(g.n, 1, dtype=np.uint32)
        capfd.readouterr()
        assert fn(g._h, 4, 0.03, 1, ctypes.byref(opts), _u32p(part), None) == -1
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and "vcycles" in err
        assert (part == 1).all()
    if vcycles < 0:
        from kaminpar_amd.partition import partition, partition_deep
        for drv in (partition, partition_deep):
            with pytest.raises(ValueError):
                drv(g, 4, vcycles=vcycles)
        with pytest.raises(RuntimeError):
            g.partition_native(4, vcycles=vcycles)


def test_vcycle_ex_refuses_bad_input_on_the_host(capfd):
    g = ka.Graph.rmat(8, 8, 1)
    opts = _lib.kmp_pipeline_opts_default()
    part = np.zeros(g.n, dtype=np.uint32)
    part[5] = 4  # not below k
    capfd.readouterr()
    assert _lib.kmp_vcycle_ex(g._h, 4, 0.03, 1, ctypes.byref(opts), _u32p(part), None) == -1
    assert "part_inout[5] = 4" in capfd.readouterr().err
    # a resident input needs resident = 1 and an engine
    assert _lib.kmp_vcycle_ex(g._h, 4, 0.03, 1, ctypes.byref(opts), None, None) == -1
    assert "part_inout == NULL" in capfd.readouterr().err
