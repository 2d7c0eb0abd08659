"""Host-only side of the C pipeline drivers with options: the defaults, the
ctypes mirrors' layout, the shim's preset setter and the refusal of bad options,
which is decided before any engine exists and so needs no GPU."""

import ctypes

import numpy as np
import pytest

import kaminpar_amd as ka
from kaminpar_amd import _lib, _u32p


def same_struct(a, b):
    assert bytes(a) == bytes(b)


def test_default_options():
    o = _lib.kmp_pipeline_opts_default()
    assert (o.iters, o.contraction_limit, o.stop_n, o.split_c, o.ip_reps) == (5, 0, 0, 0, 0)
    assert (o.jet, o.fm, o.resident, o.engine) == (0, -1, 0, None)
    fine, coarse = _lib.kmp_jet_params_default(0), _lib.kmp_jet_params_default(1)
    assert fine.initial_gain_temp == 0.25 and coarse.initial_gain_temp == 0.75
    for got, want in ((o.jet_fine, fine), (o.jet_coarse, coarse)):
        for name, _ in ka.JetParams._fields_:
            assert getattr(got, name) == getattr(want, name), name
    assert _lib.kmp_jet_params_valid(ctypes.byref(o.jet_fine)) == 1
    assert _lib.kmp_jet_params_valid(ctypes.byref(o.jet_coarse)) == 1
    assert _lib.kmp_jet_params_valid(None) == 0
    # the keyword form starts from the same defaults
    same_struct(ka.pipeline_opts(), o)


@pytest.mark.parametrize("mirror,size,layout", [
    (ka.PipelineOpts, "kmp_pipeline_opts_size", "kmp_pipeline_opts_layout"),
    (ka.PipelineStats, "kmp_pipeline_stats_size", "kmp_pipeline_stats_layout"),
])
def test_mirrors_match_the_library(mirror, size, layout):
    assert ctypes.sizeof(mirror) == getattr(_lib, size)()
    cap = 32
    off = (ctypes.c_uint32 * cap)()
    count = getattr(_lib, layout)(off, cap)
    assert count == len(mirror._fields_) <= cap
    assert [getattr(mirror, name).offset for name, _ in mirror._fields_] == list(off[:count])
    # a short buffer is not overrun
    short = (ctypes.c_uint32 * 3)(7, 7, 7)
    assert getattr(_lib, layout)(short, 2) == count and short[2] == 7


def test_stats_levels_view():
    st = ka.PipelineStats()
    assert ka.KMP_PIPELINE_MAX_LEVELS == len(st.level_sizes) == 64
    st.num_levels = 3
    st.level_sizes[0], st.level_sizes[1], st.level_sizes[2] = 1000, 300, 90
    assert st.levels == [1000, 300, 90]


def test_keywords_fill_the_options():
    o = ka.pipeline_opts(iters=3, jet=dict(balancer=1, max_iterations=4), fm=False,
                         resident=True, contraction_limit=100, stop_n=64, split_c=9)
    assert (o.iters, o.contraction_limit, o.stop_n, o.split_c) == (3, 100, 64, 9)
    assert (o.jet, o.fm, o.resident) == (1, 0, 1)
    for p in (o.jet_fine, o.jet_coarse):
        assert p.balancer == ka.JET_BALANCER_SELECT and p.max_iterations == 4
    assert o.jet_fine.initial_gain_temp == 0.25 and o.jet_coarse.initial_gain_temp == 0.75
    assert ka.pipeline_opts(jet=True).jet == 1 and ka.pipeline_opts(fm=True).fm == 1
    assert ka.pipeline_opts(jet={}).jet == 0  # as `if jet:` in partition()
    with pytest.raises(TypeError):
        ka.pipeline_opts(jet=dict(balance_passes=2, temperature=0.5))


def test_set_preset_return_codes():
    shm = _lib.kaminpar_amd_create(1)
    try:
        assert _lib.kaminpar_amd_set_preset(shm, b"default") == 0
        assert _lib.kaminpar_amd_set_preset(shm, b"jet") == 0
        assert _lib.kaminpar_amd_set_preset(shm, b"nope") == -1
        assert _lib.kaminpar_amd_set_preset(shm, b"") == -1
        assert _lib.kaminpar_amd_set_preset(shm, None) == -1
        assert _lib.kaminpar_amd_set_preset(shm, b"default") == 0
    finally:
        _lib.kaminpar_amd_free(shm)


def _bad_fm(o):
    o.fm = 2


def _bad_jet(o):
    o.jet = 3


def _bad_resident(o):
    o.resident = 2


def _jet_without_stop(o):
    o.jet = 1
    o.jet_fine.max_iterations = 0
    o.jet_fine.max_fruitless = 0


def _jet_bad_coarse(o):
    o.jet = 1
    o.jet_coarse.balance_iters = 0


def _jet_only(o):
    o.jet = 1


@pytest.mark.parametrize("mutate,k", [
    (_bad_fm, 4), (_bad_jet, 4), (_bad_resident, 4), (_jet_without_stop, 4),
    (_jet_bad_coarse, 4), (_jet_only, 4096),
], ids=["fm", "jet", "resident", "jet-no-stop", "jet-coarse", "jet-k4096"])
def test_bad_options_are_refused_on_the_host(mutate, k, capfd):
    """-1 with one line on stderr, before an engine is created: with a GPU or
    without one, the refusal never gets as far as needing it."""
    g = ka.Graph.rmat(8, 8, 1)
    opts = _lib.kmp_pipeline_opts_default()
    mutate(opts)
    for fn in (_lib.kmp_partition_ex, _lib.kmp_partition_deep_ex):
        part = np.full(g.n, 77, dtype=np.uint32)
        capfd.readouterr()
        assert fn(g._h, k, 0.03, 1, ctypes.byref(opts), _u32p(part), None) == -1
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("kaminpar_amd: kmp_partition")
        assert (part == 77).all()
    if mutate is _jet_only:  # the keyword form raises
        with pytest.raises(RuntimeError):
            g.partition_deep_native(k, jet=True)
