"""Host-only side of the threshold edge sparsification: parameter defaults and
validation, the refusal of bad options by the C drivers before any engine
exists, the keyword form of the options, and the CPU mirror of the drivers
(tests/sparsify_mirror.py) against its fixture. No GPU."""

import ctypes
import json
import math
import os

import numpy as np
import pytest

import kaminpar_amd as ka
import sparsify_mirror as sm
from kaminpar_amd import _lib, _u32p
from oracle_pipeline import oracle_partition

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_default_params():
    p = _lib.kmp_sparsify_params_default()
    assert (p.density_target_factor, p.edge_target_factor, p.laziness_factor) == (0.5, 0.5, 4.0)
    assert _lib.kmp_sparsify_params_valid(ctypes.byref(p)) == 1
    assert _lib.kmp_sparsify_params_valid(None) == 0
    q = ka.sparsify_params(True)
    assert bytes(q) == bytes(p) == bytes(ka.sparsify_params(None)) == bytes(ka.sparsify_params({}))
    o = _lib.kmp_pipeline_opts_default()
    assert o.sparsify == 0 and bytes(o.sparsify_params) == bytes(p)


@pytest.mark.parametrize("field", ["density_target_factor", "edge_target_factor",
                                   "laziness_factor"])
@pytest.mark.parametrize("value", [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_params_valid_rejects(field, value):
    assert not ka.sparsify_params_valid({field: value})


def test_params_valid_laziness_bound():
    assert not ka.sparsify_params_valid(dict(laziness_factor=0.999))
    assert ka.sparsify_params_valid(dict(laziness_factor=1))
    assert ka.sparsify_params_valid(dict(density_target_factor=1e-9, edge_target_factor=7))
    with pytest.raises(ValueError):
        ka.sparsify_params(dict(lazyness=2))


def test_keywords_fill_the_options():
    o = ka.pipeline_opts(sparsify=dict(laziness_factor=2))
    assert o.sparsify == 1
    p = o.sparsify_params
    assert (p.density_target_factor, p.edge_target_factor, p.laziness_factor) == (0.5, 0.5, 2.0)
    assert ka.pipeline_opts(sparsify=True).sparsify == 1
    assert ka.pipeline_opts(sparsify=True).sparsify_params.laziness_factor == 4.0
    assert ka.pipeline_opts(sparsify=False).sparsify == 0
    assert bytes(ka.pipeline_opts()) == bytes(_lib.kmp_pipeline_opts_default())


def test_stats_arcs_view():
    st = ka.PipelineStats()
    assert len(st.level_arcs) == ka.KMP_PIPELINE_MAX_LEVELS
    st.num_levels = 2
    st.level_arcs[0], st.level_arcs[1] = 1 << 33, 77
    assert st.arcs == [1 << 33, 77]


def _bad_flag(o):
    o.sparsify = 2


def _bad_zero(o):
    o.sparsify = 1
    o.sparsify_params.edge_target_factor = 0.0


def _bad_negative(o):
    o.sparsify = 1
    o.sparsify_params.density_target_factor = -0.5


def _bad_nan(o):
    o.sparsify = 1
    o.sparsify_params.density_target_factor = math.nan


def _bad_laziness(o):
    o.sparsify = 1
    o.sparsify_params.laziness_factor = 0.5


@pytest.mark.parametrize("mutate", [_bad_flag, _bad_zero, _bad_negative, _bad_nan,
                                    _bad_laziness],
                         ids=["flag", "zero", "negative", "nan", "laziness"])
def test_bad_options_are_refused_on_the_host(mutate, capfd):
    """-1 with one line on stderr, before an engine is created: with a GPU or
    without one, the refusal never gets as far as needing it."""
    g = ka.Graph.rmat(8, 8, 1)
    opts = _lib.kmp_pipeline_opts_default()
    mutate(opts)
    for fn in (_lib.kmp_partition_ex, _lib.kmp_partition_deep_ex):
        part = np.full(g.n, 77, dtype=np.uint32)
        capfd.readouterr()
        assert fn(g._h, 4, 0.03, 1, ctypes.byref(opts), _u32p(part), None) == -1
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("kaminpar_amd: kmp_partition")
        assert (part == 77).all()


# ------------------------------------------------------------- the mirror
def checksum(part):
    return int(np.bitwise_xor.reduce(
        np.asarray(part, np.uint64) * np.arange(1, len(part) + 1, dtype=np.uint64)))


def expected():
    with open(os.path.join(GOLDEN, "sparsify_expected.json")) as f:
        return json.load(f)


def same_as_fixture(result, want):
    cut, part, levels, stats = result
    assert cut == want["cut"] and levels == want["levels"]
    assert stats["level_arcs"] == want["level_arcs"]
    assert [s["m_before"] for s in stats["sparsify"]] == want["arcs_before"]
    assert [s["m_after"] for s in stats["sparsify"]] == want["arcs_after"]
    assert [s["applied"] for s in stats["sparsify"]] == want["applied"]
    assert checksum(part) == want["part_checksum"]


@pytest.mark.parametrize("driver", ["partition", "partition_deep"])
@pytest.mark.parametrize("laziness", [1, 2])
@pytest.mark.parametrize("scale", [14, 16])
def test_mirror_reproduces_the_fixture(oracle, scale, laziness, driver):
    want = expected()[f"rmat{scale}_s42_k16_lazy{laziness}"]
    g = ka.Graph.rmat(scale, 8, 42)
    opt = dict(laziness_factor=laziness)
    if driver == "partition":
        got = sm.mirror_partition(oracle, g, 16, opt, seed=1)
    else:
        got = sm.mirror_partition_deep(oracle, g, 16, opt, seed=1, split_c=2000)
    same_as_fixture(got, want[driver])
    if laziness == 1:
        assert sum(want[driver]["applied"]) > 0


def test_fixture_holds_every_case():
    want = expected()
    assert sorted(want) == sorted(f"rmat{s}_s42_k16_lazy{z}" for s in (14, 16) for z in (1, 2))
    for case in want.values():
        for drv in ("partition", "partition_deep"):
            r = case[drv]
            assert len(r["levels"]) == len(r["level_arcs"]) == len(r["arcs_after"]) + 1
            assert r["level_arcs"][1:] == r["arcs_after"]
            assert all(a <= b for a, b in zip(r["arcs_after"], r["arcs_before"]))


def test_defaults_do_not_trigger_on_rmat16(oracle):
    """With the defaults (True, or an empty dict of overrides) no level
    triggers, and the mirror equals oracle_partition bit for bit."""
    g = ka.Graph.rmat(16, 8, 42)
    assert ka.sparsify_on({}) and ka.sparsify_on(True)
    assert not ka.sparsify_on(False) and not ka.sparsify_on(None)
    assert ka.pipeline_opts(sparsify={}).sparsify == 1
    cut, part, levels, stats = sm.mirror_partition(oracle, g, 16, True, seed=1)
    assert [s["applied"] for s in stats["sparsify"]] == [0] * (len(levels) - 1)
    ocut, opart, olevels = oracle_partition(oracle, g, 16, seed=1)
    assert cut == ocut and levels == olevels and np.array_equal(part, opart)
