"""bench.py --dump-outputs writer (host-only: no engine involved)."""

import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_output_is_written_whole(tmp_path):
    labels = (np.arange(1000, dtype=np.uint32) * 7) % 16
    bench.dump_outputs(str(tmp_path / "a"), labels, 4321)
    out = _load(tmp_path / "a")
    assert sorted(out) == ["label_counts", "labels", "result"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["labels"], labels)
    assert np.array_equal(out["label_counts"][:16], np.bincount(labels))
    assert out["label_counts"].sum() == labels.size
    assert out["result"].tolist() == [4321.0]


def test_dump_large_output_is_a_fixed_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    labels = (np.arange(n, dtype=np.uint32) * 2654435761) >> 6  # ids up to 2^26
    bench.dump_outputs(str(tmp_path / "a"), labels, 1)
    bench.dump_outputs(str(tmp_path / "b"), labels, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["labels"].shape == (bench.DUMP_SAMPLE,)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert np.array_equal(a[name], b[name])
    # the sample holds real entries, exactly (float64 carries every u32)
    assert np.isin(a["labels"][:1000], labels).all()
    # one changed label anywhere shows in the whole-array digest
    labels2 = labels.copy()
    labels2[n // 2] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), labels2, 1)
    assert not np.array_equal(_load(tmp_path / "c")["label_counts"],
                              a["label_counts"])
