"""bench.py --dump-outputs on the host: what dump_outputs writes (dtypes, the size cap, the seeded row sample)."""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    a = torch.randn(3, 5)
    g = torch.randn(4, dtype=torch.float64)
    loss = torch.tensor(0.25)
    bench.dump_outputs(str(tmp_path), {"a": a, "g": g, "loss": loss})
    out = _load(tmp_path)
    assert out["a"].dtype == np.float32 and out["g"].dtype == np.float64 and out["loss"].dtype == np.float32
    assert np.array_equal(out["a"], a.numpy()) and np.array_equal(out["g"], g.numpy())
    assert out["loss"].shape == () and out["loss"] == np.float32(0.25)


def test_large_outputs_keep_the_same_seeded_rows_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 40_000)
    audio = torch.arange(64 * 100, dtype=torch.float32).reshape(64, 100)          # row r holds 100 r .. 100 r + 99
    bands = torch.arange(64 * 3 * 33, dtype=torch.float32).reshape(64, 3, 33)
    loss = torch.tensor(1.5)
    arrays = {"audio": audio, "bands": bands, "loss": loss}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 40_000
    assert a["audio"].shape[0] == a["bands"].shape[0] and 1 <= a["audio"].shape[0] < 64
    rows = (a["audio"][:, 0] // 100).astype(int)
    assert np.all(np.diff(rows) > 0)                                              # ascending, no repeats
    assert np.array_equal(a["audio"], audio.numpy()[rows])
    assert np.array_equal(a["bands"], bands.numpy()[rows])                        # the same rows of every array
    assert a["loss"] == np.float32(1.5)
    for k in a:                                                                   # the same sample on every run
        assert np.array_equal(a[k], b[k])
