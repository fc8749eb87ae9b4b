"""bench.py's command line and its --dump-outputs writer (host logic only: no device, no library)."""
import numpy as np
import torch

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    b = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert b.full and b.dump_outputs == "somewhere"


def test_sample_rows_is_whole_below_the_limit_and_fixed_above_it():
    t = torch.arange(40.0).reshape(20, 2)
    assert bench.sample_rows(t, 0, 20) is t
    s1, s2 = bench.sample_rows(t, 0, 8), bench.sample_rows(t.clone(), 0, 8)
    assert s1.shape == (8, 2) and torch.equal(s1, s2)
    assert torch.all(s1[1:, 0] > s1[:-1, 0])  # distinct rows of t, in t's order
    assert bench.sample_rows(t, 1, 1).shape == (20, 1)


def test_dump_outputs_writes_float32_arrays_within_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PIXELS", 50)
    monkeypatch.setattr(bench, "DUMP_GAUSSIANS", 16)
    g = torch.Generator().manual_seed(3)
    small, big = torch.randn(3, 5, 10, generator=g), torch.randn(1, 9, 11, generator=g)
    radii = torch.arange(100, dtype=torch.int32)
    grads = torch.randn(100, 4, 3, generator=g)
    shapes = bench.dump_outputs(str(tmp_path / "d"), {"color": small, "invdepth": big},
                                {"radii": radii, "dL_dshs": grads, "absent": None, "few": grads[:16]})
    assert shapes == {"color": [3, 5, 10], "invdepth": [1, 50], "radii": [16], "dL_dshs": [16, 4, 3],
                      "few": [16, 4, 3]}
    files = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert files == ["color.npy", "dL_dshs.npy", "few.npy", "invdepth.npy", "radii.npy"]
    out = {n[:-4]: np.load(tmp_path / "d" / n) for n in files}
    assert all(a.dtype == np.float32 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(out["color"], small.numpy()) and np.array_equal(out["few"], grads[:16].numpy())
    # every per-Gaussian array of one length keeps the same rows, so row i of each belongs to one Gaussian
    rows = out["radii"].astype(np.int64)
    assert np.array_equal(out["dL_dshs"], grads.numpy()[rows])
    assert np.isin(out["invdepth"][0], big.numpy().ravel()).all()
