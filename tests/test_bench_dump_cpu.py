"""bench.py --dump-outputs on the host: small arrays whole, large ones as a fixed seeded sample under the budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_small_arrays_whole_and_samples_large_ones(tmp_path):
    g = torch.Generator().manual_seed(0)
    frames, F = torch.rand((8, 720, 1280, 3), generator=g), torch.rand((8, 25, 2), generator=g)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"s_t_pred": frames, "F_t": F}, bench.DUMP_BUDGET_BYTES, "_rank1")
    assert sorted(os.listdir(tmp_path / "a")) == ["F_t_rank1.npy", "s_t_pred_sample_rank1.npy"]
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 64e6
    assert np.array_equal(np.load(tmp_path / "a" / "F_t_rank1.npy"), F.numpy())
    sample = np.load(tmp_path / "a" / "s_t_pred_sample_rank1.npy")
    idx = np.unique(np.random.default_rng(0).integers(0, frames.numel(), size=(bench.DUMP_BUDGET_BYTES - F.numel() * 4) // 4))
    assert sample.dtype == np.float32 and np.array_equal(sample, frames.reshape(-1).numpy()[idx])
    assert np.array_equal(sample, np.load(tmp_path / "b" / "s_t_pred_sample_rank1.npy"))


def test_dump_writes_everything_whole_when_it_fits(tmp_path):
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path), {"tf_warp_out": x}, 1 << 20)
    got = np.load(tmp_path / "tf_warp_out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
