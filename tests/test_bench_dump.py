"""bench.py --dump-outputs on the host: what fits the budget is written whole, a larger result as a fixed seeded sample of its
flat indices (the recipe in dump_outputs' docstring), in the result's own element type, never more bytes than the budget."""
import os

import numpy as np
import torch

import bench


def _out(dtype):
    return torch.arange(2 * 3 * 5 * 7, dtype=dtype).reshape(2, 3, 5, 7) * 0.5


def test_small_result_is_written_whole(tmp_path):
    out = _out(torch.float64)
    bench.dump_outputs(str(tmp_path), out, 0, 1, budget=out.numel() * 8)
    assert os.listdir(tmp_path) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float64 and np.array_equal(got, out.numpy())


def test_large_result_is_a_seeded_sample(tmp_path):
    out = _out(torch.float32)
    budget = 64 * 4
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), out, 0, 1, budget=budget)
        assert os.listdir(tmp_path / run) == ["out_sample.npy"]
        assert os.path.getsize(tmp_path / run / "out_sample.npy") <= budget + 128          # + the .npy header
    a, b = np.load(tmp_path / "a" / "out_sample.npy"), np.load(tmp_path / "b" / "out_sample.npy")
    idx = np.unique(np.random.default_rng(20240807).integers(0, out.numel(), 64))
    assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(a, out.numpy().reshape(-1)[idx])


def test_ranks_share_the_budget_and_name_their_files(tmp_path):
    out = _out(torch.float64)
    for rank in range(2):
        bench.dump_outputs(str(tmp_path), out, rank, 2, budget=out.numel() * 8)
    assert sorted(os.listdir(tmp_path)) == ["out_sample_rank0.npy", "out_sample_rank1.npy"]
    assert np.load(tmp_path / "out_sample_rank0.npy").size <= out.numel() // 2
