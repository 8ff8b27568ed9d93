"""bench.py --dump-outputs (no GPU): the arrays of the last timed step as float32 .npy files, within the size cap, with the
same fixed sample on every run when an array is larger than its share."""
import os

import numpy as np
import torch

import bench


def test_small_arrays_are_written_whole_in_float32(tmp_path):
    lat = torch.randn(1, 3, 4, 5, 6)
    pred = torch.randn(2, 3, 4, 5, 6).to(torch.bfloat16)
    shapes = bench.dump_outputs(str(tmp_path / "out"), {"latents": lat, "noise_pred": pred})
    assert shapes == {"latents": [1, 3, 4, 5, 6], "noise_pred": [2, 3, 4, 5, 6]}
    a, b = np.load(tmp_path / "out" / "latents.npy"), np.load(tmp_path / "out" / "noise_pred.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, lat.numpy()) and np.array_equal(b, pred.float().numpy())


def test_large_arrays_are_sampled_at_fixed_positions_within_the_cap(tmp_path):
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    cap = 2 * 4 * 300                                  # two arrays of 300 float32 values each
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": big, "y": -big}, max_bytes=cap)
    total = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert total <= cap
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.shape == (300,) and np.all(np.diff(x) > 0)                  # sorted distinct flat positions
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))          # the same sample on every run
    assert np.array_equal(-x, np.load(tmp_path / "a" / "y.npy"))         # and at the same positions for every array
