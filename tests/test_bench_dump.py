"""bench.py --dump-outputs: what it writes for a batch that fits the budget and for one that does not (CPU tensors: the helper only copies)."""
import numpy as np
import torch

import bench


def test_dump_writes_the_whole_batch_when_it_fits(tmp_path):
    a, b = torch.rand(4, 8, 3, 2), torch.rand(4, 8, 3, 1, dtype=torch.float64)
    rows = bench.dump_outputs(str(tmp_path), {"a": a, "b": b})
    assert rows == [0, 1, 2, 3]
    got_a, got_b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert got_a.dtype == np.float32 and got_b.dtype == np.float32
    np.testing.assert_array_equal(got_a, a.numpy())
    np.testing.assert_array_equal(got_b, b.float().numpy())


def test_dump_samples_the_same_seeded_rows_of_every_output_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * (16 + 8) * 4)   # room for 10 rows of both
    a, b = torch.rand(64, 16), torch.rand(64, 8)
    rows = bench.dump_outputs(str(tmp_path / "x"), {"a": a, "b": b})
    assert len(rows) == 10 and rows == sorted(set(rows)) and max(rows) < 64
    np.testing.assert_array_equal(np.load(tmp_path / "x" / "a.npy"), a[rows].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "x" / "b.npy"), b[rows].numpy())
    assert bench.dump_outputs(str(tmp_path / "y"), {"a": a, "b": b}) == rows
    # the benchmark's own shape (B = 256 of 512x256, three output planes per sample) stays within 64 MB
    per_row = 512 * 256 * 3 * 4
    monkeypatch.undo()
    assert (bench.DUMP_BUDGET_BYTES // per_row) * per_row <= 64e6
