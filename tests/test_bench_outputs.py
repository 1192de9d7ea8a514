"""bench.py --dump-outputs: what the last timed step computed, as float32 / float64 .npy files of at most 64 MB in all, the
same for the same arguments (a fixed seeded sample where an output is larger than its budget).  The helper runs on CPU
tensors here; bench.py hands it the GPU's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch = pytest.importorskip("torch")
import bench  # noqa: E402


def test_dump_is_bounded_seeded_and_exact(tmp_path):
    # all three past their budgets (16-byte blocks: a block table of 1.5 Mi entries), the most the dump can write
    g = torch.Generator().manual_seed(5)
    offsets = torch.cumsum(torch.randint(30, 50, ((3 << 19) + 1,), generator=g), 0)
    offsets[0] = 0
    comp = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, generator=g)
    out = torch.randint(0, 256, (64 << 20,), dtype=torch.uint8, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), offsets, comp, out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["compressed.npy", "decoded.npy", "offsets.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64_000_000
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    # exact values, in windows of consecutive elements at the seeded positions
    for name, src, seed in (("offsets", offsets, bench.DUMP_SEED), ("compressed", comp, bench.DUMP_SEED + 1), ("decoded", out, bench.DUMP_SEED + 2)):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        starts = np.sort(np.random.default_rng(seed).integers(0, src.numel() - bench.DUMP_WINDOW + 1, size=len(got) // bench.DUMP_WINDOW))
        for w in (0, 17, len(starts) - 1):
            s = int(starts[w])
            assert np.array_equal(got[w * bench.DUMP_WINDOW: (w + 1) * bench.DUMP_WINDOW], src[s: s + bench.DUMP_WINDOW].numpy().astype(got.dtype)), name


def test_small_outputs_are_dumped_whole(tmp_path):
    offsets = torch.tensor([0, 70, 95], dtype=torch.int64)
    comp = torch.arange(95, dtype=torch.int64).to(torch.uint8)
    out = torch.arange(100000, dtype=torch.int64).remainder(251).to(torch.uint8)
    bench.dump_outputs(str(tmp_path), offsets, comp, out)
    assert np.array_equal(np.load(tmp_path / "compressed.npy"), comp.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "decoded.npy"), out.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "offsets.npy"), [0.0, 70.0, 95.0])
