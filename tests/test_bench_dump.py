"""bench.py --dump-outputs on CPU: packed mask words (one rank, or every rank's padded shard) -> one float32 0/1 per
configuration in job order; above the full-dump size a seeded sample with its indices, under 64 MiB in all."""
import os

import numpy as np
import pytest

import bench
from numbotics_amd.parallel import pack_bits, shard_bounds, shard_words


def _words(flags, world):
    """The words bench.py holds after the last step: its own (N = 1) or the all-gathered ones (equal, zero-padded shards)."""
    total = flags.size
    if world == 1:
        return pack_bits(flags)
    g = shard_words(total, world)
    words = np.zeros(world * g, dtype=np.int64)
    for r in range(world):
        lo, hi = shard_bounds(total, world, r)
        pw = pack_bits(flags[lo:hi])
        words[r * g:r * g + pw.size] = pw
    return words


@pytest.mark.parametrize("total,world", [(1, 1), (1000, 1), (1_000_000, 1), (1000, 2), (130, 3), (10_000, 8)])
def test_dump_is_the_mask_in_job_order(tmp_path, total, world):
    flags = np.random.default_rng(total + world).random(total) < 0.1
    info = bench.dump_outputs(str(tmp_path), _words(flags, world), total, world)
    m = np.load(tmp_path / "in_collision.npy")
    assert m.dtype == np.float32 and np.array_equal(m, flags.astype(np.float32))
    assert sorted(os.listdir(tmp_path)) == ["in_collision.npy"]
    assert info["files"] == {"in_collision": {"configurations": total}}


def test_large_dump_is_a_seeded_sample_under_64_mib(tmp_path):
    total = bench.DUMP_MAX_FULL + 4097
    flags = np.random.default_rng(3).random(total) < 0.1
    words = _words(flags, 1)
    bench.dump_outputs(str(tmp_path / "a"), words, total, 1)
    bench.dump_outputs(str(tmp_path / "b"), words, total, 1)
    m = np.load(tmp_path / "a" / "in_collision.npy")
    idx = np.load(tmp_path / "a" / "in_collision_index.npy")
    assert m.dtype == np.float32 and idx.dtype == np.float64 and m.size == idx.size == bench.DUMP_SAMPLE
    assert np.array_equal(m, flags[idx.astype(np.int64)].astype(np.float32))
    assert np.all(np.diff(idx) > 0) and idx[-1] < total
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    for name in ("in_collision.npy", "in_collision_index.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
