"""CPU checks of bench.py's host-side helpers (the timed path itself needs a GPU)."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_chunk_seeded_shards_are_slices_of_one_cloud():
    """N > 1: every rank generates only its shard; the shards of any world size must be slices of the SAME cloud."""
    from lrm_amd import shard
    b = _bench()
    n = 2_500_000  # 2.5 chunks
    whole = b.make_shard(0, n)
    assert whole.shape == (3, n) and whole.dtype == np.float32
    assert (whole.min(axis=1) >= b.LO).all() and (whole.max(axis=1) <= b.HI).all()
    for world in (2, 3, 8):
        parts = [b.make_shard(*shard.shard_bounds(n, world, r)) for r in range(world)]
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
    # config 2 (N = 1) keeps the cloud of the tests and of the committed profiles
    from conftest import random_cloud
    assert np.array_equal(b.make_cloud(100_000, 42).T, random_cloud(100_000, seed=42))


def test_committed_profile_lookup_is_tied_to_the_kernel_sources(tmp_path):
    """bench.py prints the PMC figures of profiles/ only when they were taken with the tree's kernel sources
    (kernel_src_sha); anything else is reported as stale, never mixed in."""
    from lrm_amd.srchash import kernel_src_sha
    b = _bench()
    sha = kernel_src_sha()
    assert len(sha) == 64 and sha == kernel_src_sha()
    json.dump({"points_per_launch": 10_000_000, "mode": "tol", "step_hbm_bytes": 2.7e8, "kernel_src_sha": sha}, open(tmp_path / "r09_hbm_traffic.json", "w"))
    json.dump({"mode": "tol", "valu_insts_per_eval": 400.0, "kernel_src_sha": sha}, open(tmp_path / "r09_valu.json", "w"))
    json.dump({"points_per_launch": 10_000_000, "mode": "fast", "step_hbm_bytes": 2.5e8, "kernel_src_sha": "0" * 64}, open(tmp_path / "r09fast_hbm_traffic.json", "w"))
    p = b.committed_profile(10_000_000, "tol", str(tmp_path))
    assert p["traffic"] == 2.7e8 and p["traffic_source"] == "r09_hbm_traffic.json" and p["valu_insts_per_eval"] == 400.0 and p["kernel_src_sha"] == sha
    f = b.committed_profile(10_000_000, "fast", str(tmp_path))
    assert f["traffic"] is None and f["traffic_source"].startswith("stale") and f["valu_insts_per_eval"] is None
    assert b.committed_profile(12345, "tol", str(tmp_path))["traffic"] is None
    # the repository's own profiles: whatever matches the tree must be plausible
    p = b.committed_profile(10_000_000, "tol")
    if p["traffic"] is not None:
        assert 250e6 < p["traffic"] < 320e6          # algorithmic 251.25 MB + the fix-up's scattered accesses
    if p["valu_insts_per_eval"] is not None:
        assert 300 < p["valu_insts_per_eval"] < 800


def test_dump_outputs_writes_a_fixed_bounded_sample(tmp_path):
    """--dump-outputs: the same sorted sample of point indices in every run, float32 / float64 files of at most 64 MB,
    and each file holds the outputs of exactly the sampled points (the bit words unpacked in the shard.pack_bits layout)."""
    import torch
    from lrm_amd import shard
    b = _bench()
    n = b.DUMP_POINTS + 250_001  # larger than the sample
    idx = b.dump_sample(n)
    assert len(idx) == b.DUMP_POINTS and np.array_equal(idx, b.dump_sample(n))
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(b.dump_sample(1000), np.arange(1000))
    rng = np.random.default_rng(0)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    field = rng.standard_normal((3, n)).astype(np.float32)
    words = torch.from_numpy(shard.pack_bits(mask))
    files = b.dump_outputs(str(tmp_path / "out"), torch.from_numpy(mask), torch.from_numpy(field), words, n)
    assert files == ["dist_field.npy", "reach_bits.npy", "reach_mask.npy", "sample_index.npy"]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["sample_index"], idx.astype(np.float64))
    assert np.array_equal(got["reach_mask"], mask[idx].astype(np.float32))
    assert np.array_equal(got["reach_bits"], mask[idx].astype(np.float32))
    assert got["dist_field"].shape == (3, len(idx)) and np.array_equal(got["dist_field"], field[:, idx])


def test_steps_must_be_positive():
    b = _bench()
    assert b.parse_args(["--steps", "7"]).steps == 7
    with pytest.raises(SystemExit):
        b.parse_args(["--steps", "0"])
