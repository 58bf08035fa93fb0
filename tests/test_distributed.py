"""Multi-process (gloo, CPU) tests of the d-sharded WTA protocol (no GPU).

`stereo_matchin_amd.distributed.sharded_wta` is the host logic every rank runs
on the GPU over RCCL.  Here the same function runs in two (and three) real
processes over torch.distributed's gloo backend, with a CPU restatement of the
four per-shard stage kernels (asw_wta_local / _target_local / _second /
_finalize, include/asw.h) written in tests/wta_shard_ref.py from the reference's WTA
rules (K/asw_wta.cl:12-82).  The gathered result must equal the oracle's
unsharded WTA (oracle_wta, pinned to the reference in test_oracle_golden.py)
bit for bit, on volumes built with many exact ties and with NaN-free zero gaps.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from stereo_matchin_amd.distributed import shard_range, sharded_wta
from wta_shard_ref import CpuShardOps, well_volume


def _volume(D, H, W, seed, kind="levels"):
    if kind == "wells":  # deep wells, ties across shards, a target scan that decides
        return well_volume(D, H, W, seed)
    rng = np.random.default_rng(seed)
    # few distinct levels -> many exact ties across shards (the tie rules matter)
    C = rng.integers(1, 12, size=(D, H, W)).astype(np.float32) * np.float32(0.25)
    C[:, 0, :3] = 5.0  # a pixel row with an all-equal start
    return C


def _worker(rank, world, store, D, H, W, seed, out_path, kind="levels"):
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    try:
        C = _volume(D, H, W, seed, kind)  # plane-major [D][H][W]
        b, e = shard_range(D, rank, world)
        local = torch.from_numpy(np.ascontiguousarray(C[b:e].transpose(1, 2, 0)))

        def reduce_min(t):
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return t

        d_ref, conf_ref, d_tar, conf_tar = sharded_wta(CpuShardOps(b, e, D), local, reduce_min)
        if rank == 0:
            np.savez(out_path, d_ref=d_ref, conf_ref=conf_ref, d_tar=d_tar, conf_tar=conf_tar)
    finally:
        dist.destroy_process_group()


def _group_worker(rank, world, G, store, D, H, W, out_dir):
    """bench.py's layout: world/G frame groups, each d-sharded over its G ranks."""
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    try:
        groups, gid, grank = world // G, rank // G, rank % G
        subs = [dist.new_group(list(range(g * G, (g + 1) * G))) for g in range(groups)]
        pg = subs[gid]
        C = _volume(D, H, W, 777 + gid)  # one frame per group
        b, e = shard_range(D, grank, G)
        local = torch.from_numpy(np.ascontiguousarray(C[b:e].transpose(1, 2, 0)))

        def reduce_min(t):
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=pg)
            return t

        d_ref, conf_ref, d_tar, conf_tar = sharded_wta(CpuShardOps(b, e, D), local, reduce_min)
        stat = torch.tensor([float(rank)])
        dist.all_reduce(stat, op=dist.ReduceOp.MAX)  # the bench's max-over-ranks on the world group
        assert stat.item() == world - 1
        if grank == 0:
            np.savez(os.path.join(out_dir, f"g{gid}.npz"), d_ref=d_ref, d_tar=d_tar, conf_ref=conf_ref,
                     conf_tar=conf_tar)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,G", [(4, 0), (8, 0), (8, 8)])
def test_frame_groups_gloo(oracle, tmp_path, world, G):
    """bench.py --gpus 4 / 8 layouts on gloo: plan_groups' 2-way groups (G = 0), and one
    frame d-sharded 8 ways (--group-size 8)."""
    from stereo_matchin_amd.distributed import plan_groups
    D, H, W = 16, 4, 18
    if not G:
        G = plan_groups(D, world, min_planes=8)
        assert G == 2
    mp.start_processes(_group_worker, args=(world, G, _store(tmp_path), D, H, W, str(tmp_path)), nprocs=world,
                       join=True, start_method="spawn")
    for gid in range(world // G):
        got = np.load(tmp_path / f"g{gid}.npz")
        dr, cr, dt, ct = oracle.wta(_volume(D, H, W, 777 + gid))
        assert np.array_equal(got["d_ref"], dr) and np.array_equal(got["d_tar"], dt)
        np.testing.assert_array_equal(got["conf_ref"], cr)
        np.testing.assert_array_equal(got["conf_tar"], ct)


def test_plan_groups():
    from stereo_matchin_amd.distributed import plan_groups
    assert [plan_groups(256, n) for n in (1, 2, 4, 8)] == [1, 2, 2, 2]
    assert plan_groups(512, 8) == 2 and plan_groups(61, 2) == 1 and plan_groups(128, 8) == 2
    assert plan_groups(256, 3) == 3 and plan_groups(100, 3) == 1 and plan_groups(256, 6) == 2


def _store(tmp_path):
    """A FileStore rendezvous file in the test's own directory: no TCP port to pick, so
    concurrent tests (pytest -n) cannot race for one."""
    return str(tmp_path / "rendezvous")


_GLOO_CASES = [(2, 16, 6, 20), (3, 13, 5, 17), (2, 61, 4, 70), (8, 64, 4, 40)]


def _gloo_matches_oracle(oracle, tmp_path, world, D, H, W, kind):
    seed = 1234 + world + D
    out = str(tmp_path / "res.npz")
    mp.start_processes(_worker, args=(world, _store(tmp_path), D, H, W, seed, out, kind), nprocs=world, join=True,
                       start_method="spawn")
    got = np.load(out)
    dr, cr, dt, ct = oracle.wta(_volume(D, H, W, seed, kind))
    assert np.array_equal(got["d_ref"], dr)
    assert np.array_equal(got["d_tar"], dt)
    np.testing.assert_array_equal(got["conf_ref"], cr)
    np.testing.assert_array_equal(got["conf_tar"], ct)


@pytest.mark.parametrize("world,D,H,W", _GLOO_CASES)
def test_sharded_wta_gloo_matches_oracle(oracle, tmp_path, world, D, H, W):
    _gloo_matches_oracle(oracle, tmp_path, world, D, H, W, "levels")


@pytest.mark.parametrize("world,D,H,W", _GLOO_CASES)
def test_sharded_wta_gloo_matches_oracle_wells(oracle, tmp_path, world, D, H, W):
    """The same cases on the well volume: the minimum tied across shards and a target scan
    that leaves d_ref, often into another shard (tests/wta_shard_ref.py)."""
    _gloo_matches_oracle(oracle, tmp_path, world, D, H, W, "wells")


def test_shard_range_covers_exactly():
    for D in (1, 16, 61, 256, 512):
        for world in range(1, min(D, 9) + 1):
            spans = [shard_range(D, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == D
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(e - b for b, e in spans) - min(e - b for b, e in spans) <= 1
    with pytest.raises(ValueError):
        shard_range(4, 0, 5)
