"""Shared cases of the batched multi-pose queries (tests/test_posed_cpu.py, tests/test_gpu_posed.py): a pose table, a leg
table, queries in several index orders, and the oracle's answer computed per (pose, leg) on target - body."""
import numpy as np

from conftest import golden_cases, load_case


def random_unit_quats(n, rng):
    q = rng.standard_normal((n, 4)).astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def fixture_quats():
    seen = []
    for name in golden_cases():
        q = np.asarray(load_case(name)["quat"], np.float32).reshape(4)
        if not any(np.array_equal(q, s) for s in seen):
            seen.append(q)
    return np.array(seen, np.float32)


def pose_table(lrm, n=37, seed=5):
    """n poses: identity, every fixture quat, a spread of the reference's sweep quats, random unit quats; body positions
    random (the identity pose sits at the origin)"""
    from lrm_amd import workloads
    rng = np.random.default_rng(seed)
    sweep = workloads.reference_sweep_quats()
    fq = fixture_quats()
    qs = [np.array([1, 0, 0, 0], np.float32)] + list(fq) + list(sweep[::4])
    qs = np.array(qs[:n], np.float32)
    if len(qs) < n:
        qs = np.concatenate([qs, random_unit_quats(n - len(qs), rng)])
    body = (rng.random((n, 3), dtype=np.float32) * np.float32(4000) - np.float32(2000)).astype(np.float32)
    body[0] = 0
    return qs, body


def leg_table(lrm):
    from lrm_amd import workloads
    return np.concatenate([workloads.hexapod(lrm.get_moonbot_leg), lrm.get_M2_leg(0.7)[None]]).astype(np.float32)


def queries(nposes, nlegs, body, per_pair, rng, order="shuffled"):
    """targets around each pose's body position; pose / leg index per query in the given order:
    pair_major [pose, leg, k], interleaved [k, pose, leg] (leg fastest), shuffled (a random permutation)"""
    pose = np.repeat(np.arange(nposes, dtype=np.int32), nlegs * per_pair)
    leg = np.tile(np.repeat(np.arange(nlegs, dtype=np.uint8), per_pair), nposes)
    if order == "interleaved":
        pose = np.tile(np.repeat(np.arange(nposes, dtype=np.int32), nlegs), per_pair)
        leg = np.tile(np.arange(nlegs, dtype=np.uint8), nposes * per_pair)
    n = len(pose)
    lo = np.array([-450, -450, -400], np.float32)
    hi = np.array([450, 450, 200], np.float32)
    off = (rng.random((n, 3), dtype=np.float32) * (hi - lo) + lo).astype(np.float32)
    xyz = (off + body[pose]).astype(np.float32)
    if order == "shuffled":
        perm = rng.permutation(n)
        xyz, pose, leg = xyz[perm], pose[perm], leg[perm]
    return np.ascontiguousarray(xyz), np.ascontiguousarray(pose), np.ascontiguousarray(leg)


def oracle_answer(oracle, xyz, pose, leg, quats, body, legs):
    """(mask, valid, field) of every query, from the oracle per (pose, leg) on p = target - body (f32)"""
    n = len(xyz)
    mask, valid, field = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    p_all = (xyz - (body[pose] if body is not None else np.float32(0))).astype(np.float32)
    key = pose.astype(np.int64) * len(legs) + leg
    order = np.argsort(key, kind="stable")
    keys, starts = np.unique(key[order], return_index=True)
    for k, sel in zip(keys, np.split(order, starts[1:])):
        pi, li = int(k) // len(legs), int(k) % len(legs)
        p = np.ascontiguousarray(p_all[sel])
        mask[sel] = oracle.reach(p, legs[li], quats[pi])
        d, v = oracle.dist(p, legs[li], quats[pi])
        field[sel], valid[sel] = d, v
    return mask, valid, field
