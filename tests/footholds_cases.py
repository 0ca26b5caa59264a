"""Scenes and a numpy statement of lrm_footholds_* (include/lrm.h): per (leg, body) the count of reachable targets and
the reachable target nearest the leg's nominal point, d2 in float32 without contraction."""
import ctypes as C

import numpy as np

QUATS = {"identity": (1.0, 0.0, 0.0, 0.0), "tilted": (0.98, 0.05, -0.12, 0.1)}


def scene(nb, nt, seed, half=600.0):
    """rough terrain patch and bodies hovering 100-300 mm above it (test_gpu_positionability.py's shape, denser)"""
    rng = np.random.default_rng(seed)
    txy = rng.uniform(-half, half, (nt, 2))
    tz = 40 * np.sin(txy[:, 0] / 150) + 30 * np.cos(txy[:, 1] / 110) + rng.normal(0, 5, nt)
    targets = np.column_stack([txy, tz]).astype(np.float32)
    bxy = rng.uniform(-0.8 * half, 0.8 * half, (nb, 2))
    bz = rng.uniform(60, 330, nb)
    return np.column_stack([bxy, bz]).astype(np.float32), targets


def legs_for(lrm, nlegs, quat):
    return np.stack([lrm.rotate_leg_data(quat, lrm.get_M2_leg(2 * np.pi * k / nlegs)) for k in range(nlegs)])


def nominal_for(nlegs, seed=3):
    return np.random.default_rng(seed).uniform(-250, 250, (nlegs, 3)).astype(np.float32)


def oracle_reachable(oracle, bodies, targets, legs, quat):
    """[nlegs, nb, nt] bool from the oracle's orc_reachable_rotate_leg (several_leg.cu:48-67), one call per pair"""
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(
        C.cast(oracle.lib.orc_reachable_rotate_leg, C.c_void_p).value)
    bodies = np.ascontiguousarray(bodies, np.float32)
    targets = np.ascontiguousarray(targets, np.float32)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    q = np.ascontiguousarray(quat, np.float32)
    tp, bp, qp, lp = targets.ctypes.data, bodies.ctypes.data, q.ctypes.data, legs.ctypes.data
    out = np.zeros((len(legs), len(bodies), len(targets)), bool)
    for l in range(len(legs)):
        for b in range(len(bodies)):
            row = out[l, b]
            for t in range(len(targets)):
                row[t] = fn(tp + 12 * t, bp + 12 * b, qp, lp + 56 * l)
    return out


def expected(reach, bodies, targets, nominal):
    """count, best, best_d2 from a [nlegs, nb, nt] reachability array, with lrm.h's d2 in numpy float32"""
    nl = reach.shape[0]
    nom = np.zeros((nl, 3), np.float32) if nominal is None else np.asarray(nominal, np.float32)
    c = bodies[None, :, :] + nom[:, None, :]                       # [L, B, 3]: one f32 add per component
    d = targets[None, None, :, :] - c[:, :, None, :]               # [L, B, T, 3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    count = reach.sum(-1).astype(np.int32)
    masked = np.where(reach, d2, np.float32(np.inf))
    best = np.argmin(masked, axis=-1).astype(np.int32)           # first occurrence: ties go to the smaller index
    best_d2 = np.take_along_axis(masked, best[..., None], -1)[..., 0].astype(np.float32)
    best[count == 0] = -1
    return count, best, best_d2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
