"""An independent float64 model of the leg's joint-limit set, for the joint-angle tests on the limit faces
(tests/test_ik_boundary_cpu.py, tests/test_gpu_ik_boundary.py).  numpy only; it shares no code with csrc/.

The set: coxa, femur and tibia each within their own limits and femur + tibia within the absolute limits, the limits
being ik_cases.limits(oracle, leg, quat) taken literally: float32 values read as float64, a limit past +-pi stays as it
is.  The only geometry used is ik_cases.fk64.

nearest_in_limit searches that set for the configuration whose tip is nearest a point.  Every configuration it returns
passes in_limits and its distance is measured with fk64, so the distance is that of an in-limit tip that EXISTS: an
upper bound of the true minimum, never below it.  A test that says "the IK reports a gap, so the search must not find
an in-limit tip this close" can therefore miss a defect (where the search stops short of the minimum) but can never
blame the IK wrongly."""
import numpy as np

from ik_cases import fk64

KEYS = ("coxa", "femur", "tibia")


def bounds(L):
    """the limits as float64: (lo[3], hi[3], abs_lo, abs_hi)"""
    lo = np.array([float(L[k][0]) for k in KEYS])
    hi = np.array([float(L[k][1]) for k in KEYS])
    return lo, hi, float(L["abs"][0]), float(L["abs"][1])


def in_limits(angles, L):
    """membership, exact in float64 (inclusive bounds, femur + tibia one float64 addition) -> bool per configuration"""
    a = np.asarray(angles, np.float64).reshape(-1, 3)
    lo, hi, alo, ahi = bounds(L)
    s = a[:, 1] + a[:, 2]
    return ((a >= lo) & (a <= hi)).all(1) & (s >= alo) & (s <= ahi)


def is_empty(L):
    """no configuration at all meets the limits"""
    lo, hi, alo, ahi = bounds(L)
    return bool((lo > hi).any() or alo > ahi or lo[1] + lo[2] > ahi or hi[1] + hi[2] < alo)


def project(angles, L):
    """move configurations of any shape (..., 3) into the set: each joint into its own range, the femur into the part
    of its range that leaves the tibia a choice, then the tibia into what the absolute limits leave of its range.  The
    last float64 ulp is settled towards the inside, so the result passes in_limits (is_empty sets excepted)."""
    a = np.array(angles, np.float64)
    lo, hi, alo, ahi = bounds(L)
    a[..., 0] = np.clip(a[..., 0], lo[0], hi[0])
    f = np.clip(a[..., 1], max(lo[1], alo - hi[2]), min(hi[1], ahi - lo[2]))
    t = np.clip(a[..., 2], lo[2], hi[2])
    over = f + t > ahi
    t = np.where(over, ahi - f, t)
    under = f + t < alo
    t = np.where(under, alo - f, t)
    for _ in range(3):  # rounding of ahi - f / alo - f
        t = np.where(f + t > ahi, np.nextafter(t, -np.inf), t)
        t = np.where(f + t < alo, np.nextafter(t, np.inf), t)
    a[..., 1], a[..., 2] = f, np.clip(t, lo[2], hi[2])
    return a


def coarse_grid(L, n=40):
    """n per axis over the box, cut by the absolute limits -> (m, 3) in-limit configurations"""
    lo, hi, _, _ = bounds(L)
    axes = [np.linspace(lo[j], hi[j], n) for j in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return g[in_limits(g, L)]


def _tips(a, leg, quat):
    return fk64(a.reshape(-1, 3), leg, quat).reshape(a.shape)


def nearest_in_limit_many(P, leg, quat, L, sources=None, n=40, keep=4, rounds=36, chunk=256):
    """nearest_in_limit for the rows of P at once -> (distance[m], angles[m, 3]).  sources: None or (m, 3) source
    configurations, tried where they pass in_limits."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    m = len(P)
    grid = coarse_grid(L, n)
    if m == 0 or len(grid) == 0:
        return np.full(m, np.inf), np.full((m, 3), np.nan)
    gt = fk64(grid, leg, quat)
    g2 = (gt * gt).sum(1)
    lo, hi, _, _ = bounds(L)
    step0 = (hi - lo) / (n - 1)
    offs = np.stack(np.meshgrid(*([np.array([-1.0, -0.5, 0.0, 0.5, 1.0])] * 3), indexing="ij"), -1).reshape(-1, 3)
    best_d, best_a = np.empty(m), np.empty((m, 3))
    for s in range(0, m, chunk):
        p = P[s:s + chunk]
        d2 = g2[None, :] - 2.0 * (p @ gt.T)  # (c, g): |tip - p|^2 - |p|^2, enough to rank the grid
        k = min(keep, len(grid))
        idx = np.argpartition(d2, k - 1, axis=1)[:, :k]
        cen = grid[idx]  # (c, k, 3)
        if sources is not None:
            src = np.asarray(sources, np.float64).reshape(-1, 3)[s:s + chunk]
            ok = in_limits(src, L)
            cen = np.concatenate([cen, np.where(ok[:, None], src, cen[:, 0])[:, None, :]], 1)
        cd = np.linalg.norm(_tips(cen, leg, quat) - p[:, None, :], axis=-1)
        w = step0.copy()
        for _ in range(rounds):
            cand = project(cen[:, :, None, :] + offs[None, None, :, :] * w, L)  # (c, k, 125, 3)
            dd = np.linalg.norm(_tips(cand, leg, quat) - p[:, None, None, :], axis=-1)
            j = dd.argmin(-1)
            nd = np.take_along_axis(dd, j[..., None], -1)[..., 0]
            na = np.take_along_axis(cand, j[..., None, None], 2)[:, :, 0, :]
            better = nd < cd
            cen = np.where(better[..., None], na, cen)
            cd = np.where(better, nd, cd)
            w = w * 0.5
        j = cd.argmin(1)
        a = np.take_along_axis(cen, j[:, None, None], 1)[:, 0, :]
        best_a[s:s + chunk] = a
    ok = in_limits(best_a, L)
    best_d = np.where(ok, np.linalg.norm(fk64(best_a, leg, quat) - P, axis=1), np.inf)
    return best_d, best_a


def nearest_in_limit(p, leg, quat, L, source=None):
    """(distance, angles) of an in-limit configuration whose tip is near p: a coarse grid over the box cut by the
    absolute limits (40 per axis), then shrinking 5 x 5 x 5 grids around the best few grid points (and the source
    configuration, where given and in limits), every trial projected back into the set.  The returned configuration
    passes in_limits and the distance is |fk64(angles) - p|: an upper bound of the true minimum (see the module's
    docstring).  inf and nan angles where the set is empty."""
    d, a = nearest_in_limit_many(np.asarray(p, np.float64)[None], leg, quat, L,
                                 None if source is None else np.asarray(source, np.float64)[None])
    return float(d[0]), a[0]
