"""An independent float64 model of the trunk-leg clearance answers (tests/test_trunk_clearance_cpu.py,
tests/test_gpu_trunk_clearance.py): the TRUE minimum distance of a segment to the solid body cylinder -- a dense scan of the
squared distance h along the segment in float64, refined by a golden-section search in the two grid cells about the best node (h
is convex along a segment, so its minimum lies there) -- and the per-row answers of trunk_clearance() from it.  Nothing here is
taken from the library: the joints are leg_model64.joints64_posed's (the leg's geometry), taken into the body frame by the float64
inverse of the pose rotation; the module checks its distance on its own against a 4097-point grid (check_link_cyl_dist64).

What the contract DEFINES is kept as defined: T' = float32(T - tip_clear), radius + margin formed once in float32, the float32
cylinder scalars.  Everything after is float64.

The measured bands (measured by tests/test_trunk_clearance_cpu.py, asserted at four times the measured worst
rounded up to one digit) live here so that the CPU and the GPU tests share them."""
import numpy as np

import ik_cases
import leg_model64 as m64

F = np.float32
D = np.float64
GOLD = (np.sqrt(5.0) - 1.0) / 2.0

# mm.  measured worst -> asserted (tests/test_trunk_clearance_cpu.py prints the measured values on every run)
# BAND_LOW: d64 - d32 on the same float32 links (the header's "never under-reports"); BAND_KIND: d32 - d64 per kind of
# trunk_clearance_cases.hand_made_links / random_links; BAND_TRUNK: |d32 on the library's joints - d64 on joints64| of the main
# scene's links
BAND_LOW = 4e-4          # the largest "below" of BAND_KIND
BAND_KIND = {            # kind: (above, below) asserted; measured d32 - d64 above / below
    "through_axis": (0.0, 0.0),          # 0 / 0: the link passes through the cylinder
    "tangent_side": (6e-5, 2e-4),        # 1.49e-5 / 2.62e-5
    "crossing_cap": (0.0, 0.0),          # 0 / 0
    "nearest_rim": (7e-5, 2e-4),         # 1.68e-5 / 4.04e-5
    "parallel_inside": (0.0, 0.0),       # 0 / 0: the nearest point is an end, one exact subtraction
    "parallel_outside": (2e-4, 2e-4),    # 3.05e-5 / 2.80e-5
    "in_cap_plane": (2e-4, 2e-4),        # 2.53e-5 / 3.33e-5
    "degenerate": (2e-4, 2e-4),          # 3.51e-5 / 4.27e-5
    "wholly_inside": (0.0, 0.0),         # 0 / 0
    "random": (3e-4, 4e-4)}              # 5.97e-5 / 8.09e-5
BAND_TRUNK = 4e-4        # 9.08e-5


def h64(P, cyl):
    """the squared distance of the points P [..., 3] to the solid cylinder (radius, plus_z, minus_z) about the z axis"""
    R, pz, mz = (float(F(v)) for v in cyl)
    P = np.asarray(P, D)
    rho = np.hypot(P[..., 0], P[..., 1])
    dr = np.maximum(rho - R, 0.0)
    dz = np.maximum(np.maximum(P[..., 2] - pz, mz - P[..., 2]), 0.0)
    return dr * dr + dz * dz


def link_cyl_dist64(A, B, cyl, steps=128, refine=64):
    """the minimum distance of the segments A -> B ([n, 3]) to the solid cylinder: h at steps + 1 nodes, then a golden-section
    search over the two cells about the best node (they shrink by 0.618^64 = 4e-14); the least value seen, nodes included"""
    A, B = np.asarray(A, D).reshape(-1, 3), np.asarray(B, D).reshape(-1, 3)
    e = B - A
    u = np.linspace(0.0, 1.0, steps + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        H = np.stack([h64(A + t * e, cyl) for t in u], 1)  # [n, steps + 1]
        i = np.where(np.isnan(H).any(1), 0, np.argmin(np.where(np.isnan(H), np.inf, H), 1))
        best = H[np.arange(len(A)), i]
        lo, hi = np.maximum(i - 1, 0) / steps, np.minimum(i + 1, steps) / steps
        at = lambda t: h64(A + t[:, None] * e, cyl)
        x1, x2 = hi - GOLD * (hi - lo), lo + GOLD * (hi - lo)
        f1, f2 = at(x1), at(x2)
        for _ in range(refine):
            best = np.fmin(best, np.fmin(f1, f2))
            left = f1 <= f2  # the minimum lies in [lo, x2]; else in [x1, hi]
            hi, lo = np.where(left, x2, hi), np.where(left, lo, x1)
            xn = np.where(left, hi - GOLD * (hi - lo), lo + GOLD * (hi - lo))
            fn = at(xn)
            x1, x2, f1, f2 = np.where(left, xn, x2), np.where(left, x1, xn), np.where(left, fn, f2), np.where(left, f1, fn)
        best = np.fmin(best, np.fmin(f1, f2))
        return np.sqrt(best)


def check_link_cyl_dist64(A, B, cyl, steps=4096):
    """link_cyl_dist64 against the minimum over a (steps + 1)-point grid.  The distance to a fixed set changes by at most
    |B - A| per unit of the parameter, and some node lies within half a step of the minimiser, so
    d64 <= grid <= d64 + |B - A| / steps (twice what is needed).  -> the largest grid - d64"""
    A, B = np.asarray(A, D).reshape(-1, 3), np.asarray(B, D).reshape(-1, 3)
    d = link_cyl_dist64(A, B, cyl)
    u = np.linspace(0.0, 1.0, steps + 1)
    worst = 0.0
    for k in range(0, len(A), 256):
        a, b = A[k:k + 256], B[k:k + 256]
        grid = np.sqrt(h64(a[:, None, :] + u[None, :, None] * (b - a)[:, None, :], cyl).min(1))
        gap = np.linalg.norm(b - a, axis=1) / steps
        tiny = 1e-9
        assert (d[k:k + 256] <= grid + tiny).all(), float((d[k:k + 256] - grid).max())   # never above an attained distance
        assert (grid <= d[k:k + 256] + gap + tiny).all(), float((grid - d[k:k + 256] - gap).max())
        worst = max(worst, float((grid - d[k:k + 256]).max()))
    return worst


def body_joints64(angles, legs, quats, tip_clear=0.0, pose_of=None):
    """float64 [nlegs, n, 4, 3]: leg_model64.joints64_posed (relative to the body, caller's frame) taken into the body frame
    of each entry's pose by the float64 inverse of ik_cases.back_matrix"""
    quats = np.asarray(quats, F).reshape(-1, 4)
    J = m64.joints64_posed(angles, legs, quats, tip_clear, pose_of)
    n = J.shape[1]
    pose_of = np.arange(n) if pose_of is None else np.asarray(pose_of)
    out = np.empty_like(J)
    for p in np.unique(pose_of):
        at = np.flatnonzero(pose_of == p)
        out[:, at] = J[:, at] @ np.linalg.inv(ik_cases.back_matrix(quats[p])).T
    return out


def trunk_clearance64(body_joints, radius, margin, cyl, links=0b110, live=None):
    """body_joints [nlegs, nsets, 4, 3] in the body frame -> dict: d [nlegs, nsets, 3] (inf: not tested), valid, the float64
    radius / reach per link, pen_k [nlegs, nsets, 3] (-inf: not near) and the rows links, worst, pen, free"""
    J = np.asarray(body_joints, D)
    nl, ns = J.shape[:2]
    r32 = np.asarray(radius, F).reshape(3)
    reach = (r32 + F(margin)).astype(F).astype(D)
    r = r32.astype(D)
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    valid = np.isfinite(J).all((2, 3)) & live[None, :]
    d = np.full((nl, ns, 3), np.inf, D)
    tested = np.array([bool((links >> k) & 1) and r32[k] != 0 for k in range(3)])
    for k in range(3):
        if tested[k] and valid.any():
            dk = link_cyl_dist64(J[:, :, k][valid], J[:, :, k + 1][valid], cyl)
            d[:, :, k][valid] = dk
    hit, near = d < r, d < reach
    pen_k = np.where(near, r - d, -np.inf)
    hit_bits = sum((hit[:, :, k].astype(np.uint8) << k) for k in range(3)).astype(np.uint8)
    pen = pen_k.max(2)
    worst = np.where(np.isneginf(pen), 255, pen_k.argmax(2)).astype(np.uint8)
    return {"d": d, "valid": valid, "live": live, "radius": r, "reach": reach, "tested": tested, "pen_k": pen_k, "links": hit_bits,
            "worst": worst, "pen": pen, "free": (live & (hit_bits == 0).all(0)).astype(np.uint8)}


def trunk_doubt(m, band):
    """bool [nlegs, nsets]: some tested link of the leg has its float64 distance within band of a decision"""
    with np.errstate(invalid="ignore"):
        return ((np.abs(m["d"] - m["radius"]) <= band) | (np.abs(m["d"] - m["reach"]) <= band)).any(2) & m["valid"]


def check_trunk_rows(got, m, band):
    """the library's rows (dict of links, worst, pen [nlegs, nsets], free [nsets]) against the model m on every live row
    without a link in doubt (invalid legs included: they have the empty answer): links exactly, worst a link whose float64 pen
    is within 2 band of the float64 maximum, pen within band of that link's; free on sets none of whose rows is in doubt; dead
    sets are empty -> (rows compared, rows skipped)"""
    doubt = trunk_doubt(m, band)
    live = np.broadcast_to(m["live"], doubt.shape)
    sure, dead = live & ~doubt, ~live
    assert (got["links"][dead] == 0).all() and (got["worst"][dead] == 255).all()
    assert np.array_equal(got["links"][sure], m["links"][sure])
    assert np.array_equal(got["worst"][sure] != 255, m["worst"][sure] != 255)
    l, s = np.nonzero(sure & (m["worst"] != 255))
    pen_w = m["pen_k"][l, s, got["worst"][l, s]]
    assert (pen_w >= m["pen"][l, s] - 2 * band).all(), float((m["pen"][l, s] - pen_w).max())
    if got.get("pen") is not None:
        assert np.isneginf(got["pen"][sure & (m["worst"] == 255)]).all() and np.isneginf(got["pen"][dead]).all()
        assert (np.abs(got["pen"][l, s].astype(D) - pen_w) <= band).all(), float(np.abs(got["pen"][l, s] - pen_w).max())
    if got.get("free") is not None:
        set_sure = (sure | dead).all(0)
        assert np.array_equal(got["free"][set_sure], m["free"][set_sure])
    return int(sure.sum()), int((live & doubt).sum())
