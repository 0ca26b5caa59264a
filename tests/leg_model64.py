"""An independent float64 model of a leg and of the clearance answers (tests/test_clearance_float64_cpu.py,
tests/test_gpu_clearance_float64.py), written from the leg's geometry: four joints on a yawing coxa and a femur and tibia that
pitch in the plane holding the yaw axis, true point-segment and segment-segment distances, and the per-row answers of
leg_clearance() and self_clearance() from those.  Nothing here is taken from the library: the joints extend ik_cases.fk64 (the
tip) to J0..J3, the distances are the textbook ones, and the module checks its segment-segment distance on its own against a
dense grid over both parameters (check_link_link_dist64).

What the contract DEFINES is kept as defined: T' = float32(T - tip_clear), 0 unless positive; q = t - body[p] in float32, one
subtraction per component; radius + margin and radius + radius formed once in float32.  Everything after is float64.

The measured bands (measured by tests/test_clearance_float64_cpu.py, asserted at four times the measured
worst rounded up to one digit) live here so that the CPU and the GPU tests share them."""
import numpy as np

import ik_cases
from ik_cases import BODY, BODY_ANGLE, COXA_LEN, COXA_PITCH, FEMUR_LEN, TIBIA_LEN

F = np.float32
D = np.float64

# mm.  measured worst -> asserted (tests/test_clearance_float64_cpu.py prints the measured values on every run)
BAND_J = 7e-4            # |J_host - J64|: worst per joint J0..J3 7.9e-5, 1.1e-4, 1.4e-4, 1.65e-4 (bodies to 1500 mm added)
BAND_D = 2e-3            # |d_host - d64|, target to link: 3.5e-4 on the library's float32 joints, 3.66e-4 on joints64 (both at
#                          targets 2 m away; 7.4e-5 within twice the reach)
BAND_PAIR_LOW = 5e-4     # d64 - d32 of a link pair on the same float32 segments (the header's "never under-reports"): 1.247e-4
BAND_KIND = {            # d32 - d64 per kind of self_clearance_cases.hand_made_pairs / random_pairs, same float32 segments:
    "crossing": 9e-5,            # 2.08e-5
    "touching": 2e-3,            # 4.01e-4: the true distance is 0, so the closest points' own float32 error shows undivided
    "parallel": 9e-5,            # 2.245e-5
    "nearly_parallel": 9e-5,     # 2.19e-5
    "collinear": 7e-5,           # 1.70e-5
    "one_degenerate": 4e-4,      # 8.39e-5
    "both_degenerate": 4e-4,     # 8.31e-5
    "identical": 0.0,            # 0
    "random": 5e-4}              # 1.14e-4
BAND_SELF = 6e-4         # |d32 on the library's joints - d64 on joints64| of the main scene's link pairs: 1.49e-4


def tibia_short(leg, tip_clear):
    """T' as the contract defines it: float32(T - tip_clear), 0 unless positive"""
    t = F(F(np.asarray(leg, F)[TIBIA_LEN]) - F(tip_clear))
    return float(t) if t > 0 else 0.0


def joints64(angles, leg, quat=(1, 0, 0, 0), tip_clear=0.0):
    """float64 [n, 4, 3], relative to the body: J0 the coxa joint, J1 the coxa's end (the femur joint), J2 the knee, J3 the end
    of the tibia shortened by tip_clear.  In the coxa frame the coxa yaws about z by angles[:, 0]; femur and tibia pitch in the
    vertical plane through the yawed coxa, the femur by angles[:, 1] from the horizontal and the tibia by angles[:, 2] from
    the femur.  Then the coxa pitch about y, the body offset along x, the leg azimuth about z and the pose rotation."""
    a = np.asarray(angles, D).reshape(-1, 3)
    c, f, t = a[:, 0], a[:, 1], a[:, 2]
    leg = np.asarray(leg, D)
    C, Fm, T = leg[COXA_LEN], leg[FEMUR_LEN], tibia_short(leg, tip_clear)
    zero = np.zeros_like(c)
    # (horizontal reach, height) of every joint in the leg's plane
    h = np.stack([zero, zero + C, C + Fm * np.cos(f), C + Fm * np.cos(f) + T * np.cos(f + t)], 1)
    z = np.stack([zero, zero, Fm * np.sin(f), Fm * np.sin(f) + T * np.sin(f + t)], 1)
    x, y = np.cos(c)[:, None] * h, np.sin(c)[:, None] * h
    cp, sp = np.cos(leg[COXA_PITCH]), np.sin(leg[COXA_PITCH])
    x, z = x * cp - z * sp + leg[BODY], x * sp + z * cp
    cb, sb = np.cos(leg[BODY_ANGLE]), np.sin(leg[BODY_ANGLE])
    x, y = x * cb - y * sb, x * sb + y * cb
    return np.stack([x, y, z], 2) @ ik_cases.back_matrix(quat).T


def joints64_posed(angles, legs, quats, tip_clear=0.0, pose_of=None):
    """float64 [nlegs, n, 4, 3] for angles float[nlegs*n, 3] at [l*n + s]; entry s stands in pose pose_of[s] (default s)"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    quats = np.asarray(quats, F).reshape(-1, 4)
    nl = len(legs)
    a = np.asarray(angles, D).reshape(nl, -1, 3)
    n = a.shape[1]
    pose_of = np.arange(n) if pose_of is None else np.asarray(pose_of)
    out = np.empty((nl, n, 4, 3), D)
    with np.errstate(invalid="ignore"):
        for p in np.unique(pose_of):
            at = np.flatnonzero(pose_of == p)
            for l in range(nl):
                out[l, at] = joints64(a[l, at], legs[l], quats[p], tip_clear)
    return out


def point_link_dist64(q, A, B):
    """the distance from q to the segment AB (broadcast over leading axes); a zero-length link is the point A"""
    q, A, B = (np.asarray(v, D) for v in (q, A, B))
    u = B - A
    uu = (u * u).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(uu > 0, ((q - A) * u).sum(-1) / np.where(uu > 0, uu, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)  # the foot of the perpendicular, moved to the nearer end where it falls outside the link
    return np.linalg.norm(q - (A + s[..., None] * u), axis=-1)


def link_link_dist64(A1, B1, A2, B2):
    """the minimum distance between the segments A1B1 and A2B2: the least of the four endpoint-to-segment distances and, where
    the common perpendicular of the two lines meets both segments in their interior, its length.  (The squared distance is a
    convex quadratic of the two parameters on the unit square: its minimum is the interior critical point or lies on an edge,
    and the minimum along an edge is an endpoint-to-segment distance.)"""
    A1, B1, A2, B2 = (np.asarray(v, D) for v in (A1, B1, A2, B2))
    d = np.minimum(np.minimum(point_link_dist64(A1, A2, B2), point_link_dist64(B1, A2, B2)),
                   np.minimum(point_link_dist64(A2, A1, B1), point_link_dist64(B2, A1, B1)))
    u, v, w = B1 - A1, B2 - A2, A2 - A1
    n = np.cross(u, v)
    nn = (n * n).sum(-1)
    ok = nn > 1e-24 * (u * u).sum(-1) * (v * v).sum(-1)  # the lines are not parallel: sin^2 of their angle above 1e-24
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (np.cross(w, v) * n).sum(-1) / np.where(ok, nn, 1.0)  # A1 + s u and A2 + t v are the feet of the common perpendicular
        t = (np.cross(w, u) * n).sum(-1) / np.where(ok, nn, 1.0)
        inside = ok & (s > 0) & (s < 1) & (t > 0) & (t < 1)
        di = np.linalg.norm((A1 + s[..., None] * u) - (A2 + t[..., None] * v), axis=-1)
    return np.where(inside & (di < d), di, d)


def check_link_link_dist64(segs, steps=256):
    """link_link_dist64 against the minimum over a (steps + 1)^2 grid of both parameters.  The distance between the two points
    changes by at most |B1 - A1| per unit of s and |B2 - A2| per unit of t, and some grid node lies within half a step of the
    minimiser in each parameter, so  d64 <= grid <= d64 + (|B1 - A1| + |B2 - A2|) / (2 steps).  -> the largest grid - d64"""
    g = np.asarray(segs, D).reshape(-1, 12)
    par = np.linspace(0.0, 1.0, steps + 1)
    worst = 0.0
    for A1, B1, A2, B2 in zip(g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:12]):
        P = A1 + par[:, None] * (B1 - A1)
        Q = A2 + par[:, None] * (B2 - A2)
        grid = np.sqrt(((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1).min())
        d = float(link_link_dist64(A1, B1, A2, B2))
        gap = (np.linalg.norm(B1 - A1) + np.linalg.norm(B2 - A2)) / (2.0 * steps)
        tiny = 1e-12 * (1.0 + np.abs(g).max())
        assert d <= grid + tiny, (d, grid, A1, B1, A2, B2)          # never above an attained distance
        assert grid <= d + gap + tiny, (d, grid, gap, A1, B1, A2, B2)  # and no further below the grid than the grid's own gap
        worst = max(worst, grid - d)
    return worst


def leg_clearance64(targets, body, joints, radius, margin, live_in=None):
    """joints float64 (or float32) [nlegs, nposes, 4, 3] RELATIVE to the body -> dict:
    d [nlegs, nposes, 3, nt] the distance of q = float32(t - body[p]) to each link (inf for a link with radius 0),
    hit / near [nlegs, nposes, 3, nt], pen_t [nlegs, nposes, nt] the largest radius - d over a target's near links (-inf: none),
    valid [nlegs, nposes] (live pose, finite joints), and the rows hits, links, worst, pen [nlegs, nposes], free [nposes]"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    body = np.asarray(body, F).reshape(-1, 3)
    J = np.asarray(joints, D)
    nl, n = J.shape[:2]
    nt = len(targets)
    r = np.asarray(radius, F).reshape(3)
    reach = (r + F(margin)).astype(F).astype(D)
    r = r.astype(D)
    live = np.ones(n, bool) if live_in is None else np.asarray(live_in).astype(bool)
    valid = np.isfinite(J).all((2, 3)) & live[None, :]
    d = np.full((nl, n, 3, nt), np.inf, D)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(n):
            q = (targets - body[p]).astype(F).astype(D)
            for l in range(nl):
                if not valid[l, p]:
                    continue
                for k in range(3):
                    if r[k] > 0:
                        d[l, p, k] = point_link_dist64(q, J[l, p, k], J[l, p, k + 1])
        hit = d < r[None, None, :, None]     # nan compares false: a non-finite target or body is near nothing
        near = d < reach[None, None, :, None]
        pen_k = np.where(near, r[None, None, :, None] - d, -np.inf)
    pen_t = pen_k.max(2)
    hit_t = hit.any(2)
    hits = hit_t.sum(2).astype(np.int32)
    links = sum((hit[:, :, k].any(2).astype(np.uint8) << k) for k in range(3)).astype(np.uint8)
    pen = pen_t.max(2) if nt else np.full((nl, n), -np.inf)
    worst = np.where(np.isneginf(pen), -1, pen_t.argmax(2) if nt else -1).astype(np.int32)
    free = (live & (hits == 0).all(0)).astype(np.uint8)
    return {"d": d, "hit": hit, "near": near, "pen_t": pen_t, "valid": valid, "radius": r, "reach": reach, "hits": hits,
            "links": links, "worst": worst, "pen": pen, "free": free, "near_any": near.any((2, 3))}


def leg_doubt(m, band):
    """bool [nlegs, nposes, 3, nt]: the float64 distance is within band of the link's radius or of radius + margin"""
    r, reach = m["radius"][None, None, :, None], m["reach"][None, None, :, None]
    with np.errstate(invalid="ignore"):
        return (np.abs(m["d"] - r) <= band) | (np.abs(m["d"] - reach) <= band)


def check_leg_rows(got, m, band):
    """the library's rows (dict of hits, links, worst, pen [nlegs, nposes], free [nposes]) against the model m on every valid
    row without a decision in doubt: hits and links exactly, worst a target whose float64 pen is within 2 band of the float64
    maximum, pen within band of that target's; free on poses none of whose rows is in doubt; invalid rows are empty.
    -> (rows compared, rows skipped)"""
    sure = m["valid"] & ~leg_doubt(m, band).any((2, 3))
    empty = ~m["valid"]
    assert (got["hits"][empty] == 0).all() and (got["links"][empty] == 0).all() and (got["worst"][empty] == -1).all()
    assert np.array_equal(got["hits"][sure], m["hits"][sure])
    assert np.array_equal(got["links"][sure], m["links"][sure])
    assert np.array_equal(got["worst"][sure] >= 0, m["worst"][sure] >= 0)
    some = sure & (m["worst"] >= 0)
    l, p = np.nonzero(some)
    pen_w = m["pen_t"][l, p, got["worst"][l, p]]
    assert (pen_w >= m["pen"][l, p] - 2 * band).all(), float((m["pen"][l, p] - pen_w).max())
    if got.get("pen") is not None:
        assert np.isneginf(got["pen"][sure & (m["worst"] < 0)]).all() and np.isneginf(got["pen"][empty]).all()
        assert (np.abs(got["pen"][l, p].astype(D) - pen_w) <= band).all(), float(np.abs(got["pen"][l, p] - pen_w).max())
    if got.get("free") is not None:
        pose_sure = (sure | empty).all(0)
        assert np.array_equal(got["free"][pose_sure], m["free"][pose_sure])
    return int(sure.sum()), int((m["valid"] & ~sure).sum())


LINK_PAIRS = [(ka, kb) for ka in range(3) for kb in range(3)]


def self_clearance64(joints, radius, margin, live=None):
    """joints [nlegs, nsets, 4, 3] relative to the body -> dict: pairs, a list of (i, j, ka, kb, d [nsets], tested bool[nsets],
    rr, reach) for legs i < j; pen_code [nlegs, nsets, 72] radius sum - d of every near pair under the leg's own code
    other*9 + own_link*3 + other_link (-inf: not near); valid [nlegs, nsets]; the rows hits, with, links, worst, pen and free"""
    J = np.asarray(joints, D)
    nl, ns = J.shape[:2]
    r32 = np.asarray(radius, F).reshape(3)
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    valid = np.isfinite(J).all((2, 3)) & live[None, :]
    hits = np.zeros((nl, ns), np.int32)
    with_, links = np.zeros((nl, ns), np.uint8), np.zeros((nl, ns), np.uint8)
    pen_code = np.full((nl, ns, 72), -np.inf, D)
    pairs = []
    with np.errstate(invalid="ignore"):
        for j in range(nl):
            for i in range(j):
                ok = valid[i] & valid[j]
                for ka, kb in LINK_PAIRS:
                    if r32[ka] == 0 or r32[kb] == 0:
                        continue
                    rr32 = F(r32[ka] + r32[kb])
                    rr, reach = float(rr32), float(F(rr32 + F(margin)))
                    d = link_link_dist64(J[i, :, ka], J[i, :, ka + 1], J[j, :, kb], J[j, :, kb + 1])
                    hit, near = ok & (d < rr), ok & (d < reach)
                    for me, other, own, oth in ((i, j, ka, kb), (j, i, kb, ka)):
                        hits[me] += hit
                        with_[me] |= (hit.astype(np.uint8) << other).astype(np.uint8)
                        links[me] |= (hit.astype(np.uint8) << own).astype(np.uint8)
                        pen_code[me, :, other * 9 + own * 3 + oth] = np.where(near, rr - d, -np.inf)
                    pairs.append((i, j, ka, kb, d, ok, rr, reach))
    pen = pen_code.max(2)
    worst = np.where(np.isneginf(pen), 255, pen_code.argmax(2)).astype(np.uint8)
    free = (live & (hits == 0).all(0)).astype(np.uint8)
    return {"pairs": pairs, "pen_code": pen_code, "valid": valid, "live": live, "hits": hits, "with": with_, "links": links,
            "worst": worst, "pen": pen, "free": free}


def self_doubt(m, band):
    """bool [nlegs, nsets]: some tested link pair of the leg has its float64 distance within band of a decision"""
    nl, ns = m["hits"].shape
    doubt = np.zeros((nl, ns), bool)
    for i, j, _, _, d, ok, rr, reach in m["pairs"]:
        with np.errstate(invalid="ignore"):
            near_a_line = ok & ((np.abs(d - rr) <= band) | (np.abs(d - reach) <= band))
        doubt[i] |= near_a_line
        doubt[j] |= near_a_line
    return doubt


def check_self_rows(got, m, band):
    """the library's rows (dict of hits, with, links, worst, pen [nlegs, nsets], free [nsets]) against the model m on every live
    row without a pair in doubt (invalid legs included: they have the empty answer) -> (rows compared, rows skipped)"""
    doubt = self_doubt(m, band)
    live = np.broadcast_to(m["live"], doubt.shape)
    sure = live & ~doubt
    dead = ~live
    assert (got["hits"][dead] == 0).all() and (got["with"][dead] == 0).all() and (got["worst"][dead] == 255).all()
    for k in ("hits", "with", "links"):
        assert np.array_equal(got[k][sure], m[k][sure]), k
    assert np.array_equal(got["worst"][sure] != 255, m["worst"][sure] != 255)
    l, s = np.nonzero(sure & (m["worst"] != 255))
    pen_w = m["pen_code"][l, s, got["worst"][l, s]]
    assert (pen_w >= m["pen"][l, s] - 2 * band).all(), float((m["pen"][l, s] - pen_w).max())
    if got.get("pen") is not None:
        assert np.isneginf(got["pen"][sure & (m["worst"] == 255)]).all()
        assert (np.abs(got["pen"][l, s].astype(D) - pen_w) <= band).all(), float(np.abs(got["pen"][l, s] - pen_w).max())
    if got.get("free") is not None:
        set_sure = (sure | dead).all(0)
        assert np.array_equal(got["free"][set_sure], m["free"][set_sure])
    return int(sure.sum()), int((live & doubt).sum())
