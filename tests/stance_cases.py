"""Shared cases of the stance stability tests (tests/test_stance_cpu.py, tests/test_gpu_stance.py): brute_np restates the
definition of include/lrm.h (lrm_stance_stability_dev) in vectorised numpy float32, one rounding per operation, written
from that text and not from csrc/lrm_stance.h; margin64 is a float64 monotone-chain hull of the same planted feet; the
scenes are `main` (six legs around the body, feet from the host foothold choice on `rough`, one centre of mass off the
body origin), `synthetic` (random feet drawn from a small cloud, for the sizes no foothold search should pay for) and the
hand-made stances."""
import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

F = np.float32
NINF = F(-np.inf)
COM = np.array([95.0, -60.0, -25.0], F)  # BODY frame, mm: near the edge of a typical support polygon of `main`
TRIPODS = (0b010101, 0b101010)


def lift_each(nlegs):
    return np.array([0] + [1 << l for l in range(nlegs)], np.uint8)


def lift_all(nlegs):
    return np.arange(1 << nlegs, dtype=np.uint8) if nlegs < 8 else np.arange(256).astype(np.uint8)


def legs_n(lrm, n):
    """n M2 legs evenly around the body (pair_cases.leg_families)"""
    name = {1: "m2_1_identity", 2: "m2_2_tilted", 3: "m2_3_nonunit", 5: "m2_5_identity", 6: "m2_6_tilted", 8: "m2_8_identity"}.get(n)
    if name is not None:
        return pc.leg_families(lrm)[name][0]
    return pc.leg_families(lrm)["m2_8_identity"][0][:n]


def nominal_ring(nlegs, radius=260.0, drop=-160.0):
    """a nominal foot point per leg on a ring about the body, at the leg's azimuth"""
    az = 2 * np.pi * np.arange(nlegs) / nlegs
    return np.column_stack([radius * np.cos(az), radius * np.sin(az), np.full(nlegs, drop)]).astype(F)


# ---- the definition, restated ----------------------------------------------------------------------------------------
def _project(q, plane):
    """q: float32 [..., 3] -> (x, y) float32 arrays"""
    if plane is None:
        return q[..., 0].copy(), q[..., 1].copy()
    u, v = np.asarray(plane, F).reshape(2, 3)
    return ((q[..., 0] * u[0] + q[..., 1] * u[1]) + q[..., 2] * u[2]).astype(F), ((q[..., 0] * v[0] + q[..., 1] * v[1]) + q[..., 2] * v[2]).astype(F)


def _rotate(quats, v):
    """qtRotate(quat, v) through the coefficient sums of the pose records (unified_math_cuda.cu.h:13-27 as include/lrm.h names
    it), float32, quats [n, 4]; v float32[3]"""
    a, b, c, d = (quats[:, k].astype(F) for k in range(4))
    t2, t3, t4 = a * b, a * c, a * d
    t5, t6, t7 = -b * b, b * c, b * d
    t8, t9, t10 = -c * c, c * d, -d * d
    two = F(2)
    x = two * (((t8 + t10) * v[0] + (t6 - t4) * v[1]) + (t3 + t7) * v[2]) + v[0]
    y = two * (((t4 + t6) * v[0] + (t5 + t10) * v[1]) + (t9 - t2) * v[2]) + v[1]
    z = two * (((t7 - t3) * v[0] + (t2 + t9) * v[1]) + (t5 + t8) * v[2]) + v[2]
    return np.stack([x, y, z], -1).astype(F)


def geometry(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, live_in=None):
    """-> (fx, fy float32[nlegs, ns], valid bool[nlegs, ns], cx, cy float32[ns], dead bool[ns]): the plane points of the
    feet (garbage where not valid), the centre of mass and the dead stances"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    foot = np.ascontiguousarray(foot, np.int32)
    nl, ns = foot.shape
    nt, nposes = len(targets), len(quats)
    with np.errstate(all="ignore"):
        p = np.arange(ns, dtype=np.int64) if pose_idx is None else np.asarray(pose_idx, np.int64)
        dead = (p < 0) | (p >= nposes)
        if live_in is not None:
            dead |= np.asarray(live_in) == 0
        pc_ = np.where(dead, 0, p) if nposes else np.zeros(ns, np.int64)
        qs = quats[pc_] if nposes else np.zeros((ns, 4), F)
        b = np.zeros((ns, 3), F) if body is None or not nposes else np.ascontiguousarray(body, F).reshape(-1, 3)[pc_]
        cm = np.zeros(3, F) if com is None else np.asarray(com, F).reshape(3)
        c3 = np.zeros((ns, 3), F) if not cm.any() else _rotate(qs, cm)
        cx, cy = _project(c3, plane)
        dead |= ~(np.isfinite(cx) & np.isfinite(cy))
        inb = (foot >= 0) & (foot < nt)
        t = targets[np.where(inb, foot, 0)] if nt else np.zeros((nl, ns, 3), F)
        q = (t - b[None]).astype(F)
        valid = inb & np.isfinite(q).all(-1) & ~dead[None]
        fx, fy = _project(q, plane)
    return fx, fy, valid, cx, cy, dead


def brute_np(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None):
    """-> dict(margin float32, edge uint8, stable uint8, each [nmasks, ns]; feet uint8[ns])"""
    fx, fy, valid, cx, cy, dead = geometry(targets, foot, quats, body, pose_idx, com, plane, live_in)
    nl, ns = valid.shape
    lift = np.zeros(1, np.uint8) if lift is None else np.asarray(lift, np.uint8)
    nm = len(lift)
    zero = F(0)
    pairs = []  # (code, i, j, usable & both valid [ns], left [nl, ns], s [ns]) in rising code
    with np.errstate(all="ignore"):
        for i in range(nl):
            for j in range(nl):
                if i == j:
                    continue
                ax, ay = fx[i], fy[i]
                ex, ey = (fx[j] - ax).astype(F), (fy[j] - ay).astype(F)
                len2 = (ex * ex + ey * ey).astype(F)
                ok = valid[i] & valid[j] & (len2 > 0) & (len2 < np.inf)
                left = np.stack([(ex * (fy[k] - ay) - ey * (fx[k] - ax)).astype(F) >= 0 for k in range(nl)])
                s = ((ex * (cy - ay) - ey * (cx - ax)).astype(F) / np.sqrt(len2).astype(F)).astype(F)
                s = np.where(np.isnan(s), NINF, s + zero).astype(F)
                pairs.append((i * 8 + j, i, j, ok, left, s))
        margin = np.full((nm, ns), NINF, F)
        edge = np.full((nm, ns), 255, np.uint8)
        for m in range(nm):
            S = valid & ~np.array([(int(lift[m]) >> l) & 1 for l in range(nl)], bool)[:, None]
            enough = S.sum(0) >= 3
            have = np.zeros(ns, bool)
            best = np.zeros(ns, F)
            code_of = np.full(ns, 255, np.uint8)
            for code, i, j, ok, left, s in pairs:
                counts = ok & enough & S[i] & S[j] & (~S | left).all(0)
                take = counts & (~have | (s < best))  # rising codes: a tie keeps the smaller one
                best = np.where(take, s, best)
                code_of = np.where(take, code, code_of).astype(np.uint8)
                have |= counts
            margin[m] = np.where(have, best, NINF)
            edge[m] = np.where(have & ~np.isneginf(best), code_of, 255)
        stable = (margin > F(min_margin)).astype(np.uint8)
    feet = np.zeros(ns, np.uint8)
    for l in range(nl):
        feet |= (valid[l].astype(np.uint8) << l).astype(np.uint8)
    return {"margin": margin, "edge": edge, "stable": stable, "feet": feet}


def _hull64(pts):
    """counter-clockwise hull of float64 points by the monotone chain, collinear points dropped"""
    pts = sorted(set(map(tuple, pts)))
    if len(pts) <= 2:
        return pts
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def margin64(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, live_in=None):
    """float64 [nmasks, ns]: the smallest signed distance of the centre of mass from the hull edges of the planted feet; -inf
    below three planted feet, for a dead stance and for feet that all coincide.  The feet and the centre of mass are
    brute_np's float32 plane points (the data); hull and distances are float64."""
    fx, fy, valid, cx, cy, dead = geometry(targets, foot, quats, body, pose_idx, com, plane, live_in)
    nl, ns = valid.shape
    lift = np.zeros(1, np.uint8) if lift is None else np.asarray(lift, np.uint8)
    out = np.full((len(lift), ns), -np.inf)
    for m, lm in enumerate(lift):
        for s in range(ns):
            pl = [l for l in range(nl) if valid[l, s] and not (int(lm) >> l) & 1]
            if len(pl) < 3:
                continue
            hull = _hull64([(float(fx[l, s]), float(fy[l, s])) for l in pl])
            if len(hull) < 2:
                continue
            c = (float(cx[s]), float(cy[s]))
            d = []
            for k in range(len(hull)):
                a, b = hull[k], hull[(k + 1) % len(hull)]
                e = (b[0] - a[0], b[1] - a[1])
                d.append((e[0] * (c[1] - a[1]) - e[1] * (c[0] - a[0])) / np.hypot(*e))
            out[m, s] = min(d)
    return out


def max_rel_coordinate(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, live_in=None):
    """float64[ns]: the largest |coordinate| among a stance's valid plane points and centre of mass (0 if none)"""
    fx, fy, valid, cx, cy, dead = geometry(targets, foot, quats, body, pose_idx, com, plane, live_in)
    with np.errstate(all="ignore"):
        m = np.maximum(np.where(valid, np.abs(fx), 0).max(0), np.where(valid, np.abs(fy), 0).max(0)).astype(np.float64)
        return np.where(dead, 0.0, np.maximum(m, np.maximum(np.abs(cx), np.abs(cy))))


# ---- scenes ----------------------------------------------------------------------------------------------------------
def main_scene(lrm, nposes=240, nt=3000, seed=1, nlegs=6):
    """(targets, foot int32[nlegs, nposes], quats, body, legs): bodies over `rough`, one of the reference's sweep orientations
    per pose, feet = the host foothold choice about a ring of nominal points; every fifth body hovers out of reach (no
    foot), and the terrain's edge leaves some stances a few feet short"""
    legs = legs_n(lrm, nlegs)
    _, body, targets = fc.scene(lrm, nposes, nt, seed)
    quats = fc.sweep_pose_quats(lrm, nposes, seed)
    body = body.copy()
    body[:, :2] *= F(1.25)  # towards and past the edge of the patch
    best = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal_ring(nlegs))[1]
    return np.ascontiguousarray(targets, F), np.ascontiguousarray(best, np.int32), quats, np.ascontiguousarray(body, F), legs


def synthetic(ns, nlegs, seed, nt=600, missing=0.2, spread=350.0, offset=0.0):
    """(targets, foot, quats, body): random unit quaternions, bodies inside a flat cloud, every foot a random target within
    reach of a ring point of its leg, `missing` of the feet -1.  No leg model is consulted."""
    import posed_cases
    rng = np.random.default_rng(seed)
    targets = np.column_stack([rng.uniform(-spread, spread, (nt, 2)), rng.normal(0, 15, nt)])
    body = np.column_stack([rng.uniform(-0.3 * spread, 0.3 * spread, (ns, 2)), rng.uniform(80, 200, ns)])
    ring = nominal_ring(nlegs, radius=0.45 * spread)[:, :2].astype(np.float64)
    foot = np.empty((nlegs, ns), np.int32)
    cand = rng.integers(0, nt, (nlegs, ns, 6))
    for l in range(nlegs):  # of six random targets, the one nearest the leg's ring point
        want = body[:, None, :2] + ring[l]
        d = np.linalg.norm(targets[cand[l]][:, :, :2] - want, axis=2)
        foot[l] = cand[l][np.arange(ns), d.argmin(1)]
    foot[rng.random((nlegs, ns)) < missing] = -1
    quats = posed_cases.random_unit_quats(ns, rng)
    off = np.array([offset, -offset, 0.25 * offset])
    return (targets + off).astype(F), foot, quats, (body + off).astype(F)


def hand_made():
    """name -> (targets, foot [nlegs, 1], com, want): single stances at the identity pose, body at the origin; want = dict of
    the answers the definition gives for lift [0] (margin, edge, stable with min_margin 0), None where only brute_np says"""
    sq = [[100, 100, 0], [-100, 100, 0], [-100, -100, 0], [100, -100, 0]]
    idx = lambda n: np.arange(n, dtype=np.int32).reshape(n, 1)
    cases = {
        # four feet on the line y = 0, the centre of mass on it: every pair counts, every s is 0, the smallest code is 0*8 + 1
        "collinear": (np.array([[-100, 0, 0], [0, 0, 5], [50, 0, -5], [200, 0, 0]], F), idx(4), None, {"margin": 0.0, "edge": 1, "stable": 0}),
        "coincident": (np.array([[30, 40, 0]] * 4, F), idx(4), None, {"margin": -np.inf, "edge": 255, "stable": 0}),
        # a square and a fifth foot inside it: the inner foot changes nothing; the centre of mass 10 mm from the edge x = 100
        "inside_hull": (np.array(sq + [[20, -30, 0]], F), idx(5), [90.0, 0.0, 0.0], {"margin": 10.0, "edge": 3 * 8 + 0, "stable": 1}),
        # a fifth foot ON the edge 3 -> 0: the edges 3 -> 4, 4 -> 0 and 3 -> 0 all count and tie at 10; 3*8 + 0 is the smallest code
        "on_hull_edge": (np.array(sq + [[100, 25, 0]], F), idx(5), [90.0, 0.0, 0.0], {"margin": 10.0, "edge": 3 * 8 + 0, "stable": 1}),
        # legs 0 and 4 share target 0
        "shared_target": (np.array(sq, F), np.array([[0], [1], [2], [3], [0]], np.int32), [0.0, 50.0, 0.0], {"margin": 50.0, "edge": 0 * 8 + 1, "stable": 1}),
    }
    return cases


IDENTITY = np.array([[1, 0, 0, 0]], F)


def host(lrm, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None, **kw):
    margin, edge, stable, feet, _ = lrm.stance_stability_cpu(targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in, **kw)
    return {"margin": margin, "edge": edge, "stable": stable, "feet": feet}


def assert_same(got, want):
    """got: (margin, edge, stable, feet) arrays (edge / feet may be None); want: brute_np's or the host loop's dict"""
    margin, edge, stable, feet = got
    shape = want["margin"].shape
    assert np.array_equal(pc.bits(margin).reshape(shape), pc.bits(want["margin"]))
    if edge is not None:
        assert np.array_equal(np.asarray(edge).reshape(shape), want["edge"])
    assert np.array_equal(np.asarray(stable).reshape(shape), want["stable"])
    if feet is not None:
        assert np.array_equal(np.asarray(feet).reshape(-1), want["feet"])


def assert_consequences(want, min_margin=0.0):
    """edge 255 iff margin -inf; stable iff margin > min_margin; no nan, no -0; a stance without three valid feet is -inf"""
    m = want["margin"]
    assert not np.isnan(m).any() and not (pc.bits(m) == 0x80000000).any()
    assert np.array_equal(want["edge"] == 255, np.isneginf(m))
    assert np.array_equal(want["stable"].astype(bool), m > F(min_margin))
    few = np.array([bin(int(f)).count("1") < 3 for f in want["feet"]])
    assert np.isneginf(m[:, few]).all()
    e = want["edge"][want["edge"] != 255]
    assert ((e >> 3) != (e & 7)).all() and (e < 64).all()


def kinds(want):
    """fractions of (stance, lift set) answers: stable, unstable with a finite margin, -inf"""
    m = want["margin"]
    return float((want["stable"] == 1).mean()), float(((want["stable"] == 0) & ~np.isneginf(m)).mean()), float(np.isneginf(m).mean())
