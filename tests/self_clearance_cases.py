"""Shared cases of the leg-leg self clearance tests (tests/test_self_clearance_cpu.py, tests/test_gpu_self_clearance.py):
pair_dist_np, the link-pair distance of include/lrm.h (lrm_self_clearance_posed_dev) restated in vectorised numpy, one
rounding per operation in float32 and the same formulas in float64, written from that text and not from
csrc/lrm_self_clearance.h; hand-made and random segment pairs; and brute_np, the per-(set, leg) answers from that distance.

brute_np does not restate the joint chain: it takes RELATIVE joints from leg_clearance_cases.joints_from_fk (lrm_fk_posed_cpu
on shortened legs, body None), one pose per set.  The joints here therefore come from the library's own FK, and pair_dist_np
restates the contract's formulas; the independent check -- joints from the leg's geometry and the true minimum distance between
two segments, in float64 -- lives in tests/leg_model64.py and tests/test_clearance_float64_cpu.py."""
import numpy as np

import leg_clearance_cases as lc
import pair_cases as pc

F = np.float32
RADIUS = lc.RADIUS                 # coxa, femur, tibia link (mm)
RADIUS_COXA = (90.0, 22.0, 16.0)   # a thick coxa link: coxa bits occur
MARGIN = lc.MARGIN
TIP_CLEAR = lc.TIP_CLEAR
KEYS = ("hits", "with", "links", "worst", "pen", "free")
BRANCHES = ("both_degenerate", "first_degenerate", "second_degenerate", "t_below", "t_above", "interior")


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _clamp01(x):
    T = x.dtype.type
    return np.where(~(x > 0), T(0), np.where(x > 1, T(1), x))


def _link_dist(a, ab, den, q):
    """the point-to-link distance of lrm_leg_clearance_posed_dev's text"""
    T = a.dtype.type
    ap = q - a
    num = (ap[:, 0] * ab[:, 0] + ap[:, 1] * ab[:, 1]) + ap[:, 2] * ab[:, 2]
    s = _clamp01(np.where(den > 0, num / den, T(0)))
    e = ap - s[:, None] * ab
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def pair_dist_np(segs, T=F, detail=False):
    """segs [n, 12] = A1, B1, A2, B2 -> d [n] in T (float32: one rounding per operation; float64: the same formulas on the
    same float32 inputs).  detail=True -> (d, dict(branch int[n] indexing BRANCHES, den_pos bool[n] (general case only),
    fold bool[n, 4]: endpoint distance k lowered d))"""
    g = np.asarray(segs, F).reshape(-1, 12).astype(T)
    A1, B1, A2, B2 = g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:12]
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        d1, d2, r = B1 - A1, B2 - A2, A1 - A2
        a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        apos, epos = a > 0, e > 0
        den = a * e - b * b
        s0 = np.where(den > 0, _clamp01((b * f - c * e) / den), zero)
        tn = b * s0 + f
        below, above = ~(tn > 0), tn > e
        s_gen = np.where(below, _clamp01(-c / a), np.where(above, _clamp01((b - c) / a), s0))
        t_gen = np.where(below, zero, np.where(above, one, tn / e))
        s = np.where(~apos, zero, np.where(~epos, _clamp01(-c / a), s_gen))
        t = np.where(~apos & ~epos, zero, np.where(~apos, _clamp01(f / e), np.where(~epos, zero, t_gen)))
        w = (r + s[:, None] * d1) - t[:, None] * d2
        d = np.sqrt(_dot(w, w))
        fold = np.zeros((len(g), 4), bool)
        for k, dk in enumerate((_link_dist(A2, d2, e, A1), _link_dist(A2, d2, e, B1), _link_dist(A1, d1, a, A2), _link_dist(A1, d1, a, B2))):
            fold[:, k] = dk < d
            d = np.where(fold[:, k], dk, d)
    assert d.dtype == T
    if not detail:
        return d
    branch = np.where(~apos & ~epos, 0, np.where(~apos, 1, np.where(~epos, 2, np.where(below, 3, np.where(above, 4, 5)))))
    return d, {"branch": branch, "den_pos": (den > 0) & apos & epos, "general": apos & epos, "fold": fold}


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def hand_made_pairs(n=1500, seed=3):
    """kind -> float32 [n, 12]: coordinates to 600 mm, link lengths 5 .. 400 mm"""
    rng = np.random.default_rng(seed)
    P = lambda: rng.uniform(-400.0, 400.0, (n, 3))
    U = lambda: _unit(rng.normal(size=(n, 3)))
    L = lambda: rng.uniform(5.0, 400.0, (n, 1))
    frac = lambda lo=0.0, hi=1.0: rng.uniform(lo, hi, (n, 1))

    def perp(u):
        v = np.cross(u, U())
        return _unit(v)

    out = {}
    seg = lambda A1, B1, A2, B2: np.clip(np.concatenate([A1, B1, A2, B2], 1), -600.0, 600.0).astype(F)
    # crossing: the closest points are interior to both links, a gap of 0 .. 80 mm along the common normal
    X, u1, u2, l1, l2 = P() * 0.5, U(), U(), L(), L()
    nrm = _unit(np.cross(u1, u2))
    A1, A2 = X - u1 * l1 * frac(0.1, 0.9), X + nrm * frac(0.0, 80.0) - u2 * l2 * frac(0.1, 0.9)
    out["crossing"] = seg(A1, A1 + u1 * l1, A2, A2 + u2 * l2)
    # touching: an end of link 2, or a point inside it, lies on link 1
    X, u1, u2, l1, l2 = P() * 0.5, U(), U(), L(), L()
    A1 = X - u1 * l1 * frac()
    inside = frac() * (rng.uniform(size=(n, 1)) < 0.5)  # half of them touch with the end A2
    A2 = X - u2 * l2 * inside
    out["touching"] = seg(A1, A1 + u1 * l1, A2, A2 + u2 * l2)
    # exactly parallel: the second link is the first one's direction in float32, shifted sideways and along
    X, u1, l1, l2 = P() * 0.5, U(), L(), L()
    A1 = X.astype(F).astype(np.float64)
    dv = (u1 * l1).astype(F).astype(np.float64)
    k = rng.choice([0.25, 0.5, 1.0, 2.0], (n, 1))  # exact multiples
    off = (perp(u1) * frac(0.0, 100.0) + u1 * rng.uniform(-300.0, 300.0, (n, 1))).astype(F).astype(np.float64)
    out["parallel"] = seg(A1, A1 + dv, A1 + off, (A1 + off) + dv * k)
    # nearly parallel: the direction perturbed by 1e-6 .. 1e-1
    X, u1, l1, l2 = P() * 0.5, U(), L(), L()
    eps = 10.0 ** rng.uniform(-6.0, -1.0, (n, 1))
    u2 = _unit(u1 + perp(u1) * eps) * rng.choice([-1.0, 1.0], (n, 1))
    A1 = X
    A2 = X + perp(u1) * frac(0.0, 60.0) + u1 * rng.uniform(-200.0, 200.0, (n, 1))
    out["nearly_parallel"] = seg(A1, A1 + u1 * l1, A2, A2 + u2 * l2)
    # collinear: on one line, overlapping and disjoint
    X, u1, l1, l2 = P() * 0.5, U(), L(), L()
    A1 = X
    start = np.where(rng.uniform(size=(n, 1)) < 0.5, frac(-0.5, 0.9) * l1, l1 + frac(0.0, 200.0))  # overlapping / beyond B1
    A2 = X + u1 * start
    out["collinear"] = seg(A1, A1 + u1 * l1, A2, A2 + u1 * l2 * rng.choice([-1.0, 1.0], (n, 1)))
    # one link degenerate (a point), at either place
    A1, A2, u, l = P(), P(), U(), L()
    first = rng.uniform(size=(n, 1)) < 0.5
    out["one_degenerate"] = seg(A1, np.where(first, A1, A1 + u * l), A2, np.where(first, A2 + u * l, A2))
    A1, A2 = P(), P()
    A2[: n // 4] = A1[: n // 4]  # the same point
    out["both_degenerate"] = seg(A1, A1, A2, A2)
    A1, u, l = P(), U(), L()
    B1 = A1 + u * l
    flip = rng.uniform(size=(n, 1)) < 0.5
    out["identical"] = seg(A1, B1, np.where(flip, B1, A1), np.where(flip, A1, B1))
    return out


def random_pairs(n=100000, seed=5):
    rng = np.random.default_rng(seed)
    A1, A2 = rng.uniform(-400.0, 400.0, (n, 3)), rng.uniform(-400.0, 400.0, (n, 3))
    B1 = A1 + _unit(rng.normal(size=(n, 3))) * rng.uniform(5.0, 400.0, (n, 1))
    B2 = A2 + _unit(rng.normal(size=(n, 3))) * rng.uniform(5.0, 400.0, (n, 1))
    return np.clip(np.concatenate([A1, B1, A2, B2], 1), -600.0, 600.0).astype(F)


def all_pairs():
    """every hand-made kind and the random pairs in one float32 [n, 12] array"""
    return np.concatenate(list(hand_made_pairs().values()) + [random_pairs()])


def legs_n(lrm, n):
    """n legs: the first n of m2_6_tilted up to six, the random legs of ik_cases beyond"""
    import ik_cases
    if n <= 6:
        return np.ascontiguousarray(np.asarray(pc.leg_families(lrm)["m2_6_tilted"][0], F).reshape(-1, 14)[:n])
    return np.stack([leg for _, leg, _ in ik_cases.random_legs(lrm)][:n]).astype(F)


def set_poses(nposes, nsets, pose_idx=None, live_in=None):
    """(pose per set clipped into the poses, live bool[nsets]): a set is dead with live_in 0 or a pose outside [0, nposes)"""
    p = np.arange(nsets, dtype=np.int64) if pose_idx is None else np.asarray(pose_idx, np.int64)
    live = (p >= 0) & (p < nposes)
    if live_in is not None:
        live &= np.asarray(live_in) != 0
    return np.clip(p, 0, max(nposes - 1, 0)), live


def joints_of_sets(lrm, angles, quats, legs, tip_clear, pose_idx=None):
    """float32 [nlegs, nsets, 4, 3], RELATIVE to the body, through lrm_fk_posed_cpu (leg_clearance_cases.joints_from_fk)"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    ns = np.asarray(angles).size // (3 * len(legs))
    p, _ = set_poses(len(quats), ns, pose_idx)
    return lc.joints_from_fk(lrm, angles, np.ascontiguousarray(np.asarray(quats, F).reshape(-1, 4)[p]), None, legs, tip_clear)


def brute_np(joints, radius, margin, live=None, T=F, detail=False):
    """joints float32 [nlegs, nsets, 4, 3] relative to the body, live bool[nsets] or None -> dict of KEYS ([nlegs, nsets], free
    [nsets]).  T=float64: the same decisions from the float64 distance.  detail=True adds "pairs": a list of
    (i, j, ka, kb, d [nsets], tested bool[nsets], rr, segs float32 [nsets, 12] = A1, B1, A2, B2)"""
    nl, ns = joints.shape[:2]
    radius = np.asarray(radius, F).reshape(3)
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    valid = np.isfinite(joints).all((2, 3))
    hits = np.zeros((nl, ns), np.int32)
    with_, links = np.zeros((nl, ns), np.uint8), np.zeros((nl, ns), np.uint8)
    worst = np.full((nl, ns), 255, np.int64)
    pen = np.full((nl, ns), -np.inf, T)
    pairs = []
    with np.errstate(all="ignore"):
        for j in range(nl):
            for i in range(j):
                ok = live & valid[i] & valid[j]
                for ka in range(3):
                    for kb in range(3):
                        if radius[ka] == 0 or radius[kb] == 0:
                            continue
                        segs = np.concatenate([joints[i, :, ka], joints[i, :, ka + 1], joints[j, :, kb], joints[j, :, kb + 1]], 1)
                        d = pair_dist_np(segs, T)
                        rr = T(radius[ka] + radius[kb])  # the float32 sum
                        reach = T(F(radius[ka] + radius[kb]) + F(margin))  # formed once, in float32
                        hit, near = ok & (d < rr), ok & (d < reach)
                        pk = ((rr - d) + T(0)).astype(T)
                        for me, other, own, oth in ((i, j, ka, kb), (j, i, kb, ka)):
                            hits[me] += hit
                            with_[me] |= (hit.astype(np.uint8) << other).astype(np.uint8)
                            links[me] |= (hit.astype(np.uint8) << own).astype(np.uint8)
                            code = other * 9 + own * 3 + oth
                            better = near & ((worst[me] == 255) | (pk > pen[me]) | ((pk == pen[me]) & (code < worst[me])))
                            worst[me] = np.where(better, code, worst[me])
                            pen[me] = np.where(better, pk, pen[me])
                        if detail:
                            pairs.append((i, j, ka, kb, d, ok, rr, segs))
    out = {"hits": hits, "with": with_, "links": links, "worst": worst.astype(np.uint8), "pen": pen,
           "free": (live & (hits == 0).all(0)).astype(np.uint8)}
    if detail:
        out["pairs"] = pairs
        out["valid"] = valid
    return out


def host(lrm, quats, legs, angles, radius=RADIUS, margin=MARGIN, tip_clear=TIP_CLEAR, pose_idx=None, live_in=None, **kw):
    hits, with_, links, worst, pen, free, _ = lrm.self_clearance_posed_cpu(quats, legs, angles, radius, margin, tip_clear, pose_idx, live_in, **kw)
    return {"hits": hits, "with": with_, "links": links, "worst": worst, "pen": pen, "free": free}


def assert_same(got, want):
    """got: (hits, with, links, worst, pen, free) arrays (pen / free may be None); want: brute_np's or the host loop's"""
    shape = want["hits"].shape
    for g, k in zip(got[:4], KEYS[:4]):
        assert np.array_equal(np.asarray(g).reshape(shape), want[k]), k
    if got[4] is not None:
        assert np.array_equal(pc.bits(got[4]).reshape(shape), pc.bits(want["pen"]))
    if got[5] is not None:
        assert np.array_equal(np.asarray(got[5]), want["free"])


def assert_consequences(want, margin, live=None):
    """include/lrm.h's consequences: symmetric with, an even hit sum, pen > 0 iff hits > 0 iff with != 0 iff links != 0, margin 0
    makes worst a hit or 255, free = live and no hit, a dead set has the empty answer and free 0"""
    nl, ns = want["hits"].shape
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    w = want["with"]
    for i in range(nl):
        assert ((w[i] >> i) & 1 == 0).all()
        for j in range(nl):
            assert np.array_equal((w[i] >> j) & 1, (w[j] >> i) & 1)
    assert (w >> nl == 0).all() and (want["links"] >> 3 == 0).all()
    assert (want["hits"].sum(0) % 2 == 0).all()
    hit = want["hits"] > 0
    assert np.array_equal(want["pen"] > 0, hit) and np.array_equal(w != 0, hit) and np.array_equal(want["links"] != 0, hit)
    assert np.array_equal(want["worst"] == 255, np.isneginf(want["pen"]))
    assert np.isfinite(want["pen"][want["worst"] != 255]).all()
    some = want["worst"] != 255
    other = want["worst"] // 9
    assert (other[some] < nl).all() and (other != np.arange(nl)[:, None])[some].all()
    if margin == 0:
        assert np.array_equal(some, hit)
    assert np.array_equal(want["free"].astype(bool), live & ~hit.any(0))
    dead = ~live
    assert (want["hits"][:, dead] == 0).all() and (w[:, dead] == 0).all() and (want["links"][:, dead] == 0).all()
    assert (want["worst"][:, dead] == 255).all() and np.isneginf(want["pen"][:, dead]).all() and (want["free"][dead] == 0).all()
    if nl == 1:
        assert not hit.any() and (want["worst"] == 255).all() and np.array_equal(want["free"].astype(bool), live)
