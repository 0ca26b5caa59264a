"""Shared cases of the trunk-leg clearance tests (tests/test_trunk_clearance_cpu.py, tests/test_gpu_trunk_clearance.py):
link_dist_np, the link-to-cylinder distance of include/lrm.h (lrm_trunk_clearance_posed_dev) restated in vectorised numpy
float32, one rounding per operation -- the point-to-cylinder h, the ternary search of ROUNDS rounds and the fold of every h
evaluated -- written from that text and not from csrc/lrm_trunk_clearance.h; to_body_np, the body-frame step restated as
body_clearance_cases.brute_np restates it; hand-made and random links about a cylinder; and brute_np, the per-(set, leg)
answers from those.

brute_np does not restate the joint chain: it takes RELATIVE joints from leg_clearance_cases.joints_from_fk (lrm_fk_posed_cpu
on shortened legs, body None), as self_clearance_cases does.  The independent check -- joints from the leg's geometry and the
true minimum distance of a segment to the solid cylinder, in float64 -- lives in tests/trunk_model64.py."""
import numpy as np

import ik_cases
import leg_clearance_cases as lc
import pair_cases as pc
import self_clearance_cases as sc

F = np.float32
ROUNDS = 32                        # N of include/lrm.h
RADIUS = lc.RADIUS                 # coxa, femur, tibia link (mm)
MARGIN = lc.MARGIN
TIP_CLEAR = lc.TIP_CLEAR
LINKS = 0b110                      # femur and tibia: the coxa link starts at its mount on the trunk
KEYS = ("links", "worst", "pen", "free")
KINDS = ("through_axis", "tangent_side", "crossing_cap", "nearest_rim", "parallel_inside", "parallel_outside", "in_cap_plane",
         "degenerate", "wholly_inside")


def trunk_of(legs, beyond=5.0, plus_z=40.0, minus_z=-80.0):
    """(trunk_radius, plus_z, minus_z): a cylinder whose radius lies `beyond` mm past the farthest leg mount (the legs' body
    offset, column BODY), a few tens of mm thick"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    return float(F(np.abs(legs[:, ik_cases.BODY]).max() + beyond)), plus_z, minus_z


def h_np(P, trunk):
    """the squared distance of the body-frame points P [n, 3] to the solid cylinder, in P's dtype"""
    T = P.dtype.type
    R, pz, mz = (T(F(v)) for v in trunk)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    rho = np.sqrt(x * x + y * y)
    dr = np.where(rho > R, rho - R, T(0))
    dz = np.where(z > pz, z - pz, np.where(z < mz, mz - z, T(0)))
    return dr * dr + dz * dz


def link_dist_np(A, B, trunk, T=F, rounds=ROUNDS, detail=False):
    """body-frame links A -> B (float32 [n, 3]) -> d [n] in T (float32: one rounding per operation; float64: the same steps on
    the same float32 inputs).  detail=True -> (d, which int[n]: 0 the least h was h(A), 1 h(B), 2 a point of the search)"""
    A, B = np.asarray(A, F).reshape(-1, 3).astype(T), np.asarray(B, F).reshape(-1, 3).astype(T)
    with np.errstate(all="ignore"):
        e = B - A
        best = h_np(A, trunk)
        which = np.zeros(len(A), int)
        hb = h_np(B, trunk)
        which = np.where(hb < best, 1, which)
        best = np.where(hb < best, hb, best)
        lo, hi = np.zeros(len(A), T), np.ones(len(A), T)
        for _ in range(rounds):
            w = (hi - lo) / T(3)
            m1, m2 = lo + w, hi - w
            h1, h2 = h_np(A + m1[:, None] * e, trunk), h_np(A + m2[:, None] * e, trunk)
            which = np.where(h1 < best, 2, which)
            best = np.where(h1 < best, h1, best)
            which = np.where(h2 < best, 2, which)
            best = np.where(h2 < best, h2, best)
            take = h1 <= h2
            hi, lo = np.where(take, m2, hi), np.where(take, lo, m1)
        d = np.sqrt(best)
    assert d.dtype == T
    return (d, which) if detail else d


def to_body_np(quats, J):
    """J float32 [n, 3] in the caller's frame, one quaternion per row (float32 [n, 4]) -> the body frame: qt_invert, the
    coefficient sums t2 .. t10 and 2 * ((a vx + b vy) + c vz) + v per component, one rounding per operation"""
    q = np.asarray(quats, F).reshape(-1, 4)
    J = np.asarray(J, F).reshape(-1, 3)
    two = F(2)
    with np.errstate(all="ignore"):
        n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
        x, y, z, w = q[:, 0] / n2, -q[:, 1] / n2, -q[:, 2] / n2, -q[:, 3] / n2
        t2, t3, t4, t5, t6, t7, t8, t9, t10 = x * y, x * z, x * w, -y * y, y * z, y * w, -z * z, z * w, -w * w
        vx, vy, vz = J[:, 0], J[:, 1], J[:, 2]
        rx = two * ((t8 + t10) * vx + (t6 - t4) * vy + (t3 + t7) * vz) + vx
        ry = two * ((t4 + t6) * vx + (t5 + t10) * vy + (t9 - t2) * vz) + vy
        rz = two * ((t7 - t3) * vx + (t2 + t9) * vy + (t5 + t8) * vz) + vz
    out = np.stack([rx, ry, rz], 1)
    assert out.dtype == F
    return out


def body_joints(joints, quats, pose_idx=None):
    """joints float32 [nlegs, nsets, 4, 3] relative to the body, caller's frame -> the same in the body frame of each set's
    pose"""
    nl, ns = joints.shape[:2]
    p, _ = sc.set_poses(len(quats), ns, pose_idx)
    q = np.asarray(quats, F).reshape(-1, 4)[p] if len(quats) else np.zeros((ns, 4), F)
    qq = np.broadcast_to(q[None, :, None, :], (nl, ns, 4, 4)).reshape(-1, 4)
    return to_body_np(qq, joints.reshape(-1, 3)).reshape(nl, ns, 4, 3)


def brute_np(joints, quats, radius, margin, trunk, links=LINKS, pose_idx=None, live=None, detail=False):
    """joints float32 [nlegs, nsets, 4, 3] relative to the body (caller's frame), live bool[nsets] or None -> dict of KEYS
    ([nlegs, nsets], free [nsets]); detail=True adds "d" float32 [nlegs, nsets, 3] (inf: not tested), "valid" and "body"
    (the body-frame joints)"""
    nl, ns = joints.shape[:2]
    radius = np.asarray(radius, F).reshape(3)
    reach = (radius + F(margin)).astype(F)  # the sums formed once
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    valid = np.isfinite(joints).all((2, 3))
    V = body_joints(joints, quats, pose_idx)
    hit_bits = np.zeros((nl, ns), np.uint8)
    worst = np.full((nl, ns), 255, np.uint8)
    pen = np.full((nl, ns), -np.inf, F)
    dall = np.full((nl, ns, 3), np.inf, F)
    ok = valid & live[None, :]
    with np.errstate(all="ignore"):
        for k in range(3):
            if not (links >> k) & 1 or radius[k] == 0:
                continue
            d = link_dist_np(V[:, :, k].reshape(-1, 3), V[:, :, k + 1].reshape(-1, 3), trunk).reshape(nl, ns)
            dall[:, :, k] = np.where(ok, d, F(np.inf))
            hit, near = ok & (d < radius[k]), ok & (d < reach[k])
            pk = ((radius[k] - d) + F(0)).astype(F)
            hit_bits |= (hit.astype(np.uint8) << k).astype(np.uint8)
            better = near & ((worst == 255) | (pk > pen))  # ties stay with the smaller k
            worst = np.where(better, np.uint8(k), worst)
            pen = np.where(better, pk, pen)
    out = {"links": hit_bits, "worst": worst, "pen": pen, "free": (live & (hit_bits == 0).all(0)).astype(np.uint8)}
    if detail:
        out.update(d=dall, valid=valid, body=V)
    return out


def host(lrm, quats, legs, angles, trunk, radius=RADIUS, margin=MARGIN, tip_clear=TIP_CLEAR, links=LINKS, pose_idx=None, live_in=None, **kw):
    hit, worst, pen, free, _ = lrm.trunk_clearance_posed_cpu(quats, legs, angles, radius, trunk[0], trunk[1], trunk[2], margin, tip_clear,
                                                             links, pose_idx, live_in, **kw)
    return {"links": hit, "worst": worst, "pen": pen, "free": free}


def assert_same(got, want):
    """got: (links, worst, pen, free) arrays (pen / free may be None); want: brute_np's or the host loop's"""
    shape = want["links"].shape
    for g, k in zip(got[:2], KEYS[:2]):
        assert np.array_equal(np.asarray(g).reshape(shape), want[k]), k
    if got[2] is not None:
        assert np.array_equal(pc.bits(got[2]).reshape(shape), pc.bits(want["pen"]))
    if got[3] is not None:
        assert np.array_equal(np.asarray(got[3]), want["free"])


def assert_consequences(want, margin, links=LINKS, live=None):
    """include/lrm.h's consequences: pen > 0 iff links != 0, margin 0 makes worst a hit or 255, links == 0 gives the empty
    answer and free = live, free = live and no hit, a dead set has the empty answer and free 0"""
    nl, ns = want["links"].shape
    live = np.ones(ns, bool) if live is None else np.asarray(live, bool)
    hit = want["links"] != 0
    assert (want["links"] & ~np.uint8(links & 7) == 0).all()
    assert np.array_equal(want["pen"] > 0, hit)
    assert np.array_equal(want["worst"] == 255, np.isneginf(want["pen"]))
    some = want["worst"] != 255
    assert np.isfinite(want["pen"][some]).all() and (want["worst"][some] < 3).all() and ((links >> want["worst"][some]) & 1 == 1).all()
    assert (((want["links"] >> np.minimum(want["worst"], 2)) & 1)[hit] == 1).all()  # the deepest link of a leg with a hit is a hit
    if margin == 0:
        assert np.array_equal(some, hit)
    assert np.array_equal(want["free"].astype(bool), live & ~hit.any(0))
    dead = ~live
    assert (want["links"][:, dead] == 0).all() and (want["worst"][:, dead] == 255).all()
    assert np.isneginf(want["pen"][:, dead]).all() and (want["free"][dead] == 0).all()
    if links & 7 == 0:
        assert not hit.any() and not some.any() and np.array_equal(want["free"].astype(bool), live)


# ---- hand-made links about a cylinder ----

CYL = (150.0, 40.0, -30.0)  # the cylinder of the hand-made and random links: radius, plus_z, minus_z (mm)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def hand_made_links(n=1500, seed=4, cyl=CYL):
    """kind -> (A, B, expect): A, B float32 [n, 3] in the body frame, coordinates to 600 mm, link lengths 5 .. 400 mm; expect
    float64 [n]: the distance in closed form from the float32 ends where the kind has one (nan elsewhere), which also says
    which term of h decides: 0 (through_axis, crossing_cap, wholly_inside), the radial term alone from the plane distance of
    the axis to the link (tangent_side, in_cap_plane: dz is exactly 0), the axial term alone (parallel_inside), both from the
    link's own radius and z range (parallel_outside); nearest_rim (both terms, at an interior point of the link) and
    degenerate (h of one point) have none"""
    rng = np.random.default_rng(seed)
    R, pz, mz = cyl
    az = lambda: rng.uniform(0.0, 2 * np.pi, n)
    L = lambda lo=5.0, hi=400.0: rng.uniform(lo, hi, n)
    polar = lambda r, a, z: np.column_stack([r * np.cos(a), r * np.sin(a), z])
    horiz = lambda a: np.column_stack([np.cos(a), np.sin(a), np.zeros(n)])
    out = {}

    def axis_to_link(A, B):  # the distance of the z axis from the link's projection on the plane z = 0, float64
        a, e = A[:, :2], B[:, :2] - A[:, :2]
        ee = (e * e).sum(1)
        t = np.clip(np.where(ee > 0, -(a * e).sum(1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
        return np.linalg.norm(a + t[:, None] * e, axis=1)

    def put(kind, A, B, closed=None):
        A, B = np.clip(A, -600.0, 600.0).astype(F), np.clip(B, -600.0, 600.0).astype(F)
        a, b = A.astype(np.float64), B.astype(np.float64)
        dz = np.maximum(np.maximum(np.minimum(a[:, 2], b[:, 2]) - pz, mz - np.maximum(a[:, 2], b[:, 2])), 0.0)
        dr = np.maximum(axis_to_link(a, b) - R, 0.0)
        expect = {None: np.full(n, np.nan), "zero": np.zeros(n), "radial": dr, "axial": dz, "both": np.hypot(dr, dz)}[closed]
        out[kind] = (A, B, expect)

    # through the axis: a horizontal chord through x = y = 0 between the caps, both ends outside
    a, z = az(), rng.uniform(mz + 1.0, pz - 1.0, n)
    r1, r2 = R + L(5.0, 190.0), R + L(5.0, 190.0)
    put("through_axis", polar(r1, a, z), polar(r2, a + np.pi, z), "zero")
    # tangent to the side: a horizontal line whose foot from the axis lies at R + gap, gap 0 .. 60, between the caps
    a, z, gap, l = az(), rng.uniform(mz + 1.0, pz - 1.0, n), rng.uniform(0.0, 60.0, n), L(20.0, 400.0)
    foot, t = polar(R + gap, a, z), horiz(a + np.pi / 2)
    s = rng.uniform(0.1, 0.9, n)
    put("tangent_side", foot - t * (l * s)[:, None], foot + t * (l * (1 - s))[:, None], "radial")
    # crossing a cap: from above the top cap (or below the bottom one) down into the cylinder, inside the radius
    a1, a2 = az(), az()
    top = rng.uniform(size=n) < 0.5
    zo = np.where(top, pz + L(5.0, 200.0), mz - L(5.0, 200.0))
    zi = rng.uniform(mz + 1.0, pz - 1.0, n)
    put("crossing_cap", polar(rng.uniform(0.0, R - 5.0, n), a1, zo), polar(rng.uniform(0.0, R - 5.0, n), a2, zi), "zero")
    # nearest to the rim: a link outside both the radius and a cap plane, crossing the rim's corner region
    a, l = az(), L(5.0, 300.0)
    top = rng.uniform(size=n) < 0.5
    c = polar(R + rng.uniform(1.0, 120.0, n), a, np.where(top, pz + rng.uniform(1.0, 120.0, n), mz - rng.uniform(1.0, 120.0, n)))
    u = _unit(np.column_stack([-np.sin(a) * rng.normal(size=n), np.cos(a) * rng.normal(size=n), 0.2 * rng.normal(size=n)]) +
              1e-3 * rng.normal(size=(n, 3)))
    s = rng.uniform(0.1, 0.9, n)
    put("nearest_rim", c - u * (l * s)[:, None], c + u * (l * (1 - s))[:, None])
    # parallel to the axis, inside the radius: above, through and below the slab
    a, r, z0, l = az(), rng.uniform(0.0, R - 1.0, n), rng.uniform(-400.0, 300.0, n), L(5.0, 300.0)
    put("parallel_inside", polar(r, a, z0), polar(r, a, z0 + l), "axial")
    # parallel to the axis, outside the radius
    a, r, z0, l = az(), R + rng.uniform(0.0, 200.0, n), rng.uniform(-400.0, 300.0, n), L(5.0, 300.0)
    put("parallel_outside", polar(r, a, z0), polar(r, a, z0 + l), "both")
    # lying in a cap plane: z = plus_z or minus_z exactly, anywhere in the plane
    zc = np.where(rng.uniform(size=n) < 0.5, pz, mz)
    a1, a2 = az(), az()
    A = polar(rng.uniform(0.0, 400.0, n), a1, zc)
    B = A + horiz(a2) * L(5.0, 400.0)[:, None]
    put("in_cap_plane", A, B, "radial")
    # degenerate: A = B anywhere
    A = rng.uniform(-400.0, 400.0, (n, 3))
    A[: n // 4] = polar(rng.uniform(0.0, R, n), az(), rng.uniform(mz, pz, n))[: n // 4]  # a quarter inside
    put("degenerate", A, A)
    # wholly inside
    A = polar(rng.uniform(0.0, R - 1.0, n), az(), rng.uniform(mz + 0.5, pz - 0.5, n))
    B = polar(rng.uniform(0.0, R - 1.0, n), az(), rng.uniform(mz + 0.5, pz - 0.5, n))
    put("wholly_inside", A, B, "zero")
    assert tuple(out) == KINDS
    return out


def random_links(n=100000, seed=6):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-400.0, 400.0, (n, 3))
    B = A + _unit(rng.normal(size=(n, 3))) * rng.uniform(5.0, 400.0, (n, 1))
    return np.clip(A, -600.0, 600.0).astype(F), np.clip(B, -600.0, 600.0).astype(F)
