"""Boundary clouds for the joint-angle tests: tips of configurations ON the faces, edges and corners of the joint-limit
set, at full extension and full fold, on and behind the coxa axis and beside the yaw limits; each as it is and moved by
1e-4 .. 1 mm.  Deterministic (seeded per case), written from the formulas of include/lrm.h and ik_cases.fk64 only.

cloud(oracle, leg, quat) returns a dict of parallel arrays:
  pts   float32 (n, 3)  the query points
  src   float32 (n, 3)  the source configuration (coxa, femur, tibia) of each point's tip, float32 so that lrm_fk_* can
                        take it as it stands; the tip itself is fk64 of these values
  cls   int8 (n,)       index into CLASSES
  move  float64 (n,)    how far the tip was moved (mm); 0: as it is
  dirn  int8 (n,)       0 not moved, 1 seeded random direction, 2 along the outward normal, 3 against it
A case holds at most MAX_POINTS points."""
import itertools
import zlib

import numpy as np

import ik_model64 as m64
from ik_cases import (COXA_LEN, FEMUR_LEN, TIBIA_LEN, check_contract, fk64, golden_cases, limits, load_case,
                      random_cloud, random_legs, standard_cases)

CLASSES = ("faces", "edges_corners", "extension", "axis", "behind", "yaw_faces")
FAR = len(CLASSES)  # the class index of the far points a Case can mix in (no source configuration)
GAP_NEAR = 1e-3  # mm: the reference's CIRCLE_MARGIN, half of LRM_IK_TOL_F; the other half is float32's
MOVES = (1e-4, 1e-3, 3e-3, 1e-2, 1.0)  # mm
YAW_PUSHES = (10.0, 100.0)  # mm, yaw_faces only: well out of the yaw range, where the clamped and mirrored yaws compete
MAX_POINTS = 16_000
FACE_GRID = 14

# the eight faces: (joint or "abs", 0 lower / 1 upper)
FACES = tuple((k, s) for k in ("coxa", "femur", "tibia", "abs") for s in (0, 1))


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _settle(a, L):
    """float32 configurations that pass in_limits: rounding to float32 can leave the absolute limits by an ulp; the
    tibia then steps inwards (the own limits are float32 values already, so they hold)"""
    a = _f32(a).reshape(-1, 3)
    _, _, alo, ahi = m64.bounds(L)
    for _ in range(4):
        t32 = a[:, 2].astype(np.float32)
        s = a[:, 1] + a[:, 2]
        t32 = np.where(s > ahi, np.nextafter(t32, np.float32(-np.inf)), t32)
        t32 = np.where(s < alo, np.nextafter(t32, np.float32(np.inf)), t32)
        a[:, 2] = t32.astype(np.float64)
    return a[m64.in_limits(a, L)]


def _axis(L, k, n):
    lo, hi = float(L[k][0]), float(L[k][1])
    return np.linspace(lo, hi, n)


def _on_face(L, face, n_c, n_ft):
    """configurations with one limit at its bound, the others on a grid"""
    k, s = face
    b = float(L[k][s])
    c, f, t = _axis(L, "coxa", n_c), _axis(L, "femur", n_ft), _axis(L, "tibia", n_ft)
    if k == "coxa":
        g = np.stack(np.meshgrid([b], f, t, indexing="ij"), -1)
    elif k == "femur":
        g = np.stack(np.meshgrid(c, [b], t, indexing="ij"), -1)
    elif k == "tibia":
        g = np.stack(np.meshgrid(c, f, [b], indexing="ij"), -1)
    else:
        g = np.stack(np.meshgrid(c, f, [0.0], indexing="ij"), -1)
        g[..., 2] = b - g[..., 1]
    return g.reshape(-1, 3)


def _outward(a, face, leg, quat, h=1e-6):
    """unit outward normal of `face` at the tips of configurations a (m, 3): the cross product of the face's two tangent
    vectors, signed along the derivative that leaves the set; where the tangents are parallel (a singular
    configuration) that derivative itself; zero where that vanishes too"""
    k, s = face
    J = []
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        J.append((fk64(a + e, leg, quat) - fk64(a - e, leg, quat)) / (2 * h))
    sign = 1.0 if s else -1.0
    if k == "abs":
        out, t1, t2 = sign * J[2], J[0], J[1] - J[2]
    else:
        j = ("coxa", "femur", "tibia").index(k)
        o = [i for i in range(3) if i != j]
        out, t1, t2 = sign * J[j], J[o[0]], J[o[1]]
    nrm = np.cross(t1, t2)
    ln = np.linalg.norm(nrm, axis=1)
    flat = ln < 1e-3 * np.linalg.norm(t1, axis=1) * np.linalg.norm(t2, axis=1) + 1e-12
    nrm = np.where(flat[:, None], out, nrm * np.sign((nrm * out).sum(1))[:, None])
    ln = np.linalg.norm(nrm, axis=1)
    return np.where(ln[:, None] > 1e-9, nrm / np.maximum(ln, 1e-300)[:, None], 0.0)


def _h(a, leg):
    lg = np.asarray(leg, np.float64)
    return lg[COXA_LEN] + lg[FEMUR_LEN] * np.cos(a[:, 1]) + lg[TIBIA_LEN] * np.cos(a[:, 1] + a[:, 2])


def _spread(a, n):
    """n rows of a, evenly through it"""
    if len(a) <= n:
        return a
    return a[np.linspace(0, len(a) - 1, n).round().astype(int)]


def _faces(L, leg, quat):
    out = []
    for face in FACES:
        a = _settle(_on_face(L, face, 5 if face[0] != "coxa" else 1, FACE_GRID if face[0] != "coxa" else 10), L)
        out.append((a, _outward(a, face, leg, quat)))
    return out


def _edges_corners(L, leg, quat):
    """two or three limits at their bounds: every compatible pair of faces with the free joint on 4 values, every
    compatible triple"""
    out = []
    for fa, fb in itertools.combinations(FACES, 2):
        if fa[0] == fb[0]:
            continue
        a = _on_face(L, fa, 4, 4)
        if fb[0] == "abs":  # fa is a joint face: the other of femur / tibia follows, or (coxa face) the tibia does
            b = float(L["abs"][fb[1]])
            if fa[0] == "tibia":
                a[:, 1] = b - a[:, 2]
            else:
                a[:, 2] = b - a[:, 1]
        else:
            a[:, ("coxa", "femur", "tibia").index(fb[0])] = float(L[fb[0]][fb[1]])
        a = np.unique(_settle(a, L), axis=0)
        if len(a):
            n = _outward(a, fa, leg, quat) + _outward(a, fb, leg, quat)
            out.append((a, n))
    for sc, sf, st in itertools.product((0, 1), repeat=3):  # box corners, and a femur or tibia bound meeting an abs one
        c = float(L["coxa"][sc])
        rows = [[c, float(L["femur"][sf]), float(L["tibia"][st])]]
        for sa in (0, 1):
            b = float(L["abs"][sa])
            rows.append([c, float(L["femur"][sf]), b - float(L["femur"][sf])])
            rows.append([c, b - float(L["tibia"][st]), float(L["tibia"][st])])
        a = np.unique(_settle(np.array(rows), L), axis=0)
        if len(a):
            n = _outward(a, ("coxa", sc), leg, quat) + _outward(a, ("femur", sf), leg, quat)
            out.append((a, n))
    return out


def _extension(L, leg, quat):
    """tibia = 0, +-1e-4, +-1e-3 rad (full extension) and the tibia limits (full fold); the normal is the direction of
    the tibia link: outwards at full extension"""
    ts = [0.0, 1e-4, -1e-4, 1e-3, -1e-3, float(L["tibia"][0]), float(L["tibia"][1])]
    g = np.stack(np.meshgrid(_axis(L, "coxa", 2), _axis(L, "femur", 7), ts, indexing="ij"), -1).reshape(-1, 3)
    a = _settle(g, L)
    longer = np.array(leg, np.float64)
    longer[TIBIA_LEN] += 1.0
    n = fk64(a, longer, quat) - fk64(a, leg, quat)
    n[np.abs(a[:, 2]) > 0.5] *= -1.0  # folded: the workspace's inner rim, outwards is towards the knee
    return [(a, n)]


def _axis_tips(L, leg, quat):
    """in-limit configurations with h = C + F cos f + T cos(f + t) = 0, the tip on the coxa axis: for each femur angle
    cos(f + t) = -(C + F cos f) / T solved for the tibia in float64.  Empty where the leg has none."""
    lg = np.asarray(leg, np.float64)
    f = _axis(L, "femur", 41)
    x = -(lg[COXA_LEN] + lg[FEMUR_LEN] * np.cos(f)) / lg[TIBIA_LEN]
    ok = np.abs(x) <= 1.0
    rows = []
    for sgn in (1.0, -1.0):
        for turn in (-2 * np.pi, 0.0, 2 * np.pi):
            s = sgn * np.arccos(np.clip(x[ok], -1, 1)) + turn
            for c in _axis(L, "coxa", 3):
                rows.append(np.stack([np.full(ok.sum(), c), f[ok], s - f[ok]], 1))
    a = _settle(np.concatenate(rows), L) if rows else np.zeros((0, 3))
    return [(_spread(a, 36), np.zeros((min(len(a), 36), 3)))]


def _behind(L, leg, quat):
    """in-limit configurations with h < -1 mm: the tip lies behind the coxa axis, at the mirrored yaw"""
    g = np.stack(np.meshgrid(_axis(L, "coxa", 3), _axis(L, "femur", 25), _axis(L, "tibia", 25), indexing="ij"),
                 -1).reshape(-1, 3)
    a = _settle(g, L)
    a = _spread(a[_h(a, leg) < -1.0], 36)
    return [(a, np.zeros((len(a), 3)))]


def _yaw_faces(L, leg, quat):
    out = []
    for s in (0, 1):
        a = _settle(_on_face(L, ("coxa", s), 1, 4), L)
        out.append((a, _outward(a, ("coxa", s), leg, quat)))
    return out


BUILDERS = (_faces, _edges_corners, _extension, _axis_tips, _behind, _yaw_faces)


def cloud(oracle, leg, quat, seed=0):
    L = limits(oracle, leg, quat)
    rng = np.random.default_rng(seed)
    pts, src, cls, move, dirn = [], [], [], [], []

    def emit(tip, a, k, mv, dr):
        pts.append(tip)
        src.append(a)
        cls.append(np.full(len(a), k, np.int8))
        move.append(np.full(len(a), mv))
        dirn.append(np.full(len(a), dr, np.int8))

    if not m64.is_empty(L):
        for k, build in enumerate(BUILDERS):
            for a, nrm in build(L, leg, quat):
                if len(a) == 0:
                    continue
                tip = fk64(a, leg, quat)
                ln = np.linalg.norm(nrm, axis=1)
                has = ln > 1e-9
                nrm = np.where(has[:, None], nrm / np.maximum(ln, 1e-300)[:, None], 0.0)
                emit(tip, a, k, 0.0, 0)
                pushes = MOVES + (YAW_PUSHES if CLASSES[k] == "yaw_faces" else ())
                for mv in pushes:
                    r = rng.normal(size=tip.shape)
                    r /= np.linalg.norm(r, axis=1)[:, None]
                    emit(tip + mv * r, a, k, mv, 1)
                    if has.any():
                        emit(tip[has] + mv * nrm[has], a[has], k, mv, 2)
                        if mv <= 1.0:
                            emit(tip[has] - mv * nrm[has], a[has], k, mv, 3)
    if not pts:
        z = np.zeros((0, 3), np.float32)
        return {"pts": z, "src": z.copy(), "cls": np.zeros(0, np.int8), "move": np.zeros(0), "dirn": np.zeros(0, np.int8)}
    out = {"pts": np.ascontiguousarray(np.concatenate(pts), np.float32),
           "src": np.ascontiguousarray(np.concatenate(src), np.float32), "cls": np.concatenate(cls),
           "move": np.concatenate(move), "dirn": np.concatenate(dirn)}
    assert len(out["pts"]) <= MAX_POINTS, len(out["pts"])
    return out


def case_seed(name):
    return zlib.crc32(name.encode())


def boundary_cases(lrm):
    """(name, leg, quat, family): the 30 standard cases, the 12 random legs, and each golden fixture's leg with its own
    (not normalised) quaternion, one case per distinct (leg, quaternion)"""
    out = [(n, leg, q, "standard") for n, leg, q in standard_cases(lrm)]
    out += [(n, leg, q, "random") for n, leg, q in random_legs(lrm)]
    seen = set()
    for name in golden_cases():
        c = load_case(name)
        if "leg" not in c or "quat" not in c:
            continue
        leg, q = np.asarray(c["leg"], np.float32), np.asarray(c["quat"], np.float32)
        key = leg.tobytes() + q.tobytes()
        if key not in seen:
            seen.add(key)
            out.append((f"golden_{name}", leg, q, "golden"))
    return out


def case_by_name(lrm, name):
    for c in boundary_cases(lrm):
        if c[0] == name:
            return c
    raise KeyError(name)


class Case:
    """One (leg, quaternion) with its cloud, the oracle's mask and |d| of every point, and, after solve(), an IK answer
    with its float64 miss.  far > 0 mixes that many config-2 points in (class FAR, nan source); mixed=True shuffles the
    cloud (seeded), so that 64 consecutive points hold faces, extension, axis and far points side by side."""

    def __init__(self, oracle, name, leg, quat, family, far=0, mixed=False):
        self.name, self.leg, self.quat, self.family = name, leg, quat, family
        self.L = limits(oracle, leg, quat)
        c = cloud(oracle, leg, quat, case_seed(name))
        self.pts, self.src, self.cls, self.move = c["pts"], c["src"], c["cls"], c["move"]
        if far:
            self.pts = np.concatenate([self.pts, random_cloud(far, seed=case_seed(name) % 1000)])
            self.src = np.concatenate([self.src, np.full((far, 3), np.nan, np.float32)])
            self.cls = np.concatenate([self.cls, np.full(far, FAR, np.int8)])
            self.move = np.concatenate([self.move, np.full(far, np.nan)])
        if mixed:
            o = np.random.default_rng(case_seed(name)).permutation(len(self.pts))
            self.pts, self.src = np.ascontiguousarray(self.pts[o]), np.ascontiguousarray(self.src[o])
            self.cls, self.move = self.cls[o], self.move[o]
        self.mask = oracle.reach(self.pts, leg, quat).astype(bool)
        d, _ = oracle.dist(self.pts, leg, quat)
        self.dn = np.linalg.norm(d.astype(np.float64), axis=1)

    def solve(self, ang, st):
        self.ang, self.st = np.ascontiguousarray(ang, np.float32), np.ascontiguousarray(st, np.uint8)
        self.miss = np.linalg.norm(fk64(self.ang, self.leg, self.quat) - self.pts.astype(np.float64), axis=1)
        self.gap = np.isin(self.st, (3, 4))
        self._search = None
        return self

    def search(self):
        """the model's nearest in-limit tip of every status-3/4 point: (distance, angles), computed once per answer"""
        if self._search is None:
            g = self.gap
            self._search = m64.nearest_in_limit_many(self.pts[g], self.leg, self.quat, self.L, self.src[g])
        return self._search

    def wraps(self):
        """a limit passes +-pi: the limit set then holds configurations the circle model's angles cannot name"""
        return any(abs(float(v)) > np.pi for pair in self.L.values() for v in pair)


def assert_contract_by_class(oracle, c):
    """contract items 1-4 (ik_cases.check_contract, clean=False) on every class of the case's answer"""
    for k in np.unique(c.cls):
        sel = c.cls == k
        try:
            check_contract(oracle, c.pts[sel], c.leg, c.quat, c.ang[sel], c.st[sel], clean=False)
        except AssertionError as e:
            raise AssertionError(f"{c.name} / {(CLASSES + ('far',))[k]}: {e}") from e


def assert_gaps_are_real(c):
    """status 3 or 4 => the float64 search finds no in-limit tip within GAP_NEAR of p, on EVERY such point; so no tip
    moved by GAP_NEAR or less has a gap status"""
    sd, _ = c.search()
    near = sd <= GAP_NEAR
    assert not near.any(), (f"{c.name}: {near.sum()} gap points with an in-limit tip within {GAP_NEAR} mm, e.g. p = "
                            f"{c.pts[c.gap][near][0]} status {c.st[c.gap][near][0]} nearest {sd[near][0]:.3e} mm")
    assert not c.gap[c.move <= GAP_NEAR].any(), f"{c.name}: a tip moved by <= {GAP_NEAR} mm got status 3 / 4"


def assert_fk(c, xyz):
    """FK positions of the source configurations against the float64 FK: the round trip's bound"""
    has = np.isfinite(c.src).all(1)
    err = np.linalg.norm(np.asarray(xyz, np.float64)[has] - fk64(c.src[has], c.leg, c.quat), axis=1)
    assert err.max() <= 1e-3, f"{c.name}: {err.max():.3e} mm"


def other_knee(src, leg):
    """the other knee of the same tip: tibia -> -tibia, the femur turned by twice the knee's offset angle"""
    lg = np.asarray(leg, np.float64)
    F, T = lg[FEMUR_LEN], lg[TIBIA_LEN]
    a = np.asarray(src, np.float64)
    t = a[:, 2]
    f2 = a[:, 1] + 2.0 * np.arctan2(T * np.sin(t), F + T * np.cos(t))
    return np.stack([a[:, 0], f2, -t], 1)


def seed_plan(c, margin=1e-3):
    """per-point seeds: the source configuration, and on every second point the other knee where it lies inside the
    limits by `margin` rad -> (seed float32 (n, 3), want float64 (n, 3), judged bool (n,), other knee bool (n,)).
    Judged: tips as they are (not moved) with |tibia| > 0.01 and h > 1 mm, where the angles follow from the position,
    and |d| <= 2e-3 mm (LRM_IK_TOL_F), where the IK's goal is the tip.  The circle model puts some in-limit tips outside
    its workspace (the standard legs' up to 70 mm, random0's yaw beyond 90 degrees up to 54 mm); their goal is p - d,
    another point.  Far points have a nan seed: no seed."""
    src = c.src.astype(np.float64)
    alt = other_knee(src, c.leg)
    lo, hi, alo, ahi = m64.bounds(c.L)
    s = alt[:, 1] + alt[:, 2]
    inside = ((alt > lo + margin) & (alt < hi - margin)).all(1) & (s > alo + margin) & (s < ahi - margin)
    use_alt = inside & (np.arange(len(src)) % 2 == 1)
    want = np.where(use_alt[:, None], alt, src)
    with np.errstate(invalid="ignore"):
        judged = (c.move == 0) & (np.abs(src[:, 2]) > 0.01) & (_h(src, c.leg) > 1.0) & (c.dn <= 2e-3)
    return want.astype(np.float32), want, judged, use_alt
