"""An independent float64 model of stance stability (tests/test_stance_float64_cpu.py, tests/test_gpu_stance_float64.py), written
from geometry: the centre of mass through the textbook rotation matrix of the pose's unit quaternion, the plane points as
float64 dot products with the caller's basis, the support polygon as the convex hull of the planted plane points by gift
wrapping under an exact orientation test (collinear points dropped), the margin as the smallest signed distance of the centre
of mass from the hull's directed counter-clockwise edges.  Nothing here is taken from the library, from stance_cases.brute_np
or from stance_cases.geometry(); the module checks its own hull and margin (check_model64) before anything is measured with it.

What the contract DEFINES is kept as defined: a foot is valid iff its index is in the cloud and q = float32(t - body[p]), one
subtraction per component, is finite; a stance is dead for live_in 0, a pose outside [0, nposes) or a centre of mass that is not
finite; fewer than three planted feet give -inf.  The quaternion, com and the plane basis are the float32 values the library
receives.  Everything after is float64.

Domain: quaternions normalised in float64 and rounded to float32 (is_unit).  A non-unit quaternion scales the centre of mass;
the bit-for-bit tests (tests/test_stance_cpu.py) cover those.

A degenerate hull (every planted foot coincident or on one line, exactly) is reported as a flag, its margin64 is nan: the
library then answers a margin <= band, never stable.  In a MIRRORED basis the planted feet keep their hull but the model still
measures from counter-clockwise edges of the projected coordinates, as the contract does, so the margin keeps its meaning.

The measured bands (measured by tests/test_stance_float64_cpu.py, asserted at four times the measured worst
rounded up to one digit) live here so that the CPU and the GPU tests share them."""
from fractions import Fraction

import numpy as np

F = np.float32
D = np.float64

# mm, |margin - margin64| / factor (see SEP) per kind of scene.  measured worst -> asserted (the CPU test prints the measured values on every run)
BAND = {
    "main": 3e-4,        # 5.11e-5: stance_cases.main_scene, six legs, every lift set
    "synthetic": 2e-4,   # 4.49e-5: stance_cases.synthetic with 3 to 8 legs, every plane, pose_idx and live_in form, invalid feet,
    #                      4000 stances under a yawed tilted basis
    "collinear": 3e-4,   # 5.75e-5: collinear_family (4.60e-5 with plane None, 5.75e-5 tilted, 4.28e-5 mirrored)
    "far": 2e-4,         # 2.53e-5: cloud and bodies 1e4 and 4e6 mm from the origin; the relative coordinates are the same
    "large": 2e-2,       # 3.21e-3: relative coordinates to 5e4 mm
    "hand_made": 1e-5,   # 2.37e-6: stance_cases.hand_made under every lift set
}
WITHIN = 2000.0  # mm: every scene but "large" keeps its relative coordinates below this
# Short edges.  The library's plane points are float32: each is off by some eps R (R the size of the relative coordinates), which
# turns an edge of length |e| by eps R / |e| and moves the signed distance of c by that angle times |c - a|.  The error of a
# margin therefore grows like 1 / |e| once two feet stand close together (measured: 7e-4 mm for two feet 2 mm apart under a tilted
# basis, against 5e-5 mm otherwise).  The band of a stance is BAND[kind] * max(1, SEP / sep), sep the least distance between two
# distinct valid plane points of the stance: the plain band wherever no two feet are closer than a foot is wide.
SEP = 30.0


def is_unit(quat):
    q = np.asarray(quat, D)
    return bool(np.isfinite(q).all() and abs(np.linalg.norm(q) - 1.0) <= 1e-6)


def rotation64(quat):
    """the rotation matrix of the unit quaternion (w, x, y, z): v -> q v q*"""
    w, x, y, z = np.asarray(quat, D) / np.linalg.norm(np.asarray(quat, D))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], D)


def gravity_basis(gravity, yaw=0.0, mirrored=False):
    """float64 [2, 3]: an orthonormal basis (u, v) of the plane normal to `gravity` (a robot on a slope: gravity not along -z of
    the caller's frame).  u is the caller's x axis taken into that plane (y where x is along gravity), turned by `yaw` about
    gravity; v = up x u with up = -gravity / |gravity|, so that (u, v, up) is right-handed and a polygon keeps its sense seen
    from above; mirrored swaps the handedness (v -> -v)."""
    up = -np.asarray(gravity, D)
    up = up / np.linalg.norm(up)
    x = np.array([1.0, 0, 0]) if abs(up[0]) < 0.9 else np.array([0, 1.0, 0])
    u = x - (x @ up) * up
    u /= np.linalg.norm(u)
    v = np.cross(up, u)
    u, v = np.cos(yaw) * u + np.sin(yaw) * v, np.cos(yaw) * v - np.sin(yaw) * u
    return np.stack([u, -v if mirrored else v])


# ---- the near-collinear family -------------------------------------------------------------------------------------------
PERTURB = (0.0, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)  # mm across the line, + outwards
OFFSETS = (1e-3, -1e-3, 1e-2, -1e-2, 0.1, -0.1, 1.0, -1.0, 10.0, -10.0, 40.0, -40.0)  # mm of c from the side, + inside
COLLINEAR_COM = np.array([40.0, -25.0, -30.0], F)


def collinear_family(ns, seed, nlegs=8):
    """(targets, foot int32[nlegs, ns], quats, body, info): per stance 3 to nlegs feet, the corners of a convex triangle or
    quadrilateral and the rest spread over one or two of its sides, at most three to a side and no two feet closer than SEP, so
    that two to five feet lie on one straight line of the world
    (the polygon's plane is tilted a little, its sides stay lines in 3-d and under every plane basis); each extra foot moved
    across its line by PERTURB[s % 9]; everything turned by a random yaw and rounded to float32, so collinearity survives only up
    to rounding; the legs in a random order, the missing ones -1; the body placed so that the centre of mass COLLINEAR_COM under
    the stance's random unit quaternion lies OFFSETS[s % 12] mm inside (+) or outside (-) of a side that holds extra feet.
    info: dict of side_feet (the most feet on one line), offset and perturb per stance."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((ns, 4))
    quats = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    targets = np.zeros((nlegs * ns, 3), F)
    foot = np.full((nlegs, ns), -1, np.int32)
    body = rng.uniform(-300.0, 300.0, (ns, 3)).astype(F)
    info = {"side_feet": np.zeros(ns, int), "offset": np.zeros(ns), "perturb": np.zeros(ns)}
    for s in range(ns):
        n = int(rng.integers(3, nlegs + 1))
        k = 3 if n < 5 or rng.random() < 0.5 else 4
        az = np.sort((np.arange(k) + rng.uniform(-0.25, 0.25, k)) * 2 * np.pi / k + rng.uniform(0, 2 * np.pi))
        corners = rng.uniform(200.0, 380.0) * np.stack([np.cos(az), np.sin(az)], 1)  # on a circle, counter-clockwise: convex
        sides = rng.permutation(k)[:max(int(rng.integers(1, 3)), -(-(n - k) // 3))]
        on_side = sides[np.arange(n - k) % len(sides)]
        pts = list(corners)
        delta, d_in = PERTURB[s % len(PERTURB)], OFFSETS[s % len(OFFSETS)]
        for x, side in enumerate(on_side):
            a, b = corners[side], corners[(side + 1) % k]
            e = (b - a) / np.linalg.norm(b - a)
            out = np.array([e[1], -e[0]])  # to the right of a counter-clockwise edge: outwards
            here, nth = int((on_side == side).sum()), int((on_side[:x] == side).sum())
            pts.append(a + (0.1 + 0.8 * (nth + 0.5 + rng.uniform(-0.1, 0.1)) / here) * (b - a) + delta * out)
        side = int(on_side[0]) if len(on_side) else int(rng.integers(0, k))
        a, b = corners[side], corners[(side + 1) % k]
        e = (b - a) / np.linalg.norm(b - a)
        w = a + rng.uniform(0.1, 0.9) * (b - a) - d_in * np.array([e[1], -e[0]])
        slope = rng.uniform(-0.1, 0.1, 2)
        local = np.array([[p[0] - w[0], p[1] - w[1], slope @ (np.asarray(p) - w)] for p in pts])
        yaw = rng.uniform(0, 2 * np.pi)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        rel = local @ Rz.T + rotation64(quats[s]) @ COLLINEAR_COM.astype(D)
        legs = rng.permutation(nlegs)[:n]
        targets[nlegs * s + legs] = (rel + body[s].astype(D)).astype(F)
        foot[legs, s] = nlegs * s + legs
        info["side_feet"][s] = 2 + (max(np.bincount(on_side)) if len(on_side) else 0)
        info["offset"][s], info["perturb"][s] = d_in, delta
    return targets, foot, quats, body, info


# ---- the hull ----------------------------------------------------------------------------------------------------------
def orient(a, b, p):
    """the sign of (b - a) x (p - a), exact: float64 where the result is past its own rounding error, rationals otherwise"""
    l, r = (b[0] - a[0]) * (p[1] - a[1]), (b[1] - a[1]) * (p[0] - a[0])
    det = l - r
    if abs(det) > 1e-14 * (abs(l) + abs(r)):
        return 1 if det > 0 else -1
    ax, ay, bx, by, px, py = (Fraction(float(v)) for v in (a[0], a[1], b[0], b[1], p[0], p[1]))
    det = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return (det > 0) - (det < 0)


def hull_gift_wrap(pts):
    """indices into pts of the counter-clockwise convex hull, by gift wrapping: from the lowest (then leftmost) point, the next
    vertex is the point no other point lies to the right of; of points in one direction the furthest, so collinear points are
    dropped.  Coincident points count once (the first index).  One vertex: all coincident; two: all on one line."""
    first = {}
    for k, p in enumerate(pts):
        first.setdefault((float(p[0]), float(p[1])), k)
    idx = list(first.values())
    P = [(float(pts[k][0]), float(pts[k][1])) for k in idx]
    n = len(P)
    if n == 1:
        return [idx[0]]
    start = min(range(n), key=lambda k: (P[k][1], P[k][0]))
    hull, cur = [start], start
    while True:
        nxt = (cur + 1) % n
        for r in range(n):
            if r == cur or r == nxt:
                continue
            o = orient(P[cur], P[nxt], P[r])
            if o < 0:
                nxt = r
            elif o == 0:
                dn = (P[nxt][0] - P[cur][0]) ** 2 + (P[nxt][1] - P[cur][1]) ** 2
                dr = (P[r][0] - P[cur][0]) ** 2 + (P[r][1] - P[cur][1]) ** 2
                if dr > dn:
                    nxt = r
        if nxt == start:
            break
        hull.append(nxt)
        cur = nxt
        assert len(hull) <= n, "gift wrapping does not close"
    return [idx[k] for k in hull]


def signed_dist(a, b, c):
    """signed distance of c from the directed line a -> b, positive to its left"""
    ex, ey = b[0] - a[0], b[1] - a[1]
    return (ex * (c[1] - a[1]) - ey * (c[0] - a[0])) / np.hypot(ex, ey)


def margin_of_hull(poly, c):
    return min(signed_dist(poly[k], poly[(k + 1) % len(poly)], c) for k in range(len(poly)))


# ---- the model ---------------------------------------------------------------------------------------------------------
def stance64(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, live_in=None):
    """-> dict: margin64 float64 [nmasks, ns] (-inf: dead or fewer than three planted feet; nan: a degenerate hull), degenerate
    bool [nmasks, ns], hull [nmasks][ns] tuples of leg indices counter-clockwise (of coincident feet the lowest leg), planted
    uint8 [nmasks, ns], feet uint8 [ns], dead bool [ns], pts float64 [ns, nlegs, 2] (nan where not valid), c float64 [ns, 2],
    size float64 [ns] the largest |coordinate| of a stance's plane points and centre of mass, factor float64 [ns] what the
    stance's band is multiplied by (short_edge_factor), lift uint8 [nmasks]"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    foot = np.ascontiguousarray(foot, np.int32)
    nl, ns = foot.shape
    nt, nposes = len(targets), len(quats)
    lift = np.zeros(1, np.uint8) if lift is None else np.asarray(lift, np.uint8)
    nm = len(lift)
    body = None if body is None else np.ascontiguousarray(body, F).reshape(-1, 3)
    cm = np.zeros(3, D) if com is None else np.asarray(com, F).reshape(3).astype(D)
    basis = np.array([[1.0, 0, 0], [0, 1.0, 0]]) if plane is None else np.asarray(plane, F).reshape(2, 3).astype(D)
    pose = np.arange(ns) if pose_idx is None else np.asarray(pose_idx, np.int64)

    dead = np.zeros(ns, bool)
    c = np.zeros((ns, 2), D)
    pts = np.full((ns, nl, 2), np.nan, D)
    feet = np.zeros(ns, np.uint8)
    rot = {}
    for s in range(ns):
        p = int(pose[s])
        if (live_in is not None and live_in[s] == 0) or p < 0 or p >= nposes:
            dead[s] = True
            continue
        if cm.any():
            if not np.isfinite(quats[p]).all():
                dead[s] = True  # the centre of mass is not finite
                continue
            if p not in rot:
                assert is_unit(quats[p]), "outside the model's domain: not a unit quaternion"
                rot[p] = basis @ (rotation64(quats[p]) @ cm)
            c[s] = rot[p]
        b = np.zeros(3, F) if body is None else body[p]
        for l in range(nl):
            ft = int(foot[l, s])
            if ft < 0 or ft >= nt:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                q = (targets[ft] - b).astype(F)
            if not np.isfinite(q).all():
                continue
            pts[s, l] = basis @ q.astype(D)
            feet[s] |= np.uint8(1 << l)

    margin = np.full((nm, ns), -np.inf, D)
    degenerate = np.zeros((nm, ns), bool)
    planted = np.zeros((nm, ns), np.uint8)
    hulls = [[() for _ in range(ns)] for _ in range(nm)]
    for s in range(ns):
        cache = {}  # planted set -> (hull, margin)
        for m in range(nm):
            S = int(feet[s]) & ~int(lift[m]) & 0xff
            planted[m, s] = S
            if bin(S).count("1") < 3:
                continue
            if S not in cache:
                legs = [l for l in range(nl) if (S >> l) & 1]
                h = tuple(legs[k] for k in hull_gift_wrap([pts[s, l] for l in legs]))
                cache[S] = (h, margin_of_hull([pts[s, l] for l in h], c[s]) if len(h) >= 3 else np.nan)
            hulls[m][s], margin[m, s] = cache[S]
            degenerate[m, s] = len(hulls[m][s]) < 3
    with np.errstate(invalid="ignore"):
        size = np.nan_to_num(np.nanmax(np.abs(np.concatenate([pts.reshape(ns, -1), c], 1)), axis=1))
    return {"margin64": margin, "degenerate": degenerate, "hull": hulls, "planted": planted, "feet": feet, "dead": dead, "pts": pts,
            "c": c, "size": size, "factor": short_edge_factor(pts), "lift": lift}


def short_edge_factor(pts):
    """pts float64 [ns, nlegs, 2] (nan where not valid) -> float64 [ns]: max(1, SEP / sep), see SEP"""
    with np.errstate(invalid="ignore"):
        d = np.linalg.norm(pts[:, :, None, :] - pts[:, None, :, :], axis=-1)
        d[~(d > 0)] = np.inf  # a foot and itself, coincident feet, invalid feet
    return np.maximum(1.0, SEP / d.min((1, 2)))


# ---- the model checks itself ---------------------------------------------------------------------------------------------
def crossing_number_inside(poly, p):
    """is p inside the polygon: the parity of the polygon's crossings of the ray from p towards +x"""
    inside = False
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
        if (y0 > p[1]) != (y1 > p[1]) and p[0] < x0 + (p[1] - y0) * (x1 - x0) / (y1 - y0):
            inside = not inside
    return inside


def point_segment_dist(p, a, b):
    a, b, p = (np.asarray(v, D) for v in (a, b, p))
    e = b - a
    t = np.clip(((p - a) @ e) / (e @ e), 0.0, 1.0)
    return float(np.linalg.norm(p - (a + t * e)))


def check_model64(model, samples=64, every=1):
    """the model's own hull and margin, on every `every`-th (stance, lift set) answer with a proper hull:
    c inside (margin64 > 0): margin64 is the Euclidean distance to the boundary -- against the minimum over samples + 1 points per
      edge, d <= sampled <= sqrt(d^2 + (L / 2 samples)^2) with L the nearest edge's length -- and the disc about c of radius
      0.999999 margin64 passes a crossing-number point-in-polygon test in 360 directions;
    c outside: -dist(c, polygon) <= margin64 < 0, and the crossing number says outside;
    the hull against stance_cases._hull64 (monotone chain) as a set of vertices, a vertex of only one of them within 1e-9 mm of
      the other's boundary (the chain's orientation test is plain float64).
    -> (inside, outside) counts"""
    import stance_cases
    nm, ns = model["margin64"].shape
    par = np.linspace(0.0, 1.0, samples + 1)[:, None]
    ang = np.deg2rad(np.arange(360))
    ring = np.stack([np.cos(ang), np.sin(ang)], 1)
    n_in = n_out = 0
    seen = set()
    at = 0
    for m in range(nm):
        for s in range(ns):
            h = model["hull"][m][s]
            if len(h) < 3 or (s, h) in seen:
                continue
            at += 1
            if at % every:
                continue
            seen.add((s, h))
            poly = [tuple(model["pts"][s, l]) for l in h]
            c, d = model["c"][s], model["margin64"][m, s]
            tiny = 1e-12 * (1.0 + model["size"][s])
            S = int(model["planted"][m, s])
            allp = [tuple(model["pts"][s, l]) for l in range(8) if (S >> l) & 1]
            other = stance_cases._hull64(allp)
            for only, against in ((set(poly) - set(other), other), (set(other) - set(poly), poly)):
                for v in only:
                    assert min(point_segment_dist(v, against[k], against[(k + 1) % len(against)]) for k in range(len(against))) <= 1e-9, (s, h)
            area2 = sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1] for k in range(len(poly)))
            assert area2 > 0, "the hull is not counter-clockwise"
            for p in allp:  # every planted foot inside or on the hull
                assert margin_of_hull(poly, p) >= -tiny
            if d > tiny:
                n_in += 1
                A = np.array(poly)
                B = np.roll(A, -1, 0)
                per_edge = [np.linalg.norm(a + par * (b - a) - c, axis=1).min() for a, b in zip(A, B)]
                lines = [signed_dist(a, b, c) for a, b in zip(A, B)]
                L = np.linalg.norm(B[int(np.argmin(lines))] - A[int(np.argmin(lines))])
                assert d - tiny <= min(per_edge) <= np.sqrt(d * d + (L / (2 * samples)) ** 2) + tiny, (s, h, d, min(per_edge))
                assert all(crossing_number_inside(poly, c + 0.999999 * d * r) for r in ring), (s, h)
            elif d < -tiny:
                n_out += 1
                dist = min(point_segment_dist(c, poly[k], poly[(k + 1) % len(poly)]) for k in range(len(poly)))
                assert -dist - tiny <= d < 0, (s, h, d, dist)
                assert not crossing_number_inside(poly, c), (s, h)
    return n_in, n_out


# ---- the library's rows against the model ----------------------------------------------------------------------------------
def doubt(model, band, min_margin):
    """bool [nmasks, ns]: a proper hull whose margin64 lies within the stance's band of min_margin: stable is not compared there"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(model["margin64"]) & (np.abs(model["margin64"] - min_margin) <= band * model["factor"][None, :])


def check_stance_rows(got, model, band, min_margin, exact_ties=False, measure=None):
    """the library's rows (dict of margin, edge, stable [nmasks, ns], feet [ns]; edge and feet may be None) against the model:
    feet exactly; a dead stance -inf / 255 / 0; -inf exactly wherever the model has fewer than three planted feet; on a degenerate
    hull a margin <= band (or -inf), never stable; elsewhere |margin - margin64| <= band, stable = margin64 > min_margin wherever
    |margin64 - min_margin| > band; the edge decodes to i != j, both planted, the float64 signed distance of c from the line
    f_i -> f_j is within 2 band of margin64 and every planted foot lies to its left to within band.  Ties: of the ordered pairs
    whose ends coincide with the winning edge's ends (shared targets: the same arithmetic) the smallest code wins; with
    exact_ties (hand-made stances, whose float64 quotients are exact) of every hull-line pair whose float64 distance equals
    margin64.  band: the kind's (BAND); a stance's band is band * model["factor"].  measure: a dict that receives the worst
    (margin - margin64) / factor below and above.
    -> (answers compared, answers skipped for doubt)"""
    m64, deg = model["margin64"], model["degenerate"]
    nm, ns = m64.shape
    base, band = float(band), float(band) * model["factor"]
    margin = np.asarray(got["margin"]).reshape(nm, ns)
    stable = np.asarray(got["stable"]).reshape(nm, ns)
    edge = None if got.get("edge") is None else np.asarray(got["edge"]).reshape(nm, ns)
    if got.get("feet") is not None:
        assert np.array_equal(np.asarray(got["feet"]).reshape(-1), model["feet"])
    assert not np.isnan(margin).any()
    dead = model["dead"]
    assert np.isneginf(margin[:, dead]).all() and (stable[:, dead] == 0).all() and (model["feet"][dead] == 0).all()
    few = np.isneginf(m64)
    assert np.isneginf(margin[few]).all() and (stable[few] == 0).all()
    assert (margin[deg] <= np.broadcast_to(band, (nm, ns))[deg]).all() and (stable[deg] == 0).all()
    proper = ~few & ~deg
    diff = margin.astype(D) - np.where(proper, m64, 0.0)
    if measure is not None and proper.any():
        scaled = (diff / model["factor"][None, :])[proper]
        measure["below"] = max(measure.get("below", 0.0), float(-scaled.min()))
        measure["above"] = max(measure.get("above", 0.0), float(scaled.max()))
        measure["answers"] = int(proper.sum())
    bad = proper & ~(np.abs(diff) <= band[None, :])
    assert not bad.any(), ("margin outside the band", [(int(m), int(s), float(margin[m, s]), float(m64[m, s])) for m, s in np.argwhere(bad)[:5]])
    skip = doubt(model, base, min_margin)
    sure = proper & ~skip
    assert np.array_equal(stable[sure], (m64 > min_margin)[sure].astype(np.uint8))
    assert np.array_equal(stable.astype(bool), margin > F(min_margin))
    if edge is not None:
        assert (edge[np.isneginf(margin)] == 255).all() and (edge[~np.isneginf(margin)] < 64).all()
        done = set()  # (stance, planted set, code): lift sets that leave the same feet planted share their answer
        for m, s in np.argwhere(proper):
            i, j = int(edge[m, s]) >> 3, int(edge[m, s]) & 7
            S = int(model["planted"][m, s])
            if (s, S, int(edge[m, s])) in done:
                continue
            done.add((s, S, int(edge[m, s])))
            assert i != j and (S >> i) & 1 and (S >> j) & 1, (m, s, i, j)
            P, c, b = model["pts"][s], model["c"][s], band[s]
            assert tuple(P[i]) != tuple(P[j]), (m, s, i, j)
            assert abs(signed_dist(P[i], P[j], c) - m64[m, s]) <= 2 * b, (m, s, i, j, signed_dist(P[i], P[j], c), m64[m, s])
            legs = [l for l in range(P.shape[0]) if (S >> l) & 1]
            assert all(signed_dist(P[i], P[j], P[k]) >= -b for k in legs), (m, s, i, j)
            tied = [a * 8 + e for a in legs for e in legs if tuple(P[a]) == tuple(P[i]) and tuple(P[e]) == tuple(P[j])]
            if exact_ties:
                tied += [a * 8 + e for a in legs for e in legs if tuple(P[a]) != tuple(P[e]) and signed_dist(P[a], P[e], c) == m64[m, s]
                         and all(orient(P[a], P[e], P[k]) >= 0 for k in legs)]
            assert int(edge[m, s]) == min(tied), (m, s, int(edge[m, s]), sorted(tied))
    return int(sure.sum()), int((proper & skip).sum())


# ---- properties of the library alone: no model, so they run at any scale -------------------------------------------------
def check_properties(run, targets, foot, body, band, basis, basis_yawed, seed=0):
    """run(foot, plane, lift) -> dict(margin, edge, stable, feet) of the library, host or device, on one scene (plane None and
    the two bases given, which differ by a yaw about gravity).  Asserted, all vectorised:
    1. the yaw of the basis changes a margin by <= 2 band (one of the two -inf: the other <= band, a degenerate polygon);
    2. relabelling the legs keeps every margin's bits and maps the edge codes, but for ties between pairs on one line;
    3. lifting a leg whose foot lies strictly inside a triangle of three other valid feet -- no hull vertex -- changes the
       margin of the stance with every valid foot planted by <= 2 band;
    4. lifting one more leg never raises a margin >= 0 by more than 2 band (the polygon only shrinks round a centre of mass
       inside it; the library's own margin stands for the model's, which is within band of it).
    -> the number of (stance, leg) entries of property 3"""
    foot = np.ascontiguousarray(foot, np.int32)
    nl, ns = foot.shape
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore", over="ignore"):
        bd = np.zeros((ns, 3), F) if body is None else np.asarray(body, F).reshape(-1, 3)[:ns]
        inb = (foot >= 0) & (foot < len(targets))
        q = (np.asarray(targets, F).reshape(-1, 3)[np.where(inb, foot, 0)] - bd[None]).astype(F)
        q = np.where((inb & np.isfinite(q).all(-1))[..., None], q.astype(D), np.nan)  # [nl, ns, 3]
    # the stance's band under each of the three bases (short_edge_factor): plane None, basis, basis_yawed
    planes = [np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.asarray(basis, F).astype(D), np.asarray(basis_yawed, F).astype(D)]
    band = band * np.max([short_edge_factor(np.moveaxis(q @ b.T, 0, 1)) for b in planes], axis=0)
    every = np.arange(1 << nl).astype(np.uint8)
    each = np.array([0] + [1 << l for l in range(nl)], np.uint8)
    base = run(foot, None, every)
    margin = base["margin"].astype(D)

    a, b = run(foot, basis, each)["margin"].astype(D), run(foot, basis_yawed, each)["margin"].astype(D)
    both = np.isfinite(a) & np.isfinite(b)
    a, b = np.where(both, a, np.where(np.isfinite(a), a, 0.0)), np.where(both, b, np.where(np.isfinite(b), b, 0.0))  # -inf out of the way
    wide = np.broadcast_to(band, a.shape)
    assert both.any() and (np.abs(a - b)[both] <= 2 * wide[both]).all(), float((np.abs(a - b)[both] / wide[both]).max())
    one = ~both & ((a != 0) | (b != 0))  # one of the two -inf
    assert (np.where(a != 0, a, b)[one] <= wide[one]).all()

    ok = ~np.isnan(q[..., 0]) & (base["feet"][None, :] != 0)
    P = np.where(ok[..., None], q[..., :2], np.nan)  # [nl, ns, 2], plane None
    assert np.array_equal(sum((ok[l].astype(np.uint8) << l) for l in range(nl)).astype(np.uint8), base["feet"])

    perm = rng.permutation(nl)
    foot2 = np.empty_like(foot)
    foot2[perm] = foot
    lift2 = np.array([sum(((int(m) >> l) & 1) << int(perm[l]) for l in range(nl)) for m in every], np.uint8)
    re = run(foot2, None, lift2)
    assert np.array_equal(re["margin"].view(np.uint32), base["margin"].view(np.uint32))
    e = base["edge"].astype(int)
    mapped = np.where(e == 255, 255, perm[np.minimum(e >> 3, nl - 1)] * 8 + perm[np.minimum(e & 7, nl - 1)])
    cross = lambda o, p, r: (p[0] - o[0]) * (r[1] - o[1]) - (p[1] - o[1]) * (r[0] - o[0])
    inv = np.argsort(perm)
    for m, s in np.argwhere(mapped != re["edge"]):  # a tie: both pairs on one line, exactly
        i, j = e[m, s] >> 3, e[m, s] & 7
        i2, j2 = inv[int(re["edge"][m, s]) >> 3], inv[int(re["edge"][m, s]) & 7]
        assert cross(P[i, s], P[j, s], P[i2, s]) == 0 and cross(P[i, s], P[j, s], P[j2, s]) == 0, (m, s)

    entries = 0
    for k in range(nl):
        inside = np.zeros(ns, bool)
        others = [l for l in range(nl) if l != k]
        for x in range(len(others)):
            for y in range(x + 1, len(others)):
                for z in range(y + 1, len(others)):
                    A, B, C_ = P[others[x]], P[others[y]], P[others[z]]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        area = cross(A.T, B.T, C_.T)
                        w = np.stack([cross(B.T, C_.T, P[k].T), cross(C_.T, A.T, P[k].T), cross(A.T, B.T, P[k].T)]) / area
                        inside |= (np.abs(area) > 1.0) & (w > 1e-3).all(0)  # nan compares false: an invalid foot is in no triangle
        if inside.any():
            with np.errstate(invalid="ignore"):
                d = np.nan_to_num(np.abs(margin[0, inside] - margin[1 << k, inside]))
            assert np.array_equal(np.isfinite(margin[0, inside]), np.isfinite(margin[1 << k, inside])) and (d <= 2 * band[inside]).all(), (k, float(d.max()))
        entries += int(inside.sum())
    assert entries > 0

    for m in range(1 << nl):
        for l in range(nl):
            if not (m >> l) & 1:
                inside = margin[m] >= 0
                assert (margin[m | (1 << l), inside] <= margin[m, inside] + 2 * band[inside]).all(), (m, l)
    return entries
