"""Clouds built on the plane table's own lattice and seams.  numpy only, no library call when a cloud is built (ik_cases gives the
orientation matrix, shell_cases the legs); shared by tests/test_lattice_cpu.py, tests/test_gpu_lattice.py and tools/stress_tol.py.

The table-guided kernels (LRM_MODE_TOL_REL, LRM_MODE_TOL, the table-guided LRM_MODE_FAST) answer a point by finding the cells of its
candidate plane points (csrc/lrm_point_tol.h: lrm_toltab_lookup2).  A plane point is (abscissa - coxa_length, z) in the coxa frame,
its abscissa one of {r, -r, uM, um}: the point's own meridian plane, the opposite one, the max / min yaw-limit plane.  The cell
index is one FMA and a truncation of each coordinate; the coordinates carry a few 1e-5 mm of rounding, and the builder
(csrc/lrm_toltab_build.h: lrm_tb_slack) widens every cell by 1.6e-5 H + 1e-3 mm to cover it.  A uniform cloud puts one point in 1e5
that close to a cell edge with the neighbour answering differently.  The families here put nearly all of theirs there: on the
1 mm / 16 mm / 32 mm lines of the inner grid, the 8 mm / 128 mm lines of the outer one, the seam between the two grids
(max(r + coxa_length, |z|) = far_limit), the end of the outer grid and beyond it.

Everything is chosen in the coxa frame in float64 -- cylindrical (r, phi, z) -- and mapped to the caller's frame by the chain of
shell_cases.coxa_axis_cloud (coxa pitch, body offset, azimuth, body orientation), with ik_cases.back_matrix for the orientation:
the exact inverse of the reference's frame change also for the fixture orientations, which are not unit quaternions.  Frame.to_coxa
is the same chain backwards; it only serves to CHECK the aim on the float32-rounded points, from this model alone.

The lattice constants are read from csrc/lrm_types.h, so a changed constant moves the clouds (and test_constants_match_the_sources
fails loudly)."""
import os
import re

import numpy as np

from ik_cases import back_matrix
import shell_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged-robot-movability-cuda_amd", "csrc")

INNER_FAMILIES = ("sub_edges", "coarse_edges", "flip_edges", "limit_edges")
FAMILIES = INNER_FAMILIES + ("far_seam", "outer_edges", "grid_end", "beyond")
ALL_FAR = ("outer_edges", "grid_end", "beyond")   # every point of these lies on the outer grid
LANE_ORDERS = ("blocks", "one_far_lane", "one_near_lane", "shuffled")
FAR_LANES = (0, 31, 32, 63)
# the legs of shell_cases with the widest (149 degrees) and the narrowest (81 degrees) yaw range; tests/test_lattice_cpu.py checks that they are
WIDEST_YAW_LEG, NARROWEST_YAW_LEG = "rnd_0", "rnd_4"

# what a point's aimed coordinate is (column `kind` of an aim record)
NONE, X_OWN, X_FLIP, X_MAX, X_MIN, Z, FAR_R, FAR_Z = range(8)

# windows of the aim conditions (mm): below lrm_tb_slack of the grid they belong to
AIM_INNER = 3.0e-4
AIM_OUTER = 1.2e-3
MIN_AIMED = 0.9
MIN_EACH_SIDE = 0.3


def constants():
    """dict(N, SUB, NB, H_INNER, H_OUTER, FAR_LIMIT) as csrc/lrm_types.h defines them; the far limit as lrm_toltab.cpp and
    lrm_toltab_dev.hip set it: 0.5 N H_INNER - 1"""
    src = open(os.path.join(CSRC, "lrm_types.h")).read()

    def grab(name, pattern):
        m = re.search(r"#define %s\s+%s" % (name, pattern), src)
        assert m, name
        return m.group(1)
    c = dict(N=int(grab("LRM_TT_N", r"(\d+)\b")), SUB=int(grab("LRM_TT_SUB", r"(\d+)\b")), NB=int(grab("LRM_TT_NB", r"(\d+)\b")),
             H_INNER=float(grab("LRM_TT_H_INNER", r"([0-9.eE+-]+)f")), H_OUTER=float(grab("LRM_TT_H_OUTER", r"([0-9.eE+-]+)f")))
    c["FAR_LIMIT"] = 0.5 * c["N"] * c["H_INNER"] - 1.0
    return c


def slack(H):
    """lrm_tb_slack (csrc/lrm_toltab_build.h): the margin the builder puts around every cell of a grid with coarse cells of H mm"""
    return 1.6e-5 * H + 1.0e-3


class Frame:
    """the float64 maps between the coxa frame and the caller's frame of (leg, quat), and the table's coordinates of a point.
    yaw = (min, max) yaw limits (rad), as ik_cases.limits(oracle, leg, quat)["coxa"] gives them"""

    def __init__(self, leg, quat, yaw):
        leg = np.asarray(leg, np.float64).reshape(-1)
        self.body_angle, self.body, self.pitch, self.coxa = (float(leg[k]) for k in range(4))
        self.arm = float(leg[4] + leg[5])  # tibia + femur: the workspace lies within this of the femur joint
        self.yaw_min, self.yaw_max = float(yaw[0]), float(yaw[1])
        self.back = back_matrix(sc.IDENTITY if quat is None else quat)
        self.fwd = np.linalg.inv(self.back)
        self.k = constants()

    def from_coxa(self, c):
        """coxa-frame points (float64 [n, 3]) in the caller's frame, float64"""
        c = np.asarray(c, np.float64).reshape(-1, 3)
        cp, sp = np.cos(self.pitch), np.sin(self.pitch)
        x, y, z = c[:, 0] * cp - c[:, 2] * sp + self.body, c[:, 1], c[:, 0] * sp + c[:, 2] * cp
        cb, sb = np.cos(self.body_angle), np.sin(self.body_angle)
        return np.column_stack([x * cb - y * sb, x * sb + y * cb, z]) @ self.back.T

    def to_coxa(self, points32):
        """float32 points of the caller's frame in the coxa frame, float64: from_coxa backwards"""
        v = np.asarray(points32, np.float32).reshape(-1, 3).astype(np.float64) @ self.fwd.T
        cb, sb = np.cos(self.body_angle), np.sin(self.body_angle)
        x, y, z = v[:, 0] * cb + v[:, 1] * sb - self.body, -v[:, 0] * sb + v[:, 1] * cb, v[:, 2]
        cp, sp = np.cos(self.pitch), np.sin(self.pitch)
        return np.column_stack([x * cp + z * sp, y, -x * sp + z * cp])

    def cyl(self, r, phi, z):
        """(r, phi, z) of the coxa frame as float32 points of the caller's frame"""
        return self.from_coxa(np.column_stack([r * np.cos(phi), r * np.sin(phi), z])).astype(np.float32)

    def coords(self, points32):
        """the table's coordinates of float32 points, from the float64 model: dict(r, phi, z, the four abscissae - coxa_length
        indexed by X_OWN .. X_MIN, far)"""
        c = self.to_coxa(points32)
        r, phi = np.hypot(c[:, 0], c[:, 1]), np.arctan2(c[:, 1], c[:, 0])
        out = {"r": r, "phi": phi, "z": c[:, 2], X_OWN: r - self.coxa, X_FLIP: -r - self.coxa,
               X_MAX: r * np.cos(phi - self.yaw_max) - self.coxa, X_MIN: r * np.cos(phi - self.yaw_min) - self.coxa}
        out["far"] = ~(np.maximum(r + self.coxa, np.abs(c[:, 2])) < self.k["FAR_LIMIT"])
        return out

    def aimed(self, points32, kind):
        """the coordinate each point aims with (float64 [n]; nan where kind is NONE), of the float32-rounded points"""
        co = self.coords(points32)
        vals = {NONE: np.full(len(co["r"]), np.nan), Z: co["z"], FAR_R: co["r"] + self.coxa, FAR_Z: np.abs(co["z"])}
        vals.update({k: co[k] for k in (X_OWN, X_FLIP, X_MAX, X_MIN)})
        kind = np.asarray(kind)
        return np.select([kind == k for k in range(8)], [vals[k] for k in range(8)])


# ---- offsets ---------------------------------------------------------------------------------------------------------------
def offsets_inner(h):
    return np.array([0.0, 1e-6, -1e-6, 2.0 ** -17 * h, -2.0 ** -17 * h, 1e-4, -1e-4])


OFFSETS_SEAM = np.array([0.0, 6e-5, -6e-5, 2e-4, -2e-4])
OFFSETS_OUTER = np.array([0.0, 5e-4, -5e-4, 2.0 ** -17 * 8, -2.0 ** -17 * 8, 2e-3, -2e-3])
OFFSETS_END = np.array([0.0, 5e-4, -5e-4, 2e-3, -2e-3, 1e-2, -1e-2])
WIDE_SHARE = 0.06  # of a family's offsets, those beyond its aim window together (the condition asks for 0.9 inside the window)


def draw(rng, offsets, n, window=None):
    """n offsets; with a window, the offsets beyond it are drawn WIDE_SHARE of the time (all of them equally), the others equally"""
    offsets = np.asarray(offsets, np.float64)
    if window is None or (np.abs(offsets) <= window).all():
        return rng.choice(offsets, n)
    wide = np.abs(offsets) > window
    p = np.where(wide, WIDE_SHARE / wide.sum(), (1.0 - WIDE_SHARE) / (~wide).sum())
    return rng.choice(offsets, n, p=p)


def phis(rng, n):
    return rng.uniform(-3.1, 3.1, n)


def ints(rng, lo, hi, n):
    """n integers of [lo, hi] (scalars or per-point arrays), as float64"""
    return np.floor(rng.uniform(np.ceil(lo), np.floor(hi) + 1.0, n))


# ---- families: each -> (float32 [n, 3], aim record) ----------------------------------------------------------------------
# An aim record is dict(kind int [n, 2], line float64 [n, 2]): up to two aimed coordinates per point (a cell corner has two),
# each with the line it aims at; kind NONE and line nan where there is none.
def _record(n):
    return dict(kind=np.zeros((n, 2), np.int64), line=np.full((n, 2), np.nan))


def _set(rec, col, sel, kind, line):
    rec["kind"][sel, col] = kind
    rec["line"][sel, col] = line


def _grid_edges(f, n, rng, h, span, x_free_hi, z_free, offsets, window=None, flip_share=0.0, near_share=0.0):
    """a third of the points with the abscissa on a line k h, a third with z on one, a third with both; line positions within
    +-span.  The abscissa is the point's own (r - coxa_length), or, for flip_share of the points, the flipped candidate's
    (-r - coxa_length); the coordinate that is not aimed is uniform (r - coxa_length up to x_free_hi, |z| up to z_free).
    near_share of the points keep both coordinates within tibia + femur of the femur joint, where the workspace is, half of them
    with a yaw inside the leg's range: the valid side of the table is exercised as well."""
    rec = _record(n)
    third = np.arange(n) % 3
    on_x, on_z = third != 1, third != 0
    flip = rng.random(n) < flip_share
    near = rng.random(n) < near_share
    span, x_free_hi, z_free = (np.where(near, np.minimum(f.arm, v), v) for v in (span, x_free_hi, z_free))
    # r - coxa_length = k h + d (own), r + coxa_length = k h - d (flip: -r - coxa_length = -k h + d): r > 0 either way
    k_own = ints(rng, (1.0 - f.coxa) / h, span / h, n)
    k_flip = ints(rng, (1.0 + f.coxa) / h, span / h, n)
    d = draw(rng, offsets, n, window)
    r = np.where(flip, k_flip * h - d - f.coxa, k_own * h + d + f.coxa)
    r = np.where(on_x, r, rng.uniform(1.0, x_free_hi + f.coxa, n))
    zline = ints(rng, -span / h, span / h, n) * h
    z = np.where(on_z, zline + draw(rng, offsets, n, window), rng.uniform(-z_free, z_free, n))
    _set(rec, 0, on_x & ~flip, X_OWN, (k_own * h)[on_x & ~flip])
    _set(rec, 0, on_x & flip, X_FLIP, (-k_flip * h)[on_x & flip])
    _set(rec, 1, on_z, Z, zline[on_z])
    # phi uniform in +-3.1 rad: every yaw sector and both candidate orders occur; half of the near points inside the yaw range
    phi = np.where(near & (rng.random(n) < 0.5), rng.uniform(f.yaw_min, f.yaw_max, n), phis(rng, n))
    return f.cyl(r, phi, z), rec


def sub_edges(f, n, rng):
    """inner grid, the 1 mm sub-cell lines within +-500 mm: abscissa on a line, z on a line, both (cell corners)"""
    h = f.k["H_INNER"] / f.k["SUB"]
    return _grid_edges(f, n, rng, h, 500.0, 500.0, 500.0, offsets_inner(h), near_share=0.5)


def coarse_edges(f, n, rng):
    """the 16 mm coarse lines over +-1008 mm (every other one a 32 mm bound-cell line); half of the aimed abscissae are the
    flipped candidate's, so that the lines left of -coxa_length carry points as well"""
    h = f.k["H_INNER"]
    span = h * (f.k["N"] // 2 - 1)
    return _grid_edges(f, n, rng, h, span, 900.0, 1000.0, offsets_inner(h), flip_share=0.5)


def flip_edges(f, n, rng):
    """the flipped candidate's abscissa on the 1 mm lines: -r - coxa_length = k h, within -500 mm"""
    h = f.k["H_INNER"] / f.k["SUB"]
    return _grid_edges(f, n, rng, h, 500.0, 500.0, 500.0, offsets_inner(h), flip_share=1.0, near_share=0.5)


def limit_edges(f, n, rng):
    """points outside the yaw range, within pi / 2 of a limit, whose abscissa in that limit's plane sits on a 1 mm line:
    uM - coxa_length = k h with wM beyond the limit, and the same for um; a third also with z on a line"""
    h = f.k["H_INNER"] / f.k["SUB"]
    rec = _record(n)
    use_max = rng.random(n) < 0.5
    k = ints(rng, (1.0 - f.coxa) / h, 500.0 / h, n)
    u = k * h + draw(rng, offsets_inner(h), n) + f.coxa
    # beyond the limit by delta: the candidate is clamped to the limit; r = u / cos(delta) stays on the inner grid
    dmax = np.minimum(1.45, np.arccos(np.clip(u / (f.k["FAR_LIMIT"] - f.coxa - 2.0), 0.0, 1.0)))
    delta = 0.02 + rng.random(n) * (dmax - 0.02)
    phi = np.where(use_max, f.yaw_max + delta, f.yaw_min - delta)
    r = u / np.cos(delta)
    on_z = np.arange(n) % 3 == 0
    zline = ints(rng, -500.0 / h, 500.0 / h, n) * h
    z = np.where(on_z, zline + draw(rng, offsets_inner(h), n), rng.uniform(-500.0, 500.0, n))
    _set(rec, 0, use_max, X_MAX, (k * h)[use_max])
    _set(rec, 0, ~use_max, X_MIN, (k * h)[~use_max])
    _set(rec, 1, on_z, Z, zline[on_z])
    return f.cyl(r, phi, z), rec


def far_seam(f, n, rng):
    """the seam between the grids: half with r + coxa_length = far_limit + d and |z| uniform below it, half with
    |z| = far_limit + d and r + coxa_length uniform below it"""
    lim = f.k["FAR_LIMIT"]
    rec = _record(n)
    on_r = np.arange(n) % 2 == 0
    d = draw(rng, OFFSETS_SEAM, n)
    r = np.where(on_r, lim + d - f.coxa, rng.uniform(1.0, lim - f.coxa - 1.0, n))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    z = np.where(on_r, rng.uniform(-(lim - 1.0), lim - 1.0, n), sign * (lim + d))
    _set(rec, 0, on_r, FAR_R, lim)
    _set(rec, 0, ~on_r, FAR_Z, lim)
    return f.cyl(r, phis(rng, n), z), rec


def outer_edges(f, n, rng):
    """outer grid: the 8 mm sub-cell lines and (half of the aimed coordinates) the 128 mm coarse lines over +-8100 mm, points with
    max(r + coxa_length, |z|) >= far_limit only; a quarter of the aimed abscissae are the flipped candidate's"""
    H, lim = f.k["H_OUTER"], f.k["FAR_LIMIT"]
    hs = H / f.k["SUB"]
    parts, recs, have = [], [], 0
    while have < n:
        m = n
        h = np.where(rng.random(m) < 0.5, H, hs)
        # _grid_edges with a per-point spacing: lines k h within +-8100 mm
        rec = _record(m)
        third = np.arange(m) % 3
        on_x, on_z = third != 1, third != 0
        flip = rng.random(m) < 0.25
        k_own = ints(rng, (1.0 - f.coxa) / h, 8100.0 / h, m)
        k_flip = ints(rng, (1.0 + f.coxa) / h, 8100.0 / h, m)
        d = draw(rng, OFFSETS_OUTER, m, AIM_OUTER)
        r = np.where(flip, k_flip * h - d - f.coxa, k_own * h + d + f.coxa)
        r = np.where(on_x, r, rng.uniform(1.0, 8100.0, m))
        zline = ints(rng, -np.floor(8100.0 / h), 8100.0 / h, m) * h
        z = np.where(on_z, zline + draw(rng, OFFSETS_OUTER, m, AIM_OUTER), rng.uniform(-8100.0, 8100.0, m))
        _set(rec, 0, on_x & ~flip, X_OWN, (k_own * h)[on_x & ~flip])
        _set(rec, 0, on_x & flip, X_FLIP, (-k_flip * h)[on_x & flip])
        _set(rec, 1, on_z, Z, zline[on_z])
        keep = np.maximum(r + f.coxa, np.abs(z)) >= lim + 1.0  # (a millimetre clear of the seam: far for the kernel too)
        parts.append(f.cyl(r[keep], phis(rng, int(keep.sum())), z[keep]))
        recs.append({a: rec[a][keep] for a in rec})
        have += int(keep.sum())
    return np.ascontiguousarray(np.concatenate(parts)[:n]), {a: np.concatenate([q[a] for q in recs])[:n] for a in recs[0]}


def grid_end(f, n, rng):
    """the end of the outer grid: the point's own abscissa at +L, the flipped one at -L, or z at +-L, for L = 8184, 8188 (the
    kernel's clamp: N SUB - 0.5 sub-cells) and 8192 mm (the grid's edge)"""
    half = 0.5 * f.k["N"] * f.k["H_OUTER"]
    hs = f.k["H_OUTER"] / f.k["SUB"]
    rec = _record(n)
    L = rng.choice([half - hs, half - 0.5 * hs, half], n)
    d = draw(rng, OFFSETS_END, n, AIM_OUTER)
    which = np.arange(n) % 3  # 0 own abscissa, 1 flipped abscissa, 2 z
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    r = np.select([which == 0, which == 1], [L + d + f.coxa, L - d - f.coxa], rng.uniform(1.0, 8100.0, n))
    z = np.where(which == 2, sign * L + d, rng.uniform(-8100.0, 8100.0, n))
    _set(rec, 0, which == 0, X_OWN, L[which == 0])
    _set(rec, 0, which == 1, X_FLIP, -L[which == 1])
    _set(rec, 1, which == 2, Z, (sign * L)[which == 2])
    return f.cyl(r, phis(rng, n), z), rec


def beyond(f, n, rng):
    """beyond the outer grid: r in 8000..20000 mm, z in +-20000 mm (the outer band limit at |p|_1 = 16384 mm lies inside)"""
    return f.cyl(rng.uniform(8000.0, 20000.0, n), phis(rng, n), rng.uniform(-20000.0, 20000.0, n)), _record(n)


_BUILDERS = dict(sub_edges=sub_edges, coarse_edges=coarse_edges, flip_edges=flip_edges, limit_edges=limit_edges, far_seam=far_seam,
                 outer_edges=outer_edges, grid_end=grid_end, beyond=beyond)


def make(family, n, leg, quat, yaw, seed, with_aim=False):
    """n points of `family` for (leg, quat), float32 [n, 3]; yaw = the (min, max) yaw limits.  with_aim: also the aim record"""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    pts, rec = _BUILDERS[family](Frame(leg, quat, yaw), n, rng)
    pts = np.ascontiguousarray(pts, np.float32)
    assert pts.shape == (n, 3) and len(rec["kind"]) == n
    return (pts, rec) if with_aim else pts


def aim_figures(frame, pts, rec):
    """of the aimed coordinates of a cloud (two per corner point), measured on the float32 points through Frame.to_coxa:
    dict(n, miss = |coordinate - line| per aimed coordinate, below / above = the shares strictly on either side of the line)"""
    miss = []
    for col in range(2):
        sel = rec["kind"][:, col] != NONE
        miss.append(frame.aimed(pts[sel], rec["kind"][sel, col]) - rec["line"][sel, col])
    miss = np.concatenate(miss)
    return dict(n=len(miss), miss=np.abs(miss), below=float((miss < 0).mean()) if len(miss) else 0.0,
                above=float((miss > 0).mean()) if len(miss) else 0.0)


# ---- lane orders ----------------------------------------------------------------------------------------------------------
def lane_order(order, far, rng):
    """indices into a cloud with the float64 model's `far` flags.  "blocks" and "shuffled" are permutations; "one_far_lane" /
    "one_near_lane" take as many full waves of 64 as the cloud's rarer kind allows (every wave one far / near point, at lane 0,
    31, 32, 63 in turn, 63 of the other kind) and leave the rest out."""
    far = np.asarray(far, bool)
    idx_far, idx_near = np.flatnonzero(far), np.flatnonzero(~far)
    if order == "blocks":
        return np.concatenate([idx_near, idx_far])
    if order == "shuffled":
        return rng.permutation(len(far))
    assert order in ("one_far_lane", "one_near_lane"), order
    one, rest = (idx_far, idx_near) if order == "one_far_lane" else (idx_near, idx_far)
    waves = min(len(one), len(rest) // 63)
    out = rng.permutation(rest)[:waves * 63].reshape(waves, 63)
    out = np.concatenate([out, np.zeros((waves, 1), np.int64)], axis=1)
    lanes = np.asarray(FAR_LANES)[np.arange(waves) % len(FAR_LANES)]
    single = rng.permutation(one)[:waves]
    for lane in FAR_LANES:  # move the last column to `lane`
        w = lanes == lane
        out[w, lane + 1:] = out[w, lane:63]
        out[w, lane] = single[w]
    return out.reshape(-1)


# ---- cases ----------------------------------------------------------------------------------------------------------------
def case_keys(leg_names=sc.LEG_NAMES, orientations=None):
    """[(family, leg name, orientation name)]: every family meets every leg once; the orientation rotates with (leg, family) as in
    shell_cases.case_keys (identity, the two tilted fixture orientations and, for a random leg, its own quaternion), or through
    `orientations` when given"""
    out = []
    for li, name in enumerate(leg_names):
        orients = list(orientations) if orientations else ["id", "tilt_y", "tilt_z"] + (["rnd"] if name.startswith("rnd_") else [])
        for fi, family in enumerate(FAMILIES):
            out.append((family, name, orients[(li + fi + 1) % len(orients)]))
    return out


case_id = sc.case_id
resolve = sc.resolve
