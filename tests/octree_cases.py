"""Case generators of tests/test_gpu_octree_shapes.py (the octree kernels of csrc/lrm_octree.hip across chunk, tile, block, round,
grid-stride and box boundaries); their preconditions are checked on the host by tests/test_octree_cases_cpu.py.

* launch_constants / launch_plan: the launch arithmetic of oct_level_plan (csrc/lrm_octree.hip), restated independently;
  tests/test_octree_cases_cpu.py holds it against lrm_dbg_oct_plan, which calls the function the launch consumes.
* oracle_tree: octree_oracle.apply_oct with the level records kept (sizes, missing axes, dead quadrants, parent_valid, flags).
* morton_keys: oct_keys_kernel's key, so that a case can say where in memory a foothold ends up.
* decider_cloud: a few footholds that decide the tree plus any number of inert ones -- any cloud size is cheap for the oracle.
* relief / sparse_tiles: dense clouds on which the two-level box cull drops most tiles and chunks.
* face_points: footholds on the faces of a child's elongated box, in float32, with their neighbours.
"""
import math
import os
import re

import numpy as np

from octree_oracle import child_flags, create_child_box, octree_legs, quat_from_angle_index

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
KNOBS = ("LRM_OCT_BRUTE", "LRM_OCT_NOCULL", "LRM_OCT_CHUNKED_FROM", "LRM_OCT_TPR", "LRM_OCT_WGS", "LRM_OCT_DEFER_FROM", "LRM_OCT_DEFER_CAP")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 32_768, 32_769, 262_143, 262_144, 262_145, 262_209)
FAR = 4.0e6  # mm: the far root of the box-geometry cases (one float32 ulp there is 0.25 mm)


# ---- the launch arithmetic, restated ------------------------------------------------------------
def launch_constants():
    """the numbers of oct_level_plan and of the kernels' geometry the sizes of the suite are built around"""
    return {"block": 256, "chunk": 64, "tile": 1024, "chunked_from": 9, "every_cap": 1024, "chunked_cap": 16384, "first_level_wgs": 2048,
            "tpr": (2048, 32, 8192, 128), "wgs": (2048, 32768, 8192, 8192, 4096), "max_splits": 256, "defer_from": 256, "brute_max": 65535}


def launch_plan(nc, nf, env=None):
    """what oct_level_plan says for a level of nc children on nf footholds under the knobs in env"""
    K, env = launch_constants(), env or {}
    ntiles = (nf + K["tile"] - 1) // K["tile"]
    brute = env.get("LRM_OCT_BRUTE", "0")[0] == "1" and nc <= K["brute_max"]
    has_from = "LRM_OCT_CHUNKED_FROM" in env
    chunked_from = int(env["LRM_OCT_CHUNKED_FROM"]) if has_from else K["chunked_from"]
    if not ((nc >= chunked_from or (not has_from and nc * ((ntiles + 31) // 32) >= K["first_level_wgs"])) and not brute):
        gx = min((nf + K["block"] - 1) // K["block"], K["every_cap"])
        nf_pad = (nf + 63) & ~63
        return {"kernel": "every", "grid": gx, "trips": -(-nf_pad // (gx * K["block"])) if gx else 0, "deferred": False}
    a, t0, b, t1 = K["tpr"]
    tpr = t0 if nc < a else (t1 if nc < b else K["block"])
    if "LRM_OCT_TPR" in env:
        tpr = min(max(int(env["LRM_OCT_TPR"]), 1), K["block"])
    a, w0, b, w1, w2 = K["wgs"]
    want = w0 if nc < a else (w1 if nc < b else w2)
    if "LRM_OCT_WGS" in env:
        want = int(env["LRM_OCT_WGS"])
    splits = 1 if nc >= want else (want + nc - 1) // nc
    splits = min(splits, max(1, (ntiles + tpr - 1) // tpr), K["max_splits"])
    return {"kernel": "chunked", "tpr": tpr, "splits": splits, "workgroups": nc * splits, "grid": min(nc * splits, K["chunked_cap"]),
            "deferred": nc >= (int(env["LRM_OCT_DEFER_FROM"]) if "LRM_OCT_DEFER_FROM" in env else K["defer_from"])}


def max_legs():
    src = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "lrm.h")).read()
    return int(re.search(r"#define LRM_MAX_LEGS (\d+)", src).group(1))


# ---- settings, the oracle with its levels -----------------------------------------------------
def reach_len(dim):
    return F(F(F(dim[1] + dim[3]) + dim[5]) + dim[4])


def settings(lrm, center=(0.0, 0.0, 0.0), size=400.0, depth=4, stab=3, legs=4, mounts=None, rot_below=50.0, min_box=None,
             angle_sample=None):
    st = lrm.octree_default_settings()
    size = (size,) * 3 if np.isscalar(size) else size
    for i in range(3):
        st.box_center[i] = center[i]
        st.box_size[i] = size[i]
        if angle_sample is not None:
            st.angle_sample[i] = angle_sample[i]
    st.max_depth = depth
    st.leg_number_for_stab = stab
    st.leg_count = legs
    st.enable_rot_below = rot_below
    if min_box is not None:
        st.min_box = min_box
    if mounts is None and legs != 4:
        mounts = [2 * math.pi * l / legs for l in range(legs)]
    for i, m in enumerate(mounts or ()):
        st.leg_mount[i] = m
    return st


def oracle_tree(oracle, footholds, dim, st):
    """octree_oracle.apply_oct with the levels kept -> (leaves, levels); levels[d] is a list of records
    {c, h, ph, parent_valid, rot, skip, dead, missing, flags}, flags = reach | 2 leaf | 4 edge as the kernels return them (0 for a
    skipped child).  The CPU tests check its leaves against apply_oct's."""
    footholds = np.ascontiguousarray(footholds, F).reshape(-1, 3)
    n_angles = st.angle_sample[0] * st.angle_sample[1] * st.angle_sample[2]
    quats = [quat_from_angle_index(oracle, a, st) for a in range(n_angles)]
    legs = octree_legs(dim, st)
    rl = reach_len(dim)
    root = dict(c=np.array(list(st.box_center), F), h=np.array(list(st.box_size), F), validity=False, leaf=False, raw=True,
                on_edge=False, dead=False, children=None)
    expand, levels = [root], []
    for depth in range(st.max_depth):
        if not expand:
            break
        level = []
        for parent in expand:
            parent["children"] = []
            rot = bool(parent["h"][0] < F(st.enable_rot_below))
            for ci in range(8):
                r = create_child_box(parent["c"], parent["h"], ci, st.min_box)
                if r is None:
                    n = dict(c=np.zeros(3, F), h=np.zeros(3, F), validity=True, leaf=True, raw=False, on_edge=True, dead=True,
                             children=None, missing=None)
                else:
                    n = dict(c=r[0], h=r[1], validity=False, leaf=r[2] >= 3, raw=r[2] < 3, on_edge=False, dead=False, children=None,
                             missing=r[2])
                n.update(ph=parent["h"].copy(), parent_valid=bool(parent["validity"]), rot=rot, skip=bool(n["validity"]), flags=0)
                parent["children"].append(n)
                level.append(n)
            parent["raw"] = False
        for n in level:
            if n["skip"]:
                continue
            near = footholds[(np.abs(footholds - n["c"]) <= n["ph"] + rl + F(1)).all(axis=1)]  # (child_flags culls exactly)
            r, l, e = child_flags(oracle, near, n["c"], n["h"], n["ph"], n["parent_valid"], rot=n["rot"], st=st, legs=legs, quats=quats,
                                  reach_len=rl)
            n["flags"] = int(r) | (int(l) << 1) | (int(e) << 2)
            n["validity"] = n["validity"] or r
            n["leaf"] = n["leaf"] or l
            n["on_edge"] = e and not l
        levels.append(level)
        expand = []
        if depth + 1 < st.max_depth:
            for n in level:
                if not n["on_edge"]:
                    n["leaf"] = True
                if not n["leaf"]:
                    expand.append(n)
    out = []

    def walk(node):
        for c in node["children"] or []:
            if not (c["leaf"] or c["raw"] or c["dead"]):
                walk(c)
            elif not c["dead"] and c["validity"]:
                out.append(c["c"])
    walk(root)
    return np.array(out, F).reshape(-1, 3), levels


def level_sizes(levels):
    return [len(l) for l in levels]


def trace_records(levels, st):
    """the levels as lrm_dbg_oct_trace_read returns them: float32[n, 12]"""
    many = st.angle_sample[0] * st.angle_sample[1] * st.angle_sample[2] > 1
    rec = [list(n["c"]) + list(n["h"]) + list(n["ph"]) + [n["flags"], n["parent_valid"] + 2 * (n["rot"] and many) + 4 * n["skip"], d]
           for d, level in enumerate(levels) for n in level]
    return np.array(rec, F).reshape(-1, 12)


# ---- where a foothold ends up in memory -------------------------------------------------------
def _spread10(v):
    v = v & 0x3ff
    v = (v | (v << 16)) & 0x030000ff
    v = (v | (v << 8)) & 0x0300f00f
    v = (v | (v << 4)) & 0x030c30c3
    return (v | (v << 2)) & 0x09249249


def morton_keys(f):
    """oct_keys_kernel on the bounds apply_oct_impl computes (nan rows and flat or non-finite spans as there)"""
    f = np.ascontiguousarray(f, F).reshape(-1, 3)
    keys = np.zeros(len(f), np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            col = f[:, a]
            ok = ~np.isnan(col)
            lo = F(min(col[ok].min(), F(3.0e38))) if ok.any() else F(3.0e38)
            hi = F(max(col[ok].max(), F(-3.0e38))) if ok.any() else F(-3.0e38)
            span = F(hi - lo)
            inv = F(F(1) / span) if hi > lo and np.isfinite(span) else F(0)
            t = ((col - lo).astype(F) * inv).astype(F)
            t = np.where(t >= 0, t, F(0))
            t = np.where(t > 1, F(1), t).astype(F)
            keys |= _spread10((t * F(1023)).astype(F).astype(np.int64)) << a
    return keys


# ---- decider clouds ---------------------------------------------------------------------------
# Eight footholds under a robot at the root centre (M2 leg, four legs, three needed), found by a search over random sets:
# the first is the greatest of the set on every axis, the last the smallest on every axis, and the tree changes when either
# is taken away -- also from the first two alone (test_octree_cases_cpu.py keeps all of that as assertions).
DECIDERS = np.array([[277.375, 334.875, -83.625], [-297.625, 223.25, -126.25], [-154.375, 90.625, -190.375], [-9.5, 173.125, -114.5],
                     [228.375, 239.875, -100.0], [12.625, 278.5, -109.75], [246.75, 106.625, -197.125], [-324.5, 46.375, -239.25]], F)
DECIDER_HALF, DECIDER_DEPTH, DECIDER_STAB = 400.0, 4, 3


def deciders(layout, center=(0.0, 0.0, 0.0)):
    """the decider set with its extreme foothold first: 'last' -> the componentwise greatest, 'first' -> the smallest"""
    d = DECIDERS if layout == "last" else DECIDERS[::-1]
    return (d + np.array(center, F)).astype(F)


def inert_limit(size, rl):
    return (F(2) * np.abs(np.array(size, F) * np.ones(3, F)) + rl).astype(F)


def is_inert(f, center, size, rl):
    """outside 2 root_half + reach_len of the root centre on at least one axis: in no child's elongated box (a child's centre is
    within root_half of the root's, its parent's half size is at most root_half)"""
    return (np.abs(f - np.array(center, F)) > inert_limit(size, rl)).any(axis=1)


def decider_cloud(dec, nf, layout, center, size, rl, seed=0):
    """nf footholds: the first min(len(dec), nf) rows of dec and inert ones, wholly below the root box on x, y and z ('last': dec[0],
    the greatest decider on every axis, is the last foothold in memory) or wholly above ('first': dec[0], the smallest, is the first).
    Rows in random order: the library sorts.  -> (cloud, the deciders in it)"""
    rng = np.random.default_rng(seed + nf)
    dec = dec[:min(len(dec), nf)]
    side = F(-1) if layout == "last" else F(1)
    off = inert_limit(size, rl) + F(64) + (rng.random((nf - len(dec), 3)) * 512).astype(F)
    f = np.concatenate([dec, (np.array(center, F) + side * off).astype(F)]).astype(F)
    return f[rng.permutation(nf)], dec


def extreme_is_at_the_end(f, e, layout):
    """is e the one foothold whose key is strictly the greatest ('last') or the smallest ('first') of the cloud's?"""
    k = morton_keys(f)
    mine = (f.view(np.uint32) == e.view(np.uint32)).all(axis=1)
    if mine.sum() != 1:
        return False
    if mine.all():
        return True
    return bool(k[mine][0] > k[~mine].max()) if layout == "last" else bool(k[mine][0] < k[~mine].min())


# ---- dense clouds -----------------------------------------------------------------------------
def relief(n, seed, spread, center=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-spread, spread, (n, 2))
    z = 20 * np.sin(xy[:, 0] / 120) + rng.normal(0, 4, n) - 150
    return (np.column_stack([xy, z]) + np.array(center, np.float64)).astype(F)


def sparse_tiles(rl, half, seed=3):
    """8 x 1024 footholds; in memory every tile is ONE chunk inside the root box among fifteen chunks of inert footholds.
    The cloud's bounding box is a cube of half width W = 2 (2 half + reach_len) + 200 around the root; its eight octants are the
    key's top three bits, so each is one tile; inside an octant the next three bits are its sub-octants.  The 64 near footholds sit
    in the sub-octant at the root, the 960 far ones in the seven others (at least W / 2 from the root on some axis), a multiple
    of 64 in each: the near run starts on a chunk boundary.  -> (cloud, near mask)"""
    rng = np.random.default_rng(seed)
    W = 2.0 * (2.0 * half + float(rl)) + 200.0
    out, near = [], []
    for o in range(8):
        neg = [not (o >> a) & 1 for a in range(3)]
        at_root = sum((1 if neg[a] else 0) << a for a in range(3))
        others = [t for t in range(8) if t != at_root]
        for t in range(8):
            if t == at_root:
                # (a relief below the body; the near footholds of the upper octants are above it, inside the elongated boxes only)
                p = np.column_stack([(-1 if neg[a] else 1) * rng.uniform(16.0, 0.9 * half, 64) for a in range(2)] +
                                    [-rng.uniform(110.0, 190.0, 64) if neg[2] else rng.uniform(300.0, 0.9 * half, 64)])
            else:
                n = 128 + (64 if t == others[-1] else 0)
                lo = [(-W if neg[a] else 0.0) + ((t >> a) & 1) * W / 2 for a in range(3)]
                p = np.column_stack([rng.uniform(lo[a] + 16.0, lo[a] + W / 2 - 16.0, n) for a in range(3)])
            out.append(p)
            near.append(np.full(len(p), t == at_root))
    f = np.concatenate(out).astype(F)
    f[0], f[-1] = (-W, -W, -W), (W, W, W)  # the corners of the bounding box: far footholds of the first and the last octant
    return f, np.concatenate(near)


# ---- faces of the elongated box ---------------------------------------------------------------
def face_points(c, ph, rl, axis, other):
    """float32 c[axis] + H and c[axis] - H, H = |ph[axis] + reach_len|, each with its nextafter neighbours on both sides; the
    two other coordinates from `other` -> float32[6, 3], and in_box's own verdict per row (float32 subtraction, asymmetric)"""
    H = np.abs(F(ph[axis] + rl))
    hi, lo = F(c[axis] + H), F(c[axis] - H)
    vals = [np.nextafter(hi, F(-np.inf)), hi, np.nextafter(hi, F(np.inf)), np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
    pts = np.tile(np.array(other, F), (6, 1))
    pts[:, axis] = vals
    v = (pts[:, axis] - F(c[axis])).astype(F)
    return pts, (H >= v) & (-H < v)


# ---- the cases --------------------------------------------------------------------------------
class Case:
    """a cloud, a leg, settings, and the footholds the oracle needs for the expected tree (the whole cloud when `decide` is None)"""

    def __init__(self, f, dim, st, decide=None, env=None, extreme=None, layout=None):
        self.f, self.dim, self.st, self.decide, self.env, self.extreme, self.layout = f, dim, st, decide, env or {}, extreme, layout

    def oracle_cloud(self):
        return self.f if self.decide is None else self.decide


def decider_case(lrm, nf, layout, center=(0.0, 0.0, 0.0), env=None, seed=0):
    dim = lrm.get_M2_leg(0.0)
    st = settings(lrm, center=center, size=DECIDER_HALF, depth=DECIDER_DEPTH, stab=DECIDER_STAB)
    f, dec = decider_cloud(deciders(layout, center), nf, layout, center, DECIDER_HALF, reach_len(dim), seed)
    return Case(f, dim, st, decide=dec, env=env, extreme=dec[0], layout=layout)


SPLIT_ENV = {"LRM_OCT_TPR": "1", "LRM_OCT_WGS": "32768"}


def knob_cases(lrm):
    """section 2: several workgroups per child (splits 5 and 9), and more workgroups than the chunked kernel's grid cap"""
    out = {f"splits_{nf}_{layout}": decider_case(lrm, nf, layout, env=SPLIT_ENV) for nf in (4097, 8193) for layout in ("first", "last")}
    out.update({f"cap_65537_{layout}": decider_case(lrm, 65_537, layout, env=SPLIT_ENV) for layout in ("first", "last")})
    return out


DENSE_HALF = 800.0


def dense_cases(lrm):
    """section 3: clouds 4 root half-sizes wide -- most tiles and chunks are outside most children's elongated boxes"""
    dim = lrm.get_M2_leg(0.0)
    out = {f"relief_{nf}": Case(relief(nf, 500 + nf, k * DENSE_HALF), dim, settings(lrm, size=DENSE_HALF, depth=4, stab=2))
           for nf, k in ((65, 3), (1025, 6), (4097, 6))}
    f, _ = sparse_tiles(reach_len(dim), DENSE_HALF)
    out["sparse_tiles"] = Case(f, dim, settings(lrm, size=DENSE_HALF, depth=4, stab=3))
    out["rotations_257"] = Case(relief(257, 757, 2000.0), dim, settings(lrm, size=400.0, depth=3, stab=2, legs=2, mounts=[0.0, 1.2], rot_below=500.0))
    return out


OFF_ORIGIN = (1234.5, -987.25, 310.0)
FAR_ROOT = (FAR, -FAR, FAR)


def geometry_cases(lrm):
    """section 4, but for the faces: small clouds, whole-tree oracle"""
    dim = lrm.get_M2_leg(0.0)
    f = relief(160, 404, 600.0)
    out = {"off_origin": Case(relief(160, 404, 600.0, OFF_ORIGIN), dim, settings(lrm, center=OFF_ORIGIN, size=400.0, depth=4, stab=3)),
           "far_root": Case(relief(160, 404, 600.0, FAR_ROOT), dim, settings(lrm, center=FAR_ROOT, size=400.0, depth=4, stab=3)),
           # z below min_box from the root on, y from the second level on, x at the fifth: missing 1, 2 and 3, dead quadrants
           "flat_box": Case(f, dim, settings(lrm, size=(400.0, 180.0, 90.0), center=(0.0, 0.0, 40.0), depth=5, stab=2)),
           "flat_box_off_origin": Case(relief(160, 404, 600.0, OFF_ORIGIN), dim,
                                       settings(lrm, size=(333.3, 90.0, 170.0), center=OFF_ORIGIN, depth=4, stab=2)),
           # rotations start when the PARENT's x half size is below enable_rot_below: here at the second level, y and z never
           "rot_thin_x": Case(f[:80], dim, settings(lrm, size=(120.0, 400.0, 400.0), depth=4, stab=3, rot_below=100.0)),
           # ... and here at the third level, while y and z are below it from the first
           "rot_thick_x": Case(f[:80], dim, settings(lrm, size=(380.0, 90.0, 90.0), center=(0.0, 0.0, 30.0), depth=3, stab=2, rot_below=100.0, min_box=20.0)),
           "one_leg": Case(f, dim, settings(lrm, depth=4, stab=1, legs=1, mounts=[0.3])),
           "max_legs_stab_1": Case(f, dim, settings(lrm, depth=3, stab=1, legs=max_legs())),
           "max_legs_stab_all": Case(f, dim, settings(lrm, size=300.0, depth=3, stab=max_legs(), legs=max_legs(), mounts=[0.05 * l for l in range(max_legs())])),
           "two_legs_stab_all": Case(f, dim, settings(lrm, depth=4, stab=2, legs=2, mounts=[0.0, 1.2])),
           "one_orientation": Case(f[:80], dim, settings(lrm, size=300.0, depth=3, stab=3, rot_below=400.0, angle_sample=(1, 1, 1))),
           "six_orientations": Case(f[:80], dim, settings(lrm, size=300.0, depth=3, stab=3, rot_below=400.0, angle_sample=(2, 1, 3))),
           "depth_0": Case(f, dim, settings(lrm, depth=0, stab=1))}
    return out


FACE_ROOTS = {"origin": ((0.0, 0.0, 0.0), 400.0), "off_origin": (OFF_ORIGIN, 410.7), "far": (FAR_ROOT, 410.7)}
FACE_DEPTH, FACE_STAB = 3, 3
# three footholds (found by a search) under which valid, still expanding first-level children have children that see edges only
FACE_BASE = np.array([[26.375, 62.0, -90.0], [84.125, -40.5, -163.125], [232.125, 201.375, -120.5]], F)


def face_cases(lrm, oracle, root):
    """{(axis, side, k): Case}: FACE_BASE around `root`, 64 copies of ONE foothold on a face of the elongated box of a child whose
    parent is valid and still expanding and which nothing else turns into a leaf (flags reach | edge without it), and inert
    footholds up to 192.  The copies have the greatest (side +1) or smallest (side -1) key of the cloud: they are the last or the
    first chunk, whose box is that one point -- only the box cull can drop it.  k: -1 / 0 / +1 = the nextafter neighbour towards
    -inf, the face value, the neighbour towards +inf.  Also returns the child per (axis, side) and in_box's verdicts."""
    center, half = FACE_ROOTS[root]
    dim = lrm.get_M2_leg(0.0)
    rl = reach_len(dim)
    st = settings(lrm, center=center, size=half, depth=FACE_DEPTH, stab=FACE_STAB)
    base = (FACE_BASE + np.array(center, F)).astype(F)
    _, levels = oracle_tree(oracle, base, dim, st)
    cand = [n for level in levels[1:] for n in level if n["parent_valid"] and not n["skip"] and n["flags"] == 5]
    cases, picked = {}, {}
    for axis in range(3):
        for side in (1, -1):
            other = (base.max(axis=0) + F(24)) if side > 0 else (base.min(axis=0) - F(24))
            for n in cand:
                pts, inside = face_points(n["c"], n["ph"], rl, axis, other)
                pts, inside = (pts[:3], inside[:3]) if side > 0 else (pts[3:], inside[3:])
                H = np.abs(n["ph"] + rl)
                o = [a for a in range(3) if a != axis]
                beyond = pts[1, axis] > base[:, axis].max() + 24 if side > 0 else pts[1, axis] < base[:, axis].min() - 24
                if beyond and (np.abs(other[o] - n["c"][o]) < H[o] - 1).all():
                    break
            else:
                continue
            picked[axis, side] = (n, inside)
            layout = "last" if side > 0 else "first"
            for k in (-1, 0, 1):
                dec = np.concatenate([np.tile(pts[k + 1], (64, 1)), base]).astype(F)
                f, _ = decider_cloud(dec, 192, layout, center, half, rl, seed=axis)
                cases[axis, side, k] = Case(f, dim, st, decide=dec, extreme=pts[k + 1], layout=layout)
    return cases, picked, base


def nonfinite_cases(lrm):
    """section 5: decider clouds of 4097 footholds with non-finite rows added; the expected tree is the finite footholds'.
    A nan coordinate gives key bits 0 on its axis (oct_keys_kernel), so all-nan rows have key 0 and come first in memory."""
    out = {}
    nan, inf, big, tiny = F(np.nan), F(np.inf), F(3.2e38), F(1e-41)
    # 'first': the extreme decider has key 0 too -- chunk 0 is that decider and 63 rows with one, two or three nan coordinates
    first = decider_case(lrm, 4097, "first")
    e = first.extreme
    pat = [[nan, e[1], e[2]], [e[0], nan, e[2]], [e[0], e[1], nan], [nan, nan, e[2]], [nan, e[1], nan], [e[0], nan, nan], [nan, nan, nan]]
    out["nan_in_the_deciders_chunk"] = Case(np.concatenate([np.array((pat * 9)[:63], F), first.f]), first.dim, first.st, decide=first.decide,
                                            extreme=e, layout="first")
    # +-inf, +-3.2e38 (beyond the box sentinel of oct_boxes_kernel) and subnormals, which are ordinary footholds at the origin:
    # a span that is not finite gives every foothold key bits 0 on that axis
    last = decider_case(lrm, 4097, "last")
    sub = np.array([[tiny, -tiny, -150.0], [-tiny, tiny, -120.0], [tiny, tiny, -tiny]], F)
    e = last.extreme
    bad = [[inf, e[1], e[2]], [e[0], -inf, e[2]], [e[0], e[1], inf], [big, e[1], e[2]], [e[0], -big, e[2]], [e[0], e[1], big],
           [-big, -big, -big], [inf, inf, inf], [-inf, nan, big], [nan, inf, -inf]]
    out["inf_huge_and_subnormal"] = Case(np.concatenate([last.f, np.array(bad * 3, F), sub]), last.dim, last.st,
                                         decide=np.concatenate([last.decide, sub]))
    out["huge_on_one_side"] = Case(np.concatenate([last.f, np.array([[big, e[1], e[2]], [e[0], big, e[2]], [big, big, big]] * 5, F)]), last.dim,
                                   last.st, decide=last.decide)
    out["a_chunk_of_nan"] = Case(np.concatenate([last.f, np.full((64, 3), nan, F)]), last.dim, last.st, decide=last.decide, extreme=e, layout="last")
    out["a_tile_of_nan"] = Case(np.concatenate([np.full((1024, 3), nan, F), last.f]), last.dim, last.st, decide=last.decide, extreme=e, layout="last")
    out["nan_only"] = Case(np.full((1025, 3), nan, F), last.dim, last.st, decide=np.zeros((0, 3), F))
    return out
