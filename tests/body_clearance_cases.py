"""Shared cases of the body clearance tests (tests/test_body_clearance_cpu.py, tests/test_gpu_body_clearance.py): the
scenes of footholds_posed_cases with a per-pose height offset added to the bodies and every target present twice (an
exact height tie between two column targets wherever a column is not empty), and a brute force that skips nothing, built
from the oracle alone: orc_qt_invert once per pose, orc_qt_rotate and orc_in_cylinder (about the origin, once with
floor_z and once with minus_z) per (pose, target) on target - body[pose] in float32; the height vz - minus_z and its
order in numpy float32, the first index at the maximum.

brute_np is the same arithmetic restated in vectorised numpy float32 (oracle/oracle.c's qt_invert, qt_rotate and
in_cylinder, operation for operation) for the one scale case, where a Python call per pair would take minutes; the CPU
tests hold it to brute() bit for bit on every scene they run."""
import ctypes as C

import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

MAX_PAIRS = 2e6  # per oracle brute force: three library calls per (pose, target), about a microsecond each
BODY = pc.BODY
# the reference's body cylinder (several_leg.cu:504-630): top 250 mm over the body origin, belly 110 or 45 mm under it
PLUS_Z, MINUS_Z = 250.0, (-110.0, -45.0)
# height offsets of the bodies, cycled over the poses: buried, grazing, standing, hovering (nothing under the floor)
OFFSETS = np.array([-260.0, -150.0, -60.0, 0.0, 90.0, 700.0, -110.0, 240.0, 1500.0], np.float32)


def scene(lrm, nposes, nt, seed, kind="rough", twins=True):
    """(quats, body, targets): footholds_posed_cases.scene on nt // 2 targets followed by a shuffled second copy of them
    (pair_cases.with_spread_duplicates; twins=False or nt < 2: nt targets, no copies), the bodies moved along z by OFFSETS"""
    if twins and nt >= 2:
        quats, body, targets = fc.scene(lrm, nposes, nt // 2, seed, kind)
        targets = pc.with_spread_duplicates(targets, seed)[0]
        if len(targets) < nt:  # odd nt: one more copy of target 0
            targets = np.concatenate([targets, targets[:nt - len(targets)]])
    else:
        quats, body, targets = fc.scene(lrm, nposes, nt, seed, kind)
    body = body.copy()
    body[:, 2] += OFFSETS[np.arange(nposes) % len(OFFSETS)]
    return quats, np.ascontiguousarray(body, np.float32), np.ascontiguousarray(targets, np.float32)


def floor_of(minus_z, depth=300.0):
    return float(np.float32(minus_z) - np.float32(depth))


def _finish(col, hit, vz, minus_z, live):
    """(hits, top, height, free) of one pose from its two masks and vz: float32 numpy, the first index at the maximum"""
    if not live:
        return 0, -1, np.float32(-np.inf), 0
    with np.errstate(over="ignore", invalid="ignore"):
        h = (vz - np.float32(minus_z)) + np.float32(0.0)  # -0 -> +0
    hits = int(hit.sum())
    if not col.any():
        return hits, -1, np.float32(-np.inf), int(hits == 0)
    masked = np.where(col, h, np.float32(-np.inf))
    mx = masked.max()
    return hits, int(np.argmax(col & (masked == mx))), mx, int(hits == 0)


def _pack(rows):
    return {"hits": np.array([r[0] for r in rows], np.int32).reshape(-1), "top": np.array([r[1] for r in rows], np.int32).reshape(-1),
            "height": np.array([r[2] for r in rows], np.float32).reshape(-1), "free": np.array([r[3] for r in rows], np.uint8).reshape(-1)}


def brute(oracle, targets, quats, body, radius, plus_z, minus_z, floor_z=None, live_in=None, masks=False):
    """-> dict(hits, top int32[P], height float32[P], free uint8[P]) from the oracle alone; masks=True adds the two
    [P, T] masks "column" and "hit" and the heights "h" [P, T] (meaningful where column is set)"""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    quats = np.ascontiguousarray(quats, np.float32).reshape(-1, 4)
    floor_z = minus_z if floor_z is None else floor_z
    npz, nt = len(quats), len(targets)
    assert npz * nt <= MAX_PAIRS, "brute force too large"
    L = oracle.lib
    rot, cyl = L.orc_qt_rotate, L.orc_in_cylinder
    r_, p_, m_, f_ = C.c_float(radius), C.c_float(plus_z), C.c_float(minus_z), C.c_float(floor_z)
    zero = np.zeros(3, np.float32)
    zp = C.c_void_p(zero.ctypes.data)
    qinv = np.zeros(4, np.float32)
    qp = C.c_void_p(qinv.ctypes.data)
    v = np.zeros((max(nt, 1), 3), np.float32)
    rows, cols, hitm, hs = [], [], [], []
    for p in range(npz):
        live = live_in is None or bool(live_in[p])
        col, hit = np.zeros(nt, bool), np.zeros(nt, bool)
        if live:
            with np.errstate(over="ignore", invalid="ignore"):
                rel = np.ascontiguousarray((targets - body[p]).astype(np.float32))  # one f32 subtraction per component
            L.orc_qt_invert(C.c_void_p(quats[p].ctypes.data), qp)
            ra, va = rel.ctypes.data, v.ctypes.data
            for t in range(nt):
                vp = C.c_void_p(va + 12 * t)
                rot(qp, C.c_void_p(ra + 12 * t), vp)
                col[t] = cyl(r_, p_, f_, zp, vp)
                hit[t] = cyl(r_, p_, m_, zp, vp)
        row = _finish(col, hit, v[:nt, 2], minus_z, live)
        rows.append(row)
        if masks:
            cols.append(col)
            hitm.append(hit)
            with np.errstate(over="ignore", invalid="ignore"):
                h = (v[:nt, 2] - np.float32(minus_z)) + np.float32(0.0)
            hs.append(h)
    out = _pack(rows) if npz else _pack([])
    if masks:
        out.update(column=np.array(cols, bool).reshape(npz, nt), hit=np.array(hitm, bool).reshape(npz, nt),
                   h=np.array(hs, np.float32).reshape(npz, nt))
    return out


def brute_np(targets, quats, body, radius, plus_z, minus_z, floor_z=None, live_in=None):
    """brute() with oracle/oracle.c's three functions restated in numpy float32, one rounding per operation, in their
    order: qt_invert (n2 = x*x + y*y + z*z + w*w; x/n2, -y/n2, -z/n2, -w/n2), qt_rotate (t2 .. t10, then
    2 * (a*vx + b*vy + c*vz) + v per component) and in_cylinder about the origin"""
    f = np.float32
    targets = np.ascontiguousarray(targets, f).reshape(-1, 3)
    quats = np.ascontiguousarray(quats, f).reshape(-1, 4)
    floor_z = minus_z if floor_z is None else floor_z
    rows = []
    with np.errstate(all="ignore"):
        for p in range(len(quats)):
            live = live_in is None or bool(live_in[p])
            if not live:
                rows.append(_finish(None, None, None, minus_z, False))
                continue
            q = quats[p]
            n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
            x, y, z, w = q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2
            t2, t3, t4, t5, t6, t7, t8, t9, t10 = x * y, x * z, x * w, -y * y, y * z, y * w, -z * z, z * w, -w * w
            rel = (targets - body[p]).astype(f)
            vx, vy, vz = rel[:, 0], rel[:, 1], rel[:, 2]
            rx = f(2) * ((t8 + t10) * vx + (t6 - t4) * vy + (t3 + t7) * vz) + vx
            ry = f(2) * ((t4 + t6) * vx + (t5 + t10) * vy + (t9 - t2) * vz) + vy
            rz = f(2) * ((t7 - t3) * vx + (t2 + t9) * vy + (t5 + t8) * vz) + vz
            inside = (np.sqrt(rx * rx + ry * ry + f(0)) < f(radius)) & (rz < f(plus_z))
            rows.append(_finish(inside & (rz > f(floor_z)), inside & (rz > f(minus_z)), rz, minus_z, True))
    return _pack(rows)


def host(lrm, targets, quats, body, legs, radius, plus_z, minus_z, floor_z=None, live_in=None):
    hits, top, height, free, _ = lrm.body_clearance_posed_cpu(targets, quats, body, legs, radius, plus_z, minus_z, floor_z, live_in)
    return {"hits": hits, "top": top, "height": height, "free": free}


def assert_same(got, want):
    """got: (hits, top, height, free) arrays (height / free may be None); want: brute()'s or the host loop's"""
    hits, top, height, free = got
    assert np.array_equal(hits, want["hits"])
    assert np.array_equal(top, want["top"])
    if height is not None:
        assert np.array_equal(pc.bits(height), pc.bits(want["height"]))
    if free is not None:
        assert np.array_equal(free, want["free"])
    empty = want["top"] < 0
    assert np.isneginf(want["height"][empty]).all() and (want["hits"][empty] == 0).all()
    assert np.isfinite(want["height"][~empty]).all()


def assert_consequences(want, live_in=None):
    """for live poses: hits > 0 iff height > 0 iff free == 0; a skipped pose has the empty answer with free = 0"""
    live = np.ones(len(want["hits"]), bool) if live_in is None else np.asarray(live_in).astype(bool)
    assert np.array_equal(want["hits"][live] > 0, want["height"][live] > 0)
    assert np.array_equal(want["hits"][live] > 0, want["free"][live] == 0)
    dead = ~live
    assert (want["hits"][dead] == 0).all() and (want["top"][dead] == -1).all() and np.isneginf(want["height"][dead]).all()
    assert (want["free"][dead] == 0).all()


def live_forms(lrm, targets, quats, body, legs):
    """the four live_in forms of the issue: NULL, all 1, all 0, and all_legs of lrm_footholds_posed_cpu"""
    n = len(quats)
    all_legs = lrm.footholds_posed_cpu(targets, quats, body, legs, None)[3]
    return {"null": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "all_legs": all_legs}


def assert_not_vacuous(want, share=0.10):
    """by the oracle alone (want: brute(masks=True) with every pose live): at least `share` of the poses collide, at least
    `share` are free over a non-empty column, at least `share` have an empty column, and some pose has an exact height tie
    between two column targets, resolved to the smaller index"""
    n = len(want["hits"])
    collide, empty = want["hits"] > 0, want["top"] < 0
    assert collide.mean() >= share, float(collide.mean())
    assert (~collide & ~empty).mean() >= share, float((~collide & ~empty).mean())
    assert empty.mean() >= share, float(empty.mean())
    tied = 0
    for p in np.flatnonzero(~empty):
        at_max = np.flatnonzero(want["column"][p] & (want["h"][p] == want["height"][p]))
        assert want["top"][p] == at_max[0]
        tied += len(at_max) >= 2
    assert tied > 0 and n > 0
