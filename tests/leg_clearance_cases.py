"""Shared cases of the leg link clearance tests (tests/test_leg_clearance_cpu.py, tests/test_gpu_leg_clearance.py): the
scenes of footholds_posed_cases with the bodies lowered towards the terrain and every target present twice (an exact pen
tie for every winner), joint angles from the host IK on the host foothold choice, and brute_np: the per-(link, target)
arithmetic of include/lrm.h (lrm_leg_clearance_posed_dev) restated in vectorised numpy float32, one rounding per
operation, written from that text and not from csrc/lrm_leg_clearance.h.

brute_np does not restate the joint chain: it takes the joints from lrm_fk_posed_cpu (an older call with tests of its
own) on legs whose link lengths are zeroed or shortened, with a zero body -- the identities the joint tests assert of
lrm_leg_joints_posed_cpu bit for bit (J3 = the tip with tibia_length T', J2 with tibia_length 0, J1 with femur and tibia 0,
J0 with all three 0).  The joints here therefore come from the library's own FK; that they are where a leg of these dimensions
has them, and that d is the distance to a link, is checked against the independent float64 model of tests/leg_model64.py in
tests/test_clearance_float64_cpu.py."""
import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

F = np.float32
COXA_LEN, TIBIA_LEN, FEMUR_LEN = pc.COXA_LEN, pc.TIBIA_LEN, pc.FEMUR_LEN
RADIUS = (28.0, 22.0, 16.0)  # coxa, femur, tibia link (mm)
MARGIN = 10.0                # radius + margin stays below TIP_CLEAR: a stance is not near its own foothold either
TIP_CLEAR = 30.0             # exceeds the tibia radius: a stance does not collide with its own foothold
# body height offsets, cycled over the poses: from crouching in the terrain to standing tall
OFFSETS = np.array([-150.0, -90.0, -40.0, 0.0, 60.0, -120.0, 30.0, -60.0, 120.0], F)


def layout(nposes, nlegs):
    """(pose_idx int32, leg_idx uint8) of the [l*nposes + p] order"""
    return np.tile(np.arange(nposes, dtype=np.int32), nlegs), np.repeat(np.arange(nlegs, dtype=np.uint8), nposes)


def scene(lrm, nposes, nt, seed, kind="rough", twins=True):
    """(quats, body, targets): footholds_posed_cases.scene on nt // 2 targets followed by a shuffled second copy of them
    (twins=False or nt < 2: nt targets, no copies), the bodies moved along z by OFFSETS"""
    if twins and nt >= 2:
        quats, body, targets = fc.scene(lrm, nposes, nt // 2, seed, kind)
        targets = pc.with_spread_duplicates(targets, seed)[0]
        if len(targets) < nt:
            targets = np.concatenate([targets, targets[:nt - len(targets)]])
    else:
        quats, body, targets = fc.scene(lrm, nposes, nt, seed, kind)
    body = body.copy()
    body[:, 2] += OFFSETS[np.arange(nposes) % len(OFFSETS)]
    return quats, np.ascontiguousarray(body, F), np.ascontiguousarray(targets, F)


def main_scene(lrm, nposes=150, nt=3000, seed=1):
    """the non-vacuity scene: bodies low over `rough`, one unit quaternion of the reference's sweep per pose (a non-unit
    quaternion scales lengths, tip_clear among them, and a stance could then touch its own foothold)"""
    _, body, targets = scene(lrm, nposes, nt, seed)
    return fc.sweep_pose_quats(lrm, nposes, seed), body, targets


def stance_angles(lrm, targets, quats, body, legs):
    """angles float32[nlegs*nposes, 3] at [l*nposes + p]: lrm_ik_posed_cpu on lrm_footholds_posed_cpu's best (nan where a leg
    reaches nothing), the status bytes and best"""
    best = lrm.footholds_posed_cpu(targets, quats, body, legs, None)[1]
    pi, li = layout(len(quats), len(legs))
    ang, st, _ = lrm.apply_ik_posed_cpu(targets, pi, li, quats, body, legs, target_idx=best.reshape(-1))
    return ang, st, best


def random_angles(nposes, nlegs, seed):
    """angles inside the sincos range but not from any IK: every leg is valid, links point anywhere"""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-1.2, 1.2, nposes * nlegs), rng.uniform(-1.4, 1.0, nposes * nlegs),
                            rng.uniform(-2.4, 0.2, nposes * nlegs)]).astype(F)


def with_lengths(legs, coxa=None, femur=None, tibia=None):
    legs = np.array(legs, F).reshape(-1, 14).copy()
    for col, v in ((COXA_LEN, coxa), (FEMUR_LEN, femur), (TIBIA_LEN, tibia)):
        if v is not None:
            legs[:, col] = v
    return legs


def tibia_short(legs, tip_clear):
    """T' of every leg: T - tip_clear in float32, 0 unless > 0"""
    t = (np.array(legs, F).reshape(-1, 14)[:, TIBIA_LEN] - F(tip_clear)).astype(F)
    return np.where(t > 0, t, F(0)).astype(F)


def joints_from_fk(lrm, angles, quats, body, legs, tip_clear):
    """float32[nlegs, nposes, 4, 3]: J0..J3 through lrm_fk_posed_cpu on shortened legs; body None = relative joints"""
    legs = np.array(legs, F).reshape(-1, 14)
    nl, n = len(legs), len(quats)
    pi, li = layout(n, nl)
    variants = (with_lengths(legs, 0.0, 0.0, 0.0), with_lengths(legs, None, 0.0, 0.0), with_lengths(legs, None, None, 0.0),
                with_lengths(legs, None, None, tibia_short(legs, tip_clear)))
    out = np.zeros((nl, n, 4, 3), F)
    for k, lg in enumerate(variants):
        out[:, :, k, :] = lrm.apply_fk_posed_cpu(angles, pi, li, quats, body, lg)[0].reshape(nl, n, 3)
    return out


def brute_np(targets, body, joints, radius, margin, live_in=None, detail=False):
    """joints: float32[nlegs, nposes, 4, 3] RELATIVE to the body.  -> dict(hits, links, worst, pen [nlegs, nposes], free
    [nposes]); detail=True adds valid [nlegs, nposes] and near_any [nlegs, nposes] (some target near some link) and, per
    (leg, pose), the hit mask over the targets in "hit" [nlegs, nposes, nt] and the float32 distance of every decision in "d"
    [nlegs, nposes, 3, nt] (inf where none was computed: a dead pose, an invalid leg, a link with radius 0)"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    nl, n = joints.shape[:2]
    nt = len(targets)
    radius = np.asarray(radius, F).reshape(3)
    reach = (radius + F(margin)).astype(F)  # the sum formed once
    hits, links = np.zeros((nl, n), np.int32), np.zeros((nl, n), np.uint8)
    worst, pen = np.full((nl, n), -1, np.int32), np.full((nl, n), -np.inf, F)
    free = np.zeros(n, np.uint8)
    valid, near_any = np.zeros((nl, n), bool), np.zeros((nl, n), bool)
    hitm = np.zeros((nl, n, nt), bool) if detail else None
    dm = np.full((nl, n, 3, nt), np.inf, F) if detail else None
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        for p in range(n):
            live = live_in is None or bool(live_in[p])
            if not live:
                continue
            q = (targets - np.asarray(body[p], F)).astype(F)  # one subtraction per component
            for l in range(nl):
                J = joints[l, p]
                valid[l, p] = bool(np.isfinite(J).all())
                if not valid[l, p]:
                    continue
                near = np.zeros(nt, bool)
                hit = np.zeros(nt, bool)
                best = np.full(nt, -np.inf, F)
                for k in range(3):
                    if radius[k] == 0:
                        continue
                    A, B = J[k], J[k + 1]
                    ab = (B - A).astype(F)
                    ap = (q - A).astype(F)
                    den = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]
                    num = (ap[:, 0] * ab[0] + ap[:, 1] * ab[1]) + ap[:, 2] * ab[2]
                    s = (num / den).astype(F) if den > 0 else np.zeros(nt, F)
                    s = np.where(~(s > zero), zero, np.where(s > one, one, s)).astype(F)
                    e = (ap - (s[:, None] * ab).astype(F)).astype(F)
                    d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(F)
                    if detail:
                        dm[l, p, k] = d
                    hk, nk = d < radius[k], d < reach[k]
                    pk = ((radius[k] - d) + zero).astype(F)
                    best = np.where(nk & (~near | (pk > best)), pk, best)
                    near |= nk
                    hit |= hk
                    if hk.any():
                        links[l, p] |= 1 << k
                hits[l, p] = hit.sum()
                near_any[l, p] = near.any()
                if detail:
                    hitm[l, p] = hit
                if near.any():
                    masked = np.where(near, best, F(-np.inf))
                    mx = masked.max()
                    worst[l, p] = int(np.argmax(near & (masked == mx)))  # ties to the smaller index
                    pen[l, p] = mx
            free[p] = int((hits[:, p] == 0).all())
    out = {"hits": hits, "links": links, "worst": worst, "pen": pen, "free": free}
    if detail:
        out.update(valid=valid, near_any=near_any, hit=hitm, d=dm)
    return out


def host(lrm, targets, quats, body, legs, angles, radius=RADIUS, margin=MARGIN, tip_clear=TIP_CLEAR, live_in=None, **kw):
    hits, links, worst, pen, free, _ = lrm.leg_clearance_posed_cpu(targets, quats, body, legs, angles, radius, margin, tip_clear,
                                                                   live_in, **kw)
    return {"hits": hits, "links": links, "worst": worst, "pen": pen, "free": free}


def assert_same(got, want):
    """got: (hits, links, worst, pen, free) arrays (pen / free may be None); want: brute_np's or the host loop's"""
    hits, links, worst, pen, free = got
    shape = want["hits"].shape
    assert np.array_equal(np.asarray(hits).reshape(shape), want["hits"])
    assert np.array_equal(np.asarray(links).reshape(shape), want["links"])
    assert np.array_equal(np.asarray(worst).reshape(shape), want["worst"])
    if pen is not None:
        assert np.array_equal(pc.bits(pen).reshape(shape), pc.bits(want["pen"]))
    if free is not None:
        assert np.array_equal(free, want["free"])


def assert_consequences(want, margin, live_in=None):
    """pen > 0 iff hits > 0 iff links != 0; margin 0 makes worst a hit or -1; free = live and no leg hit; a skipped pose
    has the empty answer with free 0"""
    n = want["hits"].shape[1]
    live = np.ones(n, bool) if live_in is None else np.asarray(live_in).astype(bool)
    assert np.array_equal(want["pen"] > 0, want["hits"] > 0)
    assert np.array_equal(want["links"] != 0, want["hits"] > 0)
    assert np.array_equal(want["worst"] < 0, np.isneginf(want["pen"]))
    assert np.isfinite(want["pen"][want["worst"] >= 0]).all()
    if margin == 0:
        assert np.array_equal(want["worst"] >= 0, want["hits"] > 0)
    assert np.array_equal(want["free"].astype(bool), live & (want["hits"] == 0).all(0))
    dead = ~live
    assert (want["hits"][:, dead] == 0).all() and (want["links"][:, dead] == 0).all() and (want["worst"][:, dead] == -1).all()
    assert np.isneginf(want["pen"][:, dead]).all() and (want["free"][dead] == 0).all()


def live_forms(lrm, targets, quats, body, legs):
    """NULL, all 1, all 0, and all_legs of lrm_footholds_posed_cpu"""
    n = len(quats)
    all_legs = lrm.footholds_posed_cpu(targets, quats, body, legs, None)[3]
    return {"null": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "all_legs": all_legs}
