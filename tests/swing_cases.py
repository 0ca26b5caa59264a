"""Shared cases of the swing transit tests (tests/test_swing_cpu.py, tests/test_gpu_swing.py):

* path_np: a vectorised numpy float32 restatement of the foot path, written from include/lrm.h (every operation a separate
  float32 operation in the stated order; the two end points copied, not computed);
* brute_reach: every sample of every swinging (edge, leg) as one query of lrm_reach_dist_posed_cpu on a pose table that holds
  lrm_dbg_edge_transit_samples_host's sample poses, with the restated feet as targets; every reach output folded in numpy;
* the scenes, the host-loop wrapper and the bit-for-bit comparison."""
import numpy as np

import pair_cases as pc
import transit_cases as tr

F = np.float32
REACH_KEYS = ("mask", "reached", "first_miss", "worst", "worst_d2")
TERRAIN_KEYS = ("hits", "hit_seg", "near", "pen")
EDGE_KEYS = ("swinging", "clear")
KEYS = REACH_KEYS + TERRAIN_KEYS + EDGE_KEYS
OPTIONAL = ("mask", "worst", "worst_d2", "pen", "swinging", "clear")
I32 = np.iinfo(np.int32)


def up_of(up):
    return np.array([0, 0, 1], F) if up is None else np.asarray(up, F).reshape(3)


def path_np(A, B, S, lift, up=None):
    """A, B float32 [n, 3] -> (P float32 [n, S, 3] relative to A, feet float32 [n, S, 3] in the caller's frame)"""
    A, B = np.asarray(A, F).reshape(-1, 3), np.asarray(B, F).reshape(-1, 3)
    up, lift = up_of(up), F(lift)
    P = np.zeros((len(A), S, 3), F)
    with np.errstate(all="ignore"):
        D = (B - A).astype(F)
        for s in range(1, S - 1):
            u = F(s) / F(S - 1)
            w = F(1) - u
            h = F(lift * F(F(F(4) * u) * w))
            P[:, s] = (u * D).astype(F) + (h * up).astype(F)[None, :]
        P[:, S - 1] = D
        feet = (A[:, None, :] + P).astype(F)
    feet[:, 0], feet[:, S - 1] = A, B
    return P, feet


def swinging_of(nt, nposes, ea, eb, ffrom, fto, live_in=None):
    live = tr.live_of(nposes, ea, eb, live_in)
    ffrom, fto = np.asarray(ffrom, np.int64), np.asarray(fto, np.int64)
    return live, live[None, :] & (ffrom >= 0) & (ffrom < nt) & (fto >= 0) & (fto < nt)


def brute_reach(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, lift=0.0, up=None, live_in=None):
    """-> dict of REACH_KEYS and "swinging", by lrm_reach_dist_posed_cpu on the library's sample poses and the restated feet"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, F).reshape(-1, 14)
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    nl, ne, nt = len(legs), len(ea), len(targets)
    ffrom, fto = np.asarray(ffrom, np.int64).reshape(nl, ne), np.asarray(fto, np.int64).reshape(nl, ne)
    live, swinging = swinging_of(nt, len(quats), ea, eb, ffrom, fto, live_in)
    out = {"mask": np.zeros((nl, ne), np.uint64), "reached": np.full((nl, ne), -1, np.int32), "first_miss": np.full((nl, ne), -1, np.int32),
           "worst": np.full((nl, ne), -1, np.int32), "worst_d2": np.zeros((nl, ne), F)}
    ls, es = np.nonzero(swinging)
    if len(ls):
        smp = lrm.dbg_edge_transit_samples_host(quats, body, ea, eb, S)  # [ne, S, 7]
        _, feet = path_np(targets[ffrom[ls, es]], targets[fto[ls, es]], S, lift, up)
        pose = (es[:, None] * S + np.arange(S)[None, :]).reshape(-1).astype(np.int32)
        leg = np.repeat(ls, S).astype(np.uint8)
        m, _, d, _ = lrm.apply_reach_dist_posed_cpu(feet.reshape(-1, 3), pose, leg, smp[..., :4].reshape(-1, 4), smp[..., 4:].reshape(-1, 3), legs)
        r = m.reshape(-1, S) != 0
        d = d.reshape(-1, S, 3)
        with np.errstate(all="ignore"):
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.where(np.isnan(d2), F(np.inf), d2).astype(F)
        bit = np.uint64(1) << np.arange(S, dtype=np.uint64)
        miss = ~r
        any_miss = miss.any(1)
        key = np.where(miss, d2, F(-1))
        worst = np.argmax(key, axis=1)  # the first sample at the maximum
        out["mask"][ls, es] = (r * bit[None, :]).sum(1, dtype=np.uint64)
        out["reached"][ls, es] = r.sum(1)
        out["first_miss"][ls, es] = np.where(any_miss, np.argmax(miss, axis=1), -1)
        out["worst"][ls, es] = np.where(any_miss, worst, -1)
        out["worst_d2"][ls, es] = np.where(any_miss, key[np.arange(len(ls)), worst], F(0))
    out["swinging"] = (swinging * (1 << np.arange(nl))[:, None]).sum(0).astype(np.uint8)
    return out


def host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, live_in=None, lift=0.0, up=None, foot_radius=0.0, margin=0.0,
         skip=0, **kw):
    got = lrm.swing_transit_posed_cpu(targets, quats, body, legs, ea, eb, ffrom, fto, S, lift, up, foot_radius, margin, skip, live_in, **kw)
    return dict(zip(KEYS, got[:11]))


def assert_same(got, want, keys=KEYS):
    """every output equal, the floats bit for bit; a None in got (an output not asked for) is skipped"""
    for k in keys:
        if got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        if k in ("worst_d2", "pen"):
            g, w = pc.bits(g), pc.bits(w)
        elif k == "mask":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def assert_consistent(o, S):
    """what the contract promises of any answer: hits > 0 iff hit_seg >= 0 iff pen > 0; an entry that is not swinging is empty;
    clear is the fold of the per-leg outputs"""
    hits, seg, near, pen = o["hits"], o["hit_seg"], o["near"], o["pen"]
    assert np.array_equal(hits > 0, seg >= 0) and np.array_equal(hits > 0, pen > 0)
    assert np.array_equal(near >= 0, np.isfinite(pen)) and (pen[near < 0] == -np.inf).all()
    nl = hits.shape[0]
    sw = (o["swinging"][None, :] >> np.arange(nl)[:, None]) & 1 != 0
    assert np.array_equal(sw, o["reached"] >= 0)
    assert (hits[~sw] == 0).all() and (seg[~sw] == -1).all() and (near[~sw] == -1).all()
    bad = sw & ((o["reached"] != S) | (hits != 0))
    assert ((o["clear"] == 1) <= ~bad.any(0)).all()


def lift_one(best, ea, eb, lifted=None):
    """foot_from / foot_to [nl, ne] from footholds' best [nl, nposes]: edge e lifts leg lifted[e] (default e mod nl), the
    others are -1 -- device.swing_layout's job in numpy"""
    nl, ne = best.shape[0], len(ea)
    lifted = np.arange(ne) % nl if lifted is None else np.asarray(lifted)
    on = np.arange(nl)[:, None] == lifted[None, :]
    ok = (np.asarray(ea) >= 0) & (np.asarray(ea) < best.shape[1]) & (np.asarray(eb) >= 0) & (np.asarray(eb) < best.shape[1])
    a, b = np.where(ok, ea, 0), np.where(ok, eb, 0)
    ffrom = np.where(on, best[:, a], -1).astype(np.int32)
    fto = np.where(on, best[:, b], -1).astype(np.int32)
    return np.ascontiguousarray(ffrom), np.ascontiguousarray(fto)


# the main scene's step: the bump, the foot and what of the ends is left out
MAIN = dict(lift=20.0, foot_radius=12.0, margin=15.0, skip=1)


def main_scene(lrm):
    """transit_cases' main scene (48 poses with a neighbour each, 4000 rough targets, six legs) and per edge one lifted leg that
    goes from its best foothold under pose a to its best foothold under pose b
    -> (quats, body, targets, ea, eb, legs, foot_from, foot_to)"""
    quats, body, targets, ea, eb, legs, nominal = tr.main_scene(lrm)
    _, best, _, _, _ = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)
    ffrom, fto = lift_one(best, ea, eb)
    return quats, body, targets, ea, eb, legs, ffrom, fto


def all_legs_scene(lrm):
    """the main scene with EVERY leg swinging on every edge (from = best under a, to = best under b)"""
    quats, body, targets, ea, eb, legs, nominal = tr.main_scene(lrm)
    _, best, _, _, _ = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)
    return quats, body, targets, ea, eb, legs, np.ascontiguousarray(best[:, ea]), np.ascontiguousarray(best[:, eb])


def hostile_feet(ffrom, fto, nt, seed=1):
    """copies with -1, nt, INT32_MIN, INT32_MAX, nt + 1 and -2 sprinkled over either array of every leg"""
    rng = np.random.default_rng(seed)
    f, t = np.array(ffrom, np.int32), np.array(fto, np.int32)
    bad = np.array([-1, nt, I32.min, I32.max, nt + 1, -2], np.int64)
    for l in range(f.shape[0]):
        for k, arr in enumerate((f, t)):
            idx = rng.choice(f.shape[1], max(1, f.shape[1] // 6), replace=False)
            arr[l, idx] = bad[rng.integers(0, len(bad), len(idx))].astype(np.int32)
    return f, t


def grid_scene(lrm, nt, ne, nl, seed=0, nposes=32, shift=None):
    """a synthetic step scene of any size: nt targets on a jittered 15 mm grid sorted by x (so that tiles and chunks are
    compact strips and a box cull has something to skip), ne edges over nposes gently tilted poses with a neighbour each, and
    per (edge, leg) a take-off target under the body's side and a landing up to eight grid cells away.  Bodies hover 190 mm
    over the ground so that some feet reach and some do not.  shift moves cloud and bodies together.
    -> (quats, body, targets, ea, eb, legs, foot_from, foot_to); every leg swings (lift_some() thins them out)"""
    rng = np.random.default_rng(seed * 7919 + nt + 31 * ne + nl)
    ny = max(1, int(np.ceil(np.sqrt(max(nt, 1)))))
    i = np.arange(nt)
    targets = np.column_stack([(i // ny) * 15.0, (i % ny) * 15.0, np.zeros(nt)]) + rng.uniform(-5, 5, (nt, 3)) * [1, 1, 2]
    legs = np.stack([lrm.get_M2_leg(F(2 * np.pi * k / nl)) for k in range(nl)]).astype(F).reshape(nl, 14)
    q = np.random.default_rng(seed + 1).standard_normal((2 * nposes, 4)) * 0.08
    q[:, 0] = 1.0
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ea = (np.arange(ne) % nposes).astype(np.int32)
    eb = (ea + nposes).astype(np.int32)
    side = max(ny * 15.0, 1.0)
    body = np.empty((2 * nposes, 3))
    body[:nposes] = np.column_stack([rng.uniform(0.2, 0.8, nposes) * min(side, (max(nt, 1) // ny + 1) * 15.0), rng.uniform(0.2, 0.8, nposes) * side,
                                     np.full(nposes, 190.0)])
    body[nposes:] = body[:nposes] + rng.uniform(-60, 60, (nposes, 3)) * [1, 1, 0.2]
    ffrom = np.full((nl, ne), -1, np.int32)
    fto = np.full((nl, ne), -1, np.int32)
    if nt:
        ang = 2 * np.pi * np.arange(nl) / nl
        for l in range(nl):
            spot = body[ea][:, :2] + 260.0 * np.column_stack([np.cos(ang[l]), np.sin(ang[l])]) + rng.uniform(-40, 40, (ne, 2))
            ix = np.clip(np.rint(spot[:, 0] / 15.0), 0, max(nt // ny, 0)).astype(np.int64)
            iy = np.clip(np.rint(spot[:, 1] / 15.0), 0, ny - 1).astype(np.int64)
            ffrom[l] = np.clip(ix * ny + iy, 0, nt - 1)
            jx = np.clip(ix + rng.integers(-8, 9, ne), 0, max(nt // ny, 0))
            jy = np.clip(iy + rng.integers(-8, 9, ne), 0, ny - 1)
            fto[l] = np.clip(jx * ny + jy, 0, nt - 1)
    if shift is not None:
        targets, body = targets + np.asarray(shift, np.float64), body + np.asarray(shift, np.float64)
    return q.astype(F), body.astype(F), np.ascontiguousarray(targets, F), ea, eb, legs, ffrom, fto


def lift_some(ffrom, fto, keep=1, seed=0):
    """copies in which each edge keeps `keep` swinging legs (chosen at random) and the others get -1"""
    rng = np.random.default_rng(seed)
    nl, ne = ffrom.shape
    on = np.zeros((nl, ne), bool)
    for e in range(ne):
        on[rng.choice(nl, min(keep, nl), replace=False), e] = True
    return np.where(on, ffrom, -1).astype(np.int32), np.where(on, fto, -1).astype(np.int32)


def nonfinite_scene(scene):
    """the scene with a nan take-off, an infinite landing, a landing that overflows D, three non-finite bystanders, nan and
    zero quaternions and infinite and nan bodies -> (scene, [(leg, edge)] of the three entries with a non-finite path)"""
    quats, body, targets, ea, eb, legs, ffrom, fto = scene
    quats, body, targets = quats.copy(), body.copy(), targets.copy()
    e = np.flatnonzero((ffrom >= 0).any(0) & (fto >= 0).any(0))
    l = np.argmax(ffrom[:, e] >= 0, axis=0)
    targets[ffrom[l[0], e[0]]] = np.nan
    targets[fto[l[1], e[1]], 2] = np.inf
    targets[fto[l[2], e[2]]] = 3e38
    bystander = np.setdiff1d(np.arange(len(targets)), np.concatenate([ffrom.ravel(), fto.ravel()]))[:3]
    targets[bystander] = [[np.nan, 0, 0], [np.inf, -np.inf, 0], [3e38, 3e38, -3e38]]
    quats[ea[e[3]]] = np.nan
    quats[eb[e[4]]] = 0
    body[ea[e[5]]] = np.inf
    body[eb[e[6]]] = np.nan
    return (quats, body, targets, ea, eb, legs, ffrom, fto), [(l[k], e[k]) for k in range(3)]
