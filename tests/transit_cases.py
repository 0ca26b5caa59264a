"""Shared cases of the edge transit tests (tests/test_edge_transit_cpu.py, tests/test_gpu_edge_transit.py):

* samples_np: a vectorised numpy float32 restatement of the sampled path, written from include/lrm.h (every operation a
  separate float32 operation in the stated order; samples 0 and S-1 copied, not computed);
* brute: every sample of every planted (edge, leg) as one query of lrm_reach_dist_posed_cpu -- which tests/test_posed_cpu.py
  ties to the oracle -- on a pose table that holds the restated samples, (target[foot], pose e*S + s, leg l); the squared
  distance in numpy float32 and every output folded in numpy;
* the scenes."""
import numpy as np

import foothold_edges_cases as fe
import footholds_posed_cases as fc
import pair_cases as pc
import posed_cases

F = np.float32
KEYS = ("mask", "reached", "first_miss", "worst", "worst_d2", "planted", "clear", "advance")
# S - 1 a power of two: u = s / (S - 1) is exact, so 1 - u is exact and equals (S - 1 - s) / (S - 1): swapping the ends of an
# edge then reverses the samples exactly
REVERSIBLE_S = (2, 3, 5, 9)


def samples_np(quats, body, ea, eb, S):
    """-> (q float32 [E, S, 4], b float32 [E, S, 3], ok bool [E]); rows of an edge with an end out of range are nan"""
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    nposes = len(quats)
    body = np.zeros((nposes, 3), F) if body is None else np.ascontiguousarray(body, F).reshape(-1, 3)
    ea, eb = np.asarray(ea, np.int64), np.asarray(eb, np.int64)
    ok = (ea >= 0) & (ea < nposes) & (eb >= 0) & (eb < nposes)
    a, b = np.where(ok, ea, 0), np.where(ok, eb, 0)
    if nposes == 0:
        return np.full((len(ea), S, 4), np.nan, F), np.full((len(ea), S, 3), np.nan, F), ok
    qa, qb, ba, bb = quats[a], quats[b], body[a], body[b]
    q = np.empty((len(ea), S, 4), F)
    p = np.empty((len(ea), S, 3), F)
    with np.errstate(all="ignore"):
        dot = ((qa[:, 0] * qb[:, 0] + qa[:, 1] * qb[:, 1]) + qa[:, 2] * qb[:, 2]) + qa[:, 3] * qb[:, 3]
        sg = np.where(dot < 0, F(-1), F(1)).astype(F)
        for s in range(S):
            u = F(s) / F(S - 1)
            w = F(1) - u
            m = w * qa + u * (sg[:, None] * qb)
            n2 = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]) + m[:, 3] * m[:, 3]
            q[:, s] = m / np.sqrt(n2)[:, None]
            p[:, s] = ba + u * (bb - ba)
    q[:, 0], p[:, 0] = qa, ba
    q[:, S - 1], p[:, S - 1] = qb, bb
    q[~ok], p[~ok] = np.nan, np.nan
    return q, p, ok


def live_of(nposes, ea, eb, live_in=None):
    ea, eb = np.asarray(ea, np.int64), np.asarray(eb, np.int64)
    live = (ea >= 0) & (ea < nposes) & (eb >= 0) & (eb < nposes)
    if live_in is not None:
        live &= np.asarray(live_in).reshape(-1) != 0
    return live


def brute(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in=None):
    """-> dict of KEYS, by lrm_reach_dist_posed_cpu on the restated samples and numpy folds"""
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, F).reshape(-1, 14)
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    nl, ne, nt = len(legs), len(ea), len(targets)
    foot = np.asarray(foot, np.int64).reshape(nl, ne)
    live = live_of(len(quats), ea, eb, live_in)
    planted = live[None, :] & (foot >= 0) & (foot < nt)
    out = {"mask": np.zeros((nl, ne), np.uint64), "reached": np.full((nl, ne), -1, np.int32), "first_miss": np.full((nl, ne), -1, np.int32),
           "worst": np.full((nl, ne), -1, np.int32), "worst_d2": np.zeros((nl, ne), F)}
    ls, es = np.nonzero(planted)
    if len(ls):
        q, p, _ = samples_np(quats, body, ea, eb, S)
        xyz = np.repeat(targets[foot[ls, es]], S, axis=0)
        pose = (es[:, None] * S + np.arange(S)[None, :]).reshape(-1).astype(np.int32)
        leg = np.repeat(ls, S).astype(np.uint8)
        m, _, d, _ = lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, q.reshape(-1, 4), p.reshape(-1, 3), legs)
        r = m.reshape(-1, S) != 0
        d = d.reshape(-1, S, 3)
        with np.errstate(all="ignore"):
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.where(np.isnan(d2), F(np.inf), d2).astype(F)
        bit = np.uint64(1) << np.arange(S, dtype=np.uint64)
        mask = (r * bit[None, :]).sum(1, dtype=np.uint64)
        miss = ~r
        any_miss = miss.any(1)
        key = np.where(miss, d2, F(-1))
        worst = np.argmax(key, axis=1)  # the first sample at the maximum
        out["mask"][ls, es] = mask
        out["reached"][ls, es] = r.sum(1)
        out["first_miss"][ls, es] = np.where(any_miss, np.argmax(miss, axis=1), -1)
        out["worst"][ls, es] = np.where(any_miss, worst, -1)
        out["worst_d2"][ls, es] = np.where(any_miss, key[np.arange(len(ls)), worst], F(0))
    fm = np.where(planted & (out["first_miss"] >= 0), out["first_miss"], S)
    out["planted"] = (planted * (1 << np.arange(nl))[:, None]).sum(0).astype(np.uint8)
    out["clear"] = (live & (fm == S).all(0)).astype(np.uint8)
    out["advance"] = np.where(live, fm.min(0), 0).astype(np.int32)
    return out


def host(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in=None, **kw):
    got = lrm.edge_transit_posed_cpu(targets, quats, body, legs, ea, eb, foot, S, live_in, **kw)
    return dict(zip(KEYS, got[:8]))


def assert_same(got, want):
    """every output equal, worst_d2 bit for bit; a None in got (an output not asked for) is skipped"""
    for k in KEYS:
        if got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        if k == "worst_d2":
            g, w = pc.bits(g), pc.bits(w)
        elif k == "mask":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def foot_of(lrm, targets, quats, body, legs, nominal, ea, eb):
    """foothold_edges' best as it stands, and its all_legs"""
    _, best, _, all_legs, _ = lrm.foothold_edges_posed_cpu(targets, quats, body, legs, ea, eb, nominal)
    return best, all_legs


def m2_legs(lrm):
    return np.ascontiguousarray(pc.leg_families(lrm)["m2_6_tilted"][0], F).reshape(-1, 14)


def main_scene(lrm, rotate=True):
    """(quats, body, targets, edge_a, edge_b, legs, nominal): 48 poses over footholds_posed_cases' rough cloud, each with a
    neighbour 50-150 mm away; gently tilted unit quaternions (0.8 identity + 0.2 random, renormalised), the neighbour of an odd
    pose with the next pose's quaternion; rotate=False: pure translation (the neighbour keeps the quaternion)"""
    _, body, targets = fc.scene(lrm, 48, 4000, seed=13)
    q = posed_cases.random_unit_quats(48, np.random.default_rng(13)).astype(np.float64)
    q *= np.where(q[:, :1] < 0, -1.0, 1.0)
    q = 0.2 * q
    q[:, 0] += 0.8
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    quats, body = fe.with_neighbours(q.astype(F), body, 13, 50.0, 150.0)
    ea, eb = fe.edges_of(48, 13, extra=False)
    if not rotate:
        quats[eb] = quats[ea]
    return quats, body, targets, ea, eb, m2_legs(lrm), pc.nominal_for(6)


def hostile_feet(foot, nt, seed=1):
    """a copy of foot with -1, nt, INT32_MIN, INT32_MAX and nt + 1 sprinkled over every leg"""
    rng = np.random.default_rng(seed)
    f = np.array(foot, np.int32)
    bad = np.array([-1, nt, np.iinfo(np.int32).min, np.iinfo(np.int32).max, nt + 1, -2], np.int64)
    for l in range(f.shape[0]):
        idx = rng.choice(f.shape[1], max(1, f.shape[1] // 4), replace=False)
        f[l, idx] = bad[rng.integers(0, len(bad), len(idx))].astype(np.int32)
    return f


def hostile_edges(ea, eb, nposes, where):
    """copies of (ea, eb) with an index out of range at the given edge positions, in turn -1, nposes, INT32_MIN, INT32_MAX"""
    a, b = np.array(ea, np.int32), np.array(eb, np.int32)
    bad = [-1, nposes, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    for k, e in enumerate(where):
        (a if k % 2 == 0 else b)[e] = bad[k % 4]
    return a, b
