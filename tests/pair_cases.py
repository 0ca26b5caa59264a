"""Shared cases of the body x target x leg ("pair") tests (tests/test_pair_cpu.py, tests/test_gpu_pair_shapes.py): a
brute-force reference built on the oracle alone, the leg families and orientations, and the scenes that aim at the four
ways the pair kernels skip work (body reach radius, per-leg bounding sphere, tile / chunk boxes, the survivor queue).

The reference never skips anything: oracle.reach_pairs evaluates reachable_rotate_leg for every (leg, body, target), and
count / argmin / d2 follow footholds_cases.expected (numpy float32, no contraction, first occurrence of the minimum
among the reachable targets), one block of targets at a time so that 2e5-target clouds fit in memory."""
import numpy as np

from footholds_cases import QUATS, scene as rough_scene  # noqa: F401
from ik_cases import random_legs
from posed_cases import fixture_quats

# LegDimensions field order (include/lrm.h)
BODY, COXA_LEN, TIBIA_LEN, FEMUR_LEN = 1, 3, 4, 5
MAX_TRIPLES = 3e8  # per brute-force call; the oracle takes about 0.16 us per (leg, body, target)


# ---- reference ------------------------------------------------------------------------------------------------------
def brute(oracle, bodies, targets, legs, quat=None, nominal=None):
    """-> dict(count, best, first (the smallest reachable index) int32[L, B], best_d2 float32[L, B], any uint8[L, B]) from
    the oracle alone"""
    bodies = np.ascontiguousarray(bodies, np.float32).reshape(-1, 3)
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    q = (1, 0, 0, 0) if quat is None else quat
    nl, nb, nt = len(legs), len(bodies), len(targets)
    assert nl * nb * nt <= MAX_TRIPLES, "brute force too large: use the host loop validated by tests/test_pair_cpu.py"
    nom = np.zeros((nl, 3), np.float32) if nominal is None else np.asarray(nominal, np.float32).reshape(nl, 3)
    count = np.zeros((nl, nb), np.int64)
    best = np.full((nl, nb), -1, np.int64)
    best_d2 = np.full((nl, nb), np.inf, np.float32)
    first_hit = np.full((nl, nb), -1, np.int64)  # the smallest reachable index
    step = max(64, int(4e6 // max(nb, 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for t0 in range(0, nt, step):
            tg = targets[t0:t0 + step]
            reach = oracle.reach_pairs(bodies, tg, legs, q).astype(bool)  # [L, B, T]
            for l in range(nl):
                c = bodies + nom[l]                                         # one f32 add per component
                d = tg[None, :, :] - c[:, None, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                r = reach[l]
                has = r.any(-1)
                masked = np.where(r, d2, np.float32(np.inf))
                mn = masked.min(-1)
                first = np.argmax(r & (masked == mn[:, None]), axis=-1)     # first reachable target at the minimum
                fresh = has & (count[l] == 0)
                first_hit[l][fresh] = t0 + np.argmax(r, axis=-1)[fresh]
                take = has & ((count[l] == 0) | (mn < best_d2[l]))          # a later block wins only when strictly nearer
                best[l][take] = t0 + first[take]
                best_d2[l][take] = mn[take]
                count[l] += r.sum(-1)
    return {"count": count.astype(np.int32), "best": best.astype(np.int32), "best_d2": best_d2,
            "any": (count > 0).astype(np.uint8), "first": first_hit.astype(np.int32)}


def any_in_sphere(centres, pts, radius):
    """collision.cu.h:5-10 in float32, the operation order of tests/test_gpu_positionability.py; blocks of centres"""
    out = np.zeros(len(centres), bool)
    step = max(1, int(4e6 // max(len(pts), 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, len(centres), step):
            d = centres[c0:c0 + step, None, :] - pts[None, :, :]
            out[c0:c0 + step] = (np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                                 < np.float32(radius)).any(1)
    return out


def any_in_cylinder(centres, pts, radius, plus_z, minus_z):
    """collision.cu.h:12-23 in float32; blocks of centres"""
    out = np.zeros(len(centres), bool)
    step = max(1, int(4e6 // max(len(pts), 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, len(centres), step):
            d = pts[None, :, :] - centres[c0:c0 + step, None, :]
            rad = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + np.float32(0)) < np.float32(radius)
            out[c0:c0 + step] = (rad & (d[..., 2] < np.float32(plus_z)) & (d[..., 2] > np.float32(minus_z))).any(1)
    return out


def assert_both_outcomes(ref):
    """a scene must hold empty, occupied and crowded (leg, body) pairs, by the oracle alone"""
    c = ref["count"]
    assert (c > 0).any() and (c == 0).any() and (c > 2).any(), (int((c > 0).sum()), int((c == 0).sum()), int(c.max()))


def body_radius(leg):
    """the body reach radius of the pair kernels as lrm_types.h documents it: stretched leg + 1 mm, 1e-4 relative slack
    on the square -> r^2 in float32 arithmetic"""
    leg = np.asarray(leg, np.float32)
    reach = np.float32(leg[BODY] + leg[COXA_LEN]) + leg[FEMUR_LEN]
    reach = np.float32(np.float32(reach + leg[TIBIA_LEN]) + np.float32(1.0))
    return np.float32(np.float32(reach * reach) * np.float32(1.0001))


def filter_eligible(lrm, leg, quat=None):
    """fast_ok of lrm_compile_leg: the filtered host evaluation refuses an ineligible leg"""
    try:
        lrm.dbg_fused_reach_host(np.zeros((1, 3), np.float32), leg, quat)
        return True
    except lrm.LrmError:
        return False


# ---- legs and orientations ------------------------------------------------------------------------------------------
def quats():
    """identity, the tilted unit quaternion of footholds_cases, and the first fixture quaternion that is not unit"""
    nonunit = next(q for q in fixture_quats() if abs(float(np.linalg.norm(q.astype(np.float64))) - 1.0) > 1e-3)
    return {"identity": np.array(QUATS["identity"], np.float32), "tilted": np.array(QUATS["tilted"], np.float32),
            "nonunit": np.asarray(nonunit, np.float32)}


def _rotated(lrm, legs, quat):
    return np.stack([lrm.rotate_leg_data(quat, leg) for leg in legs]).astype(np.float32)


def short_leg(lrm, az):
    return lrm.leg_factory(az, 60.0, -10.0, 30.0, 70.0, 80.0, 60.0, 80.0, 110.0, 0.0, 0.0)


def long_leg(lrm, az):
    return lrm.leg_factory(az, 240.0, -20.0, 90.0, 160.0, 170.0, 70.0, 90.0, 130.0, -5.0, 5.0)


def wide_leg(lrm, az, coxa_deg=130.0):
    """coxa half-range above 87 degrees: the bounding sphere falls back to the whole ball"""
    return lrm.leg_factory(az, 150.0, -30.0, 60.0, 120.0, 130.0, coxa_deg, 80.0, 115.0, -5.0, 0.0)


def leg_families(lrm):
    """name -> (legs [n, 14] as the calls take them (rotate_leg_data applied), quat)"""
    Q = quats()
    hexa = lambda make, n: [make(np.float32(2 * np.pi * k / n)) for k in range(n)]
    rnd = [leg for _, leg, _ in random_legs(lrm)]
    fam = {}
    for n, qn in ((1, "identity"), (2, "tilted"), (3, "nonunit"), (5, "identity"), (6, "tilted"), (7, "nonunit"), (8, "identity")):
        fam[f"m2_{n}_{qn}"] = (hexa(lrm.get_M2_leg, n), Q[qn])
    for n, qn in ((6, "identity"), (3, "tilted"), (5, "nonunit")):
        fam[f"moonbot_{n}_{qn}"] = (hexa(lrm.get_moonbot_leg, n), Q[qn])
    fam["random_8_identity"] = (rnd[:8], Q["identity"])       # legs 0, 3, 6: coxa half-range 95-150 degrees
    fam["random_7_tilted"] = (rnd[5:12], Q["tilted"])
    fam["random_wide_3_nonunit"] = (rnd[0:12:3][:3], Q["nonunit"])
    fam["random_2_tilted"] = ([rnd[9], rnd[10]], Q["tilted"])
    # short and long legs in one call (r2max is the long leg's), one wide (filter-ineligible) leg among eligible ones
    fam["mixed_5_tilted"] = ([short_leg(lrm, 0.3), long_leg(lrm, 2.2), wide_leg(lrm, -1.4), lrm.get_M2_leg(1.2),
                              short_leg(lrm, -2.6)], Q["tilted"])
    fam["mixed_2_identity"] = ([short_leg(lrm, 0.0), long_leg(lrm, 3.0)], Q["identity"])
    return {k: (_rotated(lrm, legs, q), q) for k, (legs, q) in fam.items()}


def nominal_for(nlegs, seed=3):
    return np.random.default_rng(seed).uniform(-250, 250, (nlegs, 3)).astype(np.float32)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def rough(nb, nt, seed, density_half=900.0, sort_x=False):
    """footholds_cases.scene at the density of 20 000 targets on a +-900 mm patch; sort_x puts the cloud in x order, so
    that a body at large x reaches only the last tiles; every fifth body is lifted out of reach"""
    half = density_half * max(1.0, np.sqrt(nt / 20000.0))
    bodies, targets = rough_scene(nb, nt, seed, half=half)
    bodies[4::5, 2] += np.float32(900.0)  # every fifth body hovers out of every leg's reach
    if sort_x and nt:
        targets = np.ascontiguousarray(targets[np.argsort(targets[:, 0], kind="stable")])
    return bodies, targets


def sized(nb, nt, split, seed):
    """rough(sort_x) up to `split` targets; beyond it the targets past index `split` form a second patch 30 m away and a
    third of the bodies hover around THAT patch (150-350 mm beside one of its targets, 100-250 mm above it), so their
    answers come from the targets behind `split` alone"""
    if nt <= split:
        return rough(nb, nt, seed, sort_x=True)
    rng = np.random.default_rng(seed + 1)
    bodies, first = rough(nb, split, seed, sort_x=True)
    _, extra = rough(1, nt - split, seed + 2, sort_x=True)
    extra = extra + np.array([3e4, 2e4, 0], np.float32)
    k = nb // 3
    at = extra[rng.integers(0, len(extra), k)]
    ang, rad = rng.uniform(0, 2 * np.pi, k), rng.uniform(150, 350, k)
    bodies[:k] = np.column_stack([at[:, 0] + rad * np.cos(ang), at[:, 1] + rad * np.sin(ang),
                                  at[:, 2] + rng.uniform(100, 250, k)]).astype(np.float32)
    return bodies, np.ascontiguousarray(np.concatenate([first, extra]))


def raster(lrm, n_side, nb, seed=3):
    """(bodies, {raster, shuffled, morton: (targets, order)}): workloads.terrain in three memory orders;
    targets == ground[order]"""
    from lrm_amd import workloads
    ground = workloads.terrain(n_side)
    bodies = workloads.body_lattice(ground, nb, seed=seed)
    orders = {"raster": np.arange(len(ground)), "shuffled": np.random.default_rng(seed).permutation(len(ground)),
              "morton": lrm.morton_order(ground)}
    return bodies, {k: (np.ascontiguousarray(ground[o]), o) for k, o in orders.items()}


def dense_cluster(nb, nt, seed):
    """a 200 x 200 x 60 mm block of targets inside every body's reach radius (M2: 511 mm), bodies 120-260 mm from its
    centre: 64 of 64 lanes survive the radius test chunk after chunk.  One far target in the first chunk leaves 63 in
    the queue, so every later full chunk fills it to 127 and the move-to-front copy carries 63 entries; far targets
    sprinkled behind index 2048 walk the remainder through the other lengths."""
    rng = np.random.default_rng(seed)
    targets = (rng.uniform(-1, 1, (nt, 3)) * [100.0, 100.0, 30.0]).astype(np.float32)
    far = np.zeros(nt, bool)
    far[5] = True
    far[2048:] = rng.random(max(nt - 2048, 0)) < 0.03
    targets[far] += np.float32(5000.0)
    ang = rng.uniform(0, 2 * np.pi, nb)
    rad = rng.uniform(120, 260, nb)
    bodies = np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(60, 180, nb)]).astype(np.float32)
    return bodies, targets


def sparse_tiles(nb, ntiles, seed):
    """every 1024-target tile holds one populated 64-target chunk (chunk (3 * tile) % 16) of rough terrain and fifteen
    chunks 1e5 mm away: the tile box is huge, only the chunk boxes can skip"""
    rng = np.random.default_rng(seed)
    nt = ntiles * 1024
    bodies, near = rough_scene(nb, ntiles * 64, seed, half=500.0)
    targets = (rng.uniform(-300, 300, (nt, 3)) + [1e5, -1e5, 2e4]).astype(np.float32)
    for tile in range(ntiles):
        c0 = tile * 1024 + ((3 * tile) % 16) * 64
        targets[c0:c0 + 64] = near[tile * 64:(tile + 1) * 64]
    return bodies, targets


def repeated(targets, k):
    return np.ascontiguousarray(np.concatenate([targets] * k))


def with_spread_duplicates(targets, seed, extra=None):
    """the cloud followed by a shuffled second copy of itself: every target has a twin in another lane, chunk and (for
    long clouds) tile or 64-tile group.  -> (cloud, twin_of[i] = index of the other copy)"""
    n = len(targets)
    perm = np.random.default_rng(seed).permutation(n)
    cloud = np.ascontiguousarray(np.concatenate([targets, targets[perm]]))
    twin = np.empty(2 * n, np.int64)
    twin[perm] = n + np.arange(n)
    twin[n + np.arange(n)] = perm
    return cloud, twin


def translated(bodies, targets, offset):
    """bodies and targets moved together by `offset` mm along (1, -1, 0.25), rounded to float32: the reference is the
    brute force on THESE arrays"""
    off = np.array([offset, -offset, 0.25 * offset], np.float64)
    return (bodies.astype(np.float64) + off).astype(np.float32), (targets.astype(np.float64) + off).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
