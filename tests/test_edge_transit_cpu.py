"""Planted-foot reach along pose transitions on the host (lrm_edge_transit_posed_cpu, include/lrm.h; no GPU): the host loop --
the reference of tests/test_gpu_edge_transit.py -- against transit_cases.brute (lrm_reach_dist_posed_cpu on a numpy float32
restatement of the sampled path, folded in numpy) bit for bit on every output; the end samples against the posed call on the
two poses; the consequences of the definition; non-vacuity decided by the brute force alone; forms, bad indices and refusals;
and the float32 path against tests/transit_model64.py, an independent float64 model, measured on 100 000 random edges and
asserted at four times the measured worst."""
import ctypes as C

import numpy as np
import pytest

import foothold_edges_cases as fe
import pair_cases as pc
import transit_cases as tr
import transit_model64 as t64
from test_pair_cpu import FAMILIES

F = np.float32
LRM_EINVAL = -1
ALL_S = (2, 3, 9, 33, 64)

# Worst deviation of the host's float32 samples from the float64 model over transit_model64.random_edges (seed 0; arcs of 0 to
# just under 90 degrees of quaternion angle, half of them given the long way round; bodies to 4e6 mm), per S, measured:
#            unit     plane    range    order    angle    segment  body
#   S = 3    1.3e-7   8.8e-8   0        0        7.9e-8   5.8e-8   5.9e-8     (100 000 edges)
#   S = 9    1.3e-7   1.1e-7   1.6e-8   6.6e-8   1.1e-7   1.2e-7   1.4e-7     (100 000 edges)
#   S = 64   1.5e-7   1.2e-7   3.0e-8   8.6e-8   1.5e-7   1.7e-7   1.7e-7     (100 000 edges)
# (quaternion figures absolute on unit quaternions, angles in radians, body figures relative to max(|ba|, |bb|, 1)).  The bands
# are four times the worst of a column, one digit; tests/test_gpu_edge_transit.py holds the device to the same bands.
BANDS = {"unit": 6e-7, "plane": 5e-7, "range": 1e-7, "order": 3e-7, "angle": 6e-7, "segment": 7e-7, "body": 7e-7}


def check(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in=None):
    """the host loop against the brute force, bit for bit -> the brute force's answer"""
    want = tr.brute(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in)
    tr.assert_same(tr.host(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in), want)
    return want


@pytest.fixture(scope="module")
def main(lrm):
    """the main scene with foothold_edges' own choice: (quats, body, targets, ea, eb, legs, foot, all_legs)"""
    quats, body, targets, ea, eb, legs, nominal = tr.main_scene(lrm)
    foot, all_legs = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    return quats, body, targets, ea, eb, legs, foot, all_legs


@pytest.mark.parametrize("S", ALL_S)
def test_host_loop_matches_bruteforce_on_the_main_scene(lrm, main, S):
    quats, body, targets, ea, eb, legs, foot, _ = main
    want = check(lrm, targets, quats, body, legs, ea, eb, foot, S)
    pl = want["reached"] >= 0
    # foothold_edges chose targets reachable under both ends: bits 0 and S - 1 of every planted entry are set
    assert pl.any() and ((want["mask"][pl] & np.uint64(1)) == 1).all() and (((want["mask"][pl] >> np.uint64(S - 1)) & np.uint64(1)) == 1).all()
    assert np.array_equal(pl, foot >= 0)


def test_main_scene_is_not_vacuous(lrm, main):
    """by the brute force alone, at S = 9.  The restated scene gives 205 planted entries of 288, 31 that lose the chosen
    foothold at an interior sample and 174 that keep it; of the 21 edges foothold_edges calls feasible 9 are clear and 12 are
    not; worst != first_miss at 28 losing entries and worst == first_miss at 3.  The floors are half of these."""
    quats, body, targets, ea, eb, legs, foot, all_legs = main
    want = tr.brute(lrm, targets, quats, body, legs, ea, eb, foot, 9)
    pl = want["reached"] >= 0
    lose = pl & (want["reached"] < 9)
    feasible = all_legs != 0
    assert lose.sum() >= 15 and (pl & ~lose).sum() >= 87
    assert (feasible & (want["clear"] != 0)).sum() >= 4 and (feasible & (want["clear"] == 0)).sum() >= 6
    assert (lose & (want["worst"] != want["first_miss"])).sum() >= 14 and (lose & (want["worst"] == want["first_miss"])).sum() >= 1
    # the excursions are millimetres, not rounding
    assert np.sqrt(want["worst_d2"][lose].astype(np.float64)).max() > 5.0
    # advance: between 1 and 8 on a feasible edge that is not clear, 9 on a clear one
    assert (want["advance"][feasible & (want["clear"] == 0)] >= 1).all() and (want["advance"][feasible & (want["clear"] == 0)] <= 8).all()
    assert (want["advance"][want["clear"] != 0] == 9).all()


def test_pure_translation_loses_feet_too(lrm):
    """b's quaternion := a's: the restated scene gives 209 planted, 28 losing entries; floor at half"""
    quats, body, targets, ea, eb, legs, nominal = tr.main_scene(lrm, rotate=False)
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    want = check(lrm, targets, quats, body, legs, ea, eb, foot, 9)
    assert ((want["reached"] >= 0) & (want["reached"] < 9)).sum() >= 14


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, family):
    """foothold_edges_cases.scene as it stands: its pool has non-unit and nan quaternions at one end and at both, reversed,
    a == b, duplicate and far edges"""
    legs, _ = pc.leg_families(lrm)[family]
    legs = np.ascontiguousarray(legs, F).reshape(-1, 14)
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=len(family) + len(legs))
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, pc.nominal_for(len(legs)), ea, eb)
    for S in (3, 9):
        want = check(lrm, targets, quats, body, legs, ea, eb, foot, S)
    nan = np.isnan(quats).any(1)
    assert nan.any() and (want["reached"][:, nan[ea] | nan[eb]] == -1).all()  # foothold_edges plants nothing under a nan pose
    # feet of its own choosing under hostile poses: every leg takes target e % nt, so nan and non-unit ends are evaluated
    own = np.tile(np.arange(len(ea), dtype=np.int32) % len(targets), (len(legs), 1))
    want = check(lrm, targets, quats, body, legs, ea, eb, own, 9)
    assert (want["reached"][:, nan[ea] | nan[eb]] >= 0).all() and (want["reached"][:, nan[ea] & nan[eb]] == 0).all()


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
@pytest.mark.parametrize("S", ALL_S)
def test_host_loop_matches_bruteforce_on_every_scene(lrm, kind, S):
    legs = tr.m2_legs(lrm)
    quats, body, targets, ea, eb = fe.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind)
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, pc.nominal_for(6, seed=5), ea, eb)
    want = check(lrm, targets, quats, body, legs, ea, eb, foot, S)
    assert (want["reached"] >= 0).any()


@pytest.mark.parametrize("S", ALL_S)
def test_end_samples_equal_the_posed_call_on_the_two_poses(lrm, main, S):
    """samples 0 and S - 1 are lrm_reach_dist_posed_cpu's answers for (target, pose a, leg) and (target, pose b, leg); the feet
    are random targets, so that both outcomes occur at both ends"""
    quats, body, targets, ea, eb, legs, _, _ = main
    nl, ne = len(legs), len(ea)
    foot = np.random.default_rng(S).integers(0, len(targets), (nl, ne)).astype(np.int32)
    near = np.argmin(np.linalg.norm(targets[None, :, :2] - body[ea][:, None, :2], axis=2), axis=1)
    foot[:, ::2] = near[None, ::2]  # a target under the body: within reach of some legs
    got = tr.host(lrm, targets, quats, body, legs, ea, eb, foot, S)
    leg = np.repeat(np.arange(nl), ne).astype(np.uint8)
    for pose, bit in ((np.tile(ea, nl), 0), (np.tile(eb, nl), S - 1)):
        m, _, _, _ = lrm.apply_reach_dist_posed_cpu(targets[foot.reshape(-1)], pose.astype(np.int32), leg, quats, body, legs)
        assert np.array_equal(m.reshape(nl, ne), ((got["mask"] >> np.uint64(bit)) & np.uint64(1)).astype(np.uint8))
        assert m.any() and not m.all()


def test_equal_ends_make_every_sample_equal(lrm, main):
    quats, body, targets, ea, _, legs, foot, _ = main
    for S in ALL_S:
        want = check(lrm, targets, quats, body, legs, ea, ea, foot, S)
        full = np.uint64(2 ** S - 1)
        pl = want["reached"] >= 0
        assert pl.any() and np.isin(want["mask"][pl], [np.uint64(0), full]).all()
    # with feet that some legs do not reach, both all ones and all zeros occur
    own = np.tile(foot[0], (len(legs), 1))
    want = check(lrm, targets, quats, body, legs, ea, ea, own, 9)
    pl = want["reached"] >= 0
    assert set(np.unique(want["reached"][pl])) == {0, 9}
    # the interior samples are the pose's quaternion NORMALISED (w*q + u*q over its norm): equal to the ends up to rounding,
    # not bit for bit, so worst may name any sample, and its d2 is that of sample 0 up to rounding
    none = want["reached"] == 0
    assert (want["worst"][none] >= 0).all() and (want["worst"][none] < 9).all()
    d0 = tr.brute(lrm, targets, quats, body, legs, ea, ea, own, 2)["worst_d2"]
    assert np.allclose(want["worst_d2"][none], d0[none], rtol=1e-3)


@pytest.mark.parametrize("S", tr.REVERSIBLE_S)
def test_swapped_ends_reverse_the_mask(lrm, main, S):
    """where S - 1 is a power of two u = s / (S - 1) is exact, 1 - u is exact and equal to (S - 1 - s) / (S - 1), and the blend
    w*qa + u*(sg*qb) is the same float either way round (the addition commutes): sample s of (b, a) is sample S - 1 - s of
    (a, b) bit for bit, up to the body, whose blend ba + u*(bb - ba) is not symmetric -- so the scene here keeps one body"""
    quats, body, targets, ea, eb, legs, foot, _ = main
    body = body.copy()
    body[eb] = body[ea]
    fwd = check(lrm, targets, quats, body, legs, ea, eb, foot, S)
    rev = check(lrm, targets, quats, body, legs, eb, ea, foot, S)
    flipped = np.zeros_like(fwd["mask"])
    for s in range(S):
        flipped |= ((fwd["mask"] >> np.uint64(s)) & np.uint64(1)) << np.uint64(S - 1 - s)
    assert np.array_equal(rev["mask"], flipped) and np.array_equal(rev["reached"], fwd["reached"])
    lose = (fwd["reached"] >= 0) & (fwd["reached"] < S)
    assert lose.any() or S == 2
    assert np.array_equal(pc.bits(rev["worst_d2"]), pc.bits(fwd["worst_d2"]))


def test_live_in_forms(lrm, main):
    quats, body, targets, ea, eb, legs, foot, _ = main
    ne = len(ea)
    base = check(lrm, targets, quats, body, legs, ea, eb, foot, 9)
    ones = check(lrm, targets, quats, body, legs, ea, eb, foot, 9, np.full(ne, 7, np.uint8))
    tr.assert_same(ones, base)
    live = (np.arange(ne) % 3 != 1).astype(np.uint8)
    part = check(lrm, targets, quats, body, legs, ea, eb, foot, 9, live)
    dead = live == 0
    assert (part["reached"][:, dead] == -1).all() and (part["first_miss"][:, dead] == -1).all() and (part["worst"][:, dead] == -1).all()
    assert (part["mask"][:, dead] == 0).all() and (part["worst_d2"][:, dead] == 0).all()
    assert (part["planted"][dead] == 0).all() and (part["clear"][dead] == 0).all() and (part["advance"][dead] == 0).all()
    for k in tr.KEYS:
        assert np.array_equal(part[k][..., ~dead], base[k][..., ~dead]), k
    none = check(lrm, targets, quats, body, legs, ea, eb, foot, 9, np.zeros(ne, np.uint8))
    assert (none["reached"] == -1).all() and (none["clear"] == 0).all()


def test_feet_in_the_air_and_out_of_range_at_every_leg(lrm, main):
    quats, body, targets, ea, eb, legs, foot, _ = main
    bad = tr.hostile_feet(foot, len(targets))
    want = check(lrm, targets, quats, body, legs, ea, eb, bad, 9)
    out = (bad < 0) | (bad >= len(targets))
    assert out.any(1).all() and (want["reached"][out] == -1).all() and (want["reached"][~out] >= 0).all()
    assert np.array_equal(want["planted"], ((~out) * (1 << np.arange(len(legs)))[:, None]).sum(0).astype(np.uint8))
    # an edge with no planted leg is clear, and advance is S
    none = check(lrm, targets, quats, body, legs, ea, eb, np.full_like(foot, -1), 9)
    assert (none["planted"] == 0).all() and (none["clear"] == 1).all() and (none["advance"] == 9).all()
    # a single planted leg, the first or the last, decides clear and advance alone
    for l in (0, len(legs) - 1):
        one = np.full_like(foot, -1)
        one[l] = np.where(foot[l] >= 0, foot[l], 0)
        want = check(lrm, targets, quats, body, legs, ea, eb, one, 9)
        assert (want["planted"] == 1 << l).all()
        assert np.array_equal(want["clear"], (want["reached"][l] == 9).astype(np.uint8))
        assert np.array_equal(want["advance"], np.where(want["first_miss"][l] >= 0, want["first_miss"][l], 9))
        assert (want["clear"] == 0).any() and (want["clear"] == 1).any()


def test_bad_edges(lrm, main):
    quats, body, targets, ea, eb, legs, foot, _ = main
    where = [0, 3, 5, 7, 9, len(ea) - 1]
    a, b = tr.hostile_edges(ea, eb, len(quats), where)
    a[11], b[11] = np.iinfo(np.int32).max, -7
    want = check(lrm, targets, quats, body, legs, a, b, foot, 9)
    bad = where + [11]
    assert (want["reached"][:, bad] == -1).all() and (want["mask"][:, bad] == 0).all()
    assert (want["planted"][bad] == 0).all() and (want["clear"][bad] == 0).all() and (want["advance"][bad] == 0).all()


def test_degenerate_interior_quaternions_are_evaluated_as_they_come(lrm, main):
    """antipodal ends (the sign turns -q into q: the blend stays q), zero ends (n2 = 0: 0 / 0), nan, inf, huge (n2 = inf) and
    tiny quaternions: the host loop equals lrm_reach_dist_posed_cpu on the same four floats"""
    _, body, targets, ea, eb, legs, foot, _ = main
    rng = np.random.default_rng(5)
    quats = np.zeros((len(body), 4), F)
    quats[:, 0] = 1
    pool = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0], [3e38, 3e38, 0, 0],
                     [1e-30, 0, 1e-30, 0], [0, 1, 0, 0], [0, -1, 0, 0], [2, 0, 0, 0.5], [1e20, 0, 0, -1e20]], F)
    quats[ea] = pool[rng.integers(0, len(pool), len(ea))]
    quats[eb] = pool[rng.integers(0, len(pool), len(eb))]
    quats[ea[:4]], quats[eb[:4]] = pool[[0, 7, 9, 2]], pool[[1, 8, 0, 2]]
    own = np.where(foot >= 0, foot, 0)
    with np.errstate(all="ignore"):
        for S in (3, 9, 64):
            check(lrm, targets, quats, body, legs, ea, eb, own, S)
    with np.errstate(all="ignore"):
        q, _, _ = tr.samples_np(quats, None, ea[:4], eb[:4], 3)
    assert np.array_equal(q[0, 1], pool[0]) and np.isnan(q[3, 1]).all()  # -q is q; 0 / sqrt(0)


def test_far_bodies_and_nonfinite_bodies_and_targets(lrm, main):
    quats, body, targets, ea, eb, legs, foot, _ = main
    body, targets = body.copy(), targets.copy()
    body[ea[0]] = np.nan
    body[eb[1]] = np.inf
    body[ea[2]] += F(4e6)
    targets[foot[0, 3]] = np.nan
    targets[foot[1, 4]] = -np.inf
    with np.errstate(all="ignore"):
        check(lrm, targets, quats, body, legs, ea, eb, np.where(foot >= 0, foot, 1), 9)
        check(lrm, targets, quats, None, legs, ea, eb, np.where(foot >= 0, foot, 1), 5)  # body NULL = 0


def test_argument_checks_in_order_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(F)
    f = np.zeros(64, F)
    i = np.zeros(64, np.int32)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], F)

    def cpu(nt, nposes, nlegs, nedges, S, tg=p(f), qs=p(q), lg=p(legs), ea=p(i), eb=p(i), ft=p(i), rc=p(i), fm=p(i)):
        return L.lrm_edge_transit_posed_cpu(tg, nt, qs, None, nposes, lg, nlegs, ea, eb, nedges, ft, S, None, None, rc, fm, None, None,
                                            None, None, None, None)

    def gpu(nt, nposes, nlegs, nedges, S, tg=d, qs=d, lg=p(legs), ea=d, eb=d, ft=d, rc=d, fm=d):
        return L.lrm_edge_transit_posed_dev(tg, d, d, nt, qs, None, nposes, lg, nlegs, ea, eb, nedges, ft, S, None, None, rc, fm, None, None,
                                            None, None, None, None)

    # the range checks come first, before nedges == 0 returns: nlegs, then S, then nt / nposes, then nedges * nlegs
    for args in ((4, 1, 0, 0, 9), (4, 1, 9, 0, 9), (4, 1, 6, 0, 1), (4, 1, 6, 0, 0), (4, 1, 6, 0, 65), (2 ** 31, 1, 6, 0, 9),
                 (4, 2 ** 31, 2, 0, 9), (4, 1, 6, (2 ** 32 - 1) // 6 + 1, 9), (4, 1, 1, 2 ** 32, 9)):
        assert cpu(*args) == LRM_EINVAL, args
        assert gpu(*args) == LRM_EINVAL, args
    # the order: the message names the first violated rule
    for args, word in (((2 ** 31, 1, 0, 0, 1), "nlegs"), ((2 ** 31, 1, 6, 0, 1), "nsamples"), ((2 ** 31, 1, 6, 2 ** 32, 9), "INT32_MAX"),
                       ((4, 1, 6, 2 ** 32, 9), "outputs")):
        assert cpu(*args) == LRM_EINVAL and word in L.lrm_last_error().decode(), (args, L.lrm_last_error())
        assert gpu(*args) == LRM_EINVAL and word in L.lrm_last_error().decode(), (args, L.lrm_last_error())
    # nedges == 0: a no-op after the checks, whatever the pointers
    assert L.lrm_edge_transit_posed_cpu(None, 2 ** 31 - 1, None, None, 1, None, 8, None, None, 0, None, 64, None, None, None, None, None, None,
                                        None, None, None, None) == 0
    assert L.lrm_edge_transit_posed_dev(None, None, None, 2 ** 31 - 1, None, None, 1, None, 8, None, None, 0, None, 2, None, None, None, None,
                                        None, None, None, None, None, None) == 0
    # then the NULL forms
    for kw in ({"qs": None}, {"lg": None}, {"ea": None}, {"eb": None}, {"ft": None}, {"rc": None}, {"fm": None}, {"tg": None}):
        assert cpu(4, 1, 2, 1, 9, **kw) == LRM_EINVAL and gpu(4, 1, 2, 1, 9, **kw) == LRM_EINVAL, kw
    # nt == 0 plants nothing, and the cloud may then be NULL
    rc, fm = np.full((2, 3), 9, np.int32), np.full((2, 3), 9, np.int32)
    pl, cl, ad = np.full(3, 9, np.uint8), np.full(3, 9, np.uint8), np.full(3, 9, np.int32)
    e = np.zeros(3, np.int32)
    assert L.lrm_edge_transit_posed_cpu(None, 0, p(q), None, 1, p(legs), 2, p(e), p(e), 3, p(i), 9, None, None, p(rc), p(fm), None, None,
                                        p(pl), p(cl), p(ad), None) == 0
    assert (rc == -1).all() and (fm == -1).all() and (pl == 0).all() and (cl == 1).all() and (ad == 9).all()
    # the wrapper's own checks
    with pytest.raises(ValueError):
        lrm.edge_transit_posed_cpu(np.zeros((4, 3), F), q, None, legs[:2], e, e[:2], np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError):
        lrm.edge_transit_posed_cpu(np.zeros((4, 3), F), q, None, legs[:2], e, e, np.zeros((2, 4), np.int32))
    with pytest.raises(lrm.LrmError):
        lrm.edge_transit_posed_cpu(np.zeros((4, 3), F), q, None, legs[:2], e, e, np.zeros((2, 3), np.int32), nsamples=65)


def test_null_outputs_and_sentinels_behind_the_outputs(lrm, main):
    """the C ABI writes nlegs * nedges (and nedges) entries and nothing behind them; every optional output may be NULL alone"""
    L = lrm.load()
    p = lrm._capi._ptr
    quats, body, targets, ea, eb, legs, foot, _ = main
    nl, ne = foot.shape
    n = nl * ne
    want = tr.host(lrm, targets, quats, body, legs, ea, eb, foot, 9)
    optional = ("mask", "worst", "worst_d2", "planted", "clear", "advance")
    for drop in (None,) + optional + ("all",):
        buf = {"mask": np.full(n + 8, 0xA5A5A5A5A5A5A5A5, np.uint64), "reached": np.full(n + 8, -7, np.int32),
               "first_miss": np.full(n + 8, -7, np.int32), "worst": np.full(n + 8, -7, np.int32), "worst_d2": np.full(n + 8, -7.0, F),
               "planted": np.full(ne + 8, 0xA5, np.uint8), "clear": np.full(ne + 8, 0xA5, np.uint8), "advance": np.full(ne + 8, -7, np.int32)}
        keep = {k: not (k == drop or (drop == "all" and k in optional)) for k in tr.KEYS}
        sent = {k: v.copy() for k, v in buf.items()}
        a = [p(buf[k]) if keep[k] else None for k in tr.KEYS]
        rc = L.lrm_edge_transit_posed_cpu(p(targets), len(targets), p(quats), p(body), len(quats), p(legs), nl, p(ea), p(eb), ne, p(foot), 9,
                                          None, *a, None)
        assert rc == 0, drop
        got = {}
        for k in tr.KEYS:
            m = ne if k in ("planted", "clear", "advance") else n
            if keep[k]:
                got[k] = buf[k][:m].reshape(want[k].shape)
                assert np.array_equal(buf[k][m:].view(np.uint8), sent[k][m:].view(np.uint8)), (drop, k)
            else:
                got[k] = None
                assert np.array_equal(buf[k].view(np.uint8), sent[k].view(np.uint8)), (drop, k)
        tr.assert_same(got, want)


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_edge_transit_posed_dev", "lrm_edge_transit_posed_cpu", "lrm_dbg_edge_transit_samples_host",
             "lrm_dbg_edge_transit_samples_dev"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())


# ---- the path against the independent float64 model ---------------------------------------------------------------------
def test_restated_path_equals_the_hosts_samples_bit_for_bit(lrm):
    qa, qb, ba, bb = t64.random_edges(3000, seed=2)
    n = len(qa)
    quats, body = np.concatenate([qa, qb]), np.concatenate([ba, bb])
    ea, eb = np.arange(n, dtype=np.int32), (n + np.arange(n)).astype(np.int32)
    ea[5], eb[9] = -1, 2 * n
    for S in ALL_S + (4, 7, 63):
        q, b, _ = tr.samples_np(quats, body, ea, eb, S)
        got = lrm.dbg_edge_transit_samples_host(quats, body, ea, eb, S)
        assert np.array_equal(np.concatenate([q, b], 2).view(np.uint32), got.view(np.uint32)), S
    assert np.isnan(got[5]).all() and np.isnan(got[9]).all()


def test_the_model_holds_an_exact_slerp_and_rejects_a_wrong_path():
    """the model on its own: float64 slerp samples deviate by rounding only; a path the long way round, an unnormalised blend
    and a body off the segment are far outside every band"""
    qa, qb, ba, bb = t64.random_edges(2000, seed=3)
    a, b = qa.astype(np.float64), qb.astype(np.float64)
    b = b * np.where((a * b).sum(1, keepdims=True) < 0, -1, 1)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    om = np.arccos(np.clip((a * b).sum(1), -1, 1))[:, None, None]
    u = (np.arange(9) / 8)[None, :, None]
    so = np.where(om > 1e-6, np.sin(om), 1.0)
    sl = np.where(om > 1e-6, (np.sin((1 - u) * om) * a[:, None, :] + np.sin(u * om) * b[:, None, :]) / so, a[:, None, :] + 0 * u)
    seg = ba.astype(np.float64)[:, None, :] + u * (bb.astype(np.float64) - ba)[:, None, :]
    dev = t64.deviations(qa, qb, ba, bb, sl, seg)
    for k in ("unit", "plane", "range", "order", "segment", "body"):
        assert dev[k].max() < 1e-9, k  # slerp moves along the arc at another speed: "angle" is not its property
    assert dev["angle"].max() > 1e-3  # ... and the model sees that
    wrong = t64.deviations(qa, qb, ba, bb, 0.5 * sl, seg + 1.0)
    assert wrong["unit"].max() > 0.4 and wrong["segment"].max() > 1e-3
    long_way = t64.deviations(qa, -qb, ba, bb, -sl[:, ::-1], seg)  # starts at -qb: outside [0, Theta]
    assert long_way["range"].max() > 1.0 or long_way["order"].max() > 1.0


@pytest.mark.parametrize("S,n", [(9, 100000), (3, 20000), (64, 20000)])
def test_float32_path_stays_within_the_measured_bands_of_the_float64_model(lrm, S, n):
    got = t64.table(t64.random_edges(n, seed=0), lrm.dbg_edge_transit_samples_host, S)
    print(S, got)
    for k, band in BANDS.items():
        assert got[k] <= band, (S, k, got[k], band)
    assert got["unit"] > 1e-8  # float32 samples, not the model's own
