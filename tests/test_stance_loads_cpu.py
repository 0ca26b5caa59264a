"""Static foot loads and joint torques on the host (no GPU): lrm_stance_loads_posed_cpu, the serial loop that the GPU tests
compare with bit for bit, against tests/loads_model64.py -- a float64 model from the leg's geometry and from statics that
shares no code with the library (joint axes by cross products of the model's own joints, loads by numpy.linalg.lstsq on the
feet the library reports as carrying) -- on seeded corpora, on hand-made stances with known answers, against
lrm_stance_stability_cpu on a cloud made of the FK tips, and on the contract's input rules.

The bands are MEASURED (test_the_band_is_measured prints them), asserted at four times the worst value seen and checked on a
corpus they were not measured on."""
import ctypes as C

import numpy as np
import pytest

import loads_cases as lc
import loads_model64 as m64

F = np.float32
CONFIGS = ((6, 0), (8, 2), (4, 0), (3, 0))  # (legs, every which one a moonbot leg)
PLANES = (None, lc.PLANE_TILTED)


def measure(lrm, seed, ns, into):
    statuses = np.zeros(5, np.int64)
    for nlegs, mb in CONFIGS:
        legs, quats, ang = lc.corpus(lrm, seed * 100 + nlegs, ns, nlegs, mb)
        lift = lrm.stance_lift("each", nlegs)
        for com in lc.COMS:
            for plane in PLANES:
                got = lc.host(lrm, quats, legs, ang, com=com, plane=plane, lift=lift)
                m64.measure(got, m64.statics64(ang, legs, quats, None, com, plane), lift, into)
                statuses += np.bincount(got["status"].ravel(), minlength=5)
    return statuses


def test_the_band_is_measured(lrm):
    """equilibrium (sum of loads 1, both moments 0), loads >= 0, +0 off the planted set, and loads and torques against the
    model: measured on corpus 1, asserted on corpus 2"""
    worst = {}
    statuses = measure(lrm, 1, 600, worst)
    print("corpus 1:", {k: float(f"{v:.4g}") for k, v in worst.items()}, "statuses", statuses)
    for k, measured in m64.MEASURED.items():
        assert worst[k] <= measured * 1.0001, k  # the figures written in loads_model64.py are this corpus's
    assert worst["load"] > 1e-9 and worst["tau"] > 1e-7  # float32 answers, not the model's own
    assert worst["answers"] > 50000
    other = {}
    measure(lrm, 2, 300, other)
    print("corpus 2:", {k: float(f"{v:.4g}") for k, v in other.items()})
    for k, band in m64.BAND.items():
        assert other[k] <= band, (k, other[k], band)


def test_every_status_occurs(lrm):
    """0 (dead), 1 (all), 2 (dropped), 3 (tripod: spread-out feet, an eccentric centre of mass) and 4 (none)"""
    legs, quats, ang = lc.corpus(lrm, 108, 600, 8, 2)
    live = np.ones(600, np.uint8)
    live[::7] = 0
    got = lc.host(lrm, quats, legs, ang, com=lc.COMS[2], lift="each", live_in=live)
    n = np.bincount(got["status"].ravel(), minlength=5)
    print("statuses 0..4:", n)
    assert (n[:5] > 0).all() and n[5:].sum() == 0
    dead = live == 0
    assert (got["status"][:, dead] == lrm.LOADS_DEAD).all() and (got["status"][:, ~dead] != lrm.LOADS_DEAD).all()
    assert (got["load"][:, :, dead] == 0).all() and (got["tau"][:, :, :, dead] == 0).all()
    assert np.isneginf(got["peak"][:, dead]).all() and (got["peak_at"][:, dead] == 255).all() and (got["holdable"][:, dead] == 0).all()
    none = got["status"] == lrm.LOADS_NONE
    assert np.isneginf(got["peak"][none]).all() and (got["peak_at"][none] == 255).all() and (got["holdable"][none] == 0).all()
    # status 4: nan (0x7fc00000) on the planted feet, +0 on the others; fewer than three planted feet is status 4
    m, s = np.argwhere(none)[0]
    w = got["load"][m, :, s]
    assert set(w.view(np.uint32)) <= {0x7fc00000, 0}
    t = got["tau"][m, :, :, s]
    assert np.array_equal(np.isnan(t), np.repeat(np.isnan(w)[:, None], 3, 1))
    solved = (got["status"] >= 1) & (got["status"] <= 3)
    assert np.isfinite(got["load"].transpose(0, 2, 1)[solved]).all()
    # the peak is the largest ratio, its code names it, holdable is the comparison itself
    ratio = np.abs(got["tau"]) / lc.TAU_MAX[None, None, :, None]
    planted = got["load"] > 0
    peak = np.where(planted[:, :, None, :], ratio, -np.inf).max((1, 2))
    assert np.array_equal(peak[solved], got["peak"][solved])
    code = got["peak_at"][solved].astype(int)
    mm, ss = np.nonzero(solved)
    assert np.array_equal(ratio[mm, code // 4, code % 4, ss], got["peak"][solved])
    fits = (np.abs(got["tau"]) <= lc.TAU_MAX[None, None, :, None]).all((1, 2))
    assert np.array_equal(got["holdable"].astype(bool), solved & fits)
    assert 0 < got["holdable"][solved].mean() < 1


# ---- hand-made stances with known answers --------------------------------------------------------------------------------
SAME = np.array([0.0, -0.2, -1.3], F)  # every leg alike: the feet stand on a circle about the body's z axis


def ring(lrm, nlegs):
    return lc.legs_n(lrm, nlegs), np.array([[1, 0, 0, 0]], F), np.tile(SAME, (nlegs, 1))


def test_symmetric_tripod_and_square(lrm):
    for nlegs in (3, 4):
        legs, quats, ang = ring(lrm, nlegs)
        got = lc.host(lrm, quats, legs, ang)
        assert got["status"][0, 0] == lrm.LOADS_ALL
        assert np.abs(got["load"][0, :, 0] - 1.0 / nlegs).max() < 2e-6, got["load"][0, :, 0]
        assert np.abs(got["tau"][0, :, :, 0] - got["tau"][0, 0, :, 0]).max() < 2e-4  # every leg holds the same
    # six legs, each tripod lifted in turn: the other three carry a third each
    legs, quats, ang = ring(lrm, 6)
    got = lc.host(lrm, quats, legs, ang, lift=[0b010101, 0b101010])
    assert (got["status"] == lrm.LOADS_ALL).all()
    for m, up_legs in enumerate(([0, 2, 4], [1, 3, 5])):
        down = [l for l in range(6) if l not in up_legs]
        assert (got["load"][m, up_legs, 0] == 0).all() and np.abs(got["load"][m, down, 0] - 1 / 3).max() < 2e-6


def test_a_yaw_axis_along_up_carries_no_coxa_torque(lrm):
    """a leg whose yaw axis is vertical under `up` (no coxa pitch, a level body): turning the coxa does not raise the foot"""
    legs = np.stack([lrm.leg_factory(az, 120.0, 0.0, 60.0, 130.0, 150.0, 60.0, 90.0, 120.0, 0.0, 0.0) for az in (0.0, 2.0, 4.0, 5.5)]).astype(F)
    rng = np.random.default_rng(5)
    ns = 64
    ang = np.column_stack([rng.uniform(-0.7, 0.7, 4 * ns), rng.uniform(-0.6, 0.5, 4 * ns), rng.uniform(-2.2, -0.6, 4 * ns)]).astype(F)
    quats = np.tile(np.array([1, 0, 0, 0], F), (ns, 1))
    got = lc.host(lrm, quats, legs, ang)
    assert ((got["status"] >= 1) & (got["status"] <= 3)).any()
    assert (got["tau"][:, :, 0, :][~np.isnan(got["tau"][:, :, 0, :])] == 0).all()  # exactly: the column has no z and `up` only z
    M = m64.statics64(ang, legs, quats)
    assert np.abs(M["arm"][:, :, 0]).max() < 1e-9
    assert np.abs(M["arm"][:, :, 1:]).max() > 50.0


def test_a_foot_exactly_on_the_centre_of_mass_carries_everything(lrm):
    legs, quats, ang = ring(lrm, 3)
    ang[1] = [0.3, -0.4, -1.0]
    tips = np.stack([lrm.apply_fk_cpu(ang[l:l + 1], legs[l])[0][0] for l in range(3)])
    for l in range(3):
        got = lc.host(lrm, quats, legs, ang, com=tips[l])  # plane None, identity: c = (com.x, com.y) exactly
        assert got["status"][0, 0] in (lrm.LOADS_ALL, lrm.LOADS_TRIPOD)
        want = np.zeros(3, F)
        want[l] = 1
        assert np.abs(got["load"][0, :, 0] - want).max() < 2e-6, (l, got["load"][0, :, 0])
        if got["status"][0, 0] == lrm.LOADS_TRIPOD:  # the barycentric numerators are then d itself, 0 and 0
            assert np.array_equal(got["load"][0, :, 0].view(np.uint32), want.view(np.uint32)), (l, got["load"][0, :, 0])
    legs, quats, ang = ring(lrm, 6)
    tip = lrm.apply_fk_cpu(ang[2:3], legs[2])[0][0]
    got = lc.host(lrm, quats, legs, ang, com=tip)
    assert 1 <= got["status"][0, 0] <= 3
    m64.measure(got, m64.statics64(ang, legs, quats, None, tip), [0])


def test_collinear_feet_have_no_answer(lrm):
    legs, quats, ang = lc.corpus(lrm, 9, 40, 6)
    for plane in ([[1, 0, 0], [1, 0, 0]], [[0.6, 0.8, 0], [0, 0, 0]]):  # both plane coordinates alike; one of them always 0
        got = lc.host(lrm, quats, legs, ang, plane=plane, lift="each")
        assert (got["status"] == lrm.LOADS_NONE).all()
        assert np.isnan(got["load"]).sum() == (6 + 6 * 5) * 40 and (got["holdable"] == 0).all()


# ---- against the support polygon of stance_stability ---------------------------------------------------------------------
STEPS = (0.0, 1e-5, -1e-5, 3e-5, -3e-5, 1e-4, -1e-4, 3e-4, -3e-4, 1e-3, -1e-3, 3e-3, -3e-3, 1e-2, -1e-2, 3e-2, -3e-2, 0.1, -0.1)  # mm across the edge, + outwards


def margins_and_statuses(lrm, seed, ns, boundary):
    """-> (margin, status), flat over every (lift set, set) with at least three planted feet.  The cloud is made of the FK
    tips plus the body, so that stance_stability sees the feet stance_loads computes.  boundary: as many single-set calls
    whose centre of mass is put on (and just beside) the nearest edge of the support polygon"""
    rng = np.random.default_rng(seed)
    margins, statuses = [], []

    def both(legs, quats, body, ang, com, plane, lift):
        nl, n = len(legs), len(quats)
        tips = lrm.leg_joints_posed_cpu(ang, quats, body, legs)[0][:, :, 3].reshape(-1, 3)
        foot = np.arange(nl * n, dtype=np.int32).reshape(nl, n)
        margin, edge = lrm.stance_stability_cpu(tips, foot, quats, body, com=com, plane=plane, lift=lift)[:2]
        got = lc.host(lrm, quats, legs, ang, com=com, plane=plane, lift=lift)
        return margin, edge, got["status"], tips

    for nlegs, mb in CONFIGS:
        legs, quats, ang = lc.corpus(lrm, seed * 100 + 50 + nlegs, ns, nlegs, mb)
        body = rng.uniform(-300, 300, (ns, 3)).astype(F)
        lift = lrm.stance_lift("each", nlegs)
        for com in lc.COMS:
            for plane in PLANES:
                margin, _, status, _ = both(legs, quats, body, ang, com, plane, lift)
                keep = np.isfinite(margin) | (status != lrm.LOADS_NONE)
                margins.append(margin[keep]), statuses.append(status[keep])
    legs, quats, ang = lc.corpus(lrm, seed * 100 + 77, boundary, 6)
    quats[:] = [1, 0, 0, 0]
    ang = ang.reshape(6, boundary, 3)
    for s in range(boundary):
        a, q, b = ang[:, s], quats[s:s + 1], np.zeros((1, 3), F)
        margin, edge, _, tips = both(legs, q, b, a, None, None, None)
        if not np.isfinite(margin[0, 0]):
            continue
        i, j = int(edge[0, 0]) // 8, int(edge[0, 0]) % 8
        mid = ((tips[i].astype(np.float64) + tips[j]) / 2)
        out = np.array([tips[j][1] - tips[i][1], -(tips[j][0] - tips[i][0]), 0.0])  # to the right of i -> j: outwards
        out /= np.linalg.norm(out)
        for step in STEPS:
            margin, _, status, _ = both(legs, q, b, a, (mid + step * out).astype(F), None, None)
            margins.append(margin.ravel()), statuses.append(status.ravel())
    return np.concatenate(margins), np.concatenate(statuses)


def gap(margin, status):
    """the smallest b with: margin > b => status in 1..3, and status in 1..3 => margin >= -b"""
    solved = (status >= 1) & (status <= 3)
    return max(float(margin[~solved].max(initial=-np.inf)), float(-margin[solved].min(initial=np.inf)), 0.0)


def test_cross_check_with_stance_stability(lrm):
    margin, status = margins_and_statuses(lrm, 1, 300, 200)
    measured = gap(margin, status)
    print(f"corpus 1: b measured {measured:.4g} mm over {len(margin)} answers; MEASURED_MARGIN {m64.MEASURED_MARGIN:g}, BAND_MARGIN {m64.BAND_MARGIN:g}")
    assert measured <= m64.MEASURED_MARGIN * 1.0001
    assert measured > 0  # the boundary family does put answers on the wrong side of 0
    margin, status = margins_and_statuses(lrm, 2, 300, 20)
    b = m64.BAND_MARGIN
    solved = (status >= 1) & (status <= 3)
    skipped = np.abs(margin) <= b
    print(f"corpus 2: {len(margin)} answers, {int(skipped.sum())} with |margin| <= b ({100.0 * skipped.mean():.3f} %), gap {gap(margin, status):.4g} mm")
    assert solved[margin > b].all()
    assert (margin[solved] >= -b).all()
    assert skipped.mean() < 0.01
    assert solved.sum() > 10000 and (~solved).sum() > 1000


# ---- input handling ------------------------------------------------------------------------------------------------------
def random_angles(rng, n):
    return np.column_stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.6, 0.5, n), rng.uniform(-2.2, -0.6, n)]).astype(F)


def test_ties_go_to_the_smaller_leg_and_the_first_triple(lrm):
    """Exact ties, made two ways.  MIRRORED legs (azimuths +-t, yaw angles +-c, a level body, the centre of mass on the axis):
    the feet are mirror images to the bit, so the loads of a pair tie and the drop stage must let the smaller leg go first.
    TWIN legs (legs 1 and 2 the same leg under the same angles): their feet coincide, so the triples (0, 1, 3) and (0, 2, 3)
    tie and the first must win, and where both twins carry, their torque ratios tie and the peak must name the smaller code."""
    rng = np.random.default_rng(3)
    legs = np.stack([lrm.get_M2_leg(sign * t) for t in (0.5, 1.6, 2.6) for sign in (1, -1)]).astype(F)
    ns = 4000
    half = random_angles(rng, 3 * ns).reshape(3, ns, 3)
    ang = np.repeat(half, 2, 0)
    ang[1::2, :, 0] *= -1
    quats = np.tile(np.array([1, 0, 0, 0], F), (ns, 1))
    tips = lrm.leg_joints_posed_cpu(ang.reshape(-1, 3), quats, None, legs)[0][:, :, 3]
    assert np.array_equal(tips[0::2, :, 0], tips[1::2, :, 0]) and np.array_equal(tips[0::2, :, 1], -tips[1::2, :, 1])
    seen = 0
    for cx in range(150, 310, 10):
        got = lc.host(lrm, quats, legs, ang.reshape(-1, 3), com=[cx, 0, 0])
        w = got["load"][0]
        lopsided = (got["status"][0] == lrm.LOADS_DROPPED) & (w[0::2] != w[1::2]).any(0)
        for k in range(3):  # where one leg of a pair left and its mirror image stayed, the smaller one left
            assert not (lopsided & (w[2 * k] > 0) & (w[2 * k + 1] == 0)).any(), (cx, k)
            seen += int((lopsided & (w[2 * k] == 0) & (w[2 * k + 1] > 0)).sum())
    print("mirrored pairs whose smaller leg was dropped and whose larger leg carries:", seen)
    assert seen > 0

    rng = np.random.default_rng(4)
    legs = lc.legs_n(lrm, 4)
    legs[2] = legs[1]
    quat = np.array([[1, 0, 0, 0]], F)
    first = 0
    for _ in range(200):  # the centre of mass half way between foot 0 and the twins: only a triple with one twin carries it
        a = random_angles(rng, 4)
        a[2] = a[1]
        tips = lrm.leg_joints_posed_cpu(a, quat, None, legs)[0][:, 0, 3]
        got = lc.host(lrm, quat, legs, a, com=((tips[0].astype(np.float64) + tips[1]) / 2).astype(F))
        if got["status"][0, 0] == lrm.LOADS_TRIPOD:
            w = got["load"][0, :, 0]
            assert w[1] > 0 and w[2] == 0, w
            first += 1
    print("tripod stages decided between the twins' triples:", first)
    assert first > 10

    legs = lc.legs_n(lrm, 5)
    legs[2] = legs[1]
    ns = 1000
    quats = lc.unit_quats(rng, ns)
    ang = random_angles(rng, 5 * ns).reshape(5, ns, 3)
    ang[2] = ang[1]
    got = lc.host(lrm, quats, legs, ang.reshape(-1, 3), com=lc.COMS[1])
    st, w, at = got["status"][0], got["load"][0], got["peak_at"][0]
    both = (st >= 1) & (st <= 3) & (w[1] > 0) & (w[2] > 0)
    assert np.array_equal(w[1][both].view(np.uint32), w[2][both].view(np.uint32))
    assert not (both & (at // 4 == 2)).any() and (both & (at // 4 == 1)).sum() > 50


class Raw:
    """lrm_stance_loads_posed_cpu through ctypes, every argument replaceable"""

    def __init__(self, lrm, nlegs=6, ns=8, nm=3):
        self.lrm = lrm
        legs, quats, ang = lc.corpus(lrm, 3, ns, nlegs)
        self.a = dict(quats=quats, nposes=ns, legs=legs, nlegs=nlegs, pose_idx=None, nsets=ns, angles=ang, com=np.zeros(3, F),
                      plane=None, lift=np.array([0, 1, 2][:nm], np.uint8), nmasks=nm, tau_max=lc.TAU_MAX.copy(), live_in=None,
                      status=np.full((nm, ns), 99, np.uint8), holdable=np.full((nm, ns), 99, np.uint8), peak=np.full((nm, ns), 7, F),
                      peak_at=np.full((nm, ns), 99, np.uint8), load=np.full((nm, nlegs, ns), 7, F), tau=np.full((nm, nlegs, 3, ns), 7, F))

    def __call__(self, **edit):
        a = dict(self.a, **edit)
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        rc = self.lrm.lib().lrm_stance_loads_posed_cpu(p(a["quats"]), a["nposes"], p(a["legs"]), a["nlegs"], p(a["pose_idx"]), a["nsets"],
                                                       p(a["angles"]), p(a["com"]), p(a["plane"]), p(a["lift"]), a["nmasks"], p(a["tau_max"]),
                                                       p(a["live_in"]), p(a["status"]), p(a["holdable"]), p(a["peak"]), p(a["peak_at"]),
                                                       p(a["load"]), p(a["tau"]), None)
        return rc, self.lrm.lib().lrm_last_error().decode()


# the refusals in their documented order: (what is wrong, a word of its message)
REFUSALS = [
    (dict(nlegs=9), "nlegs"), (dict(nmasks=257), "nmasks"), (dict(nsets=1 << 31), "INT32_MAX"),
    (dict(nsets=(1 << 32) // (6 * 3 * 3) + 1), "2^32"), (dict(lift=None), "null"), (dict(lift=np.array([0, 64, 2], np.uint8)), "lift set"),
    (dict(tau_max=np.array([1, np.nan, 1], F)), "tau_max"), (dict(com=np.array([0, np.inf, 0], F)), "com"),
    (dict(plane=np.array([1, 0, 0, 0, np.nan, 0], F)), "plane"), (dict(nsets=9), "without pose_idx"),
]


def test_refusals_come_first_and_in_order(lrm):
    raw = Raw(lrm)
    assert raw()[0] == 0
    for k, (edit, word) in enumerate(REFUSALS):
        rc, msg = raw(**edit)
        assert rc != 0 and word in msg, (edit, msg)
        for later, _ in REFUSALS[k + 1:]:
            if set(later) & set(edit):
                continue  # both change the same argument
            rc, msg = raw(**dict(later, **edit))
            assert rc != 0 and word in msg, (edit, later, msg)
    for bad in ([0, 1, 1], [-1, 1, 1], [1, 1, -np.inf], [1, -0.0, 1]):
        assert raw(tau_max=np.array(bad, F))[0] != 0
    assert raw(tau_max=None)[0] != 0 and raw(nlegs=0)[0] != 0 and raw(nmasks=0)[0] != 0
    assert raw(tau_max=np.array([np.inf, np.inf, 1e-30], F))[0] == 0
    # after the refusals nsets == 0 is a no-op whatever the pointers; the refusals still come before it
    assert raw(nsets=0, quats=None, legs=None, angles=None, status=None, holdable=None, peak=None)[0] == 0
    assert raw(nsets=0, nlegs=9)[0] != 0 and raw(nsets=0, tau_max=np.array([1, 0, 1], F))[0] != 0
    for k in ("quats", "legs", "angles", "status", "holdable", "peak"):
        assert raw(**{k: None})[0] != 0, k
    assert np.all(raw.a["status"] != 99)  # the good calls wrote


def test_every_optional_pointer_may_be_null(lrm):
    raw = Raw(lrm)
    assert raw()[0] == 0
    full = {k: raw.a[k].copy() for k in ("status", "holdable", "peak", "peak_at", "load", "tau")}
    for drop in (("peak_at",), ("load",), ("tau",), ("peak_at", "load", "tau"), ("com",), ("live_in",)):
        for k in full:
            raw.a[k][...] = 99 if raw.a[k].dtype == np.uint8 else 7
        assert raw(**{k: None for k in drop})[0] == 0
        for k in full:
            if k in drop:
                assert (raw.a[k] == (99 if raw.a[k].dtype == np.uint8 else 7)).all()
            else:
                assert np.array_equal(raw.a[k].view(np.uint8), full[k].view(np.uint8)), (drop, k)


def test_nan_angles_live_in_bad_poses_and_a_non_unit_quaternion(lrm):
    legs, quats, ang = lc.corpus(lrm, 4, 64, 6)
    base = lc.host(lrm, quats, legs, ang, lift="each")
    # a leg with nan angles (IK status 0) is a lifted leg: load 0, tau 0, the others as if it were lifted
    a2 = ang.reshape(6, 64, 3).copy()
    a2[2, ::3] = np.nan
    a2[4, 5] = [0.1, np.inf, 0.2]
    a2[0, 7] = [500.0, 0.1, 0.2]  # outside the sincos range
    got = lc.host(lrm, quats, legs, a2.reshape(-1, 3), lift="each")
    assert (got["load"][:, 2, ::3] == 0).all() and (got["tau"][:, 2, :, ::3] == 0).all()
    assert (got["load"][:, 4, 5] == 0).all() and (got["load"][:, 0, 7] == 0).all()
    for k in ("status", "load", "tau", "peak", "holdable"):  # lift set 3 = leg 2 lifted: the same answer as with leg 2 invalid
        assert np.array_equal(got[k][3][..., 0:64:3].copy().view(np.uint8), base[k][3][..., 0:64:3].copy().view(np.uint8)), k
    untouched = np.ones(64, bool)
    untouched[::3] = False
    untouched[[5, 7]] = False
    assert np.array_equal(got["load"][..., untouched].copy().view(np.uint32), base["load"][..., untouched].copy().view(np.uint32))
    # live_in and pose indices
    live = (np.arange(64) % 5 != 0).astype(np.uint8)
    live[3] = 255
    pose = np.arange(64, dtype=np.int32)
    pose[[10, 11, 12, 13]] = [-1, 64, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    got = lc.host(lrm, quats, legs, ang, pose_idx=pose, lift="each", live_in=live)
    dead = (live == 0) | np.isin(np.arange(64), [10, 11, 12, 13])
    assert (got["status"][:, dead] == 0).all() and (got["status"][:, ~dead] != 0).all()
    assert np.array_equal(got["load"][..., ~dead].copy().view(np.uint32), base["load"][..., ~dead].copy().view(np.uint32))
    # sets that share a pose, in any order
    pose = np.arange(64, dtype=np.int32)[::-1].copy()
    rev = lc.host(lrm, quats[::-1].copy(), legs, ang, pose_idx=pose, lift="each")
    assert np.array_equal(rev["tau"].view(np.uint32), base["tau"].view(np.uint32))
    # a non-unit, a zero and a nan quaternion: an answer or status 4 / 0, never a crash; a zero com is exact whatever the quaternion
    q2 = quats.copy()
    q2[0] *= 1.3
    q2[1] = 0
    q2[2] = np.nan
    q2[3] = [3, -2, 1, 4]
    got = lc.host(lrm, q2, legs, ang, lift="each", com=[10, 5, 0])
    assert got["status"][0, 2] == 0 and set(np.unique(got["status"])) <= {0, 1, 2, 3, 4}
    zero = lc.host(lrm, q2, legs, ang, lift="each")
    assert zero["status"][0, 2] in (0, 4) and (zero["status"][:, 4:] == base["status"][:, 4:]).all()
    with pytest.raises(ValueError):
        lc.host(lrm, quats, legs, ang, tau_max=[1, 2])
    with pytest.raises(ValueError):
        lc.host(lrm, quats, legs, ang, live_in=np.ones(3, np.uint8))
