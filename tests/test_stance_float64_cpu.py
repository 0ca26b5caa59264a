"""Stance stability on the host (no GPU) against tests/stance_model64.py, a float64 model written from geometry and not from the
library or its restatement: the centre of mass through the textbook rotation matrix, the plane points as float64 dot products,
the support polygon by gift wrapping, the margin as the smallest signed distance from its counter-clockwise edges.  The model
first checks itself (sampled boundary distance, disc test, the monotone-chain hull as a vertex set); then every scene runs through
lrm.stance_stability_cpu and stance_model64.check_stance_rows: margin, stable, feet and the winning edge's code against
geometry.  Every test prints the worst margin - margin64 it measured, below and above, next to the band asserted: the constants
of stance_model64.BAND (four times the measured worst, one significant digit), shared with tests/test_gpu_stance_float64.py.

The caps on what doubt may hide (2 % of a scene's answers) and the non-vacuity counts are taken from the model alone."""
import numpy as np
import pytest

import ik_cases
import stance_cases as sc
import stance_model64 as sm

F = np.float32
COM = [20.0, -10.0, 5.0]
SLOPE = np.deg2rad(20.0)
GRAVITY = [0.0, np.sin(SLOPE), -np.cos(SLOPE)]  # a slope of 20 degrees
PLANES = {"none": None, "unit": [[1, 0, 0], [0, 1, 0]], "tilted": sm.gravity_basis(GRAVITY), "mirrored": sm.gravity_basis(GRAVITY, mirrored=True),
          "yawed": sm.gravity_basis(GRAVITY, yaw=0.7)}


def lifts_of(name, nlegs=6):
    return {"none": np.zeros(1, np.uint8), "each": sc.lift_each(nlegs), "tripods": np.array(sc.TRIPODS, np.uint8), "all": sc.lift_all(nlegs)}[name]


def unit_rows(quats):
    q = np.asarray(quats, np.float64)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def run_scene(lrm, name, kind, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, live_in=None,
              min_margins=(0.0,), exact_ties=False, cap=0.02):
    """the scene through the model (once) and the host loop (per min_margin) -> (model, the last got)"""
    lift = lrm.stance_lift(lift, len(foot))
    model = sm.stance64(targets, foot, quats, body, pose_idx, com, plane, lift, live_in)
    band = sm.BAND[kind]
    if kind != "large":
        assert (model["size"] < sm.WITHIN).all()
    measure = {}
    for min_margin in min_margins:
        total = int(np.isfinite(model["margin64"]).sum())
        in_doubt = int(sm.doubt(model, band, min_margin).sum())
        assert in_doubt <= cap * max(total, 1), (name, in_doubt, total)  # from the model alone, before the library is consulted
        got = sc.host(lrm, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in)
        try:
            compared, skipped = sm.check_stance_rows(got, model, band, min_margin, exact_ties, measure)
        finally:
            print(f"{name} [{kind}] min_margin {min_margin:g}: {measure.get('answers', 0)} finite answers, worst (margin - margin64) / factor "
                  f"{measure.get('below', 0.0):.3g} mm below, {measure.get('above', 0.0):.3g} mm above (band {band:g}); {in_doubt} of {total} in doubt "
                  f"({100.0 * in_doubt / max(total, 1):.3f} %, cap {100 * cap:g} %)")
        assert skipped == in_doubt
    return model, got


# ---- the model on its own ------------------------------------------------------------------------------------------------
def test_gravity_basis_is_orthonormal_in_both_handednesses():
    for g in (GRAVITY, [0, 0, -1.0], [0.3, -0.2, -0.9], [-5.0, 0, 0.1]):
        for yaw in (0.0, 0.7, -2.0):
            u, v = sm.gravity_basis(g, yaw)
            up = -np.asarray(g) / np.linalg.norm(g)
            assert np.allclose([u @ u, v @ v, u @ v, u @ up, v @ up], [1, 1, 0, 0, 0], atol=1e-14)
            assert np.allclose(np.cross(u, v), up, atol=1e-14)
            um, vm = sm.gravity_basis(g, yaw, mirrored=True)
            assert np.allclose(np.cross(um, vm), -up, atol=1e-14)
    assert np.allclose(sm.gravity_basis([0, 0, -9.81]), [[1, 0, 0], [0, 1, 0]], atol=1e-15)


def test_rotation64_special_values():
    h = np.sqrt(0.5)
    assert np.allclose(sm.rotation64([1, 0, 0, 0]), np.eye(3), atol=0)
    assert np.allclose(sm.rotation64([h, 0, 0, h]) @ [1, 0, 0], [0, 1, 0], atol=1e-15)  # a quarter turn about z takes x to y
    assert np.allclose(sm.rotation64([h, h, 0, 0]) @ [0, 1, 0], [0, 0, 1], atol=1e-15)  # about x: y to z
    assert np.allclose(sm.rotation64([h, 0, h, 0]) @ [0, 0, 1], [1, 0, 0], atol=1e-15)  # about y: z to x
    for q in ik_cases.random_cloud(20, 3)[:, :3]:
        quat = ik_cases.unit(np.concatenate([[0.3], q / 500.0]))
        R = sm.rotation64(quat)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R), 1.0)
        assert np.allclose(R @ quat[1:].astype(np.float64), quat[1:].astype(np.float64), atol=1e-14)  # the axis stays


def test_hull_special_values():
    sq = [(100, 100), (-100, 100), (-100, -100), (100, -100)]
    assert sm.hull_gift_wrap(sq + [(20, -30)]) == [2, 3, 0, 1]
    assert sm.hull_gift_wrap(sq + [(100, 25), (0, 100), (-100, 0)]) == [2, 3, 0, 1]  # feet on the edges are dropped
    assert sm.hull_gift_wrap([(0, 0), (1, 1), (3, 3), (2, 2)]) == [0, 2]  # one line
    assert sm.hull_gift_wrap([(3, 4)] * 4) == [0]
    assert sm.hull_gift_wrap([(0, 0), (0, 0), (1, 0), (0, 1), (1, 0)]) == [0, 2, 3]
    assert sm.orient((0, 0), (1e8, 1e8 + 1), (2e8, 2e8 + 2)) == 0 and sm.orient((0, 0), (1 / 3, 1 / 7), (1.0, (1 / 7) / (1 / 3))) in (-1, 0, 1)
    assert sm.margin_of_hull(sq, (90, 0)) == 10.0 and sm.margin_of_hull(sq, (130, 0)) == -30.0


def test_the_model_checks_itself(lrm):
    """hull, margin and point-in-polygon of the model on stances of every kind of scene, before anything is measured with it"""
    n_in = n_out = 0
    targets, foot, quats, body = sc.synthetic(150, 8, seed=8)
    for plane in ("none", "tilted", "mirrored"):
        a, b = sm.check_model64(sm.stance64(targets, foot, quats, body, com=COM, plane=PLANES[plane], lift=sc.lift_all(8)), every=60)
        n_in, n_out = n_in + a, n_out + b
    targets, foot, quats, body, _ = sm.collinear_family(300, seed=2)
    for plane in ("none", "tilted"):
        a, b = sm.check_model64(sm.stance64(targets, foot, quats, body, com=sm.COLLINEAR_COM, plane=PLANES[plane], lift=sc.lift_each(8)), every=6)
        n_in, n_out = n_in + a, n_out + b
    targets, foot, quats, body = sc.synthetic(100, 6, seed=9, offset=4e6)
    a, b = sm.check_model64(sm.stance64(targets, foot, quats, body, com=COM, lift=sc.lift_all(6)), every=9)
    print(f"the model checked itself on {n_in + a} hulls with c inside and {n_out + b} with c outside")
    assert n_in + a > 250 and n_out + b > 250


# ---- the scenes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main(lrm):
    targets, foot, quats, body, legs = sc.main_scene(lrm)
    return targets, foot, unit_rows(quats), body


@pytest.mark.parametrize("lift", ["none", "each", "tripods", "all"])
def test_main_scene(lrm, main, lift):
    targets, foot, quats, body = main
    model, got = run_scene(lrm, f"main, lift {lift}", "main", targets, foot, quats, body, com=sc.COM, lift=lifts_of(lift), min_margins=(0.0, 25.0))
    if lift == "each":  # non-vacuity, from the model alone
        m64 = model["margin64"]
        shares = float((m64 > 0).mean()), float((np.isfinite(m64) & (m64 <= 0)).mean()), float(np.isneginf(m64).mean())
        print(f"main scene: {100 * shares[0]:.1f} % stable, {100 * shares[1]:.1f} % finite and unstable, {100 * shares[2]:.1f} % -inf")
        assert min(shares) >= 0.10, shares
    if lift == "all":
        assert len(set(int(e) for e in got["edge"].ravel() if e != 255)) >= 20


@pytest.mark.parametrize("nlegs", [3, 4, 6, 8])
def test_leg_counts_with_every_subset(lrm, nlegs):
    targets, foot, quats, body = sc.synthetic(100 if nlegs == 8 else 150, nlegs, seed=nlegs, missing=0.1)
    model, got = run_scene(lrm, f"{nlegs} legs", "synthetic", targets, foot, quats, body, com=COM, lift=sc.lift_all(nlegs), min_margins=(0.0, 25.0))
    assert model["margin64"].shape[0] == 1 << nlegs and (model["margin64"] > 0).any() and np.isneginf(model["margin64"]).any()
    sizes = {len(h) for row in model["hull"] for h in row}
    if nlegs == 8:
        print(f"hull sizes of eight legs: {sorted(sizes)}; {len(set(got['edge'].ravel().tolist()) - {255})} distinct winning edge codes")
    assert sizes >= set(range(3, min(nlegs, 7) + 1)), sizes


def test_hull_sizes_three_to_eight_all_occur(lrm):
    """eight feet on a jittered ring: hulls of every size from three to eight under the 256 lift sets"""
    rng = np.random.default_rng(5)
    ns = 60
    az = 2 * np.pi * (np.arange(8)[:, None] + rng.uniform(-0.2, 0.2, (8, ns))) / 8
    r = rng.uniform(240.0, 300.0, (8, ns))
    targets = np.stack([r * np.cos(az), r * np.sin(az), rng.normal(0, 20, (8, ns))], -1).reshape(-1, 3).astype(F)
    foot = np.arange(8 * ns, dtype=np.int32).reshape(8, ns)
    quats = unit_rows(rng.standard_normal((ns, 4)))
    model, got = run_scene(lrm, "ring of eight", "synthetic", targets, foot, quats, None, com=[60.0, 30.0, -20.0], lift=sc.lift_all(8))
    sizes = {len(h) for row in model["hull"] for h in row}
    codes = set(got["edge"].ravel().tolist()) - {255}
    print(f"hull sizes {sorted(sizes)}, {len(codes)} distinct winning edge codes")
    assert sizes >= set(range(3, 9)) and len(codes) >= 20


@pytest.mark.parametrize("plane", sorted(PLANES))
def test_plane_forms(lrm, plane):
    targets, foot, quats, body = sc.synthetic(140, 6, seed=15)
    model, got = run_scene(lrm, f"plane {plane}", "synthetic", targets, foot, quats, body, com=[25.0, -15.0, 10.0], plane=PLANES[plane],
                           lift=sc.lift_all(6), min_margins=(0.0, 25.0))
    assert (model["margin64"] > 0).any()
    if plane == "mirrored":  # the feet keep their hull, the edges run the other way round in the caller's frame
        same = sm.stance64(targets, foot, quats, body, com=[25.0, -15.0, 10.0], plane=PLANES["tilted"], lift=sc.lift_all(6))
        assert np.allclose(np.nan_to_num(same["margin64"], neginf=-1e9), np.nan_to_num(model["margin64"], neginf=-1e9), rtol=0, atol=1e-9)
        assert all(set(a) == set(b) for ra, rb in zip(same["hull"], model["hull"]) for a, b in zip(ra, rb))


def test_many_stances_under_a_yawed_tilted_basis(lrm):
    """the tail of the error: 4000 stances instead of 140, among them feet a few mm apart (stance_model64.SEP)"""
    targets, foot, quats, body = sc.synthetic(4000, 6, seed=32)
    model, _ = run_scene(lrm, "4000 stances, plane yawed", "synthetic", targets, foot, quats, body, com=COM, plane=PLANES["yawed"], lift="each")
    print(f"{int((model['factor'] > 1).sum())} stances with two feet closer than {sm.SEP:g} mm, the closest {sm.SEP / model['factor'].max():.3g} mm")
    assert (model["factor"] > 3).any()


def test_pose_idx_and_live_in_forms(lrm):
    targets, foot, quats, body = sc.synthetic(120, 6, seed=12, missing=0.05)
    rng = np.random.default_rng(4)
    t2, f2, _, _ = sc.synthetic(500, 6, seed=13)
    pi = rng.permutation(120).astype(np.int32)
    pi[[0, 50]], pi[[1, 51]], pi[2] = -1, 120, np.iinfo(np.int32).min
    for name, (t, f, p) in {"permuted": (targets, foot, rng.permutation(120)), "repeated": (t2, f2, rng.integers(0, 120, 500)),
                            "one pose": (targets, foot, np.full(120, 17)), "dead entries": (targets, foot, pi)}.items():
        model, _ = run_scene(lrm, f"pose_idx {name}", "synthetic", t, f, quats, body, np.asarray(p, np.int32), com=COM, lift="each")
        if name == "dead entries":
            assert model["dead"][[0, 1, 2, 50, 51]].all() and model["dead"].sum() == 5
    live = np.ones(120, np.uint8)
    live[::3], live[7] = 0, 200
    for lv in (np.ones(120, np.uint8), np.zeros(120, np.uint8), live):
        model, _ = run_scene(lrm, f"live_in ({int((lv != 0).sum())} live)", "synthetic", targets, foot, quats, body, com=COM, lift="each", live_in=lv)
        assert np.array_equal(model["dead"], lv == 0)
    model, _ = run_scene(lrm, "body None, com None", "synthetic", targets, foot, quats, None, lift="each")
    assert (model["c"] == 0).all()


def test_invalid_feet(lrm):
    targets, foot, quats, body = sc.synthetic(200, 6, seed=11, missing=0.0)
    nt = len(targets)
    foot[0, ::7], foot[1, 1::7], foot[2, 2::7], foot[3, 3::7] = -1, nt, np.iinfo(np.int32).min, np.iinfo(np.int32).max
    targets[foot[4, 4::9]] = np.nan
    targets[foot[5, 5::11], 1] = np.inf
    model, _ = run_scene(lrm, "invalid feet", "synthetic", targets, foot, quats, body, com=[10.0, 0.0, 0.0], lift="each")
    assert (model["feet"] != 63).sum() > 60 and (model["feet"] == 63).any()
    bad_q = quats.copy()
    bad_q[3, 1], bad_q[9, 0] = np.nan, np.inf
    model, _ = run_scene(lrm, "non-finite quaternions", "synthetic", targets, foot, bad_q, body, com=[10.0, 0.0, 0.0], lift="each")
    assert model["dead"][[3, 9]].all() and model["dead"].sum() == 2
    bad_b = body.copy()
    bad_b[5], bad_b[6, 0] = np.nan, np.inf
    model, _ = run_scene(lrm, "non-finite bodies", "synthetic", targets, foot, quats, bad_b, com=[10.0, 0.0, 0.0], lift="each")
    assert (model["feet"][[5, 6]] == 0).all() and not model["dead"][[5, 6]].any()


@pytest.mark.parametrize("offset", [1e4, 4e6])
def test_bodies_far_from_the_origin(lrm, offset):
    """cloud and bodies far out: q = float32(t - body) is the model's input, so the band is that of the relative coordinates; at
    4e6 mm float32 steps by 0.25 to 0.5 mm, feet coincide and fall on one line exactly"""
    targets, foot, quats, body = sc.synthetic(256, 6, seed=9, offset=offset)
    model, _ = run_scene(lrm, f"bodies {offset:g} mm out", "far", targets, foot, quats, body, com=[30.0, 10.0, -5.0], lift=sc.lift_all(6), cap=0.02)
    assert (model["margin64"] > 0).sum() > 40
    if offset == 4e6:
        print(f"4e6 mm out: {int(model['degenerate'].sum())} degenerate hulls")
        assert model["degenerate"].any()


def test_large_stances(lrm):
    """relative coordinates up to some 5e4 mm: the float32 error grows with them, the band is measured on its own"""
    targets, foot, quats, body = sc.synthetic(200, 6, seed=21, spread=35000.0)
    model, _ = run_scene(lrm, "large", "large", targets, foot, quats, body, com=[2000.0, -1000.0, 500.0], lift=sc.lift_all(6), min_margins=(0.0, 2500.0))
    assert model["size"].max() > 2e4 and (model["margin64"] > 0).any()


@pytest.mark.parametrize("plane", ["none", "tilted", "mirrored"])
def test_near_collinear_family(lrm, plane):
    """aimed at a dropped side of the hull: feet on one line up to rounding, c close to that side.  A margin above margin64 + band
    is a failure (check_stance_rows), and so is a winning edge that leaves a planted foot to its right."""
    targets, foot, quats, body, info = sm.collinear_family(900, seed=3)
    lift = np.concatenate([sc.lift_each(8), [0b00000011, 0b00010100, 0b10100000, 0b01001001]]).astype(np.uint8)
    model, _ = run_scene(lrm, f"near-collinear, plane {plane}", "collinear", targets, foot, quats, body, com=sm.COLLINEAR_COM, plane=PLANES[plane], lift=lift)
    m0 = model["margin64"][0]
    print(f"near-collinear: {int((m0 > 0).sum())} stances with c inside, {int((m0 < 0).sum())} outside; feet on one line: "
          f"{np.bincount(info['side_feet'])[2:].tolist()} stances with 2, 3, ... of them")
    assert (m0 > 0).sum() > 200 and (m0 < 0).sum() > 200
    assert set(np.unique(info["side_feet"])) >= {2, 3, 4, 5}
    if plane == "none":  # c lies where the scene put it: OFFSETS from the side, unless another side is nearer
        assert (np.abs(m0 - info["offset"]) < 1e-3).mean() > 0.7


@pytest.mark.parametrize("name", sorted(sc.hand_made()))
def test_hand_made_stances(lrm, name):
    targets, foot, com, expect = sc.hand_made()[name]
    model, got = run_scene(lrm, name, "hand_made", targets, foot, sc.IDENTITY, None, com=com, lift=sc.lift_all(len(foot)), exact_ties=True, cap=1.0)
    if name in ("collinear", "coincident"):
        assert model["degenerate"][0, 0]
    else:
        assert model["margin64"][0, 0] == expect["margin"] and int(got["edge"][0, 0]) == expect["edge"]


# ---- properties of the library alone ---------------------------------------------------------------------------------------
def test_properties_of_the_library_alone(lrm):
    """the four properties of stance_model64.check_properties on the host loop (the GPU test runs them at 65 541 stances)"""
    targets, foot, quats, body = sc.synthetic(3000, 6, seed=31)
    run = lambda f, plane, lift: sc.host(lrm, targets, f, quats, body, com=COM, plane=plane, lift=lift)
    n = sm.check_properties(run, targets, foot, body, sm.BAND["synthetic"], sm.gravity_basis(GRAVITY), sm.gravity_basis(GRAVITY, yaw=1.1))
    print(f"{n} (stance, leg) entries whose foot is no hull vertex")
    assert n > 1000
