"""Body clearance on the host (lrm_body_clearance_posed_cpu, include/lrm.h): the host loop against a brute force built
from the oracle alone (tests/body_clearance_cases.py), bit for bit on the height, over leg families, quaternion kinds,
clouds, bad input, the degenerate and the uncullable scalars and the live_in forms; the consequences the header states;
the edge cases and every LRM_EINVAL of the C ABI.  The GPU tests compare the device with this host loop."""
import ctypes as C

import numpy as np
import pytest

import body_clearance_cases as bc
import footholds_posed_cases as fc
import pair_cases as pc
import posed_cases

PZ = bc.PLUS_Z


def both(lrm, oracle, targets, quats, body, legs, radius, plus_z, minus_z, floor_z=None, live_in=None):
    """host loop == oracle brute force == its numpy restatement -> the brute force's answer"""
    want = bc.brute(oracle, targets, quats, body, radius, plus_z, minus_z, floor_z, live_in)
    bc.assert_same(tuple(bc.brute_np(targets, quats, body, radius, plus_z, minus_z, floor_z, live_in)[k] for k in ("hits", "top", "height", "free")), want)
    got = bc.host(lrm, targets, quats, body, legs, radius, plus_z, minus_z, floor_z, live_in)
    bc.assert_same((got["hits"], got["top"], got["height"], got["free"]), want)
    bc.assert_consequences(want, live_in)
    return want


def test_main_scene_is_not_vacuous_and_matches(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 96, 1200, seed=3)
    r = float(legs[0][bc.BODY])
    want = bc.brute(oracle, targets, quats, body, r, PZ, -110.0, bc.floor_of(-110.0), masks=True)
    bc.assert_not_vacuous(want)
    got = bc.host(lrm, targets, quats, body, legs, r, PZ, -110.0, bc.floor_of(-110.0))
    bc.assert_same((got["hits"], got["top"], got["height"], got["free"]), want)
    bc.assert_consequences(want)
    # the quaternion kinds of the table all occur: identity, non-unit (|q| 0.5-2) and nan
    n = np.linalg.norm(quats.astype(np.float64), axis=1)
    assert np.array_equal(quats[0], [1, 0, 0, 0]) and (np.abs(n - 1) > 0.1).any() and np.isnan(n).any()
    assert (want["top"][np.isnan(n)] == -1).all()


# the keys of pair_cases.leg_families (which needs the library, so it cannot parametrise); test_the_family_list_is_complete
FAMILIES = ["m2_1_identity", "m2_2_tilted", "m2_3_nonunit", "m2_5_identity", "m2_6_tilted", "m2_7_nonunit", "m2_8_identity",
            "mixed_2_identity", "mixed_5_tilted", "moonbot_3_tilted", "moonbot_5_nonunit", "moonbot_6_identity", "random_2_tilted",
            "random_7_tilted", "random_8_identity", "random_wide_3_nonunit"]


def test_the_family_list_is_complete(lrm):
    fam = pc.leg_families(lrm)
    assert FAMILIES == sorted(fam)
    assert len({float(legs[0][bc.BODY]) for legs, _ in fam.values()}) >= 4  # several different body radii


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("minus_z", bc.MINUS_Z)
def test_every_leg_familys_body_radius(lrm, oracle, family, minus_z):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = bc.scene(lrm, 48, 700, seed=len(family))
    want = both(lrm, oracle, targets, quats, body, legs, float(legs[0][bc.BODY]), PZ, minus_z, bc.floor_of(minus_z))
    assert (want["top"] >= 0).any() and (want["top"] < 0).any()


@pytest.mark.parametrize("kind", ["identity", "fixture", "sweep", "random_unit", "non_unit", "nan"])
def test_quaternion_kinds(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 40, 800, seed=11)
    rng = np.random.default_rng(4)
    if kind == "identity":
        quats[:] = [1, 0, 0, 0]
    elif kind == "fixture":
        fq = np.asarray(posed_cases.fixture_quats(), np.float32)
        quats[:] = fq[np.arange(40) % len(fq)]
    elif kind == "sweep":
        quats = fc.sweep_pose_quats(lrm, 40)
    else:
        quats[:] = posed_cases.random_unit_quats(40, rng)
        if kind == "non_unit":
            quats *= rng.uniform(0.5, 2.0, (40, 1)).astype(np.float32)
        if kind == "nan":
            quats[np.arange(0, 40, 3), np.arange(0, 40, 3) % 4] = np.nan
    want = both(lrm, oracle, targets, quats, body, legs, 181.0, PZ, -110.0, -400.0)
    assert (want["hits"] > 0).any() and (want["top"] < 0).any()


@pytest.mark.parametrize("kind,nt", [("rough", 900), ("dense_cluster", 1000), ("sparse_tiles", 2048)])
def test_clouds(lrm, oracle, kind, nt):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 45, nt, seed=2, kind=kind)
    want = both(lrm, oracle, targets, quats, body, legs, 181.0, PZ, -45.0, -345.0)
    assert (want["hits"] > 0).any() and (want["hits"] == 0).any()


def test_nan_and_infinite_targets_and_bodies(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = bc.scene(lrm, 40, 800, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[6::17, 2] = -np.inf
    for radius, plus_z in ((181.0, PZ), (np.inf, np.inf)):
        want = bc.brute(oracle, bad_t, quats, body, radius, plus_z, -110.0, -400.0, masks=True)
        assert not want["column"][:, ~np.isfinite(bad_t).all(1)].any()  # a nan or infinite target is in no column
        got = bc.host(lrm, bad_t, quats, body, legs, radius, plus_z, -110.0, -400.0)
        bc.assert_same((got["hits"], got["top"], got["height"], got["free"]), want)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[5] = -np.inf
    bad_b[7, 2] = np.nan
    want = both(lrm, oracle, targets, quats, bad_b, legs, 181.0, PZ, -110.0, -400.0)
    assert (want["top"][[1, 2, 5, 7]] == -1).all() and (want["free"][[1, 2, 5, 7]] == 1).all()


def test_floor_equal_to_minus_z_makes_column_and_hit_coincide(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 45, 800, seed=5)
    want = bc.brute(oracle, targets, quats, body, 181.0, PZ, -110.0, -110.0, masks=True)
    assert np.array_equal(want["column"], want["hit"]) and want["hit"].any()
    assert np.array_equal(want["top"] >= 0, want["hits"] > 0) and (want["height"][want["top"] >= 0] > 0).all()
    got = bc.host(lrm, targets, quats, body, legs, 181.0, PZ, -110.0)  # floor_z None = minus_z
    bc.assert_same((got["hits"], got["top"], got["height"], got["free"]), want)


@pytest.mark.parametrize("radius,plus_z", [(np.inf, PZ), (181.0, np.inf), (np.inf, np.inf), (0.0, PZ)])
def test_uncullable_and_degenerate_scalars(lrm, oracle, radius, plus_z):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 30, 600, seed=6)
    want = both(lrm, oracle, targets, quats, body, legs, radius, plus_z, -110.0, -400.0)
    if radius == 0.0:
        assert (want["top"] == -1).all() and (want["free"] == 1).all()  # sqrt(.) < 0 never holds
    else:
        assert (want["hits"] > 0).any() and (want["top"] < 0).any()


def test_live_in_forms(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 60, 1000, seed=33)
    forms = bc.live_forms(lrm, targets, quats, body, legs)
    assert 0 < forms["all_legs"].sum() < 60
    full = both(lrm, oracle, targets, quats, body, legs, 181.0, PZ, -110.0, -400.0, None)
    for name, live in forms.items():
        want = both(lrm, oracle, targets, quats, body, legs, 181.0, PZ, -110.0, -400.0, live)
        mask = np.ones(60, bool) if live is None else live.astype(bool)
        for k in ("hits", "top", "free"):
            assert np.array_equal(want[k][mask], full[k][mask])
        if name == "zeros":
            assert (want["free"] == 0).all() and (want["top"] == -1).all()
    odd = np.zeros(60, np.uint8)
    odd[::3] = 7  # any non-zero byte is live
    both(lrm, oracle, targets, quats, body, legs, 181.0, PZ, -110.0, -400.0, odd)
    with pytest.raises(ValueError):
        lrm.body_clearance_posed_cpu(targets, quats, body, legs, 181.0, PZ, -110.0, live_in=np.ones(59, np.uint8))


def test_identity_quaternion_agrees_with_in_cylinder(lrm):
    """free is the negation of the unposed predicate (pair_cases.any_in_cylinder: collision.cu.h:12-23 in numpy float32) on
    the same cylinder and centres, and hits counts exactly its members"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = bc.scene(lrm, 120, 3000, seed=21)
    quats[:] = [1, 0, 0, 0]
    for minus_z in bc.MINUS_Z:
        got = bc.host(lrm, targets, quats, body, legs, 181.0, PZ, minus_z, bc.floor_of(minus_z))
        coll = pc.any_in_cylinder(body, targets, 181.0, PZ, minus_z)
        assert coll.any() and not coll.all()
        assert np.array_equal(got["free"], (~coll).astype(np.uint8))
        col = pc.any_in_cylinder(body, targets, 181.0, PZ, bc.floor_of(minus_z))
        assert np.array_equal(got["top"] >= 0, col)


def test_negative_zero_height_is_stored_as_positive_zero(lrm):
    """vz = -0 over minus_z = +0: the difference is -0, stored as +0; a twin at +0 height ties and the smaller index wins"""
    legs, _ = pc.leg_families(lrm)["m2_1_identity"]
    targets = np.array([[10, 0, -5], [0.0, 0.0, -0.0], [0, 0, 0.0], [20, 0, -1]], np.float32)
    quats = np.array([[1, 0, 0, 0]], np.float32)
    got = bc.host(lrm, targets, quats, np.zeros((1, 3), np.float32), legs, 100.0, 50.0, 0.0, -10.0)
    assert got["hits"][0] == 0 and got["top"][0] == 1 and pc.bits(got["height"])[0] == 0 and got["free"][0] == 1


def test_edge_cases_of_the_c_abi(lrm):
    L = lrm.load()
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    legs = np.ascontiguousarray(legs, np.float32)
    quats, body, targets = bc.scene(lrm, 12, 200, seed=1)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    hits, top = np.full(12, -7, np.int32), np.full(12, -7, np.int32)
    height, free = np.full(12, -7, np.float32), np.full(12, 0xA5, np.uint8)

    def cpu(nt=200, nposes=12, nlegs=5, r=181.0, pz=250.0, mz=-110.0, fz=-400.0, h=hits, t=top, he=height, fr=free, live=None):
        return L.lrm_body_clearance_posed_cpu(p(targets), nt, p(quats), p(body), nposes, p(legs), nlegs, r, pz, mz, fz, p(live), p(h), p(t),
                                              p(he), p(fr), None)

    def devc(nt=200, nposes=12, nlegs=5, r=181.0, pz=250.0, mz=-110.0, fz=-400.0):  # refused before any device is touched
        return L.lrm_body_clearance_posed_dev(None, None, None, nt, None, None, nposes, nlegs, r, pz, mz, fz, None, None, None, None, None, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(nt=2 ** 31), dict(nlegs=0), dict(nlegs=9), dict(nposes=2 ** 31), dict(nposes=2 ** 30, nlegs=5),
           dict(r=nan), dict(pz=nan), dict(mz=nan), dict(fz=nan), dict(r=-1.0), dict(mz=inf, pz=inf), dict(mz=-inf, fz=-inf),
           dict(fz=-inf), dict(fz=-100.0), dict(pz=-110.0), dict(pz=-200.0)]
    for kw in bad:
        assert cpu(**kw) == -1, kw
        assert devc(**kw) == -1, kw
        assert b"" != L.lrm_last_error()
    # the scalar checks come before the no-op, the NULL checks after it
    assert cpu(nposes=0, h=None, t=None) == 0 and devc(nposes=0) == 0
    assert cpu(nposes=0, r=-1.0) == -1 and devc(nposes=0, r=-1.0) == -1
    assert cpu(h=None) == -1 and cpu(t=None) == -1 and devc() == -1
    assert (hits == -7).all() and (top == -7).all() and (height == -7).all() and (free == 0xA5).all()  # nothing written so far
    # radius and plus_z may be +inf; NULL height / free leave the others written
    assert cpu(r=inf, pz=inf, he=None, fr=None) == 0
    assert (hits != -7).all() and (top != -7).all() and (height == -7).all() and (free == 0xA5).all()
    # nt == 0: 0 / -1 / -inf everywhere, free = 1 for live and 0 for skipped poses; every entry written
    live = np.ones(12, np.uint8)
    live[::4] = 0
    hits[:], top[:] = -7, -7
    assert cpu(nt=0, live=live) == 0
    assert (hits == 0).all() and (top == -1).all() and np.isneginf(height).all() and np.array_equal(free, live)
    # sentinel-filled outputs on a real scene: all written, and equal to the wrapper's
    hits[:], top[:], height[:], free[:] = -7, -7, -7, 0xA5
    assert cpu(live=live) == 0
    want = bc.host(lrm, targets, quats, body, legs, 181.0, 250.0, -110.0, -400.0, live)
    bc.assert_same((hits, top, height, free), want)
    bc.assert_consequences(want, live)


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_body_clearance_posed_dev", "lrm_body_clearance_posed_cpu"}
    assert names <= set(lrm.declared_symbols()) and names <= set(lrm.exported_symbols())
