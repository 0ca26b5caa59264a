"""The case module of the one-query-per-lane kernels (tests/query_cases.py) on the host: the pass sizes it parses are the
ones the suite is built around, the gather through src equals the posed CPU calls on the expanded arrays bit for bit,
every index pattern produces the wave classes it is there for at the sizes tests/test_gpu_query_shapes.py uses, the pool
keeps the IK contract, and the oracle's answer on the unique combinations is lrm_reach_dist_posed_cpu's.

A change of a block cap or of a *_MIN_WAVES default in lrm_posed.hip, lrm_ik.hip or lrm_ik_posed.hip must come with the
new value in test_pass_sizes_are_the_ones_the_suite_is_built_around."""
import numpy as np
import pytest

import query_cases as qc
from conftest import bits_equal
from ik_cases import check_contract

PATTERNS = ("runs", "echo", "interleaved", "shuffled", "single")


@pytest.fixture(scope="module")
def cs(lrm, oracle):
    return qc.cases(lrm, oracle)


def test_pass_sizes_are_the_ones_the_suite_is_built_around():
    assert qc.pass_constants() == {"posed_kernel": (256, 16384, 4), "ik_kernel": (256, 8192, 4), "fk_kernel": (256, 8192, None),
                                   "ik_posed_kernel": (256, 8192, 4), "fk_posed_kernel": (256, 8192, None)}
    assert qc.pass_sizes() == {"posed_kernel": 4_194_304, "ik_kernel": 2_097_152, "fk_kernel": 2_097_152,
                               "ik_posed_kernel": 2_097_152, "fk_posed_kernel": 2_097_152}


def test_walk_on_a_hand_made_case():
    """S = 512: 2 blocks, 8 waves; n = 1100: trips 0, 1 and a third with two waves, the last one partial"""
    rec = np.zeros(1100, np.int64)
    rec[64:128] = 3          # wave 1, trip 0: uniform on 3
    rec[576:640] = 3         # wave 1, trip 1: uniform on 3 again (hit)
    rec[130] = 5             # wave 2, trip 0: mixed
    rec[512:576] = 4         # wave 0, trip 1: uniform on 4 (miss after 0)
    oob = np.zeros(1100, bool)
    oob[640] = oob[200] = True
    rec[192:256] = 9         # wave 3, trip 0: uniform on 9 but for the clamped lane 200 -> mixed
    w = qc.walk(1100, 512, rec, oob)
    assert w["stride"] == 8 and list(w["trip"]) == [0] * 8 + [1] * 8 + [2, 2]
    assert list(np.flatnonzero(w["mixed"])) == [2, 3]
    # waves 2 and 3 were mixed in trip 0 and staged nothing: chunks 10 and 11 miss; the third trip meets record 0 after 4 and 3
    assert list(np.flatnonzero(w["hit"])) == [9, 12, 13, 14, 15] and w["miss"][[10, 11, 16, 17]].all()
    assert not w["hit"][8] and w["miss"][8] and w["miss"][0] and not w["miss"][2]
    assert list(np.flatnonzero(w["partial"])) == [17] and w["lane0_oob"][10] and w["oob_in_uniform"][10]
    assert w["lane0_oob"].sum() == 1 and not w["oob_in_uniform"][3]
    assert qc.walk(100, 512, np.zeros(100))["stride"] == 4  # n <= S: one trip, the grid is ceil(n / 256)


def test_walk_stays_a_model_of_the_loop_structure():
    import inspect
    src = [l for l in inspect.getsource(qc.walk).splitlines() if l.strip()]
    assert len(src) <= 40


def queries_of(cs, name, n, S, oob=False):
    """(xyz, pose, leg, seed, ang, src, src_ik, o): the expanded query arrays of a pattern; src_ik: -1 also where the
    target index is out of range (o.t_at: those queries take target_idx o.t_val)"""
    pose, leg = qc.pattern(name, n, cs.P, cs.L, S)
    o = qc.with_oob(pose, leg, S, cs.P, cs.L, cs.nu) if oob else None
    if o is not None:
        pose, leg = o.pose, o.leg
    k, src = qc.expand(pose, leg, cs.L, None if o is None else o.oob_pl)
    take = np.where(src < 0, k, src)
    return cs.xyz[take], pose, leg, cs.seed[take], cs.ang[take], src, take, o


def gather_is_sound(lrm, cs, name, oob):
    n, S = 50_000, 8192 if oob else qc.pass_sizes()["ik_posed_kernel"]
    xyz, pose, leg, seed, ang, src, take, o = queries_of(cs, name, n, S, oob)
    tab = (cs.quats, cs.body, cs.legs)
    nan = np.float32(np.nan)
    m, v, d, _ = lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, *tab)
    assert np.array_equal(m, qc.gather(cs.mask, src, 0)) and np.array_equal(v, qc.gather(cs.valid, src, 0))
    assert bits_equal(d, qc.gather(cs.field, src, nan)).all()
    # the IK through target_idx into the pool, with seeds; then on the expanded targets without either
    ti = take.astype(np.int32)
    t_bad = np.zeros(n, bool)
    if oob:
        ti[o.t_at], t_bad[o.t_at] = o.t_val, True
        assert (src[o.oob_pl] == -1).all() and o.oob_pl.sum() > 64 and o.oob_t.sum() > 10
    a, s, _ = lrm.apply_ik_posed_cpu(cs.xyz, pose, leg, *tab, target_idx=ti, seed=seed)
    assert np.array_equal(s, qc.gather(cs.iks_s, src, 0, t_bad)) and bits_equal(a, qc.gather(cs.iks_a, src, nan, t_bad)).all()
    a, s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, *tab)
    assert np.array_equal(s, qc.gather(cs.ik_s, src, 0)) and bits_equal(a, qc.gather(cs.ik_a, src, nan)).all()
    for inp, want in ((cs.ik_a, cs.fk_ik), (cs.ang, cs.fk_raw), (cs.ang_finite, cs.fk_finite)):
        p, _ = lrm.apply_fk_posed_cpu(inp[take], pose, leg, *tab)
        assert bits_equal(p, qc.gather(want, src, nan)).all()
    if oob:  # the finite angles tell an out-of-range tip (nan) from every other one
        want = qc.gather(cs.fk_finite, src, nan)
        assert np.isnan(want[o.oob_pl]).all() and np.isfinite(want[~o.oob_pl]).all()
    assert len(np.unique(qc.pick(n))) == qc.K and (qc.pick(n)[:-1] != qc.pick(n)[1:]).mean() > 0.98


@pytest.mark.parametrize("name", PATTERNS)
def test_the_gather_equals_the_calls_on_the_expanded_arrays(lrm, cs, name):
    gather_is_sound(lrm, cs, name, False)


@pytest.mark.parametrize("name", ["runs", "echo"])
def test_the_gather_with_out_of_range_indices(lrm, cs, name):
    """with_oob needs uniform waves on (0, 0) and elsewhere: runs and echo, here with a small S so that n wraps"""
    gather_is_sound(lrm, cs, name, True)


def test_single_pose_gather(lrm, cs):
    o, k = cs.one, qc.pick(5000)
    a, s, _ = lrm.apply_ik_cpu(o.xyz[k], o.leg, o.quat, seed=o.seed[k])
    assert np.array_equal(s, o.iks_s[k]) and bits_equal(a, o.iks_a[k]).all() and len(np.unique(o.iks_s)) >= 3
    a, s, _ = lrm.apply_ik_cpu(o.xyz[k], o.leg, o.quat)
    assert np.array_equal(s, o.ik_s[k]) and bits_equal(a, o.ik_a[k]).all()
    assert bits_equal(lrm.apply_fk_cpu(o.ang[k], o.leg, o.quat)[0], o.fk_raw[k]).all()


def classes(w):
    """counts of the (wave, trip) classes of the issue from walk(); trips count from 1 there: 'a trip of at least 2' is
    trip >= 1 here"""
    prev_mixed = np.zeros(len(w["mixed"]), bool)
    prev_mixed[w["stride"]:] = w["mixed"][:-w["stride"]] if len(w["mixed"]) > w["stride"] else False
    later = w["trip"] >= 1
    return {"hit_after_mixed": int((w["hit"] & prev_mixed).sum()), "hit_later": int((w["hit"] & later).sum()),
            "miss_later": int((w["miss"] & later).sum()), "mixed_later": int((w["mixed"] & later).sum()),
            "partial_uniform": int((w["partial"] & ~w["mixed"]).sum()), "partial_mixed": int((w["partial"] & w["mixed"]).sum())}


@pytest.mark.parametrize("kernel", ["posed_kernel", "ik_posed_kernel"])
def test_patterns_produce_their_wave_classes(cs, kernel):
    """A condition on the patterns, at the sizes of the GPU file.  The sizes bound what can occur: a wave's trips are S
    apart, so S + 65 holds 2 waves in the second trip, and 2 S + 63 holds S / 64 waves in the second trip and ONE in
    the third.  So: at 2 S + 63 runs and echo each hold >= 64 staged misses and >= 64 mixed waves in a later trip, and
    echo >= 64 staged hits there; at S + 65 the second trip is a miss or a mixed wave; 'uniform, mixed, uniform on the
    same record' needs three trips of many waves: echo at 3 S + 63, which the GPU file runs for that reason, holds
    >= 64 hits directly after a mixed trip.  The last wave is partial at every size; a partial mixed one comes with
    shuffled and interleaved at 2 S + 63, a partial uniform one with runs and echo."""
    S = qc.pass_sizes()[kernel]
    got = {(name, n): classes(qc.walk(n, S, np.int64(cs.L) * p + l))
           for name in ("runs", "echo") for n in (S + 65, 2 * S + 63) for p, l in [qc.pattern(name, n, cs.P, cs.L, S)]}
    for name in ("runs", "echo"):
        c = got[name, 2 * S + 63]
        assert c["miss_later"] >= 64 and c["mixed_later"] >= 64, (name, c)
        c1 = got[name, S + 65]
        assert c1["miss_later"] + c1["mixed_later"] + c1["hit_later"] == 2, (name, c1)
        assert c["partial_uniform"] + c["partial_mixed"] == 1 and c1["partial_uniform"] + c1["partial_mixed"] == 1
    assert got["echo", 2 * S + 63]["hit_later"] >= 64 and got["echo", S + 65]["miss_later"] >= 1
    n3 = 3 * S + 63
    pose, leg = qc.echo(n3, cs.P, cs.L, S)
    c3 = classes(qc.walk(n3, S, pose.astype(np.int64) * cs.L + leg))
    assert c3["hit_after_mixed"] >= 64 and c3["miss_later"] >= 64 and c3["mixed_later"] >= 64, c3
    part = {name: classes(qc.walk(2 * S + 63, S, np.int64(cs.L) * p + l))
            for name in ("shuffled", "interleaved") for p, l in [qc.pattern(name, 2 * S + 63, cs.P, cs.L, S)]}
    assert all(c["partial_mixed"] == 1 for c in part.values()), part
    assert sum(got[name, n]["partial_uniform"] for name in ("runs", "echo") for n in (S + 65, 2 * S + 63)) >= 2


@pytest.mark.parametrize("name", ["runs", "echo"])
@pytest.mark.parametrize("kernel", ["posed_kernel", "ik_posed_kernel"])
def test_with_oob_contains_its_six_placements(cs, kernel, name):
    S = qc.pass_sizes()[kernel]
    n = S + 65
    pose, leg = qc.pattern(name, n, cs.P, cs.L, S)
    o = qc.with_oob(pose, leg, S, cs.P, cs.L, cs.nu)
    bad = o.oob_pl | o.oob_t
    assert set(o.places) == set(qc.PLACEMENTS) and all(len(q) and bad[q].all() for q in o.places.values())
    assert bad.sum() == sum(len(q) for q in o.places.values())
    in_range = ((o.pose >= 0) & (o.pose < cs.P) & (o.leg < cs.L))
    assert np.array_equal(~in_range, o.oob_pl)
    rec = o.pose.astype(np.int64) * cs.L + o.leg
    w0, w = qc.walk(n, S, pose.astype(np.int64) * cs.L + leg), qc.walk(n, S, rec, o.oob_pl)
    ch = lambda p: o.places[p] // 64
    assert (o.places["lane0"] % 64 == 0).all() and (o.places["lane63"] % 64 == 63).all() and o.places["last_query"][0] == n - 1
    assert w["lane0_oob"][ch("lane0")[o.oob_pl[o.places["lane0"]]]].all()
    assert len(o.places["whole_wave"]) % 64 == 0 and o.oob_pl[o.places["whole_wave"]].any() and o.oob_t[o.places["whole_wave"]].any()
    # one lane of a uniform wave on (0, 0): the clamp keeps the wave uniform; on another record it turns the wave mixed
    on0, els = ch("lane_of_uniform_on_0"), ch("lane_of_uniform_elsewhere")
    assert o.oob_pl[o.places["lane_of_uniform_on_0"]].all() and o.oob_pl[o.places["lane_of_uniform_elsewhere"]].all()
    assert (~w0["mixed"][on0]).all() and (~w["mixed"][on0]).all() and w["oob_in_uniform"][on0].all() and (w["rec0"][on0] == 0).all()
    assert (~w0["mixed"][els]).all() and w["mixed"][els].all() and (w0["rec0"][els] != 0).all()
    # the chunks next to a planted one are untouched
    planted = np.unique(np.flatnonzero(bad) // 64)
    for nb in (planted - 1, planted + 1):
        nb = nb[(nb >= 0) & (nb < len(w["mixed"])) & ~np.isin(nb, planted)]
        assert not bad.reshape(-1)[np.minimum((nb[:, None] * 64 + np.arange(64)), n - 1)].any()


def test_the_pool_keeps_the_contract(lrm, oracle, cs):
    """items 1 to 4 of include/lrm.h (lrm_ik_*) for lrm_ik_cpu on the pool of every (pose, leg): limit-grid tips, tips
    perturbed by 1e-3 mm, points on and by the coxa axis, the coxa joint, non-finite and far targets; default and bad seeds"""
    xyz = cs.xyz.reshape(cs.P, cs.L, qc.K, 3)
    seed = cs.seed.reshape(cs.P, cs.L, qc.K, 3)
    worst = {"reached_max_mm": 0.0, "nearest_excess_max_mm": 0.0}
    seen = np.zeros(5, np.int64)
    for p in range(cs.P):
        for l in range(cs.L):
            pts = (xyz[p, l] - cs.body[p]).astype(np.float32)
            for sd in (None, seed[p, l]):
                ang, st, _ = lrm.apply_ik_cpu(pts, cs.legs[l], cs.quats[p], seed=sd)
                r = check_contract(oracle, pts, cs.legs[l], cs.quats[p], ang, st, clean=False)
                worst = {k: max(worst[k], r[k]) for k in worst}
                seen += r["counts"]
    print(f"status-1 miss <= {worst['reached_max_mm']:.3e} mm, status-2 excess <= {worst['nearest_excess_max_mm']:.3e} mm, "
          f"counts {seen}")
    assert seen[1] > 1000 and seen[2] > 1000 and not np.isfinite(cs.xyz).all()


def test_the_oracle_answer_on_the_unique_combinations_is_the_posed_cpu_call(lrm, cs):
    m, v, d, _ = lrm.apply_reach_dist_posed_cpu(cs.xyz, cs.pose, cs.leg, cs.quats, cs.body, cs.legs)
    assert np.array_equal(m, cs.mask) and np.array_equal(v, cs.valid) and bits_equal(d, cs.field).all()
    assert 0.05 < cs.mask.mean() < 0.95 and cs.valid.any() and not cs.valid.all()
