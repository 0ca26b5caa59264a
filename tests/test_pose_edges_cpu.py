"""Pose-graph edges on the host (no GPU): lrm_pose_edges_cpu against the pure-numpy float32 model of tests/pose_edges_model.py
bit for bit (counts, offsets, lists, d2, cos2) on every scene of tests/pose_edges_cases.py in both forms; the relation's
properties on the host loop's own output (form 1 is the exact symmetrisation of form 0, the list is sorted, a relabelling maps
the edge set onto itself, the lattice's touching pairs ARE neighbours and one ulp less are not); hostile offsets and
capacities with sentinels and views of longer buffers; every refusal of the three forms in its order (the device forms refuse
before they touch a device) and the NULL forms; the float64 model on continuous random poses; the symbols and the plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_edges_cases as ec
import pose_edges_model as em

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
SYMBOLS = ("lrm_pose_edges_workspace_bytes", "lrm_pose_edge_counts_dev", "lrm_pose_edges_dev", "lrm_pose_edges_cpu", "lrm_dbg_pose_edges_plan")
SENT = -77


def model(c, form):
    return em.edges32(c["quats"], c["body"], c["pose_live"], c["max_step"], c["min_dot"], form)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sorted(ec.SCENES))
def test_host_loop_against_the_model(lrm, name, form):
    c = ec.SCENES[name]()
    h, m = ec.host(lrm, c, form), model(c, form)
    ec.assert_same(h, m, (name, form))
    assert np.array_equal(h["written"], h["count"])
    counts_only, _ = lrm.pose_edges_cpu(c["quats"], c["body"], c["max_step"], c["min_dot"], c["pose_live"], form, counts_only=True)
    assert np.array_equal(counts_only, m["count"])


def test_the_scenes_are_not_vacuous():
    """asserted on the model alone"""
    n = {name: (len(model(c, 0)["edge_a"]), len(c["quats"])) for name, c in ((k, f()) for k, f in ec.SCENES.items())}
    print(n)
    assert n["lattice_touching"][0] == n["lattice_far"][0] == n["lattice_morton"][0] == n["lattice_shuffled"][0] == ec.lattice_pairs(7, 6, 5)
    assert n["lattice_just_short"][0] == 0
    assert n["lattice_diagonal"][0] > ec.lattice_pairs(6, 5, 4)
    assert n["one_point"][0] == 150 * 149 // 2
    for name in ("oriented", "oriented_plain", "cloud", "hostile", "dead_mask", "no_body", "all_steps"):
        pairs, poses = n[name]
        assert poses <= pairs < poses * (poses - 1) // 2, name  # edges, but not every pair
    # the turn limit links adjacent yaw steps only: per body 8 pairs on its own ring, per lattice pair 8 + 16 (same step and +-1)
    assert n["oriented"][0] == 30 * 8 + (5 * 5 + 6 * 4) * 24 and n["oriented_plain"][0] == 20 * 8 + (4 * 4 + 5 * 3) * 24
    c = ec.hostile()
    ok = em.valid32(c["quats"], c["body"], None)[0]
    assert (~ok).sum() == 6 * 3 + 2 and not ok[list(ec.PLACES)].any()


def test_touching_pairs_are_neighbours_and_one_ulp_less_are_not(lrm):
    """d2 == step2 bit-exactly on the 50 mm lattice, at the origin and 4e6 mm away"""
    for origin in (0.0, 4.0e6):
        c = ec.lattice(7, 6, 5, origin=origin)
        h = ec.host(lrm, c, 0)
        assert len(h["edge_a"]) == ec.lattice_pairs(7, 6, 5)
        assert (h["d2"].view(np.uint32) == np.float32(2500.0).view(np.uint32)).all() and (h["cos2"] == 1.0).all()
        short = {**c, "max_step": float(np.nextafter(np.float32(50.0), np.float32(0.0)))}
        assert ec.host(lrm, short, 0)["count"].sum() == 0 and ec.host(lrm, short, 1)["count"].sum() == 0


@pytest.mark.parametrize("name", ["lattice_morton", "oriented", "cloud", "hostile", "dead_mask", "no_body"])
def test_form_1_is_the_exact_symmetrisation_of_form_0_and_both_are_sorted(lrm, name):
    c = ec.SCENES[name]()
    up, full = ec.host(lrm, c, 0), ec.host(lrm, c, 1)
    for h in (up, full):
        key = h["edge_a"].astype(np.int64) << 32 | h["edge_b"].astype(np.int64)
        assert (np.diff(key) > 0).all()  # sorted by (a, b), no duplicate
        assert np.array_equal(np.repeat(np.arange(len(h["count"])), h["count"]), h["edge_a"])
    assert (up["edge_a"] < up["edge_b"]).all() and (full["edge_a"] != full["edge_b"]).all()
    bits = lambda h: {(a, b): (d, s) for a, b, d, s in zip(h["edge_a"].tolist(), h["edge_b"].tolist(), h["d2"].view(np.uint32).tolist(),
                                                            h["cos2"].view(np.uint32).tolist())}
    u, f = bits(up), bits(full)
    assert len(f) == 2 * len(u)
    for (a, b), v in u.items():
        assert f[(a, b)] == v and f[(b, a)] == v  # the bits of (p, q) are those of (q, p)


@pytest.mark.parametrize("name", ["lattice_touching", "oriented", "cloud", "hostile"])
def test_a_relabelling_maps_the_edge_set_onto_itself(lrm, name):
    c = ec.SCENES[name]()
    n = len(c["quats"])
    perm = np.random.default_rng(11).permutation(n)
    h, hp = ec.host(lrm, c, 1), ec.host(lrm, ec.permuted(c, perm), 1)
    assert ec.pair_set(perm[hp["edge_a"]], perm[hp["edge_b"]]) == ec.pair_set(h["edge_a"], h["edge_b"])
    # the three orders of one lattice hold the same bodies: the same number of edges and the same multiset of d2
    if name == "lattice_touching":
        for other in ("lattice_morton", "lattice_shuffled"):
            assert np.array_equal(np.sort(ec.host(lrm, ec.SCENES[other](), 1)["count"]), np.sort(h["count"]))


@pytest.mark.parametrize("form", [0, 1])
def test_hostile_offsets_and_capacities_never_write_outside(lrm, form):
    c = ec.SCENES["cloud"]()
    h = ec.host(lrm, c, form)
    assert h["count"].max() > 4
    pad = 13
    for name, offsets, capacity in ec.hostile_offsets(h["count"], 5):
        bufs = {k: np.full(capacity + 2 * pad, SENT, dt) for k, dt in (("edge_a", np.int32), ("edge_b", np.int32), ("d2", np.float32), ("cos2", np.float32))}
        written = np.full(len(h["count"]) + pad, SENT, np.int32)
        views = {k: v[pad:pad + capacity] for k, v in bufs.items()}
        got = ec.host(lrm, c, form, offsets=offsets, capacity=capacity, written=written[:len(h["count"])], **views)
        want = ec.expect_rows(h, offsets, capacity, SENT)
        for k, w in zip(("edge_a", "edge_b", "d2", "cos2"), want):
            assert (bufs[k][:pad] == SENT).all() and (bufs[k][pad + capacity:] == SENT).all(), (name, k)
            if name != "random":  # overlapping segments hold one of the rows that claim them
                assert np.array_equal(views[k].view(np.int32), w.view(np.int32)), (name, k)
        assert np.array_equal(written[:len(h["count"])], want[4]) and (written[len(h["count"]):] == SENT).all(), name
        assert np.array_equal(got["count"], h["count"]), name
    # without the optional outputs
    got = ec.host(lrm, c, form, want_d2=False, want_cos2=False)
    assert got["d2"] is None and got["cos2"] is None and np.array_equal(got["edge_b"], h["edge_b"])


class Raw:
    """the three C entry points on raw pointers, one good call's arguments that tests edit; which: "cpu", "counts", "fill" """

    def __init__(self, lrm, which):
        self.lrm, self.which = lrm, which
        c = ec.lattice(3, 2, 1)
        self.a = dict(quats=c["quats"], body=c["body"], nposes=6, pose_live=np.ones(6, np.uint8), max_step=50.0, min_dot=0.5, form=0,
                      workspace=np.zeros(16, np.float64), count=np.full(6, SENT, np.int32), offsets=np.arange(7, dtype=np.int64) * 3, capacity=18,
                      edge_a=np.full(18, SENT, np.int32), edge_b=np.full(18, SENT, np.int32), d2=np.full(18, SENT, np.float32),
                      cos2=np.full(18, SENT, np.float32), written=np.full(6, SENT, np.int32))

    def __call__(self, **edit):
        a = dict(self.a, **edit)
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        head = (p(a["quats"]), p(a["body"]), a["nposes"], p(a["pose_live"]), a["max_step"], a["min_dot"], a["form"])
        lists = (p(a["offsets"]), a["capacity"], p(a["edge_a"]), p(a["edge_b"]), p(a["d2"]), p(a["cos2"]), p(a["written"]))
        lib = self.lrm.lib()
        if self.which == "counts":  # never reaches a launch in these tests: every call is refused first
            rc_ = lib.lrm_pose_edge_counts_dev(*head, p(a["workspace"]), p(a["count"]), None)
        elif self.which == "fill":
            rc_ = lib.lrm_pose_edges_dev(*head, p(a["workspace"]), *lists, None)
        else:
            rc_ = lib.lrm_pose_edges_cpu(*head, p(a["count"]), *lists, None)
        return rc_, lib.lrm_last_error().decode()


# the refusals in their documented order: (what is wrong, a word of its message)
REFUSALS = [(dict(form=2), "form"), (dict(nposes=1 << 31), "INT32_MAX"), (dict(max_step=float("nan")), "max_step"), (dict(min_dot=1.5), "min_dot"),
            (dict(quats=None), "null")]


@pytest.mark.parametrize("which", ["cpu", "counts", "fill"])
def test_refusals_come_first_and_in_order(lrm, which):
    raw = Raw(lrm, which)
    if which == "cpu":
        assert raw()[0] == 0 and list(raw.a["count"]) == [2, 1, 2, 1, 1, 0] and list(raw.a["written"]) == [2, 1, 2, 1, 1, 0]
        assert list(raw.a["edge_b"][:3]) == [1, 2, SENT] and list(raw.a["edge_a"][6:9]) == [2, 2, SENT]
    for k, (edit, word) in enumerate(REFUSALS):
        rc_, msg = raw(**edit)
        assert rc_ == -1 and word in msg, (edit, msg)
        for later, _ in REFUSALS[k + 1:]:
            rc_, msg = raw(**dict(later, **edit))
            assert rc_ == -1 and word in msg, (edit, later, msg)
    for edit in (dict(form=-1), dict(max_step=-1.0), dict(max_step=-0.5), dict(min_dot=float("nan")), dict(min_dot=-0.25), dict(min_dot=float("inf"))):
        assert raw(**edit)[0] == -1, edit
    nulls = {"cpu": ["edge_a", "edge_b"], "counts": ["workspace", "count"], "fill": ["workspace", "offsets", "edge_a", "edge_b"]}[which]
    for k in nulls:
        assert raw(**{k: None})[0] == -1, k
    if which == "cpu":
        assert raw(count=None, offsets=None)[0] == -1  # neither counts nor lists
    else:
        assert "aligned" in raw(workspace=raw.a["workspace"].view(np.uint8)[4:])[1]
    # the range checks come before the no-op of nposes == 0, the pointer checks after it
    assert raw(nposes=0, form=2)[0] == -1 and raw(nposes=0, min_dot=2.0)[0] == -1 and raw(nposes=0, max_step=float("nan"))[0] == -1
    assert raw(nposes=0, quats=None, workspace=None, count=None, offsets=None, edge_a=None, edge_b=None)[0] == 0
    # +inf steps, no step and both ends of min_dot are values, not errors
    if which == "cpu":
        for edit in (dict(max_step=float("inf")), dict(max_step=0.0), dict(min_dot=0.0), dict(min_dot=1.0)):
            assert raw(**edit)[0] == 0, edit


def test_every_optional_pointer_may_be_null(lrm):
    raw = Raw(lrm, "cpu")
    assert raw()[0] == 0
    outs = ("count", "d2", "cos2", "written")
    full = {k: raw.a[k].copy() for k in outs + ("edge_a", "edge_b")}
    for drop in [(k,) for k in outs] + [outs]:
        for k in full:
            raw.a[k][...] = SENT
        assert raw(**{k: None for k in drop})[0] == 0, drop
        for k in full:
            assert np.array_equal(raw.a[k], np.full_like(full[k], SENT) if k in drop else full[k]), (drop, k)
    for k in ("body", "pose_live"):
        assert raw(**{k: None})[0] == 0
    # counts only: the list arguments are not read
    raw.a["count"][...] = SENT
    assert raw(offsets=None, edge_a=None, edge_b=None, d2=None, cos2=None, written=None)[0] == 0 and list(raw.a["count"]) == [2, 1, 2, 1, 1, 0]
    # capacity 0: written = 0 everywhere and nothing else (the counts, which are their own output, still come)
    for k in full:
        raw.a[k][...] = SENT
    assert raw(capacity=0)[0] == 0
    assert (raw.a["written"] == 0).all() and all((raw.a[k] == SENT).all() for k in ("edge_a", "edge_b", "d2", "cos2")) and list(raw.a["count"]) == [2, 1, 2, 1, 1, 0]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_sizes_of_nothing_one_and_two(lrm, n):
    c = ec.case(ec.identity(n), np.zeros((n, 3)), 1.0)
    for form in (0, 1):
        h = ec.host(lrm, c, form)
        ec.assert_same(h, model(c, form), n)
        assert h["count"].sum() == (0 if n < 2 else 1 + form)


# ---- the float64 model ------------------------------------------------------------------------------------------------------
# The largest |d64 - max_step| and |angle64 - max_turn| among the pairs on which the host loop and the float64 model disagree,
# measured on the host over the scenes of test_against_the_float64_model (seeds 21..24, 4080 poses each): 3.46e-6 mm and 5.20e-8 rad, and the margin: four
# times that, the project's margin in test_swing_cpu.py.
MEASURED_STEP_MM, MEASURED_TURN_RAD = 3.46e-6, 5.20e-8
BAND_STEP_MM, BAND_TURN_RAD = 4 * MEASURED_STEP_MM, 4 * MEASURED_TURN_RAD


@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_against_the_float64_model(lrm, seed):
    """Continuous random poses (4000 in a 1200 mm box, max_step 90 mm, max_turn 0.6 rad of orientations up to 0.5 rad from
    the identity, plus 80 partner poses placed on a threshold up to the rounding of their float32 coordinates, without which
    four seeds hold no disagreeing pair at all).  The host loop may disagree with the float64 model (true distance, true angle between the two rotation
    matrices; the turn limit is 2 acos(min_dot) of the float32 min_dot the call takes) only for pairs within the band of a
    threshold.  Measured on the host over the four seeds: the largest |d64 - max_step| among disagreeing pairs 3.46e-6 mm
    (MEASURED_STEP_MM), the largest |angle64 - max_turn| 5.20e-8 rad (MEASURED_TURN_RAD), on 28 to 48 disagreeing ordered pairs per
    seed; asserted: four times that, 1.38e-5 mm and 2.08e-7 rad.  The pairs inside a band are excluded from
    the comparison; their share of the candidate pairs (neighbours under either model) must stay under 1 % (measured: 0.27 to 0.39 %)."""
    c = ec.with_threshold_pairs(ec.cloud(4000, seed, box=1200.0), 40, seed)
    n = len(c["quats"])
    h = ec.host(lrm, c, 1)
    turn = 2.0 * np.arccos(np.float64(np.float32(c["min_dot"])))
    got = np.zeros((n, n), bool)
    got[h["edge_a"], h["edge_b"]] = True
    worst_d = worst_a = 0.0
    candidates = banded = 0
    for p in range(n):
        dist, ang = em.pairs64(c["quats"], c["body"], p)
        want = (dist <= c["max_step"]) & (ang <= turn)
        want[p] = False
        differ = want != got[p]
        near = (np.abs(dist - c["max_step"]) <= BAND_STEP_MM) | (np.abs(ang - turn) <= BAND_TURN_RAD)
        either = want | got[p]
        candidates += int(either.sum())
        banded += int((either & near).sum())
        for q in np.nonzero(differ)[0]:
            # a disagreement is explained by the threshold it sits on: the distance's when only that test differs ...
            d_off, a_off = abs(dist[q] - c["max_step"]), abs(ang[q] - turn)
            if min(d_off / 1.0, a_off / 1e-3) == d_off / 1.0:
                worst_d = max(worst_d, d_off)
            else:
                worst_a = max(worst_a, a_off)
        assert not (differ & ~near).any(), (p, np.nonzero(differ & ~near)[0][:5])
    print(f"seed {seed}: candidates {candidates}, in a band {banded}, worst |d64 - max_step| {worst_d:.3e} mm, worst |angle - max_turn| {worst_a:.3e} rad")
    assert candidates > 20 * n // 10 and banded < 0.01 * candidates


def test_symbols_are_declared_and_exported(lrm):
    declared, exported = lrm.declared_symbols(), lrm.exported_symbols()
    for s in SYMBOLS:
        assert s in declared and s in exported, s
    assert lrm.lib().lrm_pose_edges_workspace_bytes(64) == 64 and lrm.lib().lrm_pose_edges_workspace_bytes(65) == 96  # chunk boxes + group boxes
    assert lrm.lib().lrm_pose_edges_workspace_bytes(64 * 64 + 1) == 32 * (65 + 2)
    assert lrm.lib().lrm_pose_edges_workspace_bytes(0) == 32
    assert lrm.pose_edges_min_dot(None) == 0.0 and lrm.pose_edges_min_dot(0.0) == 1.0
    assert 0.0 < lrm.pose_edges_min_dot(np.pi) < 1e-7
    assert lrm.pose_edges_min_dot(1.0) == float(np.float32(np.cos(0.5)))
    with pytest.raises(ValueError):
        lrm.pose_edges_min_dot(4.0)


def test_the_plan_is_the_kernels(lrm):
    """lrm_dbg_pose_edges_plan against the constants parsed from the source"""
    head = open(os.path.join(CSRC, "lrm_pose_edges.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", head).group(1))
    chunk, rnd, block = const("LRM_EDGES_CHUNK"), const("LRM_EDGES_ROUND"), const("LRM_EDGES_BLOCK")
    assert chunk == 64 and rnd == 64 and block % chunk == 0
    src = open(os.path.join(CSRC, "lrm_pose_edges.hip")).read()
    for name, macro in (("kBlock", "LRM_EDGES_BLOCK"), ("kChunk", "LRM_EDGES_CHUNK"), ("kBoxFloats", "LRM_EDGES_BOX_FLOATS")):
        assert re.search(rf"constexpr \w+ {name} = {macro};", src), name
    for n in (0, 1, block - 1, block, block + 1, chunk * rnd, 20000, 2 ** 31 - 1):
        assert lrm.dbg_pose_edges_plan(n) == {"chunk": chunk, "round": rnd, "workgroups": -(-n // block), "block": block}, n
    assert lrm.lib().lrm_dbg_pose_edges_plan(1 << 31, np.zeros(4, np.uint64).ctypes.data_as(C.c_void_p)) == -1
    assert lrm.lib().lrm_dbg_pose_edges_plan(5, None) == -1
