"""Argument handling of every device entry point (run with -m gpu on an MI355X): what lrm_amd.device does with outputs and
optional device inputs BEFORE it launches.  One small scene, one table of entry points, and per entry point: a call without
outputs is the baseline; outputs given one element longer than needed (the (3, n) fields as a view of a wider buffer) come
back as the very tensors given, hold the baseline bit for bit and keep the extra element; a mistyped, short, strided or host
tensor in the place of any output is a ValueError and nothing is launched (the other outputs keep their sentinel); so is an
optional device input that is one entry short; and a PoseSet refuses a query before update() or without the table it needs.
No check here makes a kernel run on bad memory: every bad argument is rejected on the host."""
import numpy as np
import pytest

from conftest import random_cloud

pytestmark = pytest.mark.gpu

NT, NPOSES, NEDGES, NSAMPLES = 65, 3, 2, 3  # 65 targets: one past a wave
FREE = ["reach", "reach_bits", "dist", "reach_dist", "ik", "fk", "reach_any", "footholds", "foothold_offsets", "any_in_sphere",
        "any_in_cylinder", "stance_stability", "edge_transit", "swing_transit"]
FH_METHODS = ["ps.footholds", "ps.foothold_lists", "ps.foothold_edges", "ps.foothold_misses", "ps.foothold_support",
              "ps.body_clearance"]
IK_METHODS = ["ps.leg_clearance", "ps.self_clearance", "ps.trunk_clearance", "ps.leg_joints", "ps.ik", "ps.fk"]
NAMES = FREE + FH_METHODS + IK_METHODS + ["ps.reach_dist"]
FIELD = "field"  # an output kind: float32 (3, n) with contiguous rows, as against a flat buffer of (dtype, numel)


class Entry:
    """call(ps, **kw) runs the entry point on PoseSet ps with its valid arguments, kw replacing outputs or optional inputs;
    outs: {keyword: (dtype, numel) or (FIELD, n)}; ret: the keyword of every element of the returned tuple (None: not an
    output); inputs: the optional device inputs, each a valid 1-D tensor"""

    def __init__(self, call, outs, ret, inputs=None):
        self.call, self.outs, self.ret, self.inputs = call, outs, ret, inputs or {}

    def run(self, ps, **kw):
        r = self.call(ps, **{**self.inputs, **kw})
        r = r if isinstance(r, tuple) else (r,)
        assert len(r) == len(self.ret)
        return {k: v for k, v in zip(self.ret, r) if k is not None}


@pytest.fixture(scope="module")
def scene(lrm):
    import torch
    assert torch.cuda.is_available()
    d = lrm.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u8, i32, i64, f32 = torch.uint8, torch.int32, torch.int64, torch.float32
    legs = np.stack([lrm.get_M2_leg(0.0), lrm.get_M2_leg(2.0)])
    nl = len(legs)
    quats_h = np.array([[1, 0, 0, 0], [0.99, 0.05, -0.08, 0.1], [0.97, -0.1, 0.12, -0.15]], np.float32)
    quats_h /= np.linalg.norm(quats_h, axis=1, keepdims=True)
    body_h = np.array([[0, 0, 0], [30, 10, 5], [-20, 15, -10]], np.float32)
    cloud = random_cloud(NT, seed=7)
    cloud[NT // 2:, :2] = -cloud[NT // 2:, :2]  # the second leg looks the other way
    t = dev(cloud.T)
    tx, ty, tz = t[0], t[1], t[2]
    quats, body, bodies = dev(quats_h), dev(body_h), dev(body_h.T)
    ps = d.PoseSet(legs, NPOSES, ik=True, footholds=True).update(quats, body)
    count, best, _, _ = ps.footholds(tx, ty, tz)
    offsets = d.foothold_offsets(count)
    capacity = int(offsets[-1])
    assert capacity >= 2 and (best >= 0).any() and (best < 0).any()  # lists to write; legs with and without a foothold
    ea, eb = dev(np.array([0, 1], np.int32)), dev(np.array([1, 2], np.int32))
    foot_e = ps.foothold_edges(tx, ty, tz, ea, eb)[1]
    ffrom, fto = d.swing_layout(best, ea, eb, dev(np.array([1, 2], np.uint8)))
    pose_l, leg_l = d.footholds_layout(NPOSES, nl, "cuda")
    angles = ps.ik(tx, ty, tz, pose_l, leg_l, target_idx=best.view(-1))[0]
    ang = torch.stack([torch.linspace(-0.5, 0.5, NT), torch.linspace(0.2, 0.9, NT), torch.linspace(-1.0, 0.3, NT)]).cuda()
    ones = lambda n: torch.ones(n, dtype=u8, device="cuda")
    poses = torch.arange(NPOSES, dtype=i32, device="cuda")
    pose_q, leg_q = (torch.arange(NT, device="cuda") % NPOSES).to(i32), (torch.arange(NT, device="cuda") % nl).to(u8)
    leg, quat, radius = legs[0], quats_h[1], (12.0, 10.0, 8.0)
    torch.cuda.synchronize()
    per_leg = lambda n, *kinds: {k: (dt, nl * n) for k, dt in kinds}
    E = {}
    E["reach"] = Entry(lambda ps, **kw: d.reach(tx, ty, tz, leg, quat, **kw), {"out": (u8, NT)}, ("out",))
    E["reach_bits"] = Entry(lambda ps, **kw: d.reach(tx, ty, tz, leg, quat, want_bits=True, **kw),
                            {"out": (u8, NT), "bits": (i64, (NT + 63) // 64)}, ("out", "bits"))
    E["dist"] = Entry(lambda ps, **kw: d.dist(tx, ty, tz, leg, quat, **kw), {"out": (FIELD, NT), "valid": (u8, NT)}, ("out", "valid"))
    E["reach_dist"] = Entry(lambda ps, **kw: d.reach_dist(tx, ty, tz, leg, quat, **kw), {"mask": (u8, NT), "out": (FIELD, NT)},
                            ("mask", "out"))
    E["ik"] = Entry(lambda ps, **kw: d.ik(tx, ty, tz, leg, quat, **kw), {"out": (FIELD, NT), "status": (u8, NT)}, ("out", "status"))
    E["fk"] = Entry(lambda ps, **kw: d.fk(ang[0], ang[1], ang[2], leg, quat, **kw), {"out": (FIELD, NT)}, ("out",))
    E["reach_any"] = Entry(lambda ps, **kw: d.reach_any(bodies[0], bodies[1], bodies[2], tx, ty, tz, legs, **kw),
                           {"out": (u8, nl * NPOSES), "all_legs": (u8, NPOSES)}, ("out", "all_legs"))
    E["footholds"] = Entry(lambda ps, **kw: d.footholds(bodies[0], bodies[1], bodies[2], tx, ty, tz, legs, **kw),
                           per_leg(NPOSES, ("count", i32), ("best", i32), ("best_d2", f32)), ("count", "best", "best_d2"))
    E["foothold_offsets"] = Entry(lambda ps, **kw: d.foothold_offsets(count, **kw), {"out": (i64, nl * NPOSES + 1)}, ("out",))
    E["any_in_sphere"] = Entry(lambda ps, **kw: d.any_in_sphere(bodies[0], bodies[1], bodies[2], tx, ty, tz, 150.0, **kw),
                               {"out": (u8, NPOSES)}, ("out",))
    E["any_in_cylinder"] = Entry(lambda ps, **kw: d.any_in_cylinder(bodies[0], bodies[1], bodies[2], tx, ty, tz, 150.0, 80.0, -80.0, **kw),
                                 {"out": (u8, NPOSES)}, ("out",))
    stance_outs = {"margin": (f32, 3 * NPOSES), "edge": (u8, 3 * NPOSES), "stable": (u8, 3 * NPOSES), "feet": (u8, NPOSES)}
    E["stance_stability"] = Entry(lambda ps, **kw: d.stance_stability(tx, ty, tz, best, quats, body, lift="each", **kw), stance_outs,
                                  ("margin", "edge", "stable", "feet"), {"pose_idx": poses, "live_in": ones(NPOSES)})
    transit = (("mask", i64), ("reached", i32), ("first_miss", i32), ("worst", i32), ("worst_d2", f32))
    E["edge_transit"] = Entry(lambda ps, edge_b=eb, **kw: d.edge_transit(tx, ty, tz, quats, body, legs, ea, edge_b, foot_e, NSAMPLES, **kw),
                              {**per_leg(NEDGES, *transit), "planted": (u8, NEDGES), "clear": (u8, NEDGES), "advance": (i32, NEDGES)},
                              tuple(k for k, _ in transit) + ("planted", "clear", "advance"), {"live_in": ones(NEDGES), "edge_b": eb})
    swing = transit + (("hits", i32), ("hit_seg", i32), ("near", i32), ("pen", f32))
    E["swing_transit"] = Entry(lambda ps, edge_b=eb, **kw: d.swing_transit(tx, ty, tz, quats, body, legs, ea, edge_b, ffrom, fto, NSAMPLES,
                                                                           30.0, None, 5.0, 2.0, **kw),
                               {**per_leg(NEDGES, *swing), "swinging": (u8, NEDGES), "clear": (u8, NEDGES)},
                               tuple(k for k, _ in swing) + ("swinging", "clear"), {"live_in": ones(NEDGES), "edge_b": eb})
    fh_outs = per_leg(NPOSES, ("count", i32), ("best", i32), ("best_d2", f32))
    E["ps.footholds"] = Entry(lambda ps, **kw: ps.footholds(tx, ty, tz, **kw), {**fh_outs, "all_legs": (u8, NPOSES)},
                              ("count", "best", "best_d2", "all_legs"))
    E["ps.foothold_lists"] = Entry(lambda ps, **kw: ps.foothold_lists(tx, ty, tz, offsets=offsets, capacity=capacity, **kw),
                                   {"idx": (i32, capacity), "d2": (f32, capacity), "written": (i32, nl * NPOSES)},
                                   (None, "idx", "d2", "written"))
    E["ps.foothold_edges"] = Entry(lambda ps, edge_b=eb, **kw: ps.foothold_edges(tx, ty, tz, ea, edge_b, **kw),
                                   {**per_leg(NEDGES, ("count", i32), ("best", i32), ("best_d2", f32)), "all_legs": (u8, NEDGES)},
                                   ("count", "best", "best_d2", "all_legs"), {"edge_b": eb})
    E["ps.foothold_misses"] = Entry(lambda ps, **kw: ps.foothold_misses(tx, ty, tz, 50.0, **kw),
                                    {**per_leg(NPOSES, ("miss", i32), ("m2", f32), ("near", i32)), "shift": (f32, 3 * nl * NPOSES)},
                                    ("miss", "m2", "shift", "near"), {"count": count.view(-1)})
    E["ps.foothold_support"] = Entry(lambda ps, **kw: ps.foothold_support(tx, ty, tz, **kw),
                                     {**per_leg(NT, ("count", i32), ("best_pose", i32), ("best_d2", f32)), "legs_mask": (u8, NT)},
                                     ("count", "best_pose", "best_d2", "legs_mask"), {"pose_live": ones(NPOSES)})
    E["ps.body_clearance"] = Entry(lambda ps, **kw: ps.body_clearance(tx, ty, tz, 150.0, 60.0, -60.0, **kw),
                                   {"hits": (i32, NPOSES), "top": (i32, NPOSES), "height": (f32, NPOSES), "free": (u8, NPOSES)},
                                   ("hits", "top", "height", "free"), {"live_in": ones(NPOSES)})
    E["ps.leg_clearance"] = Entry(lambda ps, **kw: ps.leg_clearance(tx, ty, tz, angles, radius, 5.0, 3.0, **kw),
                                  {**per_leg(NPOSES, ("hits", i32), ("links", u8), ("worst", i32), ("pen", f32)), "free": (u8, NPOSES)},
                                  ("hits", "links", "worst", "pen", "free"), {"live_in": ones(NPOSES)})
    E["ps.self_clearance"] = Entry(lambda ps, **kw: ps.self_clearance(angles, radius, 5.0, 3.0, **kw),
                                   {**per_leg(NPOSES, ("hits", i32), ("with_", u8), ("links", u8), ("worst", u8), ("pen", f32)),
                                    "free": (u8, NPOSES)},
                                   ("hits", "with_", "links", "worst", "pen", "free"), {"pose_idx": poses, "live_in": ones(NPOSES)})
    E["ps.trunk_clearance"] = Entry(lambda ps, **kw: ps.trunk_clearance(angles, radius, 150.0, 60.0, -60.0, 5.0, 3.0, **kw),
                                    {**per_leg(NPOSES, ("hit", u8), ("worst", u8), ("pen", f32)), "free": (u8, NPOSES)},
                                    ("hit", "worst", "pen", "free"), {"pose_idx": poses, "live_in": ones(NPOSES)})
    E["ps.leg_joints"] = Entry(lambda ps, **kw: ps.leg_joints(angles, 3.0, **kw), {"out": (f32, 12 * nl * NPOSES)}, ("out",))
    nq = nl * NPOSES
    E["ps.ik"] = Entry(lambda ps, **kw: ps.ik(tx, ty, tz, target_idx=best.view(-1), **kw), {"out": (FIELD, nq), "status": (u8, nq)},
                       ("out", "status"), {"pose_idx": pose_l, "leg_idx": leg_l})
    E["ps.fk"] = Entry(lambda ps, **kw: ps.fk(angles[0], angles[1], angles[2], **kw), {"out": (FIELD, nq)}, ("out",),
                       {"pose_idx": pose_l, "leg_idx": leg_l})
    E["ps.reach_dist"] = Entry(lambda ps, **kw: ps.reach_dist(tx, ty, tz, **kw), {"mask": (u8, NT), "out": (FIELD, NT), "valid": (u8, NT)},
                               ("mask", "out", "valid"), {"pose_idx": pose_q, "leg_idx": leg_q})
    assert sorted(E) == sorted(NAMES)
    bare = d.PoseSet(legs, NPOSES).update(quats, body)  # neither table
    fresh = d.PoseSet(legs, NPOSES, ik=True, footholds=True)  # never updated
    return dict(torch=torch, E=E, ps=ps, bare=bare, fresh=fresh, t=(tx, ty, tz), quats=quats, body=body, edges=(ea, eb), foot=best,
                foot_e=foot_e, swing=(ffrom, fto))


SENTINEL = {"torch.uint8": 0xA5, "torch.int32": -7, "torch.int64": 0x25A5A5A5A5A5A5A5, "torch.float32": -7.0, "torch.float64": -7.0}


def full(torch, shape, dtype, device="cuda"):
    return torch.full(shape, SENTINEL[str(dtype)], dtype=dtype, device=device)


def untouched(torch, buf):
    return bool((buf == SENTINEL[str(buf.dtype)]).all())


def bits(torch, t):
    return t.contiguous().view(-1).view(torch.uint8)


def long_outputs(torch, entry):
    """{keyword: (the tensor to pass, the buffer behind it)}: one element more than needed, sentinel-filled"""
    out = {}
    for k, (kind, n) in entry.outs.items():
        buf = full(torch, (3, n + 1), torch.float32) if kind == FIELD else full(torch, (n + 1,), kind)
        out[k] = (buf[:, :n] if kind == FIELD else buf, buf)
    return out


def bad_outputs(torch, kind, n):
    """the four tensors no output may be: mistyped, one element short, strided, on the host"""
    if kind == FIELD:
        return {"dtype": full(torch, (3, n + 1), torch.float64)[:, :n], "short": full(torch, (3, n - 1), torch.float32),
                "strided": full(torch, (3, 2 * n), torch.float32)[:, ::2], "cpu": full(torch, (3, n + 1), torch.float32, "cpu")[:, :n]}
    return {"dtype": full(torch, (n + 1,), torch.float64), "short": full(torch, (n - 1,), kind),
            "strided": full(torch, (2 * n + 2,), kind)[::2], "cpu": full(torch, (n + 1,), kind, "cpu")}


@pytest.mark.parametrize("name", NAMES)
def test_given_outputs_are_used_as_they_are(scene, name):
    torch, entry, ps = scene["torch"], scene["E"][name], scene["ps"]
    base = entry.run(ps)
    outs = long_outputs(torch, entry)
    got = entry.run(ps, **{k: v[0] for k, v in outs.items()})
    torch.cuda.synchronize()
    assert set(got) == set(base) == set(entry.outs)
    for k, (kind, n) in entry.outs.items():
        given, buf = outs[k]
        assert got[k] is given, k
        numel = 3 * n if kind == FIELD else n
        assert base[k].numel() == numel and base[k].dtype == (torch.float32 if kind == FIELD else kind), k
        head = given if kind == FIELD else buf[:n]
        assert torch.equal(bits(torch, head), bits(torch, base[k])), k
        assert untouched(torch, buf[:, n:] if kind == FIELD else buf[n:]), k


@pytest.mark.parametrize("name", NAMES)
def test_a_bad_output_is_refused_before_any_launch(scene, name):
    torch, entry, ps = scene["torch"], scene["E"][name], scene["ps"]
    outs = long_outputs(torch, entry)
    for k, (kind, n) in entry.outs.items():
        for why, bad in bad_outputs(torch, kind, n).items():
            with pytest.raises(ValueError):  # a bad output that is accepted shows here as DID NOT RAISE under (k, why)
                entry.run(ps, **{**{o: v[0] for o, v in outs.items()}, k: bad})
            torch.cuda.synchronize()
            assert all(untouched(torch, v[1]) for o, v in outs.items() if o != k), (k, why)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in FREE[:11] + ["ps.footholds", "ps.foothold_lists", "ps.leg_joints"]])
def test_a_short_optional_input_is_refused_before_any_launch(scene, name):
    torch, entry, ps = scene["torch"], scene["E"][name], scene["ps"]
    assert entry.inputs
    outs = long_outputs(torch, entry)
    for k, valid in entry.inputs.items():
        assert valid.dim() == 1 and valid.numel() >= 2
        with pytest.raises(ValueError):
            entry.run(ps, **{**{o: v[0] for o, v in outs.items()}, k: valid[:-1]})
        torch.cuda.synchronize()
        assert all(untouched(torch, v[1]) for v in outs.values()), k


def test_every_optional_input_of_the_issue_is_covered(scene):
    seen = set().union(*(e.inputs for e in scene["E"].values()))
    assert seen >= {"live_in", "pose_live", "pose_idx", "leg_idx", "edge_b"}


@pytest.mark.parametrize("name", FH_METHODS + IK_METHODS + ["ps.reach_dist"])
def test_poseset_refuses_a_query_it_cannot_answer(scene, name):
    """before update(), and on a set built without the table the method reads"""
    entry = scene["E"][name]
    with pytest.raises(ValueError):
        entry.run(scene["fresh"])
    if name != "ps.reach_dist":  # it reads the pose records only, which every set has
        with pytest.raises(ValueError):
            entry.run(scene["bare"])
    else:
        entry.run(scene["bare"])


def test_poseset_transit_and_stance_wrappers_want_the_poses_of_the_last_update(scene):
    torch, ps, fresh = scene["torch"], scene["ps"], scene["fresh"]
    (tx, ty, tz), quats, body, (ea, eb) = scene["t"], scene["quats"], scene["body"], scene["edges"]
    ffrom, fto = scene["swing"]
    calls = {"stance_stability": lambda s, q, b, eb: s.stance_stability(tx, ty, tz, scene["foot"], q, b),
             "edge_transit": lambda s, q, b, eb: s.edge_transit(tx, ty, tz, q, b, ea, eb, scene["foot_e"], NSAMPLES),
             "swing_transit": lambda s, q, b, eb: s.swing_transit(tx, ty, tz, q, b, ea, eb, ffrom, fto, NSAMPLES)}
    for name, call in calls.items():
        with pytest.raises(ValueError):
            call(fresh, quats, body, eb)
        with pytest.raises(ValueError):
            call(ps, quats[:2], body[:2], eb)  # not the pose count of the last update()
        if name != "stance_stability":
            with pytest.raises(ValueError):
                call(ps, quats, body, eb + NPOSES)  # check=True reads the edges back
        call(ps, quats, body, eb)
    torch.cuda.synchronize()
