"""Pose-graph edges on the device (run with -m gpu on an MI355X): device.pose_edge_counts / device.pose_edges / PoseSet.edges
against the host loop lrm_pose_edges_cpu bit for bit (counts, offsets, edge_a, edge_b, d2, cos2, written) over pose counts
around the wave, the workgroup and the walk round of the exported launch plan, every scene of tests/pose_edges_cases.py in both
forms, neighbours that straddle a chunk and a round boundary, a lattice in shuffled order (no box culls anything) and in
Morton order (most boxes cull), capacity cuts and hostile offsets, refused tensors, two streams with two workspaces, one graph
capture of counts -> offsets -> edges replayed after the bodies were rewritten in place, the plan's constants, and the chain
update -> edges -> footholds -> foothold_edges -> routes on ONE PoseSet in the launch-only form against the chain of host loops.
tests/test_pose_edges_cpu.py ties that host loop to the numpy models.  Every output is prefilled with a sentinel, so an
unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import foothold_edges_cases as fe
import pair_cases as pc
import pose_edges_cases as ec
import routes_cases as rc

pytestmark = pytest.mark.gpu

SENT = -77
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
FORMS = ("upper", "full")
LISTS = (("edge_a", np.int32), ("edge_b", np.int32), ("d2", np.float32), ("cos2", np.float32))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan(lrm):
    p = lrm.dbg_pose_edges_plan(1)
    assert p["chunk"] == 64 and p["round"] == 64 and p["block"] % 64 == 0 and p["workgroups"] == 1
    return p


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tensors(torch, c):
    return {k: dev(torch, c[k]) for k in ("quats", "body", "pose_live")}


def full(torch, n, dtype):
    return torch.full((n,), SENT, dtype={np.int32: torch.int32, np.float32: torch.float32, np.int64: torch.int64}[dtype], device="cuda")


def run(lrm, torch, c, form, offsets=None, capacity=None, extra=5, t=None, drop=()):
    """counts -> offsets -> edges into sentinel-filled views of buffers `extra` longer, whose tails must stay untouched; offsets
    / capacity: hostile ones instead of the counts' scan (host array, int) -> dict of numpy arrays"""
    t = t or tensors(torch, c)
    n = len(c["quats"])
    args = (t["quats"], t["body"], c["max_step"], c["max_turn"], t["pose_live"], FORMS[form])
    count = full(torch, n + extra, np.int32)
    lrm.device.pose_edge_counts(*args, count=count[:n])
    off = full(torch, n + 1 + extra, np.int64)
    if offsets is None:
        lrm.device.foothold_offsets(count[:n], out=off[:n + 1])
        capacity = int(off[n].item()) if capacity is None else capacity
    else:
        off[:n + 1].copy_(dev(torch, offsets))
    bufs = {k: full(torch, capacity + extra, dt) for k, dt in LISTS}
    written = full(torch, n + extra, np.int32)
    give = {k: (None if k in drop else v[:capacity]) for k, v in bufs.items()}
    lrm.device.pose_edges(*args, offsets=off[:n + 1], capacity=capacity, written=written[:n], want_d2="d2" not in drop,
                          want_cos2="cos2" not in drop, **give)
    torch.cuda.synchronize()
    got = {"count": count.cpu().numpy(), "offsets": off.cpu().numpy(), "written": written.cpu().numpy(), **{k: v.cpu().numpy() for k, v in bufs.items()}}
    for k, m in (("count", n), ("offsets", n + 1), ("written", n), *((k, capacity) for k, _ in LISTS)):
        assert (got[k][m:] == SENT).all(), k
        got[k] = got[k][:m]
    return got


def check(lrm, torch, c, form, **kw):
    """device == host loop, bit for bit -> the host answer"""
    want = ec.host(lrm, c, form)
    got = run(lrm, torch, c, form, **kw)
    ec.assert_same(got, want, form)
    assert np.array_equal(got["written"], want["count"])
    return want


def sized(n, seed):
    """n continuous random poses at about six neighbours each, in random order: no box culls much"""
    return ec.cloud(n, seed, box=max(100.0, (n * 3.05e6 / 6.0) ** (1.0 / 3.0)))


def test_the_constants_are_the_kernels(lrm, plan):
    head = open(os.path.join(CSRC, "lrm_pose_edges.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", head).group(1))
    assert plan["chunk"] == const("LRM_EDGES_CHUNK") and plan["round"] == const("LRM_EDGES_ROUND") and plan["block"] == const("LRM_EDGES_BLOCK")
    src = open(os.path.join(CSRC, "lrm_pose_edges.hip")).read()
    assert "constexpr int kBlock = LRM_EDGES_BLOCK;" in src and "constexpr int kChunk = LRM_EDGES_CHUNK;" in src
    assert "g0 += LRM_EDGES_ROUND" in src and src.count("lrm_edges_plan(A.nposes, plan)") == 2 and src.count("dim3((unsigned)plan[2]), dim3(kBlock)") == 3


POSE_COUNTS = ["1", "2", "63", "64", "65", "127", "128", "129", "B-1", "B", "B+1", "R-64", "R", "R+1", "R+65", "20000"]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("which", POSE_COUNTS)
def test_every_pose_count(lrm, torch_cuda, plan, which, form):
    """around the wave, the workgroup (B) and the poses one walk round covers (R = chunk x round, read from the plan); 20 000
    poses take several rounds"""
    n = eval(which, {"B": plan["block"], "R": plan["chunk"] * plan["round"]})
    assert lrm.dbg_pose_edges_plan(n)["workgroups"] == -(-n // plan["block"])
    want = check(lrm, torch_cuda, sized(n, seed=n % 97 + form), form)
    assert n < 63 or want["count"].sum() > n


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sorted(ec.SCENES))
def test_every_scene(lrm, torch_cuda, name, form):
    check(lrm, torch_cuda, ec.SCENES[name](), form)


def test_neighbours_across_a_chunk_and_a_round_boundary(lrm, torch_cuda, plan):
    """a chain of poses 50 mm apart along x: pose i steps to i + 1 and nowhere else, also where i and i + 1 lie in two chunks
    (63 | 64) and in two walk rounds (R - 1 | R)"""
    R = plan["chunk"] * plan["round"]
    n = R + 130
    c = ec.case(ec.identity(n), np.column_stack([np.arange(n) * ec.PITCH, np.zeros(n), np.zeros(n)]), ec.PITCH)
    up = check(lrm, torch_cuda, c, 0)
    assert np.array_equal(up["edge_a"], np.arange(n - 1)) and np.array_equal(up["edge_b"], np.arange(1, n))
    full_ = check(lrm, torch_cuda, c, 1)
    pairs = ec.pair_set(full_["edge_a"], full_["edge_b"])
    for i in (63, R - 1, R + 63):
        assert (i, i + 1) in pairs and (i + 1, i) in pairs
    # and with the chain folded so that the far end of the table is next to its start: the first chunk's row reaches round 1
    fold = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)[::-1]])
    cf = ec.permuted(c, fold)
    got = check(lrm, torch_cuda, cf, 1)
    assert ec.pair_set(fold[got["edge_a"]], fold[got["edge_b"]]) == pairs and (0, n - 1) in ec.pair_set(got["edge_a"], got["edge_b"])


@pytest.mark.parametrize("form", [0, 1])
def test_a_chain_past_one_round_of_group_boxes(lrm, torch_cuda, plan, form):
    """R x round + 130 poses 50 mm apart along x (multiples of 50 below 2^24 are float32 numbers): the second round over the
    group boxes, where only this size can go wrong.  The host loop is O(n^2); the answer is known: pose i steps to i + 1 (and
    back in form 1) at d2 = 2500 bit-exactly"""
    torch = torch_cuda
    n = plan["chunk"] * plan["round"] * plan["round"] + 130
    body = np.zeros((n, 3), np.float32)
    body[:, 0] = np.arange(n, dtype=np.float64) * ec.PITCH
    assert body[-1, 0] == (n - 1) * ec.PITCH < 2 ** 24
    c = ec.case(ec.identity(n), body, ec.PITCH)
    got = run(lrm, torch, c, form)
    i = np.arange(n - 1, dtype=np.int32)
    if form == 0:
        want_a, want_b = i, i + 1
    else:
        want_a = np.repeat(np.arange(n, dtype=np.int32), 2)[1:-1]
        want_b = np.column_stack([np.arange(n, dtype=np.int32) - 1, np.arange(n, dtype=np.int32) + 1]).reshape(-1)[1:-1]
    assert np.array_equal(got["edge_a"], want_a) and np.array_equal(got["edge_b"], want_b)
    assert (got["d2"] == 2500.0).all() and (got["cos2"] == 1.0).all() and np.array_equal(got["written"], got["count"])
    assert np.array_equal(got["count"], np.bincount(want_a, minlength=n))


def test_shuffled_and_morton_order_give_the_same_edge_set(lrm, torch_cuda):
    """a 20 x 20 x 12 lattice (75 chunks, two walk rounds) with one diagonal as the step: shuffled, every chunk's box is the
    whole lattice and nothing is culled; in Morton order a chunk is a small brick and most boxes are; the pairs of bodies are
    the same"""
    shape, step = (20, 20, 12), ec.PITCH * 3 ** 0.5
    sets = {}
    for order in ("shuffled", "morton", "raster"):
        c = ec.lattice(*shape, order, max_step=step)
        h = check(lrm, torch_cuda, c, 0)
        key = lambda i: [tuple(r) for r in (c["body"][i] / ec.PITCH).astype(np.int64)]
        sets[order] = {frozenset(ab) for ab in zip(key(h["edge_a"]), key(h["edge_b"]))}
        # what the cull sees: the share of chunk pairs whose boxes are within a step
        lo = np.stack([c["body"][i:i + 64].min(0) for i in range(0, len(c["body"]), 64)]).astype(np.float64)
        hi = np.stack([c["body"][i:i + 64].max(0) for i in range(0, len(c["body"]), 64)]).astype(np.float64)
        gap = np.maximum(np.maximum(lo[None] - hi[:, None], lo[:, None] - hi[None]), 0.0)
        near = ((gap ** 2).sum(-1) <= step * step).mean()
        assert near == 1.0 if order == "shuffled" else near < 0.5, (order, near)
    assert sets["shuffled"] == sets["morton"] == sets["raster"] and len(sets["morton"]) > ec.lattice_pairs(*shape)


@pytest.mark.parametrize("form", [0, 1])
def test_capacity_cuts_and_hostile_offsets(lrm, torch_cuda, form):
    torch = torch_cuda
    c = ec.SCENES["cloud"]()
    t = tensors(torch, c)
    h = ec.host(lrm, c, form)
    for name, offsets, capacity in ec.hostile_offsets(h["count"], 5):
        got = run(lrm, torch, c, form, offsets=offsets, capacity=capacity, t=t)
        want = ec.expect_rows(h, offsets, capacity, SENT)
        assert np.array_equal(got["written"], want[4]) and np.array_equal(got["count"], h["count"]), name
        for (k, _), w in zip(LISTS, want):
            if name == "random":  # overlapping segments hold one of the rows that claim them: untouched outside them
                assert np.array_equal(got[k].view(np.int32)[w == SENT], w.view(np.int32)[w == SENT]), (name, k)
            else:
                assert np.array_equal(got[k].view(np.int32), w.view(np.int32)), (name, k)
    got = run(lrm, torch, c, form, t=t, drop=("d2", "cos2"))  # NULL d2_out and cos2_out: the sentinels stay
    assert (got["d2"] == SENT).all() and (got["cos2"] == SENT).all() and np.array_equal(got["edge_b"], h["edge_b"])


def test_the_allocating_forms(lrm, torch_cuda):
    """capacity=None reads offsets[-1] back and returns exactly the list; a capacity returns edge_a with -1 beyond it"""
    torch = torch_cuda
    c = ec.SCENES["oriented"]()
    t = tensors(torch, c)
    h = ec.host(lrm, c, 1)
    total = len(h["edge_a"])
    ea, eb, off, d2, cos2, written = lrm.device.pose_edges(t["quats"], t["body"], c["max_step"], c["max_turn"], form="full")
    got = {"edge_a": ea, "edge_b": eb, "offsets": off, "d2": d2, "cos2": cos2, "count": written}
    ec.assert_same({k: v.cpu().numpy() for k, v in got.items()}, h, "exact")
    ea, eb, off, d2, cos2, written = lrm.device.pose_edges(t["quats"], t["body"], c["max_step"], c["max_turn"], form="full", capacity=total + 100,
                                                           want_d2=False, want_cos2=False)
    assert d2 is None and cos2 is None and ea.numel() == total + 100
    assert np.array_equal(ea.cpu().numpy()[:total], h["edge_a"]) and (ea.cpu().numpy()[total:] == -1).all() and np.array_equal(eb.cpu().numpy()[:total], h["edge_b"])
    # nothing to do
    e = lrm.device.pose_edges(torch.zeros((0, 4), device="cuda"), None, 1.0)
    assert e[0].numel() == 0 and e[2].cpu().tolist() == [0]


def test_refused_tensors(lrm, torch_cuda):
    torch = torch_cuda
    c = ec.SCENES["dead_mask"]()
    t = tensors(torch, c)
    n = len(c["quats"])
    base = dict(quats=t["quats"], body=t["body"], max_step=c["max_step"], max_turn=0.5, pose_live=t["pose_live"])
    call = lambda **kw: lrm.device.pose_edges(**{**base, **kw})
    counts = lambda **kw: lrm.device.pose_edge_counts(**{**base, **kw})
    call(), counts()
    i32 = lambda m, **kw: torch.zeros(m, dtype=torch.int32, device="cuda", **kw)
    bad = [dict(quats=t["quats"].double()), dict(quats=t["quats"].cpu()), dict(quats=t["quats"][:, :3]), dict(quats=t["quats"].t().contiguous().t()),
           dict(body=t["body"][:-1]), dict(body=t["body"].cpu()), dict(body=t["body"].half()), dict(body=t["body"][:, [0, 1, 2, 0]][:, :3]),
           dict(pose_live=t["pose_live"][:-1]), dict(pose_live=t["pose_live"].int()), dict(pose_live=t["pose_live"].cpu()),
           dict(pose_live=torch.ones(2 * n, dtype=torch.uint8, device="cuda")[::2]), dict(form="lower"), dict(form=0), dict(max_step=-1.0),
           dict(max_step=float("nan")), dict(max_turn=-0.1), dict(max_turn=4.0), dict(workspace=torch.zeros(8, dtype=torch.uint8, device="cuda")),
           dict(workspace=torch.zeros(4096, dtype=torch.float32, device="cuda"))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
        with pytest.raises(ValueError):
            counts(**kw)
    for kw in (dict(count=i32(n - 1)), dict(count=i32(n).long()), dict(count=i32(n).cpu()), dict(count=i32(2 * n)[::2])):
        with pytest.raises(ValueError):
            counts(**kw)
        with pytest.raises(ValueError):
            call(**kw)
    off = lrm.device.foothold_offsets(counts())
    for kw in (dict(offsets=off[:-1]), dict(offsets=off.int()), dict(offsets=off.cpu()), dict(offsets=off, capacity=-1), dict(offsets=off, capacity=8, edge_a=i32(7)),
               dict(offsets=off, capacity=8, edge_b=i32(8).long()), dict(offsets=off, capacity=8, d2=i32(8)), dict(offsets=off, capacity=8, cos2=torch.zeros(8)),
               dict(offsets=off, capacity=8, written=i32(n - 1)), dict(offsets=off, capacity=8, edge_a=i32(16)[::2])):
        with pytest.raises(ValueError):
            call(**kw)
    ps = lrm.PoseSet(pc.leg_families(lrm)["m2_6_tilted"][0], n)
    with pytest.raises(ValueError):
        ps.edges(t["quats"], t["body"], 50.0)  # before update()
    ps.update(t["quats"], t["body"])
    with pytest.raises(ValueError):
        ps.edges(t["quats"][:-1], t["body"][:-1], 50.0)  # not the poses of the last update()
    torch.cuda.synchronize()


def test_two_streams_with_two_workspaces(lrm, torch_cuda):
    torch = torch_cuda
    cases = [sized(5000, 31), ec.lattice(17, 15, 13, "morton", max_step=ec.PITCH * 2 ** 0.5)]
    want = [ec.host(lrm, c, i) for i, c in enumerate(cases)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    t = [tensors(torch, c) for c in cases]
    ws = [lrm.device.pose_edges_workspace(len(c["quats"]), "cuda") for c in cases]
    outs = []
    for c, w in zip(cases, want):
        n, cap = len(c["quats"]), len(w["edge_a"])
        outs.append({"count": full(torch, n, np.int32), "offsets": full(torch, n + 1, np.int64), "written": full(torch, n, np.int32),
                     **{k: full(torch, cap, dt) for k, dt in LISTS}})
    torch.cuda.synchronize()
    for _ in range(3):
        for i, c in enumerate(cases):
            with torch.cuda.stream(streams[i]):
                o = outs[i]
                args = (t[i]["quats"], t[i]["body"], c["max_step"], c["max_turn"], t[i]["pose_live"], FORMS[i])
                lrm.device.pose_edge_counts(*args, workspace=ws[i], count=o["count"])
                lrm.device.foothold_offsets(o["count"], out=o["offsets"])
                lrm.device.pose_edges(*args, offsets=o["offsets"], workspace=ws[i], edge_a=o["edge_a"], edge_b=o["edge_b"], d2=o["d2"], cos2=o["cos2"],
                                      written=o["written"])
    torch.cuda.synchronize()
    for i in range(2):
        ec.assert_same({k: v.cpu().numpy() for k, v in outs[i].items()}, want[i], i)
        assert np.array_equal(outs[i]["written"].cpu().numpy(), want[i]["count"])


def test_counts_offsets_edges_replay_from_a_graph(lrm, torch_cuda):
    """one capture of counts -> offsets -> edges with a fixed capacity and every tensor given: only launches; replayed after the
    bodies were rewritten in place and compared with the host loop on the new bodies"""
    torch = torch_cuda
    c = sized(3000, 41)
    new = ec.cloud(3000, 42, box=600.0)  # denser: other counts, other offsets
    c2 = {**c, "body": new["body"]}
    want = ec.host(lrm, c2, 0)
    first = ec.host(lrm, c, 0)
    n, cap = 3000, len(want["edge_a"]) + 1000
    assert len(first["edge_a"]) < len(want["edge_a"]) and not np.array_equal(first["count"], want["count"])
    t = tensors(torch, c)
    ws = lrm.device.pose_edges_workspace(n, "cuda")
    o = {"count": full(torch, n, np.int32), "offsets": full(torch, n + 1, np.int64), "written": full(torch, n, np.int32),
         **{k: full(torch, cap, dt) for k, dt in LISTS}}
    args = (t["quats"], t["body"], c["max_step"], c["max_turn"], None, "upper")

    def work():
        lrm.device.pose_edge_counts(*args, workspace=ws, count=o["count"])
        lrm.device.foothold_offsets(o["count"], out=o["offsets"])
        lrm.device.pose_edges(*args, offsets=o["offsets"], capacity=cap, workspace=ws, edge_a=o["edge_a"], edge_b=o["edge_b"], d2=o["d2"], cos2=o["cos2"],
                              written=o["written"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        t["body"].copy_(dev(torch, c2["body"]))
        for v in o.values():
            v.fill_(SENT)
        g.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    total = len(want["edge_a"])
    for k, _ in LISTS:
        assert (got[k][total:] == SENT).all(), k
        got[k] = got[k][:total]
    ec.assert_same(got, want, "replay")
    assert np.array_equal(got["written"], want["count"])
    del g


def test_chain_on_one_pose_set_against_the_host_chain(lrm, torch_cuda):
    """update -> edges -> footholds -> foothold_edges(check=False) -> routes(edge_live = all_legs) in the launch-only form: a
    fixed capacity, edge_a prefilled with -1, nedges = capacity; no read-back between the calls"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, _, _ = fe.scene(lrm, 48, 4000, seed=13)
    n, cap, step, turn = len(quats), 2048, 200.0, 2.0
    t = dev(torch, targets.T.copy())
    q, b = dev(torch, quats), dev(torch, body)
    ps = lrm.PoseSet(legs, n, footholds=True, nominal=nominal).update(q, b)
    ea = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    eb = torch.full((cap,), SENT, dtype=torch.int32, device="cuda")
    ea, eb, off, _, _, written = ps.edges(q, b, step, turn, capacity=cap, edge_a=ea, edge_b=eb)
    _, _, _, pose_all = ps.footholds(t[0], t[1], t[2])
    _, _, _, edge_all = ps.foothold_edges(t[0], t[1], t[2], ea, eb, check=False)
    # the host chain
    h = ec.host(lrm, ec.case(quats, body, step, turn), 0)
    total = len(h["edge_a"])
    assert 40 <= total < cap
    h_ea = np.concatenate([h["edge_a"], np.full(cap - total, -1, np.int32)])
    h_eb = np.concatenate([h["edge_b"], np.full(cap - total, SENT, np.int32)])
    h_pose_all = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[3]
    h_edge_all = fe.host(lrm, targets, quats, body, legs, nominal, h_ea, h_eb)["all_legs"]
    assert 0 < h_edge_all[:total].sum() < total and not h_edge_all[total:].any()
    usable = (h_edge_all[:total] != 0) & (h_pose_all[h["edge_a"]] != 0) & (h_pose_all[h["edge_b"]] != 0)
    sources = np.concatenate([h["edge_a"][usable][:2], h["edge_b"][usable][-1:]]).astype(np.int32)
    assert usable.sum() >= 2
    for direction in (0, 1, 2):
        out = {"cost": full(torch, n, np.int64), "hops": full(torch, n, np.int32), "pred_edge": full(torch, n, np.int32),
               "pred_pose": full(torch, n, np.int32), "reached": full(torch, 1, np.int32), "done": full(torch, 1, np.int32)}
        ps.routes(ea, eb, dev(torch, sources), edge_live=edge_all, pose_live=pose_all, direction=direction, **out)
        torch.cuda.synchronize()
        want = rc.host(lrm, rc.case(n, h_ea, h_eb, sources, h_edge_all, h_pose_all), direction)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        rc.assert_same({**got, "reached": got["reached"][0]}, want, direction)
        assert want["reached"] > len(set(sources.tolist())) or direction
    assert np.array_equal(ea.cpu().numpy(), h_ea) and np.array_equal(eb.cpu().numpy(), h_eb) and np.array_equal(written.cpu().numpy(), h["count"])
    assert np.array_equal(edge_all.cpu().numpy(), h_edge_all)
