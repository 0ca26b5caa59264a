"""Pose-graph routes on the device (run with -m gpu on an MI355X): device.pose_routes / PoseSet.routes / lrm_pose_routes_dev
against the host loop lrm_pose_routes_cpu bit for bit (cost, hops, pred_edge, pred_pose, reached) over edge counts around the
wave, chunk and grid boundaries of the exported launch plan, pose counts around the wave and past the finish grid, the main
lattice of tests/routes_cases.py under every direction with and without each optional input, a chain stored back to front,
the cut (rounds = 1, then resume until done), dead and bad inputs at six places of a chunk, the NULL forms of the C ABI,
views of longer buffers, refused tensors, two streams, one graph replay after edge_live was rewritten, and the chain
update -> footholds -> foothold_edges -> edge_transit -> routes on ONE PoseSet against the host chain.
tests/test_pose_routes_cpu.py ties that host loop to the pure-Python model.  Every output is prefilled with a sentinel, so an
unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import foothold_edges_cases as fe
import pair_cases as pc
import routes_cases as rc
import transit_cases as tr

pytestmark = pytest.mark.gpu

SENT = -77
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
HEAD = open(os.path.join(CSRC, "lrm_pose_routes.h")).read()
FINISH_LANES = int(re.search(r"#define LRM_ROUTES_FINISH_GRID (\d+)", HEAD).group(1)) * int(re.search(r"#define LRM_ROUTES_BLOCK (\d+)", HEAD).group(1))
INPUTS = ("edge_live", "pose_live", "edge_cost")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan(lrm):
    p = lrm.dbg_pose_routes_plan(1)
    assert p["chunk"] % 256 == 0 and p["chunk"] >= 256 and p["grid_cap"] >= 1 and p["sweeps"] >= 1
    return p


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(torch, nposes, extra=0):
    full = lambda n, dt: torch.full((n + extra,), SENT, dtype=dt, device="cuda")
    return {"cost": full(nposes, torch.int64), "hops": full(nposes, torch.int32), "pred_edge": full(nposes, torch.int32),
            "pred_pose": full(nposes, torch.int32), "reached": full(1, torch.int32), "done": full(1, torch.int32)}


def run(lrm, torch, c, direction=0, rounds=64, drop=(), extra=0, tensors=None, **kw):
    """device.pose_routes into sentinel-filled outputs (drop: the optional outputs passed as NULL; extra: every output is a
    view of a buffer that much longer, whose tail must stay untouched) -> dict of numpy arrays, None for a dropped one"""
    n = c["nposes"]
    t = tensors or {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    out = outputs(torch, n, extra)
    give = {k: (None if k in drop else (v[:n] if k in rc.KEYS else v[:1])) for k, v in out.items()}
    want = {f"want_{k}": k not in drop for k in rc.KEYS}
    lrm.device.pose_routes(n, t["edge_a"], t["edge_b"], t["sources"], t["edge_live"], t["pose_live"], t["edge_cost"], direction, rounds,
                           **give, **want, **kw)
    torch.cuda.synchronize()
    got = {}
    for k, v in out.items():
        m = n if k in rc.KEYS else 1
        a = v.cpu().numpy()
        assert (a[m:] == SENT).all(), k
        assert k not in drop or (a == SENT).all(), k
        got[k] = None if k in drop else a[:m]
    return got


def same(got, want, what=""):
    rc.assert_same({**got, "reached": got["reached"][0]}, {k: (None if got.get(k) is None and k in rc.KEYS else v) for k, v in want.items()}, what)


def check(lrm, torch, c, direction=0, **kw):
    want = rc.host(lrm, c, direction)
    got = run(lrm, torch, c, direction, **kw)
    assert got["done"][0] >= 1
    same(got, want, direction)
    return want


def test_the_constants_are_the_kernels(lrm, plan):
    const = lambda name: int(re.search(rf"#define {name} (\d+)", HEAD).group(1))
    assert plan["chunk"] == const("LRM_ROUTES_BLOCK") * const("LRM_ROUTES_EDGES_PER_LANE") and plan["grid_cap"] == const("LRM_ROUTES_MAX_GRID")
    assert plan["sweeps"] == const("LRM_ROUTES_SWEEPS")
    src = open(os.path.join(CSRC, "lrm_pose_routes.hip")).read()
    assert "grid_for(A.nposes, LRM_ROUTES_FINISH_GRID)" in src and "constexpr int kBlock = LRM_ROUTES_BLOCK;" in src


EDGE_COUNTS = ["1", "63", "64", "65", "C-1", "C", "C+1", "2C+1", "GC+1"]


@pytest.mark.parametrize("which", EDGE_COUNTS)
def test_every_edge_count(lrm, torch_cuda, plan, which):
    """random graphs on 2 to 4 096 poses; the last count is one edge past what the capped grid takes in one stride"""
    ne = eval(which.replace("GC", "G*C").replace("2C", "2*C"), {"C": plan["chunk"], "G": plan["grid_cap"]})
    assert lrm.dbg_pose_routes_plan(ne)["workgroups"] == min(plan["grid_cap"], -(-ne // plan["chunk"]))
    c = rc.random_graph(min(4096, max(2, ne // 3)), ne, seed=len(which) + ne % 89, bad=0.02 if ne > 10 else 0.0)
    want = check(lrm, torch_cuda, c)
    assert ne < 64 or want["reached"] > c["nposes"] // 4


@pytest.mark.parametrize("nposes", [1, 2, 63, 64, 65, 257, FINISH_LANES + 1])
def test_every_pose_count(lrm, torch_cuda, nposes):
    """the last count is one pose past the finish launches' grid: a lane strides on"""
    c = rc.random_graph(nposes, 3 * nposes, seed=nposes % 71, nsources=3)
    for direction in (0, 1):
        want = check(lrm, torch_cuda, c, direction)
    assert nposes < 63 or want["reached"] > nposes // 8


@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("seed", rc.MAIN_SEEDS)
def test_the_main_lattice(lrm, torch_cuda, seed, direction):
    """with and without each optional input"""
    c = rc.main(seed)
    for drop in ((), ("edge_live",), ("pose_live",), ("edge_cost",), INPUTS):
        want = check(lrm, torch_cuda, {**c, **{k: None for k in drop}}, direction)
        assert want["reached"] > (256, 1, 0)[direction]  # node 0 is no edge's b: nothing leads out of it against the arrows


def test_a_chain_stored_back_to_front(lrm, torch_cuda):
    """the order in which a sweep gains least; 4 096 launches are enqueued and almost all of them return at once"""
    c = rc.chain(300, backwards=True)
    want = check(lrm, torch_cuda, c, rounds=4096, sync=False)
    assert want["hops"][299] == 299
    check(lrm, torch_cuda, rc.chain(300, backwards=True, cost=7), direction=1, rounds=4096, sync=False)


@pytest.mark.parametrize("name", ["chain"] + [f"lattice{s}" for s in rc.MAIN_SEEDS[:2]])
def test_the_cut(lrm, torch_cuda, name):
    """rounds = 1 cannot prove a fixed point it has just changed: done == -1; then resume = 1 with rounds = 2 until done >= 1.  The
    final bits equal the one-shot call's."""
    torch = torch_cuda
    c = rc.chain(40) if name == "chain" else rc.main(int(name[7:]))
    want = check(lrm, torch, c)
    ws = lrm.device.pose_routes_workspace(c["nposes"], 2, "cuda")
    t = {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    got = run(lrm, torch, c, rounds=1, sync=False, workspace=ws, tensors=t)
    assert got["done"][0] == -1
    calls = 0
    while got["done"][0] < 1:
        calls += 1
        assert calls <= (41 if name == "chain" else c["nposes"])
        got = run(lrm, torch, c, rounds=2, sync=False, resume=True, workspace=ws, tensors=t)
    same(got, want, name)
    # and sync=True does the same by itself
    got = run(lrm, torch, c, rounds=1, workspace=ws, tensors=t)
    assert got["done"][0] == 1
    same(got, want, name)


@pytest.mark.parametrize("kind", ["edge_live", "a_negative", "b_nposes", "a_min", "b_max", "cost", "pose_a", "pose_b"])
def test_dead_and_bad_inputs_at_six_places_of_a_chunk(lrm, torch_cuda, plan, kind):
    """the first, last and middle lanes of the first and the last wave of the first and of the second chunk"""
    C_ = plan["chunk"]
    n = 2 * C_ + 1
    e = np.arange(2 * C_)  # the chain 0 - 1 - ... at cost 1, then a by-pass i - i+2 at cost 5 for every second edge
    a, b = np.concatenate([e, e[:-1:2]]), np.concatenate([e + 1, e[:-1:2] + 2])
    base = rc.case(n, a, b, [0], np.ones(len(a), np.uint8), np.ones(n, np.uint8), np.concatenate([np.ones(2 * C_), np.full(C_, 5)]))
    clean = rc.host(lrm, base)
    assert clean["reached"] == n and clean["cost"][n - 1] == n - 1
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    places = [k * C_ + p for k in (0, 1) for p in (0, 31, 63, C_ - 64, C_ - 33, C_ - 1) if k * C_ + p > 0]
    for p in places:
        if kind == "edge_live":
            c["edge_live"][p] = 0
        elif kind == "cost":
            c["edge_cost"][p] = -1 - p
        elif kind.startswith("pose"):
            c["pose_live"][p if kind == "pose_a" else p + 1] = 0
        else:
            c["edge_" + kind[0]][p] = {"a_negative": -1, "b_nposes": n, "a_min": -2 ** 31, "b_max": 2 ** 31 - 1}[kind]
    want = check(lrm, torch_cuda, c, rounds=256)
    assert want["cost"][n - 1] > clean["cost"][n - 1] or want["reached"] < n  # the damage shows


def raw_call(lrm, torch, nposes, t, o, ws, rounds=128, direction=0, resume=0):
    rc_ = lrm.lib().lrm_pose_routes_dev(nposes, *(None if t[k] is None else t[k].data_ptr() for k in ("edge_a", "edge_b")), t["edge_a"].numel(),
                                        *(None if t[k] is None else t[k].data_ptr() for k in INPUTS),
                                        None if t["sources"] is None else t["sources"].data_ptr(), 0 if t["sources"] is None else t["sources"].numel(),
                                        direction, None if ws is None else ws.data_ptr(), rounds, resume,
                                        *(None if o[k] is None else o[k].data_ptr() for k in rc.KEYS + ("reached", "done")),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc_


def test_the_null_forms(lrm, torch_cuda):
    torch = torch_cuda
    c = rc.main(rc.MAIN_SEEDS[2])
    want = rc.host(lrm, c)
    n = c["nposes"]
    t = {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    ws = lrm.device.pose_routes_workspace(n, 128, "cuda")
    assert want["hops"].max() < 127  # a launch gains a hop at least: raw_call's 128 launches suffice whatever the order
    names = rc.KEYS + ("reached", "done")
    drops = [(k,) for k in names] + [tuple(k for k in rc.KEYS if k != keep) + ("reached", "done") for keep in rc.KEYS]
    for drop in drops:
        o = outputs(torch, n)
        assert raw_call(lrm, torch, n, t, {k: (None if k in drop else v) for k, v in o.items()}, ws) == 0, drop
        for k in names:
            a = o[k].cpu().numpy()
            if k in drop:
                assert (a == SENT).all(), (drop, k)
            elif k in rc.KEYS:
                assert np.array_equal(a, want[k]), (drop, k)
        assert "reached" in drop or o["reached"].item() == want["reached"]
        assert "done" in drop or o["done"].item() >= 1
    for drop in ([], ["pred_edge"]):  # through the Python layer too: pred_pose without pred_edge takes its minimum in place
        got = run(lrm, torch, c, direction=2, drop=drop)
        same(got, rc.host(lrm, c, 2), drop)
    # the refusals that come after the no-op
    o = outputs(torch, n)
    assert raw_call(lrm, torch, n, t, o, None) == -1
    assert raw_call(lrm, torch, n, {**t, "edge_b": None}, o, ws) == -1
    assert raw_call(lrm, torch, n, {**t, "sources": None}, {**o}, ws) == 0  # no source: nsources is 0 here
    assert (o["hops"].cpu().numpy() == -1).all() and o["reached"].item() == 0 and o["done"].item() == 1
    assert raw_call(lrm, torch, n, t, {**o, **{k: None for k in rc.KEYS}}, ws) == -1
    # nposes == 0 writes reached = 0 and done = 1, whatever the other pointers
    o = outputs(torch, 0)
    assert raw_call(lrm, torch, 0, {k: None for k in t} | {"edge_a": torch.empty(0, dtype=torch.int32, device="cuda")}, o, None) == 0
    assert o["reached"].item() == 0 and o["done"].item() == 1


def test_views_into_longer_buffers(lrm, torch_cuda):
    torch = torch_cuda
    c = rc.random_graph(500, 2600, seed=9)
    want = rc.host(lrm, c, 1)
    t = {}
    for k in rc.ARGS[1:]:
        pad = np.full(5, 3, c[k].dtype)
        t[k] = dev(torch, np.concatenate([pad, c[k], pad]))[5:5 + len(c[k])]
    ws = lrm.device.pose_routes_workspace(500, 64, "cuda")
    big = torch.zeros(ws.numel() + 64, dtype=torch.uint8, device="cuda")
    got = run(lrm, torch, c, 1, extra=7, tensors=t, workspace=big[16:])
    assert got["done"][0] >= 1
    same(got, want)


def test_refused_tensors(lrm, torch_cuda):
    torch = torch_cuda
    c = rc.main(rc.MAIN_SEEDS[0])
    n = c["nposes"]
    t = {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    call = lambda **kw: lrm.device.pose_routes(n, **{**t, **kw})
    call()
    bad = [dict(edge_a=t["edge_a"].long()), dict(edge_b=t["edge_b"].cpu()), dict(edge_b=t["edge_b"][:-1]), dict(sources=t["sources"].long()),
           dict(edge_live=t["edge_live"][1:]), dict(edge_live=t["edge_live"].int()), dict(pose_live=t["pose_live"][:-1]),
           dict(pose_live=t["pose_live"].cpu()), dict(edge_cost=t["edge_cost"].long()), dict(edge_cost=t["edge_cost"][::2]),
           dict(cost=torch.zeros(n, dtype=torch.int32, device="cuda")), dict(hops=torch.zeros(n - 1, dtype=torch.int32, device="cuda")),
           dict(pred_edge=torch.zeros(n, dtype=torch.int32)), dict(pred_pose=torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]),
           dict(reached=torch.zeros(1, dtype=torch.int64, device="cuda")), dict(done=torch.zeros(0, dtype=torch.int32, device="cuda")),
           dict(workspace=torch.zeros(8 * n, dtype=torch.uint8, device="cuda")), dict(rounds=0), dict(rounds=4097),
           dict(want_cost=False, want_hops=False, want_pred_edge=False, want_pred_pose=False)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(lrm.LrmError):
        call(direction=3)
    torch.cuda.synchronize()


def test_two_streams_with_two_workspaces(lrm, torch_cuda):
    torch = torch_cuda
    cases = [rc.main(rc.MAIN_SEEDS[3]), rc.random_graph(3000, 20000, seed=5)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    t = [{k: dev(torch, c[k]) for k in rc.ARGS[1:]} for c in cases]
    outs = [outputs(torch, c["nposes"]) for c in cases]
    ws = [lrm.device.pose_routes_workspace(c["nposes"], 256, "cuda") for c in cases]
    assert all(rc.host(lrm, c, i)["hops"].max() < 255 for i, c in enumerate(cases))  # a launch gains a hop at least: 256 suffice
    torch.cuda.synchronize()
    for _ in range(3):
        for i, c in enumerate(cases):
            with torch.cuda.stream(streams[i]):
                lrm.device.pose_routes(c["nposes"], t[i]["edge_a"], t[i]["edge_b"], t[i]["sources"], t[i]["edge_live"], t[i]["pose_live"],
                                       t[i]["edge_cost"], i, 256, sync=False, workspace=ws[i], **outs[i])
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        got = {k: v.cpu().numpy() for k, v in outs[i].items()}
        assert got["done"][0] >= 1
        same(got, rc.host(lrm, c, i), i)


def test_call_replays_from_a_graph(lrm, torch_cuda, plan):
    """one captured call with sync=False and rounds from an eager call's done plus 2: a single linear chain of launches;
    replayed after edge_live was rewritten in place and compared with the host loop on the new bytes.  How many launches a call
    needs varies from call to call (which workgroup sees which key first), so the graph is chosen for a count that cannot
    exceed the captured chain: all its edges lie in ONE chunk, whose workgroup gains at least one hop per sweep, so a deepest
    route of H hops is final after ceil(H / K) launches and proven by the next; an eager done is at least 2, and H <= 3 K."""
    torch = torch_cuda
    c = {**rc.lattice(8, 3, 0.75, 0.95), "edge_cost": None}
    n = c["nposes"]
    assert len(c["edge_a"]) <= plan["chunk"]
    t = {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    eager = run(lrm, torch, c, tensors=t)
    assert eager["done"][0] >= 2
    rounds = int(eager["done"][0]) + 2
    own = [0, 8 * 7, 2 * 8 * 7]
    assert (c["edge_a"][own] == 0).all()
    new_live = np.random.default_rng(77).permutation(c["edge_live"])
    new_live[own] = c["edge_live"][own]  # node 0 keeps its three edges as they are
    want = rc.host(lrm, {**c, "edge_live": new_live})
    assert want["reached"] > 32 and not np.array_equal(want["pred_edge"], eager["pred_edge"])
    assert -(-int(want["hops"].max()) // plan["sweeps"]) + 1 <= 4 <= rounds  # the captured chain is long enough, whatever the order
    out = outputs(torch, n)
    ws = lrm.device.pose_routes_workspace(n, rounds, "cuda")
    work = lambda: lrm.device.pose_routes(n, t["edge_a"], t["edge_b"], t["sources"], t["edge_live"], t["pose_live"], t["edge_cost"], 0, rounds,
                                          sync=False, workspace=ws, **out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        t["edge_live"].copy_(dev(torch, new_live))
        for v in out.values():
            v.fill_(SENT)
        g.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["done"][0] >= 1
    same(got, want)
    del g


def test_chain_on_one_pose_set_against_the_host_chain(lrm, torch_cuda):
    """update -> footholds -> foothold_edges(check=False) -> edge_transit -> routes(edge_live = clear, pose_live = all_legs)"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=13)
    t = dev(torch, targets.T.copy())
    q, b, a, bb = dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb)
    ps = lrm.PoseSet(legs, len(quats), footholds=True, nominal=nominal).update(q, b)
    _, _, _, pose_all = ps.footholds(t[0], t[1], t[2])
    _, best, _, _ = ps.foothold_edges(t[0], t[1], t[2], a, bb, check=False)
    clear = ps.edge_transit(t[0], t[1], t[2], q, b, a, bb, best, 9, check=False)[6]
    h_pose_all = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[3]
    h_best, _ = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    h_clear = tr.host(lrm, targets, quats, body, legs, ea, eb, h_best, 9)["clear"]
    usable = (h_clear != 0) & (ea != eb) & (h_pose_all[ea] != 0) & (h_pose_all[eb] != 0)
    sources = np.concatenate([ea[usable][:2], eb[usable][-1:]]).astype(np.int32)  # ends of transitions that survive
    assert usable.sum() >= 2 and 0 < h_clear.sum() < len(h_clear) and 0 < h_pose_all.sum() < len(h_pose_all)
    for direction in (0, 1, 2):
        out = outputs(torch, len(quats))
        ps.routes(a, bb, dev(torch, sources), edge_live=clear, pose_live=pose_all, direction=direction, **out)
        torch.cuda.synchronize()
        want = rc.host(lrm, rc.case(len(quats), ea, eb, sources, h_clear, h_pose_all), direction)
        same({k: v.cpu().numpy() for k, v in out.items()}, want, direction)
        assert want["reached"] > len(set(sources.tolist())) or direction  # the routes leave the sources


def test_route_path(lrm, torch_cuda):
    torch = torch_cuda
    c = rc.main(rc.MAIN_SEEDS[0])
    t = {k: dev(torch, c[k]) for k in rc.ARGS[1:]}
    cost, hops, pe, pp, reached, done = lrm.device.pose_routes(c["nposes"], **t)
    h = hops.cpu().numpy()
    goal = int(np.argmax(h))
    poses, edges = lrm.device.route_path(pp, pe, goal, hops)
    assert poses[0] == 0 and poses[-1] == goal and len(edges) == h[goal] == len(poses) - 1
    total = 0
    for k, e in enumerate(edges):
        assert {int(c["edge_a"][e]), int(c["edge_b"][e])} == {poses[k], poses[k + 1]} and c["edge_live"][e]
        total += int(c["edge_cost"][e])
    assert total == cost[goal].item()
    assert lrm.device.route_path(pp, pe, 0, hops) == ([0], [])
    with pytest.raises(ValueError):
        lrm.device.route_path(pp, pe, int(np.nonzero(h < 0)[0][0]), hops)
