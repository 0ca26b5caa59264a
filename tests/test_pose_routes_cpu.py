"""Pose-graph routes on the host (no GPU): lrm_pose_routes_cpu against the independent pure-Python model of
tests/routes_model.py bit for bit on every builder of tests/routes_cases.py and every direction; the definition's properties on
the host loop's own output; hand-made cases (ties, duplicates, zero-cost rings, self-loops, dead poses and sources, bad
indices, negative costs, the cost cap); every refusal of both forms in its order (the device form refuses before it touches a
device); the NULL forms; the empty sizes; the symbols; and the launch plan against the constants in the source."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import routes_cases as rc
import routes_model as rm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
SYMBOLS = ("lrm_pose_routes_dev", "lrm_pose_routes_cpu", "lrm_pose_routes_workspace_bytes", "lrm_dbg_pose_routes_plan")
BIG = 2147483647


def model(c, direction=0):
    return rm.routes(*(c[k] for k in rc.ARGS), direction)


def check(lrm, c, direction=0, what=""):
    """host == model, bit for bit -> (host answer, model answer)"""
    h, m = rc.host(lrm, c, direction), model(c, direction)
    rc.assert_same(h, rc.model_arrays(m), (what, direction))
    return h, m


BUILDERS = {
    "chain": lambda: rc.chain(40), "chain_back": lambda: rc.chain(40, backwards=True), "chain_cost": lambda: rc.chain(17, True, 3),
    "ring": lambda: rc.ring(9), "ring_zero": lambda: rc.ring(12, 0), "lattice5": lambda: rc.lattice(5, 7, 0.8, 0.9),
    "lattice32": lambda: rc.main(rc.MAIN_SEEDS[0]), "random_small": lambda: rc.random_graph(30, 200, 1), "random_sparse": lambda: rc.random_graph(400, 500, 2),
    "random_dense": lambda: rc.random_graph(64, 3000, 3, nsources=5), "random_unit": lambda: {**rc.random_graph(100, 600, 4), "edge_cost": None},
}


@pytest.mark.parametrize("name", sorted(BUILDERS))
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_host_loop_against_the_model(lrm, name, direction):
    c = BUILDERS[name]()
    h, _ = check(lrm, c, direction, name)
    if direction == 2:  # b -> a only is a -> b only on swapped arrays
        rc.assert_same(h, rc.host(lrm, rc.swapped(c), 1), name)


@pytest.mark.parametrize("seed", rc.MAIN_SEEDS)
def test_the_main_fixture_is_not_vacuous(seed):
    """asserted on the model alone: a reached share within [0.25, 0.9], a route of at least 40 hops, a pose with two tight
    incoming arcs"""
    c = rc.main(seed)
    assert len(c["edge_a"]) == rc.MAIN_EDGES and c["nposes"] == rc.MAIN_N ** 2
    m = model(c)
    print(seed, m["reached"] / c["nposes"], max(m["hops"]), max(m["tight"]))
    assert 0.25 <= m["reached"] / c["nposes"] <= 0.9
    assert max(m["hops"]) >= 40
    assert max(m["tight"]) >= 2


@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("seed", rc.MAIN_SEEDS)
def test_the_definitions_properties_on_the_host_loops_output(lrm, seed, direction):
    c = rc.main(seed) if seed in rc.MAIN_SEEDS[:2] else rc.random_graph(300, 1500, seed)
    h = rc.host(lrm, c, direction)
    arcs = rm.arcs_of(*(c[k] for k in ("nposes", "edge_a", "edge_b", "edge_live", "pose_live", "edge_cost")), direction)
    key = [None if h["hops"][p] < 0 else (int(h["cost"][p]), int(h["hops"][p])) for p in range(c["nposes"])]
    assert all((h["cost"][p] < 0) == (h["hops"][p] < 0) for p in range(c["nposes"]))
    tight_min = {}
    for e, u, v, w in arcs:
        if key[u] is None:
            continue
        cand = (key[u][0] + w, key[u][1] + 1)
        assert cand[0] > rm.CAP or (key[v] is not None and key[v] <= cand), (e, u, v)  # no usable arc offers a lower key
        if cand == key[v]:
            tight_min.setdefault(v, (e, u))
    live = lambda p: 0 <= p < c["nposes"] and (c["pose_live"] is None or c["pose_live"][p] != 0)
    sources = {int(s) for s in c["sources"] if live(int(s))}
    for p in range(c["nposes"]):
        pe, pp = int(h["pred_edge"][p]), int(h["pred_pose"][p])
        if key[p] is None or p in sources:
            assert (pe, pp) == (-1, -1) and (key[p] is None or key[p] == (0, 0))
            continue
        assert (pe, pp) == tight_min[p]  # tight, and the smallest such edge
        q, steps = p, 0
        while h["pred_pose"][q] >= 0:
            q, steps = int(h["pred_pose"][q]), steps + 1
            assert steps <= c["nposes"]
        assert q in sources and steps == key[p][1]  # the chain ends at a source after hops steps
    assert h["reached"] == sum(k is not None for k in key)


def answer(lrm, nposes, edges, sources, direction=0, **kw):
    a, b = (np.array([e[i] for e in edges], np.int32) for i in (0, 1))
    c = rc.case(nposes, a, b, sources, edge_cost=[e[2] for e in edges] if edges and len(edges[0]) > 2 else None, **kw)
    return check(lrm, c, direction)[0]


def test_a_cost_tie_goes_to_fewer_hops(lrm):
    # 0 -> 3 by 0-1-2-3 (1 + 1 + 1) or by 0-3 (3): the same cost, one arc
    h = answer(lrm, 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 3)], [0])
    assert (h["cost"][3], h["hops"][3], h["pred_edge"][3], h["pred_pose"][3]) == (3, 1, 3, 0)


def test_a_full_tie_goes_to_the_smaller_edge(lrm):
    # the diamond 0-1-3 / 0-2-3 with equal costs: both arcs into 3 are tight
    h = answer(lrm, 4, [(0, 2, 2), (0, 1, 2), (2, 3, 1), (1, 3, 1)], [0])
    assert (h["cost"][3], h["hops"][3], h["pred_edge"][3], h["pred_pose"][3]) == (3, 2, 2, 2)
    h = answer(lrm, 4, [(0, 2, 2), (0, 1, 2), (1, 3, 1), (2, 3, 1)], [0])
    assert (h["pred_edge"][3], h["pred_pose"][3]) == (2, 1)


def test_duplicate_edges(lrm):
    h = answer(lrm, 2, [(0, 1, 5), (0, 1, 2), (1, 0, 2), (0, 1, 2)], [0])
    assert (h["cost"][1], h["pred_edge"][1], h["pred_pose"][1]) == (2, 1, 0)
    h = answer(lrm, 2, [(0, 1, 5), (0, 1, 2), (1, 0, 2), (0, 1, 2)], [0], direction=2)
    assert (h["cost"][1], h["pred_edge"][1]) == (2, 2)


def test_a_zero_cost_ring_and_self_loops(lrm):
    h = answer(lrm, 5, [(0, 0, 0), (0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 0, 0), (2, 2, 0)], [0])
    assert list(h["cost"]) == [0] * 5 and list(h["hops"]) == [0, 1, 2, 2, 1]
    assert list(h["pred_edge"]) == [-1, 1, 2, 4, 5]
    h = answer(lrm, 5, [(0, 0, 0), (0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 0, 0), (2, 2, 0)], [0], direction=1)
    assert list(h["hops"]) == [0, 1, 2, 3, 4]
    h = answer(lrm, 1, [(0, 0, 0), (0, 0, 3)], [0])
    assert (h["cost"][0], h["hops"][0], h["pred_edge"][0], h["reached"]) == (0, 0, -1, 1)


def test_dead_poses_and_sources(lrm):
    chain = [(i, i + 1) for i in range(6)]
    live = np.ones(7, np.uint8)
    live[3] = 0
    h = answer(lrm, 7, chain, [0], pose_live=live)  # a dead pose in the middle of a chain
    assert list(h["hops"]) == [0, 1, 2, -1, -1, -1, -1] and h["reached"] == 3
    h = answer(lrm, 7, chain, [3], pose_live=live)  # a dead source
    assert list(h["hops"]) == [-1] * 7 and h["reached"] == 0
    h = answer(lrm, 7, chain, [3, 5, 5, -1, 7, BIG, -BIG - 1], pose_live=live)  # dead, twice, out of range
    assert list(h["hops"]) == [-1, -1, -1, -1, 1, 0, 1] and list(h["pred_pose"]) == [-1, -1, -1, -1, 5, -1, 5]
    h = answer(lrm, 7, chain, [])  # no source
    assert list(h["cost"]) == [-1] * 7 and list(h["pred_edge"]) == [-1] * 7 and h["reached"] == 0


def test_bad_indices_negative_costs_and_dead_edges(lrm):
    edges = [(0, 1, 1), (-1, 1, 0), (1, 7, 0), (1, BIG, 0), (-BIG - 1, 2, 0), (1, 2, -1), (1, 2, -BIG - 1), (1, 2, 4), (2, 3, 0), (3, 4, 1)]
    h = answer(lrm, 5, edges, [0])
    assert list(h["cost"]) == [0, 1, 5, 5, 6] and list(h["pred_edge"]) == [-1, 0, 7, 8, 9]
    el = np.ones(len(edges), np.uint8)
    el[8] = 0
    el[7] = 255
    h = answer(lrm, 5, edges, [0], edge_live=el)
    assert list(h["cost"]) == [0, 1, 5, -1, -1]


def test_the_cost_cap(lrm):
    # three edges of cost 2^31 - 1 in a row: 2 (2^31 - 1) = 4 294 967 294 is the cap itself, the third exceeds it
    h = answer(lrm, 4, [(0, 1, BIG), (1, 2, BIG), (2, 3, BIG)], [0])
    assert list(h["cost"]) == [0, BIG, 2 * BIG, -1] and list(h["hops"]) == [0, 1, 2, -1] and h["reached"] == 3
    assert h["pred_edge"][3] == -1 and h["cost"].dtype == np.int64
    h = answer(lrm, 4, [(0, 1, BIG), (1, 2, BIG), (2, 3, 0), (3, 0, 1)], [0], direction=1)  # a zero-cost arc at the cap is still a route
    assert list(h["cost"]) == [0, BIG, 2 * BIG, 2 * BIG]


def test_no_cost_means_cost_equals_hops(lrm):
    for c in (rc.main(rc.MAIN_SEEDS[1]), rc.random_graph(200, 900, 5)):
        h = rc.host(lrm, {**c, "edge_cost": None})
        assert np.array_equal(h["cost"], h["hops"].astype(np.int64)) and h["reached"] > 10


def test_a_long_chain_stored_back_to_front_is_quick(lrm):
    c = rc.chain(100000, backwards=True)
    t0 = time.perf_counter()
    h = rc.host(lrm, c)
    dt = time.perf_counter() - t0  # the call as a whole, the wrapper's copies included
    print(f"{dt * 1e3:.1f} ms")
    assert np.array_equal(h["hops"], np.arange(100000, dtype=np.int32)) and np.array_equal(h["pred_pose"][1:], np.arange(99999, dtype=np.int32))
    assert dt < 0.5  # a fraction of a second: a heap, not a sweep per hop


class Raw:
    """the two C entry points on raw pointers, one good call's arguments that tests edit"""

    def __init__(self, lrm, device):
        self.lrm, self.device = lrm, device
        c = rc.chain(6)
        self.a = dict(nposes=6, edge_a=c["edge_a"], edge_b=c["edge_b"], nedges=5, edge_live=np.ones(5, np.uint8), pose_live=np.ones(6, np.uint8),
                      edge_cost=np.arange(5, dtype=np.int32), sources=c["sources"], nsources=1, direction=0, workspace=np.zeros(64, np.uint64),
                      rounds=4, resume=0, cost=np.full(6, 77, np.int64), hops=np.full(6, 77, np.int32), pred_edge=np.full(6, 77, np.int32),
                      pred_pose=np.full(6, 77, np.int32), reached=np.full(1, 77, np.int32), done=np.full(1, 77, np.int32))

    def __call__(self, **edit):
        a = dict(self.a, **edit)
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        head = (a["nposes"], p(a["edge_a"]), p(a["edge_b"]), a["nedges"], p(a["edge_live"]), p(a["pose_live"]), p(a["edge_cost"]),
                p(a["sources"]), a["nsources"], a["direction"])
        outs = (p(a["cost"]), p(a["hops"]), p(a["pred_edge"]), p(a["pred_pose"]), p(a["reached"]))
        if self.device:  # never reaches a launch in these tests: every call is refused first
            rc_ = self.lrm.lib().lrm_pose_routes_dev(*head, p(a["workspace"]), a["rounds"], a["resume"], *outs, p(a["done"]), None)
        else:
            rc_ = self.lrm.lib().lrm_pose_routes_cpu(*head, *outs, None)
        return rc_, self.lrm.lib().lrm_last_error().decode()


# the refusals in their documented order: (what is wrong, a word of its message, the device form only)
REFUSALS = [(dict(direction=3), "direction", False), (dict(rounds=4097), "rounds", True), (dict(resume=2), "resume", True),
            (dict(nposes=1 << 31), "INT32_MAX", False), (dict(workspace=None), "workspace", True), (dict(edge_a=None), "null", False),
            (dict(sources=None), "null", False), (dict(cost=None, hops=None, pred_edge=None, pred_pose=None), "no output", False)]


@pytest.mark.parametrize("device", [False, True])
def test_refusals_come_first_and_in_order(lrm, device):
    raw = Raw(lrm, device)
    if not device:
        assert raw()[0] == 0 and list(raw.a["hops"]) == [0, 1, 2, 3, 4, 5] and list(raw.a["cost"]) == [0, 0, 1, 3, 6, 10]
    refusals = [(e, w) for e, w, dev_only in REFUSALS if device or not dev_only]
    for k, (edit, word) in enumerate(refusals):
        rc_, msg = raw(**edit)
        assert rc_ == -1 and word in msg, (edit, msg)
        for later, _ in refusals[k + 1:]:
            if word == "null" and set(later) <= {"edge_a", "sources"}:
                continue  # the two NULL refusals share their message
            rc_, msg = raw(**dict(later, **edit))
            assert rc_ == -1 and word in msg, (edit, later, msg)
    for edit in (dict(direction=-1), dict(nedges=1 << 31), dict(nsources=1 << 31), dict(edge_b=None)):
        assert raw(**edit)[0] == -1, edit
    if device:
        for edit in (dict(rounds=0), dict(resume=-1)):
            assert raw(**edit)[0] == -1, edit
        assert "aligned" in raw(workspace=raw.a["workspace"].view(np.uint8)[1:])[1]
    # the range checks come before the no-op of nposes == 0, the pointer checks after it
    assert raw(nposes=0, direction=3)[0] == -1 and raw(nposes=0, nedges=1 << 31)[0] == -1
    if not device:
        raw.a["reached"][0] = 77
        assert raw(nposes=0, edge_a=None, edge_b=None, sources=None, cost=None, hops=None, pred_edge=None, pred_pose=None)[0] == 0
        assert raw.a["reached"][0] == 0 and raw(nposes=0, reached=None)[0] == 0
        # NULL edges and sources are fine where there are none
        assert raw(nedges=0, edge_a=None, edge_b=None)[0] == 0 and list(raw.a["hops"]) == [0, -1, -1, -1, -1, -1]
        assert raw(nsources=0, sources=None)[0] == 0 and list(raw.a["hops"]) == [-1] * 6 and raw.a["reached"][0] == 0


def test_every_optional_pointer_may_be_null(lrm):
    raw = Raw(lrm, False)
    assert raw()[0] == 0
    outs = ("cost", "hops", "pred_edge", "pred_pose", "reached")
    full = {k: raw.a[k].copy() for k in outs}
    drops = [(k,) for k in outs] + [tuple(k for k in outs[:4] if k != keep) for keep in outs[:4]]
    for drop in drops:
        for k in outs:
            raw.a[k][...] = 77
        assert raw(**{k: None for k in drop})[0] == 0, drop
        for k in outs:
            assert np.array_equal(raw.a[k], np.full_like(full[k], 77) if k in drop else full[k]), (drop, k)
    for k in ("edge_live", "pose_live", "edge_cost"):
        assert raw(**{k: None})[0] == 0
    assert list(raw.a["cost"]) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("nposes", [0, 1])
@pytest.mark.parametrize("nedges", [0, 1])
@pytest.mark.parametrize("nsources", [0, 1])
def test_sizes_of_nothing_and_one(lrm, nposes, nedges, nsources):
    c = rc.case(nposes, [0] * nedges, [0] * nedges, [0] * nsources)
    h, _ = check(lrm, c)
    assert h["reached"] == (1 if nposes and nsources else 0) and len(h["cost"]) == nposes


def test_symbols_are_declared_and_exported(lrm):
    declared, exported = lrm.declared_symbols(), lrm.exported_symbols()
    for s in SYMBOLS:
        assert s in declared and s in exported, s
    assert lrm.lib().lrm_pose_routes_workspace_bytes(10, 3) == 10 * 8 + 4 * 4


def test_the_plan_is_the_kernels(lrm):
    """lrm_dbg_pose_routes_plan against the constants parsed from the source"""
    head = open(os.path.join(CSRC, "lrm_pose_routes.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", head).group(1))
    block, per_lane, K, G = const("LRM_ROUTES_BLOCK"), const("LRM_ROUTES_EDGES_PER_LANE"), const("LRM_ROUTES_SWEEPS"), const("LRM_ROUTES_MAX_GRID")
    assert "#define LRM_ROUTES_CHUNK (LRM_ROUTES_BLOCK * LRM_ROUTES_EDGES_PER_LANE)" in head
    src = open(os.path.join(CSRC, "lrm_pose_routes.hip")).read()
    for name, macro in (("kBlock", "LRM_ROUTES_BLOCK"), ("kPerLane", "LRM_ROUTES_EDGES_PER_LANE"), ("kChunk", "LRM_ROUTES_CHUNK"), ("kSweeps", "LRM_ROUTES_SWEEPS")):
        assert re.search(rf"constexpr \w+ {name} = {macro};", src), name
    Cc = block * per_lane
    for ne in (0, 1, Cc - 1, Cc, Cc + 1, 2 * Cc + 1, G * Cc, G * Cc + 1, 100 * G * Cc, 2 ** 31 - 1):
        p = lrm.dbg_pose_routes_plan(ne)
        assert p == {"chunk": Cc, "grid_cap": G, "sweeps": K, "workgroups": min(G, -(-ne // Cc))}, ne
    assert lrm.lib().lrm_dbg_pose_routes_plan(1 << 31, np.zeros(4, np.uint64).ctypes.data_as(C.c_void_p)) == -1
    assert lrm.lib().lrm_dbg_pose_routes_plan(5, None) == -1
