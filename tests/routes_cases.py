"""Shared graph builders of the pose-route tests (tests/test_pose_routes_cpu.py, tests/test_gpu_pose_routes.py): chains stored
forwards and back to front, rings, an n x n lattice with four edges per node (+x, +y, both diagonals) and random live bytes,
random graphs; the main fixture (the 32 x 32 lattice); the comparison helpers.  A case is a dict of the arguments of
lrm.pose_routes_cpu: nposes, edge_a, edge_b, sources, edge_live, pose_live, edge_cost (the last three may be None)."""
import numpy as np

KEYS = ("cost", "hops", "pred_edge", "pred_pose")
DTYPES = {"cost": np.int64, "hops": np.int32, "pred_edge": np.int32, "pred_pose": np.int32}
# The seeds of the main fixture: with this generator node 0 sits in a corner with three edges and is cut off under most seeds;
# these four are the first for which the model (tests/routes_model.py alone) reaches 0.57 to 0.75 of the poses with a deepest
# route of 52 to 85 hops and a pose with two tight incoming arcs (test_the_main_fixture_is_not_vacuous asserts the condition).
MAIN_N, MAIN_EDGES, MAIN_SEEDS = 32, 3906, (3, 8, 10, 12)
ARGS = ("nposes", "edge_a", "edge_b", "sources", "edge_live", "pose_live", "edge_cost")


def case(nposes, edge_a, edge_b, sources, edge_live=None, pose_live=None, edge_cost=None):
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8).reshape(-1)
    return {"nposes": int(nposes), "edge_a": i32(edge_a), "edge_b": i32(edge_b), "sources": i32(sources), "edge_live": u8(edge_live),
            "pose_live": u8(pose_live), "edge_cost": None if edge_cost is None else i32(edge_cost)}


def chain(n, backwards=False, cost=None):
    """poses 0 - 1 - ... - n-1, source 0; backwards: the edge (n-2, n-1) is stored first -- the order in which one sweep over the
    edges in storage order gains least"""
    a = np.arange(n - 1)
    if backwards:
        a = a[::-1]
    return case(n, a, a + 1, [0], edge_cost=None if cost is None else np.full(n - 1, cost))


def ring(n, cost=None):
    a = np.arange(n)
    return case(n, a, (a + 1) % n, [0], edge_cost=None if cost is None else np.full(n, cost))


def lattice(n, seed, p_edge=0.4, p_pose=0.85, max_cost=5):
    """the n x n lattice, node y * n + x: the +x edges, the +y edges, then the two diagonals of every cell; an edge is live with
    probability p_edge and a pose with p_pose; costs 0..max_cost; the source is node 0, forced live"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n * n).reshape(n, n)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel(), idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()])
    edge_live = (rng.random(len(a)) < p_edge).astype(np.uint8)
    pose_live = (rng.random(n * n) < p_pose).astype(np.uint8)
    pose_live[0] = 1
    return case(n * n, a, b, [0], edge_live, pose_live, rng.integers(0, max_cost + 1, len(a)))


def main(seed):
    return lattice(MAIN_N, seed)


def random_graph(nposes, nedges, seed, nsources=2, bad=0.02, max_cost=7):
    """nedges random pairs over nposes poses (self-loops and duplicates as they fall); a share `bad` of the indices is out of
    range (negative, nposes, huge), a few costs are negative, a tenth of the edges and of the poses is dead"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, nposes, nedges), rng.integers(0, nposes, nedges)
    pool = np.array([-1, nposes, -2 ** 31, 2 ** 31 - 1, nposes + 7])
    for arr in (a, b):
        hit = rng.random(nedges) < bad
        arr[hit] = rng.choice(pool, int(hit.sum()))
    cost = rng.integers(0, max_cost + 1, nedges)
    cost[rng.random(nedges) < 0.02] = -3
    edge_live = rng.choice(np.array([0, 1, 255], np.uint8), nedges, p=[0.1, 0.8, 0.1])
    pose_live = (rng.random(nposes) < 0.9).astype(np.uint8)
    sources = rng.integers(0, nposes, nsources)
    pose_live[sources[0]] = 1
    return case(nposes, a, b, sources, edge_live, pose_live, cost)


def swapped(c):
    return {**c, "edge_a": c["edge_b"], "edge_b": c["edge_a"]}


def host(lrm, c, direction=0, **want):
    """the host loop -> dict(cost, hops, pred_edge, pred_pose, reached)"""
    cost, hops, pe, pp, reached, _ = lrm.pose_routes_cpu(*(c[k] for k in ARGS), direction, **want)
    return {"cost": cost, "hops": hops, "pred_edge": pe, "pred_pose": pp, "reached": reached}


def model_arrays(m):
    return {**{k: np.asarray(m[k], DTYPES[k]) for k in KEYS}, "reached": m["reached"]}


def assert_same(got, want, what=""):
    for k in KEYS:
        if want[k] is None:
            continue
        g = np.ascontiguousarray(got[k]).reshape(-1)
        assert g.dtype == DTYPES[k] and np.array_equal(g, want[k]), (what, k, np.nonzero(g != want[k])[0][:5])
    assert int(got["reached"]) == int(want["reached"]), what
