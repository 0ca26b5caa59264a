"""The case module of the octree boundary suite (tests/octree_cases.py) on the host, with the oracle alone: the launch constants
the sizes are built around, the inert footholds, the place of the extreme decider in memory, that every case's tree depends on
the foothold its GPU test is about, and that the box-geometry cases contain the node kinds they are there for.

A change of kOctBlock, kOctChunkedFrom, the tile or chunk size, a grid cap or a tpr / want_wgs tier in lrm_octree.hip fails
test_launch_plan_is_the_plan_the_library_launches; it must come with the new values in octree_cases.launch_constants and in
test_launch_constants_are_the_ones_the_suite_is_built_around, or the boundaries move away from the tests."""
import numpy as np
import pytest

import octree_cases as oc
from octree_oracle import apply_oct as oracle_apply_oct


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tree(oracle, case, cloud=None):
    return oc.oracle_tree(oracle, case.oracle_cloud() if cloud is None else cloud, case.dim, case.st)


def test_launch_constants_are_the_ones_the_suite_is_built_around():
    assert oc.launch_constants() == {"block": 256, "chunk": 64, "tile": 1024, "chunked_from": 9, "every_cap": 1024, "chunked_cap": 16384,
                                     "first_level_wgs": 2048, "tpr": (2048, 32, 8192, 128), "wgs": (2048, 32768, 8192, 8192, 4096),
                                     "max_splits": 256, "defer_from": 256, "brute_max": 65535}
    K = oc.launch_constants()
    around = lambda n: {n - 1, n, n + 1}
    assert set(oc.SIZES) >= around(K["chunk"]) | around(K["block"]) | around(K["tile"]) | around(4 * K["tile"]) | around(K["every_cap"] * K["block"])
    assert {32 * K["tile"], 32 * K["tile"] + 1} <= set(oc.SIZES)  # one round of tpr = 32 tiles, and one foothold more
    assert max(oc.SIZES) == K["every_cap"] * K["block"] + K["chunk"] + 1  # a second trip of the grid stride with one chunk and a foothold
    assert oc.max_legs() == 8


def test_launch_plan_is_the_plan_the_library_launches(lrm, monkeypatch):
    """oc.launch_plan against lrm_dbg_oct_plan (oct_level_plan, which the level launcher consumes) under the same switches, field by
    field, with level sizes and cloud sizes on both sides of every threshold and cap; `seen` keeps the sweep honest: each
    constant of launch_constants decides some compared plan"""
    K = oc.launch_constants()
    first_level = (K["first_level_wgs"] // 8 - 1) * 32 * K["tile"]  # 8 children: ((ntiles + 31) // 32) * 8 reaches 2048 one foothold later
    ncs = (1, 8, 9, 10, 63, 64, 255, 256, 257, 2047, 2048, 8191, 8192, 65535, 65536)
    nfs = oc.SIZES + (8193, 65_537, first_level, first_level + 1)
    envs = [{}, {"LRM_OCT_BRUTE": "1"}, {"LRM_OCT_CHUNKED_FROM": "1"}, {"LRM_OCT_DEFER_FROM": "1"}, oc.SPLIT_ENV, {"LRM_OCT_TPR": "0"},
            {"LRM_OCT_TPR": "100000"}, {"LRM_OCT_TPR": "1", "LRM_OCT_WGS": "100000"}, {"LRM_OCT_TPR": "1", "LRM_OCT_WGS": "1000000"}]
    seen = set()
    for env in envs:
        with monkeypatch.context() as m:
            for knob in oc.KNOBS:
                m.delenv(knob, raising=False)
            for k, v in env.items():
                m.setenv(k, v)
            for nc in ncs:
                for nf in nfs:
                    want, got = oc.launch_plan(nc, nf, env), lrm.dbg_oct_plan(nc, nf)
                    where = (env, nc, nf, want, got)
                    assert got["kernel"] == want["kernel"] and got["deferred"] == want["deferred"] and got["grid_x"] == want["grid"], where
                    assert got["block"] == K["block"] and got["ntiles"] == -(-nf // K["tile"]), where
                    if want["kernel"] == "every":
                        assert got["grid_y"] == nc and got["tpr"] == 0 and got["splits"] == 0, where
                        assert want["trips"] == -(-((nf + 63) // 64 * 64) // (got["grid_x"] * got["block"])), where
                        seen |= {"every", "every_cap" if (nf + K["block"] - 1) // K["block"] > K["every_cap"] else "every_below_cap"}
                        seen |= {"brute"} if env.get("LRM_OCT_BRUTE") and nc >= K["chunked_from"] else set()
                        continue
                    assert got["grid_y"] == 1 and got["tpr"] == want["tpr"] and got["splits"] == want["splits"], where
                    assert got["grid_x"] == min(nc * got["splits"], K["chunked_cap"]), where
                    seen |= {"chunked", "deferred" if got["deferred"] else "inline", "tpr_%d" % got["tpr"]}
                    seen |= {"grid_cap"} if nc * got["splits"] > K["chunked_cap"] else set()
                    seen |= {"max_splits"} if got["splits"] == K["max_splits"] and got["ntiles"] > K["max_splits"] * got["tpr"] else set()
                    seen |= {"splits_by_tiles"} if 1 < got["splits"] == -(-got["ntiles"] // got["tpr"]) else set()
                    seen |= {"brute_max"} if env.get("LRM_OCT_BRUTE") else set()
                    seen |= {"first_level"} if not env and nc < K["chunked_from"] else set()
    assert seen >= {"every", "every_cap", "every_below_cap", "brute", "brute_max", "chunked", "deferred", "inline", "grid_cap", "max_splits",
                    "splits_by_tiles", "first_level", "tpr_1", "tpr_32", "tpr_128", "tpr_256"}, seen
    # the thresholds themselves, from the library alone: both sides of each
    plan = lambda nc, nf: lrm.dbg_oct_plan(nc, nf)
    assert [plan(nc, 4097)["kernel"] for nc in (8, 9)] == ["every", "chunked"]
    assert [plan(8, nf)["kernel"] for nf in (first_level, first_level + 1)] == ["every", "chunked"]
    assert [plan(nc, 1 << 20)["tpr"] for nc in (2047, 2048, 8191, 8192)] == [32, 128, 128, 256]
    assert [plan(nc, 1 << 22)["splits"] for nc in (2047, 2048, 8191, 8192)] == [17, 4, 2, 1]  # ceil(32768 / 2047), 8192 / 2048, ceil(8192 / 8191)
    assert [plan(nc, 4097)["deferred"] for nc in (255, 256)] == [False, True]
    with monkeypatch.context() as m:
        m.setenv("LRM_OCT_BRUTE", "1")
        assert [plan(nc, 4097)["kernel"] for nc in (65535, 65536)] == ["every", "chunked"]


def test_launch_plan_on_the_decider_tree(lrm, oracle):
    """every level of the decider tree under every traversal of the GPU file: which kernel, and that the three largest sizes take
    oct_validity_kernel past its block cap"""
    sizes = oc.level_sizes(tree(oracle, oc.decider_case(lrm, 4097, "last"))[1])
    assert sizes[0] == 8 and sizes[1] >= 9 and max(sizes) >= 64 and len(sizes) >= 3, sizes
    for nf in oc.SIZES:
        kinds = [oc.launch_plan(nc, nf)["kernel"] for nc in sizes]
        assert kinds[0] == "every" and set(kinds[1:]) == {"chunked"}
        assert all(oc.launch_plan(nc, nf, {"LRM_OCT_BRUTE": "1"})["kernel"] == "every" for nc in sizes)
        assert all(oc.launch_plan(nc, nf, {"LRM_OCT_CHUNKED_FROM": "1"})["kernel"] == "chunked" for nc in sizes)
        trips = oc.launch_plan(8, nf, {"LRM_OCT_BRUTE": "1"})["trips"]
        assert trips == (2 if nf > 262_144 else 1), (nf, trips)
    assert any(oc.launch_plan(nc, 4097)["deferred"] for nc in sizes) and not oc.launch_plan(sizes[0], 4097)["deferred"]
    assert all(oc.launch_plan(nc, 4097, {"LRM_OCT_DEFER_FROM": "1"})["deferred"] for nc in sizes[1:])


def test_knob_cases_split_children_and_pass_the_grid_cap(lrm, oracle):
    cases = oc.knob_cases(lrm)
    sizes = oc.level_sizes(tree(oracle, cases["splits_4097_last"])[1])
    for nf, want in ((4097, 5), (8193, 9)):
        plans = [oc.launch_plan(nc, nf, oc.SPLIT_ENV) for nc in sizes[1:]]
        assert all(p["kernel"] == "chunked" and p["splits"] == want and p["workgroups"] <= oc.launch_constants()["chunked_cap"] for p in plans), plans
    assert max(sizes) >= 512
    plans = [oc.launch_plan(nc, 65_537, oc.SPLIT_ENV) for nc in sizes if nc >= 512]
    assert plans and all(p["workgroups"] > oc.launch_constants()["chunked_cap"] == p["grid"] and p["splits"] > 1 for p in plans), plans


@pytest.mark.parametrize("layout", ["first", "last"])
def test_decider_clouds(lrm, oracle, layout):
    """the inert predicate and the extreme decider's place at every size; the oracle on a whole cloud of 4097 equals the oracle on
    its deciders; the tree changes without the extreme decider -- from the eight, from two and from one; the tree is a real one"""
    empty = None
    for nf in oc.SIZES + (8193, 65_537):
        case = oc.decider_case(lrm, nf, layout)
        rl = oc.reach_len(case.dim)
        inert = oc.is_inert(case.f, case.st.box_center, oc.DECIDER_HALF, rl)
        assert len(case.f) == nf and inert.sum() == nf - len(case.decide) and not oc.is_inert(case.decide, case.st.box_center, oc.DECIDER_HALF, rl).any()
        assert (np.abs(case.f[inert]) > 2 * oc.DECIDER_HALF + rl).all()  # wholly to one side on x, y and z
        assert oc.extreme_is_at_the_end(case.f, case.extreme, layout), nf
        if nf in (1, 2, 4097):
            with_e, levels = tree(oracle, case)
            without_e, _ = tree(oracle, case, case.decide[1:])
            assert not same(with_e, without_e) and len(with_e) >= 1, nf
            if nf == 1:
                empty = without_e
            if nf == 4097:
                whole, n_nodes = oracle_apply_oct(oracle, case.f, case.dim, case.st)
                assert same(whole, with_e) and n_nodes > 200 and n_nodes == 1 + sum(oc.level_sizes(levels))
    assert len(empty) == 0


def test_oracle_tree_is_the_oracle(lrm, oracle):
    for case in list(oc.geometry_cases(lrm).values())[2:5]:
        got, levels = tree(oracle, case)
        want, n_nodes = oracle_apply_oct(oracle, case.f, case.dim, case.st)
        assert same(got, want) and n_nodes == 1 + sum(oc.level_sizes(levels))


def test_dense_cases_are_culled_and_affordable(lrm, oracle):
    """most (child, tile) and (child, chunk) pairs of the chunked levels are dropped by the box test, restated here on the memory
    order the keys give; the sparse layout's tiles are one near chunk among fifteen far ones"""
    import time
    for name, case in oc.dense_cases(lrm).items():
        t0 = time.perf_counter()
        leaves, levels = tree(oracle, case)
        dt = time.perf_counter() - t0
        f = case.f[np.argsort(oc.morton_keys(case.f), kind="stable")]
        rl = oc.reach_len(case.dim)
        pad = np.full((-len(f) % 64, 3), np.nan, oc.F)
        ch = np.concatenate([f, pad]).reshape(-1, 64, 3)
        lo, hi = np.nanmin(ch, axis=1), np.nanmax(ch, axis=1)
        kids = [n for level in levels[1:] for n in level if not n["skip"]]
        c, H = np.array([n["c"] for n in kids]), np.array([np.abs(n["ph"] + rl) for n in kids])
        meets = ((lo[None] <= (c + H)[:, None]) & (hi[None] >= (c - H)[:, None])).all(axis=2)
        print(f"{name}: {len(case.f)} footholds, levels {oc.level_sizes(levels)}, {len(leaves)} leaves, oracle {dt:.2f} s, "
              f"{1 - meets.mean():.2f} of the (child, chunk) pairs culled")
        assert len(leaves) >= 1 and sum(oc.level_sizes(levels)) > 150 and dt < 5
        # (z is noise with its own span and the key's top bit: 16 chunks are 16 z-slabs of a quadrant each, 64 chunks a sixteenth each)
        if len(case.f) >= 4096:
            assert meets.mean() < 0.5, name
    rl = oc.reach_len(case.dim)
    f, near = oc.sparse_tiles(rl, oc.DENSE_HALF)
    k = oc.morton_keys(f)
    order = np.argsort(k, kind="stable")
    got = near[order].reshape(8, 16, 64)
    assert (got.all(axis=2).sum(axis=1) == 1).all() and (got.any(axis=2) == got.all(axis=2)).all()
    ks = k[order].reshape(128, 64)
    assert (ks[:-1].max(axis=1) < ks[1:].min(axis=1))[np.flatnonzero(got.all(axis=2).reshape(-1)[:-1] != got.all(axis=2).reshape(-1)[1:])].all()  # no ties across
    assert (k[order] >> 27 == np.repeat(np.arange(8), 1024)).all()  # a tile is an octant
    assert not oc.is_inert(f[near], (0, 0, 0), oc.DENSE_HALF, rl).any() and oc.is_inert(f[~near], (0, 0, 0), oc.DENSE_HALF, rl).all()


def test_geometry_cases_contain_their_node_kinds(lrm, oracle):
    cases = oc.geometry_cases(lrm)
    seen = {}
    for name, case in cases.items():
        leaves, levels = tree(oracle, case)
        nodes = [n for level in levels for n in level]
        seen[name] = dict(leaves=len(leaves), sizes=oc.level_sizes(levels), missing={n["missing"] for n in nodes if not n["dead"]},
                          dead=sum(n["dead"] for n in nodes), rot=[{n["rot"] for n in level} for level in levels],
                          parent_valid=sum(n["parent_valid"] and not n["skip"] for n in nodes))
        print(name, seen[name])
    for name in ("flat_box", "flat_box_off_origin"):
        assert {1, 2} <= seen[name]["missing"] and seen[name]["dead"] > 0 and seen[name]["leaves"] > 0, seen[name]
    assert 3 in seen["flat_box"]["missing"]
    assert seen["rot_thin_x"]["rot"][:2] == [{False}, {True}] and seen["rot_thick_x"]["rot"][:3] == [{False}, {False}, {True}]
    assert seen["depth_0"]["leaves"] == 0 and seen["depth_0"]["sizes"] == []
    # (eight legs of which one is needed: an edge needs all eight boundaries inside one box -- that tree ends at its first level)
    for name in set(cases) - {"depth_0"}:
        assert seen[name]["leaves"] > 0 and sum(seen[name]["sizes"]) >= (8 if name == "max_legs_stab_1" else 48), (name, seen[name])
    assert seen["one_orientation"]["rot"][0] == {True} and seen["six_orientations"]["rot"][0] == {True}


@pytest.mark.parametrize("root", list(oc.FACE_ROOTS))
def test_face_cases(lrm, oracle, root):
    """a valid, still expanding parent exists; for every axis and side a child is found; the 64 copies are the last / first chunk;
    a face foothold that in_box keeps changes the tree, and one that it drops does not turn that child into a leaf"""
    cases, picked, base = oc.face_cases(lrm, oracle, root)
    assert set(picked) == {(a, s) for a in range(3) for s in (1, -1)}
    any_case = next(iter(cases.values()))
    base_leaves, _ = oc.oracle_tree(oracle, base, any_case.dim, any_case.st)
    changed = 0
    for (axis, side, k), case in cases.items():
        n, inside = picked[axis, side]
        assert n["parent_valid"] and n["flags"] == 5
        keys = oc.morton_keys(case.f)
        mine = (case.f.view(np.uint32) == case.extreme.view(np.uint32)).all(axis=1)
        assert mine.sum() == 64 and len(case.f) == 192
        assert keys[mine].min() > keys[~mine].max() if side > 0 else keys[mine].max() < keys[~mine].min()
        leaves, levels = tree(oracle, case)
        twin = [m for level in levels for m in level if same(m["c"], n["c"]) and same(m["h"], n["h"])]
        assert len(twin) == 1
        assert bool(twin[0]["flags"] & 2) == bool(inside[k + 1]), (axis, side, k, twin[0]["flags"], inside)
        if inside[k + 1]:
            assert not same(leaves, base_leaves)
            changed += 1
    assert changed >= 6 and changed < len(cases)  # both verdicts occur


def test_nonfinite_cases(lrm, oracle):
    """the oracle itself ignores the non-finite rows; the layouts the cases claim hold for the keys the library computes"""
    cases = oc.nonfinite_cases(lrm)
    for name, case in cases.items():
        want, _ = tree(oracle, case)
        got, _ = oracle_apply_oct(oracle, case.f, case.dim, case.st)
        assert same(got, want), name
        assert np.isfinite(case.decide).all() and (len(want) > 0) == (name != "nan_only")
        keys = oc.morton_keys(case.f)
        bad = ~np.isfinite(case.f).all(axis=1)
        if name == "nan_in_the_deciders_chunk":
            first = keys == keys.min()
            mine = (case.f.view(np.uint32) == case.extreme.view(np.uint32)).all(axis=1)
            assert first.sum() == 64 and (first & mine).sum() == 1 and (first & bad).sum() == 63
        if name in ("a_chunk_of_nan", "a_tile_of_nan"):
            assert (keys[bad] == 0).all() and (keys[~bad] > 0).all() and bad.sum() in (64, 1024)
            assert len(case.f) % 64 == 1 and oc.extreme_is_at_the_end(case.f[~bad], case.extreme, "last") and keys[~bad].max() == keys.max()
