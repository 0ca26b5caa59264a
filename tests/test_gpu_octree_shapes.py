"""The octree kernels (csrc/lrm_octree.hip) across chunk, tile, block, round, grid-stride and box boundaries, against the brute-force
oracle (tests/octree_oracle.py) on every cloud: the returned leaf centres bit for bit, order included, and for the default
traversal every child's three flag bits (lrm_dbg_oct_trace) as well.  The cases come from tests/octree_cases.py; that each of them
depends on the foothold it is about is checked on the host by tests/test_octree_cases_cpu.py."""
import numpy as np
import pytest

import octree_cases as oc

pytestmark = pytest.mark.gpu

_TREES = {}  # the oracle's tree of a case: computed once per module, shared by the five modes, never written to


@pytest.fixture(autouse=True, params=["strict", "fast", "fast_tol", "fast_tab", "fast_tab_inline"])
def mode(request, lrm, monkeypatch):
    """the five arithmetic forms of tests/test_gpu_octree.py: all must give the same leaves"""
    lrm.set_mode(lrm.MODE_STRICT if request.param == "strict" else lrm.MODE_FAST)
    for knob in oc.KNOBS:
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("LRM_OCT_TOL", "1" if request.param in ("fast_tol", "fast_tab", "fast_tab_inline") else "0")
    monkeypatch.setenv("LRM_OCT_TAB", "1" if request.param in ("fast_tab", "fast_tab_inline") else "0")
    monkeypatch.setenv("LRM_OCT_DEFER", "0" if request.param == "fast_tab_inline" else "1")
    yield request.param
    lrm.set_mode(lrm.MODE_FAST)


def oracle_tree(oracle, key, case):
    if key not in _TREES:
        leaves, levels = oc.oracle_tree(oracle, case.oracle_cloud(), case.dim, case.st)
        _TREES[key] = (leaves, oc.trace_records(levels, case.st))
    return _TREES[key]


def traversals(mode):
    t = {"default": {}, "every_foothold": {"LRM_OCT_BRUTE": "1"}, "no_sphere_cull": {"LRM_OCT_NOCULL": "1"},
         "chunked_from_the_first_level": {"LRM_OCT_CHUNKED_FROM": "1"}}
    if mode == "fast_tab":
        t["deferred_at_every_chunked_level"] = {"LRM_OCT_DEFER_FROM": "1"}
        t["deferred_from_the_first_level"] = {"LRM_OCT_DEFER_FROM": "1", "LRM_OCT_CHUNKED_FROM": "1"}
    return t


def check(lrm, oracle, monkeypatch, key, case, how):
    """every traversal in `how` on the case's cloud: the oracle's leaves; the default traversal: the oracle's flags per child too"""
    want, want_rec = oracle_tree(oracle, key, case)
    for name, env in how.items():
        with monkeypatch.context() as m:
            for k, v in {**case.env, **env}.items():
                m.setenv(k, v)
            traced = name == "default"
            if traced:
                lrm.dbg_oct_trace(True)
            try:
                got, ms = lrm.apply_oct(case.f, case.dim, case.st)
                rec = lrm.dbg_oct_trace_read() if traced else None
            finally:
                if traced:
                    lrm.dbg_oct_trace(False)
        assert ms >= 0
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, name, len(got), len(want))
        if traced and len(case.f):
            assert rec.shape == want_rec.shape, (key, rec.shape, want_rec.shape)
            bad = np.flatnonzero((rec != want_rec).any(axis=1))
            assert len(bad) == 0, (key, len(bad), rec[bad[:3]], want_rec[bad[:3]])
    return want


# ---- 1. decider clouds: every size, the deciding foothold first and last in memory -----------------------------------------
@pytest.mark.parametrize("nf", oc.SIZES)
@pytest.mark.parametrize("layout", ["first", "last"])
def test_decider_cloud_at_every_boundary(lrm, oracle, monkeypatch, mode, layout, nf):
    """A few footholds decide the tree, nf - 8 lie where no child's elongated box reaches; the extreme decider is the first or the
    last foothold in memory: lane 0 of the first chunk, or the one live lane of the last chunk / wave / block / tile / round / trip
    of the grid stride at the sizes one past a boundary.  Default traversal, every level through oct_validity_kernel (the three
    largest sizes pass its 1024-block cap), every level through the chunked kernel, no sphere cull, and in fast_tab every level
    through the deferred queue."""
    case = oc.decider_case(lrm, nf, layout)
    want = check(lrm, oracle, monkeypatch, ("decider", layout, min(nf, len(oc.DECIDERS))), case, traversals(mode))
    assert len(want) >= 1


# ---- 2. the work decomposition under knobs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["splits_4097_first", "splits_4097_last", "splits_8193_first", "splits_8193_last", "cap_65537_first",
                                  "cap_65537_last"])
def test_workgroups_that_share_a_child_and_the_grid_cap(lrm, oracle, monkeypatch, mode, name):
    """LRM_OCT_TPR=1 and LRM_OCT_WGS=32768: 5 and 9 workgroups share a child through its global flag word (4097 and 8193 footholds);
    at 65 537 footholds the levels of 264 and 1696 children ask for more than the 16 384 workgroups of the grid, and the
    `w += gridDim.x` loop runs (the arithmetic: test_octree_cases_cpu.py)"""
    case = oc.knob_cases(lrm)[name]
    how = {k: v for k, v in traversals(mode).items() if k != "every_foothold"}
    check(lrm, oracle, monkeypatch, ("decider", case.layout, len(oc.DECIDERS)), case, how)


# ---- 3. dense clouds on which the box cull works ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relief_65", "relief_1025", "relief_4097", "sparse_tiles", "rotations_257"])
def test_dense_clouds_against_the_whole_tree(lrm, oracle, monkeypatch, mode, name):
    """Random relief three to six root half-sizes wide, a layout whose eight tiles are one chunk at the root among fifteen far away, and
    the 27 orientations on 257 footholds: most tiles and chunks are dropped for most children, and the whole tree must be the
    oracle's.  One oracle tree on one CPU thread: relief_65 0.2 s, relief_1025 0.3 s, relief_4097 0.4 s, sparse_tiles 2.8 s,
    rotations_257 (two legs) 2.2 s."""
    case = oc.dense_cases(lrm)[name]
    want = check(lrm, oracle, monkeypatch, ("dense", name), case, traversals(mode))
    assert len(want) >= 1


# ---- 4. box geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["off_origin", "far_root", "flat_box", "flat_box_off_origin", "rot_thin_x", "rot_thick_x", "one_leg",
                                  "max_legs_stab_1", "max_legs_stab_all", "two_legs_stab_all", "one_orientation", "six_orientations",
                                  "depth_0"])
def test_box_geometry_legs_and_orientations(lrm, oracle, monkeypatch, mode, name):
    """a root away from the origin and 4e6 mm away; boxes with one, two and three axes below min_box (the quadrant remap and the
    dead quadrants of create_child_box); boxes whose x half size crosses enable_rot_below at another depth than y and z; 1 and
    LRM_MAX_LEGS legs; 1 and all legs needed; 1 and 6 orientation samples; max_depth 0"""
    case = oc.geometry_cases(lrm)[name]
    want = check(lrm, oracle, monkeypatch, ("geometry", name), case, traversals(mode))
    assert (len(want) == 0) == (name == "depth_0")


@pytest.mark.parametrize("root", list(oc.FACE_ROOTS))
def test_footholds_on_the_faces_of_the_elongated_box(lrm, oracle, monkeypatch, mode, root):
    """c + H and c - H in float32 and their neighbours on both sides, for every axis, as a chunk of their own (64 copies at the end
    or the start of memory: the chunk's box is that point), for a child that only such a foothold turns into a valid leaf.  box_meets
    must keep every chunk whose foothold in_box keeps -- at the origin, at a root with half sizes that are no dyadic numbers, and
    4e6 mm away, where c + H rounds to a quarter of a millimetre."""
    if root not in _TREES:
        _TREES[root] = oc.face_cases(lrm, oracle, root)[0]
    how = {k: v for k, v in traversals(mode).items() if k in ("default", "chunked_from_the_first_level", "every_foothold")}
    for key, case in _TREES[root].items():
        check(lrm, oracle, monkeypatch, ("face", root) + key, case, how)


# ---- 5. non-finite footholds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nan_in_the_deciders_chunk", "inf_huge_and_subnormal", "huge_on_one_side", "a_chunk_of_nan", "a_tile_of_nan",
                                  "nan_only"])
def test_nonfinite_footholds_are_ignored(lrm, oracle, monkeypatch, mode, name):
    """nan, +-inf, +-3.2e38 and subnormal coordinates next to the deciders, a whole chunk and a whole tile of nan rows, a cloud of
    nan only: the tree of the finite footholds"""
    case = oc.nonfinite_cases(lrm)[name]
    want = check(lrm, oracle, monkeypatch, ("nonfinite", name), case, traversals(mode))
    assert (len(want) == 0) == (name == "nan_only")
