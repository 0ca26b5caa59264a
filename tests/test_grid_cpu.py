"""The queue sizing of the tolerance-mode and table-guided calls, on the host (no GPU): include/lrm.h promises that after
lrm_tol_prepare(n_max) the calls on n <= n_max points only launch -- no regrown workspace (hipFree + hipMalloc), so a graph
capture of them works.  The launch grids are not monotone in n (a cloud of one workgroup more than the table kernel's base
grid runs two rounds on half the workgroups), so the words a call requests must be the most any smaller cloud needs.
Everything comes from lrm_dbg_tol_grid, which calls the functions the launches call."""
import numpy as np
import pytest

from grid_cases import BLOCK, KERNELS, TOLTAB_MIN_POINTS, gpu_sizes, grid_table, transitions


@pytest.fixture(scope="module")
def trans(lrm):
    return sorted(transitions(lrm))


@pytest.fixture(scope="module")
def table(lrm, trans):
    return grid_table(lrm, trans[-1] + 2)


def per_workgroup_words(lrm):
    """queue words per workgroup of the table kernels and of the kernel without a table: a one-point cloud runs one workgroup"""
    g = lrm.dbg_tol_grid(1)
    assert g["tab"] == g["rel"] == g["notab"] == 1
    return g["tab_words"], g["notab_words"]


def requested(g):
    return max(g["tab_words"], g["notab_words"])


def test_the_transitions_are_the_ones_the_grids_are_built_around(lrm, trans):
    """the scan finds the grids' floors, round steps and caps (sanity check of grid_cases.transitions, not a restatement)"""
    assert len(trans) >= 8
    t = transitions(lrm)
    assert any("tab" in v for v in t.values()) and any("rel" in v for v in t.values()) and any("notab" in v for v in t.values())
    # the bug of the issue: one point past the table kernel's first transition, its grid HALVES
    first_tab = min(k for k, v in t.items() if "tab" in v)
    a, b = lrm.dbg_tol_grid(first_tab * BLOCK), lrm.dbg_tol_grid(first_tab * BLOCK + 1)
    assert b["tab"] < a["tab"]


def test_calls_request_at_least_what_their_grids_use(lrm, table):
    """every kernel's grid fits the workspace its call requests: a workgroup's count slot and its queue segment"""
    tab_w, notab_w = per_workgroup_words(lrm)
    for k in ("tab", "rel"):
        assert (table[k] * tab_w <= table["tab_words"]).all(), k
    assert (table["notab"] * notab_w <= table["notab_words"]).all()
    assert (table["rel"] <= table["tab"]).all()  # LRM_MODE_TOL_REL's grid is never the larger one (both share lrm_tol_tab_queue_words)


def test_prepare_covers_every_smaller_call_at_every_transition(lrm, trans):
    """lrm_tol_prepare(n_max) reserves at least what any call of any mode requests at any n <= n_max: n_max at every transition,
    one point past it and one workgroup past it; every multiple of 256 up to n_max and ragged sizes in between.  The 25 % slack
    of the allocation is not counted."""
    n_top = trans[-1] * BLOCK + BLOCK
    worst = 0  # most words any call on n' <= n requests, n walking up in workgroup steps
    prefix = {}
    for need in range(0, n_top // BLOCK + 1):
        for n in (need * BLOCK - 69, need * BLOCK):  # a ragged size inside the workgroup, then its multiple of 256
            if n >= 0:
                worst = max(worst, requested(lrm.dbg_tol_grid(n)))
        prefix[need] = worst
    n_maxes = sorted({t * BLOCK + d for t in trans for d in (0, 1, BLOCK)} | {TOLTAB_MIN_POINTS - 1, TOLTAB_MIN_POINTS, 1})
    bad = []
    for n_max in n_maxes:
        reserved = lrm.dbg_tol_grid(n_max)["prepare_words"]
        # calls on n <= n_max: every full workgroup below, and the ragged sizes of n_max's own last workgroup
        need_below = n_max // BLOCK
        most = max(prefix[need_below], max(requested(lrm.dbg_tol_grid(n)) for n in range(need_below * BLOCK, n_max + 1, 37)),
                   requested(lrm.dbg_tol_grid(n_max)))
        if most > reserved:
            bad.append((n_max, most, reserved))
    assert not bad, f"lrm_tol_prepare(n_max) reserves fewer queue words than a later call on fewer points requests: {bad[:6]}"


@pytest.mark.parametrize("n_max,n", [(3_670_017, 3_670_016), (7_340_033, 7_340_032), (11_010_049, 11_010_048)])
def test_prepare_covers_the_calls_of_the_issue(lrm, n_max, n):
    """the three cases the sizing bug was found with: one workgroup less than prepared needs twice the workgroups"""
    assert requested(lrm.dbg_tol_grid(n)) <= lrm.dbg_tol_grid(n_max)["prepare_words"]


def test_table_queue_words_are_monotone_up_to_2_31(lrm, trans):
    """lrm_tol_tab_queue_words (and the words without a table) never fall as n grows: every multiple of 256 through the last
    transition and a while past it, then dense windows around every multiple of the table kernel's base grid up to 2^31
    points, and a coarse walk in between"""
    t = transitions(lrm)
    base = min(k for k, v in t.items() if "tab" in v)  # the table kernel's first round step: its base grid
    needs = set(range(0, 2 * trans[-1]))
    top = (1 << 31) // BLOCK + 64
    for k in range(1, top // base + 2):
        needs.update(range(max(k * base - 128, 0), min(k * base + 129, top + 1)))
    needs.update(range(0, top + 1, 1021))
    needs = sorted(needs)
    g = [lrm.dbg_tol_grid(n * BLOCK) for n in needs]
    tab = np.array([v["tab_words"] for v in g], np.int64)
    notab = np.array([v["notab_words"] for v in g], np.int64)
    drops = np.nonzero(np.diff(tab) < 0)[0]
    assert len(drops) == 0, f"lrm_tol_tab_queue_words falls at n = {[needs[i + 1] * BLOCK for i in drops[:5]]}"
    assert (np.diff(notab) >= 0).all()
    # and the sizes right at the 32-bit edges the GPU test runs
    edge = [lrm.dbg_tol_grid(n) for n in ((1 << 31) - 1, 1 << 31, (1 << 31) + 4161)]
    assert edge[0]["tab_words"] <= edge[1]["tab_words"] <= edge[2]["tab_words"]
    assert edge[2]["prepare_words"] >= max(requested(g) for g in edge)


def test_the_gpu_shape_test_has_a_size_on_each_side_of_every_transition(lrm, trans):
    """tests/test_gpu_shapes.py runs, for every transition t, a cloud of t workgroups (the grid before) and one of t + 1 (the
    grid after), a ragged one, and the table kernels' dispatch switch"""
    sizes = gpu_sizes(lrm)
    needs = {-(-n // BLOCK) for n in sizes}
    for t in trans:
        assert t in needs and t + 1 in needs, t
        assert any(-(-n // BLOCK) in (t, t + 1) and n % 64 and n % 4 for n in sizes), t
        g0, g1 = lrm.dbg_tol_grid(t * BLOCK), lrm.dbg_tol_grid(t * BLOCK + 1)
        shape0 = [g0[k] for k in KERNELS + ("tab_words", "notab_words")] + [-(-t // g0[k]) for k in KERNELS]
        shape1 = [g1[k] for k in KERNELS + ("tab_words", "notab_words")] + [-(-(t + 1) // g1[k]) for k in KERNELS]
        assert shape0 != shape1, t  # workgroups, words or rounds differ across the transition
    assert {TOLTAB_MIN_POINTS - 1, TOLTAB_MIN_POINTS, TOLTAB_MIN_POINTS + 1} <= set(sizes)
    assert max(sizes) > 2 * trans[-1] * BLOCK  # one cloud past the rounds cap
