"""The plane table's host paths on clouds built on the table's own lattice and seams (tests/lattice_cases.py), against the oracle:
lrm_dbg_toltab_host (lrm_tab_point, the tolerance arithmetic), lrm_dbg_xtab_host (the table-guided bit-exact evaluation),
lrm_dbg_replay_host (the strict replay of lrm_tab_point's decisions) and lrm_dbg_toltab_bounds (the cells' lower bounds).

A cell index is one FMA and a truncation of a plane coordinate that carries a few 1e-5 mm of rounding; the builder's margin around
every cell (lrm_tb_slack: 1.26e-3 mm on the inner grid, 3.05e-3 mm on the outer one) is what makes the neighbour's answer good
enough for a point that lands on the wrong side of a line.  A uniform cloud puts one point in 1e5 there.  These clouds put nearly
all of theirs within 3e-4 mm (inner grid, the seam) or 1.2e-3 mm (outer grid) of a line, on both sides of it.

Every case first meets conditions checked from the float64 model of lattice_cases and from the oracle alone, before any code under
test runs: a case that misses them is a wrong case and fails.  tests/test_gpu_lattice.py asks the same of the kernels.

Each test prints its figures (-s): aim shares, doubt-free shares, bound margins; DESIGN.md section 3.1 carries the bound margins.

What these clouds can and cannot tell (tried on a scratch build of the host paths, nothing of it kept): with the inner scale used
for outer-grid lanes in lrm_toltab_lookup2, 31 of the 96 cases fail (every far_seam and coarse_edges case, most outer_edges cases).
With lrm_tb_slack set to 0 every test here still passes, and no offset can change that: a point is never further on the wrong side
of a line than its own rounding, 1e-4 mm, and every decision a cell takes for its points also holds a margin of the run-time band
(>= 2e-3 mm) or tie band (a quarter of it) beyond the cell's disc, so the neighbour's answer stays right without the slack; the
bounds keep 1.3e-3 mm without it.  The slack is a second margin, not the only one.  Shrinking the cells by twice the slack
(lrm_tb_slack = -2.5e-3 mm) fails the bounds test below on the 16 mm lines (lb - dist = 2.1e-3 mm)."""
import functools

import numpy as np
import pytest

import ik_cases
import lattice_cases as lc
import shell_cases as sc
from conftest import bits_equal
from tolcheck import TOL, field_error

N = 100_000
SEED = 1
MIN_DOUBT_FREE = 0.9      # inner families and far_seam: these tests are about the table's answers, not about the fix-up
MIN_REACHABLE_SUB = 0.05  # sub_edges, by the oracle: the valid side of the table is exercised as well
MIN_PER_COARSE_LINE = 50


@pytest.fixture(scope="module", autouse=True)
def built(lrm, oracle):
    """the library and the oracle exist before evaluate() loads them"""


def test_constants_match_the_sources():
    """today's lattice: a changed constant moves every cloud of lattice_cases, and must be looked at"""
    k = lc.constants()
    assert (k["N"], k["SUB"], k["NB"], k["H_INNER"], k["H_OUTER"], k["FAR_LIMIT"]) == (128, 16, 64, 16.0, 128.0, 1023.0)
    # the windows of the aim conditions are below the builder's margin of their grid
    assert lc.AIM_INNER < lc.slack(k["H_INNER"]) and lc.AIM_OUTER < lc.slack(k["H_OUTER"])
    assert abs(lc.slack(k["H_INNER"]) - 1.256e-3) < 1e-9 and abs(lc.slack(k["H_OUTER"]) - 3.048e-3) < 1e-9


def test_frame_maps_invert_each_other():
    """Frame.to_coxa undoes Frame.from_coxa in float64, also for the fixture orientations, which are not unit quaternions"""
    import lrm_amd as lrm
    rng = np.random.default_rng(3)
    c = rng.uniform(-900, 900, (1000, 3))
    for name, q in (("m2_a", sc.IDENTITY), ("moon_b", sc.TILT_Y), ("rnd_2", sc.TILT_Z)):
        leg = sc.legs(lrm)[name][0]
        f = lc.Frame(leg, q, (float(leg[ik_cases.MIN_COXA]), float(leg[ik_cases.MAX_COXA])))
        p = f.from_coxa(c)
        back = (p @ f.fwd.T)  # to_coxa takes float32 points: undo the orientation here, in float64
        assert np.abs(back @ f.back.T - p).max() < 1e-9
        p32 = p.astype(np.float32)
        assert np.abs(f.to_coxa(p32) - c).max() < 3e-4  # float32 rounding of |p| < 2000 mm: 3 x 6.1e-5 at the most


def test_lane_orders_have_the_lanes_they_promise():
    """one_far_lane / one_near_lane: exactly one such lane in every wave of 64, at lane 0, 31, 32, 63 in turn; blocks and shuffled
    are permutations"""
    rng = np.random.default_rng(5)
    far = rng.random(20_000) < 0.3
    for order in lc.LANE_ORDERS:
        idx = lc.lane_order(order, far, np.random.default_rng(7))
        assert len(np.unique(idx)) == len(idx)
        if order in ("blocks", "shuffled"):
            assert len(idx) == len(far)
            continue
        assert len(idx) % 64 == 0 and len(idx) >= 64 * 90
        w = far[idx].reshape(-1, 64)
        one = w if order == "one_far_lane" else ~w
        assert (one.sum(axis=1) == 1).all()
        assert np.array_equal(one.argmax(axis=1), np.asarray(lc.FAR_LANES)[np.arange(len(w)) % 4])
    b = far[lc.lane_order("blocks", far, rng)]
    assert not b[:int((~far).sum())].any() and b[int((~far).sum()):].all()


@functools.lru_cache(maxsize=None)
def evaluate(key):
    """figures and violations of one case (arrays are dropped: 96 cases of 1e5 points)"""
    import lrm_amd as lrm
    from oracle.orc import Oracle
    oracle = Oracle()
    family = key[0]
    leg, q = lc.resolve(lrm, key)
    if not lrm.dbg_tol_ok(leg, q):
        return dict(key=key, eligible=False)
    yaw = ik_cases.limits(oracle, leg, q)["coxa"]
    frame = lc.Frame(leg, q, yaw)
    pts, rec = lc.make(family, N, leg, q, yaw, SEED, with_aim=True)
    # ---- the case itself: the float64 model and the oracle
    aim = lc.aim_figures(frame, pts, rec)
    co = frame.coords(pts)
    want_m = oracle.reach(pts, leg, q)
    want_d, want_v = oracle.dist(pts, leg, q)
    out = dict(key=key, eligible=True, aimed=aim["n"], below=aim["below"], above=aim["above"], far=float(co["far"].mean()),
               reachable=float(want_m.mean()))
    if aim["n"]:
        out.update(within_inner=float((aim["miss"] <= lc.AIM_INNER).mean()), within_outer=float((aim["miss"] <= lc.AIM_OUTER).mean()),
                   worst_miss=float(aim["miss"].max()))
    if family == "coarse_edges":
        H = frame.k["H_INNER"]
        lines = np.arange(-(frame.k["N"] // 2 - 1), frame.k["N"] // 2) * H
        x_lines = rec["line"][np.isin(rec["kind"][:, 0], (lc.X_OWN, lc.X_FLIP)), 0]
        z_lines = rec["line"][rec["kind"][:, 1] == lc.Z, 1]
        # an abscissa line is reached by the point's own plane (r >= 1 mm: line + coxa_length >= 1) or by the opposite one
        x_reached = lines[(lines + frame.coxa >= 1.0) | (-lines - frame.coxa >= 1.0)]
        out["min_per_x_line"] = int(min((x_lines == v).sum() for v in x_reached))
        out["min_per_z_line"] = int(min((z_lines == v).sum() for v in lines))
        out["x_lines"] = len(x_reached)
    # ---- the code under test
    mt, dt, doubt_t, _ = lrm.dbg_toltab_host(pts, leg, q)
    mx, dx, doubt_x, _ = lrm.dbg_xtab_host(pts, leg, q)
    mr, dr, doubt_r = lrm.dbg_replay_host(pts, leg, q)
    st, sx, sr = ((d & 0xffff) == 0 for d in (doubt_t, doubt_x, doubt_r))
    e = field_error(pts[st], dt[st], want_d[st], leg)
    out.update(doubt_free=float(st.mean()), unanswered=float(((doubt_t & 0x100) != 0).mean()),
               doubt_free_x=float(sx.mean()), doubt_free_r=float(sr.mean()),
               bad_mask_t=int((mt[st] != want_m[st]).sum()), bad_valid_t=int((mt[st] != want_v[st]).sum()),
               metric=float(e["metric"].max(initial=0.0)), worst_abs_mm=float(np.nan_to_num(e["abs"]).max(initial=0.0)))
    for tag, m, d, s in (("x", mx, dx, sx), ("r", mr, dr, sr)):
        out[f"bad_mask_{tag}"] = int((m[s] != want_m[s]).sum())
        out[f"bad_valid_{tag}"] = int((m[s] != want_v[s]).sum())
        out[f"bad_bits_{tag}"] = int((~bits_equal(d[s], want_d[s]).all(axis=1)).sum())
    return out


def check_conditions(key, r):
    """from the float64 model and the oracle alone"""
    family = key[0]
    if family == "beyond":
        assert r["far"] == 1.0
        return
    window = "within_outer" if family in ("outer_edges", "grid_end") else "within_inner"
    assert r[window] >= lc.MIN_AIMED, f"a wrong case: {r[window]:.3f} of the aimed coordinates within the window (worst miss {r['worst_miss']:.2e} mm)"
    assert r["below"] >= lc.MIN_EACH_SIDE and r["above"] >= lc.MIN_EACH_SIDE, f"a wrong case: {r['below']:.2f} below / {r['above']:.2f} above the lines"
    if family == "far_seam":
        assert lc.MIN_EACH_SIDE <= r["far"] <= 1.0 - lc.MIN_EACH_SIDE, f"a wrong case: {r['far']:.2f} of the points beyond the far limit"
    if family in lc.ALL_FAR:
        assert r["far"] == 1.0
    if family in ("sub_edges", "flip_edges", "limit_edges"):
        assert r["far"] == 0.0
    if family == "coarse_edges":
        assert r["min_per_x_line"] >= MIN_PER_COARSE_LINE and r["min_per_z_line"] >= MIN_PER_COARSE_LINE, (r["min_per_x_line"], r["min_per_z_line"])
    if family == "sub_edges":
        assert r["reachable"] >= MIN_REACHABLE_SUB, f"a wrong case: {r['reachable']:.3f} reachable"


@pytest.mark.parametrize("key", lc.case_keys(), ids=lc.case_id)
def test_lattice_case_on_the_host(key):
    """Every family on every leg of shell_cases, the orientation rotating as there.  Every point without doubt: toltab's mask and
    validity are the oracle's and its field is inside the mode's metric; xtab and the replay are bit-identical to the oracle in
    mask, validity and all three floats.  The doubt-free share of the inner families and of the seam is at least 0.9 (measured:
    sub_edges 0.95-0.97, coarse_edges 0.97-0.98, flip_edges 0.93-0.97, limit_edges 0.96-0.98, far_seam 0.97-0.98); it is printed, with no
    bound, where the table has no answer by design (grid_end 0.5-0.7, beyond 0.01 with 0.99 of the cloud unanswered)."""
    r = evaluate(key)
    if not r["eligible"]:
        pytest.skip(f"leg {key[1]} under {key[2]} is not eligible for the tolerance mode (lrm.dbg_tol_ok)")
    print(f"{lc.case_id(key)}: {r['aimed']} aimed coordinates, {r.get('within_inner', 0):.3f} within {lc.AIM_INNER} mm, {r.get('within_outer', 0):.3f} within "
          f"{lc.AIM_OUTER} mm of their line (worst miss {r.get('worst_miss', 0):.2e} mm), {r['below']:.2f} below / {r['above']:.2f} above; "
          f"{r['far']:.3f} far, {r['reachable']:.3f} reachable"
          + (f", at least {r['min_per_x_line']} / {r['min_per_z_line']} points on every abscissa / z line" if key[0] == "coarse_edges" else "")
          + f"; doubt-free {r['doubt_free']:.4f} (toltab; {r['unanswered']:.3f} unanswered), {r['doubt_free_x']:.4f} (xtab), {r['doubt_free_r']:.4f} (replay); "
          f"metric {r['metric']:.2e}, worst absolute error {r['worst_abs_mm']:.2e} mm")
    check_conditions(key, r)
    assert r["bad_mask_t"] == 0 and r["bad_valid_t"] == 0, "toltab: mask or validity differs on points without doubt"
    assert r["metric"] <= TOL, f"toltab: metric {r['metric']:.3e}"
    assert r["bad_mask_x"] == 0 and r["bad_valid_x"] == 0 and r["bad_bits_x"] == 0, "xtab: a doubt-free point is not bit-identical to the oracle"
    assert r["bad_mask_r"] == 0 and r["bad_valid_r"] == 0 and r["bad_bits_r"] == 0, "replay: a doubt-free point is not bit-identical to the oracle"
    if key[0] in lc.INNER_FAMILIES + ("far_seam",):
        assert r["doubt_free"] >= MIN_DOUBT_FREE, f"{1 - r['doubt_free']:.3f} of the cloud in doubt"


def test_device_legs_have_the_widest_and_narrowest_yaw_range():
    """tests/test_gpu_lattice.py names two legs of shell_cases by hand: the ones with the widest and the narrowest yaw range"""
    import lrm_amd as lrm
    span = {name: float(leg[ik_cases.MAX_COXA] - leg[ik_cases.MIN_COXA]) for name, (leg, _) in sc.legs(lrm).items()}
    assert max(span, key=span.get) == lc.WIDEST_YAW_LEG and min(span, key=span.get) == lc.NARROWEST_YAW_LEG, span


BOUND_SPACINGS = ((1.0, 1000.0), (2.0, 1000.0), (16.0, 1000.0), (32.0, 1000.0), (8.0, 8000.0))


@pytest.mark.parametrize("legname,az,q", [("m2", 0.0, sc.IDENTITY), ("moonbot", 1.1, sc.TILT_Y), ("m2", -2.0, (0.9, 0.1, 0.2, -0.3))])
def test_plane_table_lower_bounds_hold_on_the_lattice(lrm, legname, az, q):
    """test_plane_table_lower_bounds_hold (tests/test_tol_cpu.py) with plane points aimed at the table's lines: a cell's bound is a
    quantised plane lowered until it clears the 16 x 16 sub-cell values of its 32 mm bound cell, so it binds on the lattice -- the
    1 mm lines where the cell code changes, the 2 mm lines of the (q >> 1) & 15 sub-index, the 16 / 32 mm lines where the entry
    changes, the 8 mm lines of the outer grid (whose bound is the distance beyond the outer circle).  The same three assertions,
    with that test's slack.  Smallest dist - lb over invalid plane points without doubt, measured on the host build (x86-64 CPU):
    2.66e-3 mm on the 16 mm and 32 mm lines for all three legs; on the 1 mm lines 8.8e-3 (M2) and 1.7e-2 mm (moonbot); on the 2 mm
    lines 5.6e-3 .. 7.5e-3 (M2) and 1.3e-2 mm (moonbot); on the outer grid's 8 mm lines 6.0e-3 .. 3.5e-2 mm.  Over all invalid
    points, those in doubt included: 1.5e-3 mm (moonbot, 1 mm lines).  A uniform sample of the same size
    (as test_plane_table_lower_bounds_hold draws) finds 1.9e-2 .. 2.6e-2 mm on the inner grid: the lattice is where the bound binds."""
    leg = lrm.get_M2_leg(az) if legname == "m2" else lrm.get_moonbot_leg(az)
    rng = np.random.default_rng(29)
    n = 400_000
    for h, half in BOUND_SPACINGS:
        d = np.array([0.0, 1e-6, -1e-6, 2.0 ** -17 * h, -2.0 ** -17 * h, 1e-4, -1e-4, 1.2e-3, -1.2e-3])
        kmax = int(half // h) - 1
        xz = rng.integers(-kmax, kmax + 1, (n, 2)) * h + rng.choice(d, (n, 2))
        free = rng.random((n, 2)) < 0.3
        xz = np.where(free, rng.uniform(-half, half, (n, 2)), xz).astype(np.float32)
        lb, dist, valid, doubt = lrm.dbg_toltab_bounds(xz, leg, q)
        assert np.isfinite(lb).all() and (lb >= 0).all()
        assert (lb[valid != 0] == 0).all()
        slack = np.where(doubt == 0, 1e-5 * dist + 1e-4, 0.05)
        inv = (valid == 0) & (doubt == 0)
        print(f"{legname} az {az} h {h} mm: smallest dist - lb {float((dist - lb)[inv].min()):.3e} mm over {int(inv.sum())} invalid plane points without doubt, "
              f"{float((dist - lb)[valid == 0].min()):.3e} mm over all {int((valid == 0).sum())} invalid ones")
        assert (lb <= dist + slack).all(), float((lb - dist).max())
