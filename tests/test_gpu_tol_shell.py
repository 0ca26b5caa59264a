"""LRM_MODE_TOL_REL (the bench headline) and LRM_MODE_TOL on threshold-shell clouds, on the GPU (run with -m gpu), against the oracle.

LRM_MODE_TOL_REL promises |d - d_ref| <= 1e-5 |d_ref| for EVERY vector.  Vectors that come out shorter than the kernel's threshold
(max(LRM_TOL_REL_MM, LRM_TOL_REL_BANDS bands)) are replayed bit for bit; every longer one is as good as the FP32 FMA / v_rsq_f32
arithmetic of lrm_tab_point, whose absolute error (~1e-4 mm) does not shrink with the vector.  The relative error is therefore worst
just above the threshold.  A uniform cloud has 1.6-5 % of its points there, a shell (tests/shell_cases.py) 40-85 %; the same cases as
tests/test_tol_shell_cpu.py, whose host emulation has another rsq than the device.

The bound of every assertion on the field comes from the oracle's vector (1e-5 |d_ref|, bit-identity below 16 mm, tolcheck.TOL for
LRM_MODE_TOL).  The kernel's threshold appears in one assertion only, the margin test: the arithmetic alone (LRM_MODE_TOL, nothing
replayed) must meet 1e-5 on every vector at least as long as the threshold at its point -- the contract restated; threshold /
crossover is the margin.  The bound remains empirical: no forward-error derivation stands behind it."""
import functools

import numpy as np
import pytest

import shell_cases as sc
from tolcheck import TOL, check_rel, field_error, oracle_parallel, packed, run_reach_dist, soa

pytestmark = pytest.mark.gpu

N = 200_000   # per case: the table kernel is the default from this size on
SEED = 1
OVERFLOW_KEY = ("uni_shell", "m2_a", "tilt_y")
OVERFLOW_N = 400_000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def back_to_fast(lrm):
    yield
    lrm.set_mode(lrm.MODE_FAST)


@functools.lru_cache(maxsize=None)
def case(key, n=N):
    """cloud and reference of a case, computed once and left unchanged: dict(pts, leg, q, m, d, v, nref, thr, in_band, short)"""
    import lrm_amd as lrm
    from oracle.orc import Oracle
    oracle = Oracle()
    leg, q = sc.resolve(lrm, key)
    pts = sc.make(key[0], n, lrm, leg, q, lambda p: oracle_parallel(oracle, p, leg, q)[1], SEED)
    m, d, v = oracle_parallel(oracle, pts, leg, q)
    terms = sc.band_terms(lrm, leg, q)
    in_band, short = sc.shares(pts, d, terms)
    c = dict(pts=pts, leg=leg, q=q, m=m, d=d, v=v, nref=np.linalg.norm(d.astype(np.float64), axis=1), thr=sc.thr(pts, terms),
             in_band=in_band, short=short)
    for a in (pts, m, d, v, c["nref"], c["thr"]):
        a.setflags(write=False)
    return c


def check_case_conditions(key, c):
    """from the oracle alone, before any code under test runs: a case that misses them is a wrong case"""
    assert c["in_band"] >= sc.MIN_IN_BAND, (key, c["in_band"])
    if key[0] == "mix_shell":
        assert c["short"] >= sc.MIN_SHORT_MIX, (key, c["short"])


@pytest.mark.parametrize("key", sc.case_keys(), ids=sc.case_id)
def test_rel_contract_on_every_shell(lrm, oracle, torch_cuda, key, monkeypatch):
    """The contract on every family, leg and orientation, with the table kernel (LRM_TOL_TABLE=2) and the staged kernel (0): mask and
    ballot words bit-identical, the literal bound on every point with none left out, every vector below 16 mm bit-identical.  The
    queue figures are printed, not asserted: whatever overflowed (the staged kernel on a mix_shell: hundreds of segments), the
    result must be right."""
    c = case(key)
    check_case_conditions(key, c)
    for table in ("2", "0"):
        monkeypatch.setenv("LRM_TOL_TABLE", table)
        m, d, bits, (npts, nq, nover) = run_reach_dist(lrm, torch_cuda, c, lrm.MODE_TOL_REL)
        print(f"{sc.case_id(key)} LRM_TOL_TABLE={table}: {c['in_band']:.3f} in [thr, 2 thr), {c['short']:.3f} in (0, thr); "
              f"{nq / max(npts, 1):.4f} of the cloud through the fix-up, {nover} segments overflowed")
        assert npts == len(c["pts"])
        check_rel(f"{sc.case_id(key)} table={table}", c, d, m, c["m"], bits)


@pytest.mark.parametrize("key", [k for k in sc.case_keys() if k[0] in ("grid_shell", "mix_shell")], ids=sc.case_id)
def test_rel_contract_behind_the_other_entry_points(lrm, oracle, torch_cuda, key, monkeypatch):
    """The distance-only launch (validity byte) on device SoA arrays and the host float3 arrays of the apply_kernel boundary
    (lrm_dist / lrm_reach_dist: the AoS instantiation of the table kernel, whose replay stores differ): the same assertions."""
    c = case(key)
    check_case_conditions(key, c)
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    x, y, z = soa(torch_cuda, c["pts"])
    lrm.set_mode(lrm.MODE_TOL_REL)
    d_dev, v_dev = lrm.device.dist(x, y, z, c["leg"], c["q"])
    torch_cuda.cuda.synchronize()
    d_aos, v_aos, _ = lrm.apply_dist(c["pts"], c["leg"], c["q"])
    m_aos, d2_aos, _ = lrm.apply_reach_dist(c["pts"], c["leg"], c["q"])
    lrm.set_mode(lrm.MODE_FAST)
    check_rel(f"{sc.case_id(key)} lrm_dist_dev (SoA)", c, d_dev.cpu().numpy().T, v_dev.cpu().numpy(), c["v"])
    check_rel(f"{sc.case_id(key)} lrm_dist (float3)", c, d_aos, v_aos, c["v"])
    check_rel(f"{sc.case_id(key)} lrm_reach_dist (float3)", c, d2_aos, m_aos, c["m"])


def test_rel_overflowing_doubt_segments_on_shells(lrm, oracle, torch_cuda, monkeypatch):
    """Overflow of a workgroup's doubt segment ("whole workgroup redone by the bit-exact code") on ordinary input.

    The table kernel on a tilted uni_shell, 16 % of which is in doubt -- the capacity of a segment (LRM_TOL_TAB_SEG_CAP slots per
    1536 points: 17 %): measured on an MI355X, NO size up to 400 000 points overflows (0.164 of the cloud queued, 0 segments
    overflowed at 200 000 and at 400 000): the grid grows with the cloud, and at these sizes a workgroup has fewer points than its
    segment has slots.  The test keeps the cloud and reports what it finds.

    The staged kernel (LRM_TOL_TABLE=0) queues LRM_MODE_TOL_REL's short vectors as well: on a mix_shell, half of which is short,
    390-780 segments of a 200 000-point cloud overflow (measured), and that is asserted, so that the path stays covered.

    Either way: mask and ballot words bit-identical to LRM_MODE_FAST's and the oracle's, the contract on the field."""
    for key, n, table, must_overflow in ((OVERFLOW_KEY, OVERFLOW_N, "2", False), (("mix_shell", "m2_a", "id"), N, "0", True)):
        c = case(key, n)
        check_case_conditions(key, c)
        monkeypatch.setenv("LRM_TOL_TABLE", table)
        m0, _, bits0, _ = run_reach_dist(lrm, torch_cuda, c, lrm.MODE_FAST)
        m, d, bits, (npts, nq, nover) = run_reach_dist(lrm, torch_cuda, c, lrm.MODE_TOL_REL)
        print(f"{sc.case_id(key)}, {npts} points, LRM_TOL_TABLE={table}: {nq / npts:.4f} of the cloud through the fix-up, {nover} segments overflowed")
        assert npts == n
        assert np.array_equal(m, m0) and np.array_equal(bits, bits0), "mask differs from LRM_MODE_FAST"
        check_rel(f"{sc.case_id(key)} table={table}", c, d, m, c["m"], bits)
        if must_overflow:
            assert nover > 0, "this cloud no longer overflows a doubt segment: the overflow path is not covered by it any more"


def test_rel_mix_shell_of_3e6_points_flushes_inside_the_loop(lrm, torch_cuda):
    """mix_shell on M2 at 3 000 000 points: half short vectors, half just above the threshold.  At this size a wave's 64-slot LDS
    segment has no room for its rounds of short vectors and is replayed on the spot (the in-loop flush), next to the vectors
    that matter.  Against the device's LRM_MODE_FAST (itself checked bit for bit against the oracle by tests/test_gpu_parity.py),
    as test_tol_rel_cloud_of_short_vectors_is_replayed_in_the_kernel does."""
    torch = torch_cuda
    n = 3_000_000
    leg = lrm.get_M2_leg(0.0)

    def fast_dist(p):
        x, y, z = soa(torch, p)
        lrm.set_mode(lrm.MODE_FAST)
        _, d = lrm.device.reach_dist(x, y, z, leg, None)
        torch.cuda.synchronize()
        return d.cpu().numpy().T

    pts = sc.make("mix_shell", n, lrm, leg, None, fast_dist, SEED)
    x, y, z = soa(torch, pts)
    lrm.set_mode(lrm.MODE_FAST)
    m1, d1 = lrm.device.reach_dist(x, y, z, leg, None)
    lrm.set_mode(lrm.MODE_TOL_REL)
    m2, d2 = lrm.device.reach_dist(x, y, z, leg, None)
    torch.cuda.synchronize()
    npts, nq, nover = lrm.dbg_tol_queue_counts()
    lrm.set_mode(lrm.MODE_FAST)
    in_band, short_share = sc.shares(pts, d1.cpu().numpy().T, sc.band_terms(lrm, leg, None))
    assert in_band >= sc.MIN_IN_BAND and short_share >= sc.MIN_SHORT_MIX, (in_band, short_share)
    assert torch.equal(m1, m2)
    nref = d1.double().norm(dim=0)
    err = (d2.double() - d1.double()).norm(dim=0)
    lit = torch.nan_to_num(err / nref, nan=0.0, posinf=float("inf"))
    print(f"mix_shell, {n} points: {in_band:.3f} in [thr, 2 thr), {short_share:.3f} in (0, thr); worst literal error {float(lit.max()):.3e} at "
          f"|d_ref| = {float(nref[int(lit.argmax())]):.3f} mm; {nq / npts:.4f} of the cloud through the fix-up, {nover} segments overflowed")
    assert bool((err <= TOL * nref).all())
    short = nref < 16.0
    assert bool((d1.view(torch.int32)[:, short] == d2.view(torch.int32)[:, short]).all())
    assert npts == n


@functools.lru_cache(maxsize=None)
def run_tol(key):
    """LRM_MODE_TOL (nothing replayed) on a case -> violations and figures"""
    import torch
    import lrm_amd as lrm
    c = case(key)
    m, d, bits, (npts, nq, nover) = run_reach_dist(lrm, torch, c, lrm.MODE_TOL)
    x, y, z = soa(torch, c["pts"])
    lrm.set_mode(lrm.MODE_TOL)
    _, v = lrm.device.dist(x, y, z, c["leg"], c["q"])
    torch.cuda.synchronize()
    lrm.set_mode(lrm.MODE_FAST)
    e = field_error(c["pts"], d, c["d"], c["leg"])
    nref = c["nref"]
    with np.errstate(invalid="ignore", divide="ignore"):
        lit = np.where(nref > 0, e["abs"] / nref, 0.0)
    return dict(key=key, bad_mask=int((m != c["m"]).sum()), bad_valid=int((v.cpu().numpy() != c["v"]).sum()),
                bad_bits=int((bits.view(np.uint64) != packed(c["m"])).sum()), metric=float(e["metric"].max(initial=0.0)),
                worst_abs_mm=float(np.nan_to_num(e["abs"]).max(initial=0.0)), queued=nq / max(npts, 1), nover=nover,
                worst_literal_from_thr=float(lit[nref >= c["thr"]].max(initial=0.0)),
                crossover=sc.crossover(nref, e["abs"], c["thr"]))


@pytest.mark.parametrize("key", sc.case_keys(), ids=sc.case_id)
def test_tol_mode_on_every_shell(lrm, oracle, torch_cuda, key):
    """LRM_MODE_TOL on the shells: mask, validity byte and ballot words bit-identical, the field inside the mode's own metric
    (tests/tolcheck.py)."""
    check_case_conditions(key, case(key))
    r = run_tol(key)
    print(f"{sc.case_id(key)}: metric {r['metric']:.3e}, worst absolute error {r['worst_abs_mm']:.3e} mm, {r['queued']:.4f} queued, {r['nover']} segments "
          f"overflowed; crossover {r['crossover']}")
    assert r["bad_mask"] == 0 and r["bad_valid"] == 0 and r["bad_bits"] == 0
    assert r["metric"] <= TOL


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_margin_of_the_threshold_measured(lrm, oracle, torch_cuda, family):
    """The margin, measured and not assumed: LRM_MODE_TOL replays nothing, so its field shows where the arithmetic alone stops
    meeting 1e-5 relative -- the crossover length, the longest vector that misses -- next to the threshold at that vector's point.
    Asserted: no vector at least as long as the threshold at its own point misses (crossover <= thr: the contract of
    LRM_MODE_TOL_REL restated).  thr / crossover is the margin of the setting (DESIGN.md section 3.3 carries the figures)."""
    rs = [run_tol(k) for k in sc.case_keys() if k[0] == family]
    assert len(rs) == len(sc.LEG_NAMES)
    cm = max(rs, key=lambda r: r["crossover"]["mm"])
    cf = max(rs, key=lambda r: r["crossover"]["frac"])
    wl = max(rs, key=lambda r: r["worst_literal_from_thr"])
    print(f"{family}: crossover {cm['crossover']['mm']:.3f} mm (thr there {cm['crossover']['thr_mm']:.3f} mm, {sc.case_id(cm['key'])}); as a fraction of "
          f"thr at most {cf['crossover']['frac']:.3f} ({sc.case_id(cf['key'])}): margin {1.0 / max(cf['crossover']['frac'], 1e-300):.2f}; "
          f"worst literal error from thr on {wl['worst_literal_from_thr']:.3e} ({sc.case_id(wl['key'])}); worst absolute error "
          f"{max(r['worst_abs_mm'] for r in rs):.3e} mm; queued {min(r['queued'] for r in rs):.4f}..{max(r['queued'] for r in rs):.4f}, "
          f"{sum(r['nover'] for r in rs)} segments overflowed")
    for r in rs:
        assert r["crossover"]["frac"] <= 1.0, (sc.case_id(r["key"]), r["crossover"])
