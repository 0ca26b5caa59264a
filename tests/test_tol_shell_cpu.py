"""LRM_MODE_TOL_REL on threshold-shell clouds (tests/shell_cases.py), on the host: lrm_dbg_toltab_host (the tolerance arithmetic of
lrm_tab_point, nothing replayed) and lrm_dbg_replay_host (the strict replay of its decisions, for every point) against the oracle.

The mode's contract is |d - d_ref| <= 1e-5 |d_ref| for every vector.  A vector that comes out shorter than the kernel's threshold is
replayed and bit-identical; every longer one is only as good as the FP32 arithmetic, whose absolute error does not shrink with the
vector: the relative error is worst just above the threshold, which is where a shell puts 40-85 % of its points (1.6-5 % of a
uniform cloud).  The host's rsq is not the device's: tests/test_gpu_tol_shell.py asks the same of the kernels.

Every case first meets conditions checked from the oracle alone (shell_cases.MIN_IN_BAND, MIN_SHORT_MIX): a case that misses them is
a wrong case and fails.  The bound on the field is the literal one, from the oracle's vector; the kernel's threshold only says WHICH
of the two host outputs stands for the kernel's (the select of dist_tab_kernel: |d|^2 < thr^2 of the tolerance vector itself)."""
import functools

import numpy as np
import pytest

import shell_cases as sc
from conftest import bits_equal
from tolcheck import TOL

N = 200_000
SEED = 1
MAX_LEFT_OUT = 0.25  # doubtful points belong to the fix-up; the tilted shells have up to 18 % of them


@functools.lru_cache(maxsize=None)
def evaluate(key):
    """figures and violations of one case (arrays are dropped: 48 cases of 2e5 points)"""
    import lrm_amd as lrm
    from oracle.orc import Oracle
    oracle = Oracle()
    leg, q = sc.resolve(lrm, key)
    pts = sc.make(key[0], N, lrm, leg, q, lambda p: oracle.dist(p, leg, q)[0], SEED)
    want_d, want_v = oracle.dist(pts, leg, q)
    want_m = oracle.reach(pts, leg, q)
    terms = sc.band_terms(lrm, leg, q)
    thr = sc.thr(pts, terms)
    in_band, short = sc.shares(pts, want_d, terms)
    nref = np.linalg.norm(want_d.astype(np.float64), axis=1)

    mt, dt, doubt_t, _ = lrm.dbg_toltab_host(pts, leg, q)
    mr, dr, doubt_r = lrm.dbg_replay_host(pts, leg, q)
    sure_t = (doubt_t & 0xffff) == 0
    sure_r = (doubt_r & 0xffff) == 0
    sure = sure_t & sure_r
    err_t = np.linalg.norm(dt.astype(np.float64) - want_d.astype(np.float64), axis=1)
    # the kernel's select, on the tolerance vector itself: nn = fma(x, x, fma(y, y, z z)), replayed <=> !(nn >= thr^2)
    nn = (dt[:, 0].astype(np.float64) ** 2 + (dt[:, 1].astype(np.float64) ** 2 + np.float64(dt[:, 2] * dt[:, 2]))).astype(np.float32)
    replayed = ~(nn >= thr * thr)
    kept = sure & ~replayed  # what LRM_MODE_TOL_REL leaves to the tolerance arithmetic
    with np.errstate(invalid="ignore", divide="ignore"):
        lit = np.where(nref > 0, err_t / nref, np.where(err_t > 0, np.inf, 0.0))
    same_r = bits_equal(dr, want_d).all(axis=1)
    out = dict(key=key, in_band=in_band, short=short, left_out=float(1.0 - sure.mean()), thr_min=float(thr.min()), thr_max=float(thr.max()),
               bad_mask_t=int((mt[sure_t] != want_m[sure_t]).sum()), bad_valid_t=int((mt[sure_t] != want_v[sure_t]).sum()),
               bad_mask_r=int((mr[sure_r] != want_m[sure_r]).sum()), bad_valid_r=int((mr[sure_r] != want_v[sure_r]).sum()),
               doubt_sets_differ=int((sure_t != sure_r).sum()),
               bad_literal=int((kept & (nref >= 16.0) & (err_t > TOL * nref)).sum()),
               bad_replay=int((sure_r & ~same_r).sum()),
               replayed_share=float((sure & replayed).mean()))
    k = np.flatnonzero(kept & (nref > 0))
    i = int(k[np.argmax(lit[k])])
    out["worst_literal"] = float(lit[i])
    out["worst_literal_at"] = dict(point=[float(v) for v in pts[i]], d_ref_mm=float(nref[i]), thr_mm=float(thr[i]))
    out["worst_abs_mm"] = float(err_t[sure_t].max())
    free = np.flatnonzero(sure_t)
    out["crossover"] = sc.crossover(nref[free], err_t[free], thr[free])
    return out


@pytest.fixture(scope="module", autouse=True)
def built(lrm, oracle):
    """the library and the oracle exist before evaluate() loads them"""


@pytest.mark.parametrize("key", sc.case_keys(), ids=sc.case_id)
def test_shell_case_on_the_host(key):
    r = evaluate(key)
    print(f"{sc.case_id(key)}: thr {r['thr_min']:.2f}..{r['thr_max']:.2f} mm; {r['in_band']:.3f} of the points in [thr, 2 thr), {r['short']:.3f} in (0, thr); "
          f"{r['left_out']:.4f} in doubt (left to the fix-up), {r['replayed_share']:.3f} replayed; worst literal error {r['worst_literal']:.3e} at "
          f"{r['worst_literal_at']}; worst absolute error {r['worst_abs_mm']:.3e} mm; crossover {r['crossover']}")
    # the case itself, from the oracle alone
    assert r["in_band"] >= sc.MIN_IN_BAND, "a wrong case: too few vectors just above the threshold"
    if key[0] == "mix_shell":
        assert r["short"] >= sc.MIN_SHORT_MIX, "a wrong case: too few short vectors"
    # the code under test
    assert r["bad_mask_t"] == 0 and r["bad_mask_r"] == 0, "reach mask differs on points without doubt"
    assert r["bad_valid_t"] == 0 and r["bad_valid_r"] == 0, "validity differs on points without doubt"
    assert r["doubt_sets_differ"] == 0, "the two instances of lrm_tab_point doubt different points"
    assert r["bad_literal"] == 0, f"{r['bad_literal']} vectors of at least 16 mm that are not replayed miss 1e-5 relative"
    assert r["bad_replay"] == 0, f"{r['bad_replay']} replayed vectors are not bit-identical"
    assert r["left_out"] <= MAX_LEFT_OUT


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_shell_family_report(family):
    """Per family: the worst literal error of what LRM_MODE_TOL_REL keeps from the tolerance arithmetic, the worst absolute error, and the
    crossover length of the arithmetic alone (lrm_dbg_toltab_host replays nothing): the longest doubt-free vector that misses
    1e-5, in mm and as a fraction of the threshold at its point.  A fraction below 1 is the margin of the threshold; the cases
    above assert the contract, this prints the figures (DESIGN.md section 3.3 carries them)."""
    rs = [evaluate(k) for k in sc.case_keys() if k[0] == family]
    assert len(rs) == len(sc.LEG_NAMES)
    lit = max(rs, key=lambda r: r["worst_literal"])
    cm = max(rs, key=lambda r: r["crossover"]["mm"])
    cf = max(rs, key=lambda r: r["crossover"]["frac"])
    print(f"{family}: worst literal error {lit['worst_literal']:.3e} ({sc.case_id(lit['key'])}, {lit['worst_literal_at']}); "
          f"worst absolute error {max(r['worst_abs_mm'] for r in rs):.3e} mm; "
          f"crossover {cm['crossover']['mm']:.3f} mm (thr there {cm['crossover']['thr_mm']:.3f} mm, {sc.case_id(cm['key'])}), "
          f"as a fraction of thr at most {cf['crossover']['frac']:.3f} ({sc.case_id(cf['key'])}); "
          f"in doubt {min(r['left_out'] for r in rs):.4f}..{max(r['left_out'] for r in rs):.4f}; "
          f"in band {min(r['in_band'] for r in rs):.3f}..{max(r['in_band'] for r in rs):.3f}")
    assert all(np.isfinite(r["worst_literal"]) for r in rs)


def test_threshold_follows_the_kernel_constants():
    """thr() reads LRM_TOL_REL_MM / LRM_TOL_REL_BANDS / LRM_BAND from the sources and reproduces the figures the sources quote:
    the floor near the leg, and about 34 mm where |p|_1 + body is one metre (csrc/lrm_launch.h)."""
    import lrm_amd as lrm
    mm, bands, band = sc.constants()
    assert mm > 0 and bands > 0 and band == 4.0e-6
    leg = lrm.get_M2_leg(0.0)
    terms = sc.band_terms(lrm, leg)
    t = sc.thr(np.array([[0.0, 0.0, 0.0], [1000.0 - float(leg[1]), 0.0, 0.0], [np.nan, 0.0, 0.0]], np.float32), terms)
    assert t[0] == np.float32(mm)
    assert 0.029 * bands / 2250.0 * 1000.0 <= t[1] <= 0.036 * bands / 2250.0 * 1000.0
    assert np.isnan(t[2]) or t[2] == np.float32(mm)
