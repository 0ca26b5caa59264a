"""The table kernels on clouds built on the plane table's own lattice and seams (tests/lattice_cases.py), on the GPU (run with -m gpu),
against the oracle alone: LRM_MODE_TOL_REL (the bench headline), LRM_MODE_TOL and the table-guided LRM_MODE_FAST.

tests/test_lattice_cpu.py asks the same of the host paths; the device code differs from them in v_cvt_i32_f32 instead of the host's
guarded conversion, the LDS copies of rows and bounds, v_dot4 and the half conversion of the bounds, the `anyfar` ballot with its two
instances of lrm_toltab_lookup2, and the doubt queue.  Points within 3e-4 mm of a cell edge, waves with exactly one outer-grid lane
(or exactly one inner-grid lane), positions at and beyond the end of the outer grid: every family of lattice_cases in the four lane
orders (a family without outer-grid points: shuffled only), the three modes, lrm.device.reach_dist with mask and ballot words, and
the distance-only launch.  A family whose points all lie on the outer grid (outer_edges, grid_end, beyond) gives half of its cloud
to sub_edges, so that its waves can be mixed and the inner-grid lanes of a mixed wave sit on cell edges themselves.

Every case first meets the conditions of tests/test_lattice_cpu.py that its own cloud can be held to, from the float64 model alone.
Outputs are prefilled (mask 9, vectors -7), so an entry the kernel leaves unwritten fails."""
import functools

import numpy as np
import pytest

import ik_cases
import lattice_cases as lc
import shell_cases as sc
from conftest import bits_equal
from tolcheck import TOL, check_rel, field_error, oracle_parallel, packed, soa

pytestmark = pytest.mark.gpu

N = 65_536          # per case, with LRM_TOL_TABLE=2: the table kernel runs at every size
N_DEFAULT = 200_000  # the default dispatch takes the table kernel from this size on
SEED = 1
DEVICE_LEGS = ("m2_a", "m2_b", "moon_a", "moon_b", lc.WIDEST_YAW_LEG, lc.NARROWEST_YAW_LEG)
KEYS = lc.case_keys(DEVICE_LEGS, ("id", "tilt_y"))
MODES = ("FAST", "TOL", "TOL_REL")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def back_to_fast(lrm):
    yield
    lrm.set_mode(lrm.MODE_FAST)


def reference(lrm, oracle, frame, pts, leg, q, aim=None):
    m, d, v = oracle_parallel(oracle, pts, leg, q)
    c = dict(pts=pts, leg=leg, q=q, m=m, d=d, v=v, nref=np.linalg.norm(d.astype(np.float64), axis=1),
             thr=sc.thr(pts, sc.band_terms(lrm, leg, q)), far=frame.coords(pts)["far"], aim=aim)
    for a in (pts, m, d, v, c["nref"], c["thr"], c["far"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(key):
    """cloud and reference of a case, computed once and left unchanged: dict(pts, leg, q, m, d, v, nref, thr, far, aim)"""
    import lrm_amd as lrm
    from oracle.orc import Oracle
    oracle = Oracle()
    family = key[0]
    leg, q = lc.resolve(lrm, key)
    yaw = ik_cases.limits(oracle, leg, q)["coxa"]
    frame = lc.Frame(leg, q, yaw)
    n = N // 2 if family in lc.ALL_FAR else N
    pts, rec = lc.make(family, n, leg, q, yaw, SEED, with_aim=True)
    aim = lc.aim_figures(frame, pts, rec)
    if family in lc.ALL_FAR:
        pts = np.ascontiguousarray(np.concatenate([pts, lc.make("sub_edges", N - n, leg, q, yaw, SEED)]))
    return reference(lrm, oracle, frame, pts, leg, q, aim)


def check_case_conditions(key, c):
    """from the float64 model alone, before any code under test runs: a case that misses them is a wrong case"""
    family, aim, far = key[0], c["aim"], c["far"]
    if family != "beyond":
        window = lc.AIM_OUTER if family in ("outer_edges", "grid_end") else lc.AIM_INNER
        assert (aim["miss"] <= window).mean() >= lc.MIN_AIMED, (key, float((aim["miss"] <= window).mean()))
        assert aim["below"] >= lc.MIN_EACH_SIDE and aim["above"] >= lc.MIN_EACH_SIDE, (key, aim["below"], aim["above"])
    if family in lc.ALL_FAR:
        assert far[:N // 2].all() and not far[N // 2:].any(), key
    if family == "far_seam":
        assert lc.MIN_EACH_SIDE <= far.mean() <= 1.0 - lc.MIN_EACH_SIDE, (key, float(far.mean()))


def orders_of(c):
    return lc.LANE_ORDERS if c["far"].any() and not c["far"].all() else ("shuffled",)


def ordered(key, c, order):
    """the case's cloud and reference in a lane order (lattice_cases.lane_order): the reference is indexed, never recomputed"""
    idx = lc.lane_order(order, c["far"], np.random.default_rng([SEED, lc.LANE_ORDERS.index(order)]))
    o = dict(c, **{k: np.ascontiguousarray(c[k][idx]) for k in ("pts", "m", "d", "v", "nref", "thr", "far")})
    if order in ("one_far_lane", "one_near_lane"):  # one such lane in every wave, by the model's flags
        w = o["far"].reshape(-1, 64) if order == "one_far_lane" else ~o["far"].reshape(-1, 64)
        assert len(w) >= 8 and (w.sum(axis=1) == 1).all(), (key, order, len(w))
        assert np.array_equal(w.argmax(axis=1), np.asarray(lc.FAR_LANES)[np.arange(len(w)) % len(lc.FAR_LANES)])
    return o


def run_reach_dist_prefilled(lrm, torch, c, mode):
    """lrm.device.reach_dist with mask and ballot words into prefilled outputs -> (mask, vectors [n, 3], words, queue counts)"""
    x, y, z = soa(torch, c["pts"])
    n = len(c["pts"])
    lrm.set_mode(mode)
    mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((3, n), -7.0, dtype=torch.float32, device="cuda")
    bits = torch.full(((n + 63) // 64,), 0x0909090909090909, dtype=torch.int64, device="cuda")
    m, d, bits = lrm.device.reach_dist(x, y, z, c["leg"], c["q"], mask=mask, out=out, bits=bits)
    torch.cuda.synchronize()
    counts = lrm.dbg_tol_queue_counts() if mode != lrm.MODE_FAST else None
    lrm.set_mode(lrm.MODE_FAST)
    return m.cpu().numpy(), d.cpu().numpy().T, bits.cpu().numpy(), counts


def run_dist_prefilled(lrm, torch, c, mode):
    """lrm.device.dist with the validity byte into prefilled outputs -> (vectors [n, 3], validity)"""
    x, y, z = soa(torch, c["pts"])
    n = len(c["pts"])
    lrm.set_mode(mode)
    out = torch.full((3, n), -7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    d, v = lrm.device.dist(x, y, z, c["leg"], c["q"], out=out, valid=valid)
    torch.cuda.synchronize()
    lrm.set_mode(lrm.MODE_FAST)
    return d.cpu().numpy().T, v.cpu().numpy()


def check_field(name, lrm, mode, c, d):
    """the mode's contract on the field, on every point, from the oracle's vector alone"""
    if mode == "FAST":
        assert bits_equal(d, c["d"]).all(), f"{name}: {int((~bits_equal(d, c['d']).all(axis=1)).sum())} vectors are not bit-identical to the oracle's"
    elif mode == "TOL":
        e = field_error(c["pts"], d, c["d"], c["leg"])
        i = int(np.argmax(e["metric"]))
        print(f"{name}: metric {e['metric'][i]:.3e} at point {c['pts'][i].tolist()}, worst absolute error {np.nan_to_num(e['abs']).max():.3e} mm")
        assert e["metric"][i] <= TOL, f"{name}: metric {e['metric'][i]:.3e} at point {c['pts'][i].tolist()}"
    else:
        check_rel(name, c, d)


def check_flags(name, c, m, bits):
    assert np.array_equal(m, c["m"]), f"{name}: {int((m != c['m']).sum())} mask bytes differ from the oracle ({int((m == 9).sum())} unwritten)"
    assert np.array_equal(np.asarray(bits).view(np.uint64), packed(c["m"])), f"{name}: ballot words differ from the oracle"


@pytest.mark.parametrize("key", KEYS, ids=lc.case_id)
def test_lattice_case_in_every_lane_order_and_mode(lrm, oracle, torch_cuda, key, monkeypatch):
    """Every family on M2 and moonbot at two azimuths each and on the legs of shell_cases with the widest and the narrowest yaw range,
    under the identity and TILT_Y in turn; the table kernel at every size (LRM_TOL_TABLE=2).  In every lane order and mode: mask
    and ballot words bit for bit the oracle's on every point; LRM_MODE_FAST every float bit-identical; LRM_MODE_TOL inside the
    mode's metric (tests/tolcheck.py); LRM_MODE_TOL_REL the literal contract (|d - d_ref| <= 1e-5 |d_ref|, bit-identity below
    16 mm).  The queue figures of grid_end and beyond are printed (points, queued, overflowed segments).  Measured on an MI355X:
    the outer-grid half of a `beyond` cloud is queued almost whole (0.516 of the cloud in blocks and shuffled order, 0.966-0.979
    with one inner-grid lane per wave, 0.054-0.066 with one outer-grid lane per wave), grid_end 0.18-0.24 / 0.32-0.43 / 0.046-0.059,
    and NO segment overflows in any of them: at these sizes a workgroup has fewer points than its segment has slots, as
    tests/test_gpu_tol_shell.py found for its shells.  Nothing is pinned on the overflow count here; the overflow path stays
    covered by that file's staged-kernel case."""
    c = case(key)
    check_case_conditions(key, c)
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    for order in orders_of(c):
        o = ordered(key, c, order)
        for mode in MODES:
            name = f"{lc.case_id(key)} {order} {mode}"
            m, d, bits, counts = run_reach_dist_prefilled(lrm, torch_cuda, o, getattr(lrm, "MODE_" + mode))
            if counts is not None:
                npts, nq, nover = counts
                assert npts == len(o["pts"])
                if key[0] in ("grid_end", "beyond"):
                    print(f"{name}: {npts} points, {nq} queued ({nq / npts:.4f}), {nover} segments overflowed")
            check_flags(name, o, m, bits)
            check_field(name, lrm, mode, o, d)


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] in ("sub_edges", "far_seam", "grid_end")], ids=lc.case_id)
def test_lattice_case_behind_the_distance_only_call(lrm, oracle, torch_cuda, key, monkeypatch):
    """lrm.device.dist with the validity byte (the table kernels' instance without a mask), in the three modes: the validity byte
    bit for bit the oracle's, the same contract on the field"""
    c = case(key)
    check_case_conditions(key, c)
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    o = ordered(key, c, "shuffled")
    for mode in MODES:
        name = f"{lc.case_id(key)} dist {mode}"
        d, v = run_dist_prefilled(lrm, torch_cuda, o, getattr(lrm, "MODE_" + mode))
        assert np.array_equal(v, o["v"]), f"{name}: {int((v != o['v']).sum())} validity bytes differ from the oracle ({int((v == 9).sum())} unwritten)"
        check_field(name, lrm, mode, o, d)


@functools.lru_cache(maxsize=None)
def default_case():
    """every family on M2 under TILT_Y, N_DEFAULT / 8 points each, shuffled"""
    import lrm_amd as lrm
    from oracle.orc import Oracle
    oracle = Oracle()
    leg, q = lc.resolve(lrm, ("", "m2_a", "tilt_y"))
    yaw = ik_cases.limits(oracle, leg, q)["coxa"]
    pts = np.concatenate([lc.make(f, N_DEFAULT // len(lc.FAMILIES), leg, q, yaw, SEED + 1) for f in lc.FAMILIES])
    pts = np.ascontiguousarray(pts[np.random.default_rng(SEED).permutation(len(pts))])
    return reference(lrm, oracle, lc.Frame(leg, q, yaw), pts, leg, q)


@pytest.mark.parametrize("mode", MODES)
def test_lattice_mixture_through_the_default_dispatch(lrm, oracle, torch_cuda, mode, monkeypatch):
    """LRM_TOL_TABLE unset: at 200 000 points the library itself takes the table kernels"""
    monkeypatch.delenv("LRM_TOL_TABLE", raising=False)
    monkeypatch.delenv("LRM_XTAB", raising=False)
    c = default_case()
    assert len(c["pts"]) == N_DEFAULT and 0.3 < c["far"].mean() < 0.7
    name = f"mixture {mode}"
    m, d, bits, counts = run_reach_dist_prefilled(lrm, torch_cuda, c, getattr(lrm, "MODE_" + mode))
    if counts is not None:
        print(f"{name}: {counts[0]} points, {counts[1]} queued, {counts[2]} segments overflowed")
        assert counts[0] == N_DEFAULT
    check_flags(name, c, m, bits)
    check_field(name, lrm, mode, c, d)
