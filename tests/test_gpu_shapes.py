"""The distance / fused calls at the cloud sizes where their launch grids change shape (run with -m gpu on an MI355X).

The kernel and the grid of a call depend on its size: the table kernels from 2e5 points on, their workgroup count and rounds
per workgroup (a floor, one more round every base grid, a cap of rounds), the kernel without a table with steps of its own, and
32-bit point indices in the table kernels.  tests/grid_cases.py finds the transitions through lrm_dbg_tol_grid; here every
mode runs at each of them, through three entry points, against the CPU oracle:
  LRM_MODE_STRICT, LRM_MODE_FAST  mask, validity bytes, bit words and every float of the field bit-identical
  LRM_MODE_TOL                    masks bit-identical, field within tests/tolcheck.py's TOL
  LRM_MODE_TOL_REL                masks bit-identical, |d - d_ref| <= 1e-5 |d_ref| for every vector, bit-identical below 16 mm
and no call writes past n.  Clouds up to FULL points are compared whole; larger ones on windows: both ends and every round
boundary of every grid.  Each case prints its time."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import bits_equal, random_cloud
from grid_cases import BLOCK, RAGGED, TOLTAB_MIN_POINTS, gpu_sizes, transitions
from ik_cases import is_unit, random_legs
from tolcheck import TOL, field_error

pytestmark = pytest.mark.gpu

FULL = 4_200_000      # up to here: the whole field is compared, and the host float3 entry (lrm_reach_dist) runs too
END_WIN = 1 << 18     # points compared at each end of a larger cloud
ROUND_WIN = 1 << 16   # points compared around every round boundary k * stride of every grid
SHORT_MM = 16.0       # LRM_MODE_TOL_REL: vectors shorter than this are bit-identical to the oracle
MASK_GUARD, FIELD_GUARD, BITS_GUARD = 7, -777.0, -1
POOL = 16             # oracle threads (the GPU machines give a command 16 CPUs)


def _lib():
    import lrm_amd
    lrm_amd.load()
    return lrm_amd


SIZES = gpu_sizes(_lib())
# the kernel without a table at its own transitions
NOTAB_SIZES = sorted({t * BLOCK + d for t, k in transitions(_lib()).items() if "notab" in k for d in (0, 1, -RAGGED)})
N_CLOUD = (max(SIZES) + 63) // 64 * 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


def modes(lrm):
    return {"strict": lrm.MODE_STRICT, "fast": lrm.MODE_FAST, "tol": lrm.MODE_TOL, "tol_rel": lrm.MODE_TOL_REL}


def packed(mask):
    n = len(mask)
    return np.packbits(np.pad(mask, (0, (-n) % 64)), bitorder="little").view(np.uint64)


def unit(q):
    q = np.asarray(q, np.float64)
    return tuple(np.float32(q / np.linalg.norm(q)))


def pooled(fn, n, chunk=1 << 20):
    """fn(a, b) over [0, n) in chunks on the oracle's threads (the oracle's C calls drop the GIL)"""
    with ThreadPoolExecutor(POOL) as ex:
        list(ex.map(lambda a: fn(a, min(a + chunk, n)), range(0, n, chunk)))


class Ref:
    """The oracle on a prefix of one cloud, computed once and extended on demand: clouds of every size are prefixes of it,
    so every size, mode and entry point shares it"""

    def __init__(self, oracle, pts, leg, q):
        self.oracle, self.pts, self.leg, self.q = oracle, pts, leg, q
        self.n = 0
        self.m = np.empty(len(pts), np.uint8)
        self.v = np.empty(len(pts), np.uint8)
        self.d = np.empty((len(pts), 3), np.float32)

    def upto(self, n):
        if n > self.n:
            a0 = self.n

            def part(a, b):
                a, b = a + a0, b + a0
                self.m[a:b] = self.oracle.reach(self.pts[a:b], self.leg, self.q)
                self.d[a:b], self.v[a:b] = self.oracle.dist(self.pts[a:b], self.leg, self.q)
            pooled(part, n - a0)
            self.n = n
        return self


class Clouds:
    """The config-2 cloud (tests/conftest.py random_cloud) on the host and the device, and -- per unit-quaternion leg -- the same
    cloud with every eighth point moved onto the reachable set's boundary (p - d_ref, plus 0.01 mm of jitter): those points sit
    in the decision bands, so the doubt queues fill at multi-round grids"""

    def __init__(self, torch, lrm, oracle):
        self.torch, self.lrm, self.oracle = torch, lrm, oracle
        t0 = time.perf_counter()
        self.pts = random_cloud(N_CLOUD, seed=42)
        self.dev = torch.from_numpy(np.ascontiguousarray(self.pts.T)).cuda()  # rows of N_CLOUD (a multiple of 64) stay 16-byte aligned
        self.refs = {}
        rl = next((leg, q) for _, leg, q in random_legs(lrm) if lrm.dbg_tol_ok(leg, q))
        self.legs = [("M2 0.3, unit quaternion", lrm.get_M2_leg(0.3), unit((0.9239, 0.0, 0.0, 0.3827))),
                     ("moonbot -1.1, non-unit quaternion", lrm.get_moonbot_leg(-1.1), (0.98, 0.0, 0.15, 0.05)),
                     ("random leg, unit quaternion", rl[0], tuple(np.float32(rl[1]))),
                     ("M2 -2.0, non-unit quaternion", lrm.get_M2_leg(-2.0), (0.9, 0.1, 0.2, -0.3)),
                     ("moonbot 1.0, unit quaternion", lrm.get_moonbot_leg(1.0), unit((0.96, 0.1, -0.2, 0.15)))]
        print(f"\n{N_CLOUD} cloud points generated in {time.perf_counter() - t0:.1f} s")

    def case(self, i, n):
        """leg, orientation and cloud of the i-th case: the legs in turn; boundary clouds for every other case of a unit quaternion
        (for a non-unit one the oracle's vector is no displacement), only where the cloud's prefix is at most the rounds cap"""
        name, leg, q = self.legs[i % len(self.legs)]
        boundary = is_unit(q) and i % 2 == 0 and n <= self.boundary_n()
        return name + (", boundary cloud" if boundary else ""), leg, q, boundary

    def boundary_n(self):
        return (sorted(transitions(self.lrm))[-1] + 1) * BLOCK + BLOCK

    def get(self, leg_name, leg, q, boundary):
        """(host points, device (3, N) points, Ref) of one cloud"""
        key = (leg_name, boundary)
        if key not in self.refs:
            if not boundary:
                self.refs[key] = (self.pts, self.dev, Ref(self.oracle, self.pts, leg, q))
            else:
                nb = (self.boundary_n() + 63) // 64 * 64
                pts = self.pts[:nb].copy()
                sel = np.arange(0, nb, 8)
                d = np.empty((len(sel), 3), np.float32)

                def part(a, b):
                    d[a:b], _ = self.oracle.dist(pts[sel[a:b]], leg, q)
                pooled(part, len(sel))
                jitter = np.random.default_rng(len(self.refs)).normal(0.0, 0.01, (len(sel), 3)).astype(np.float32)
                pts[sel] = pts[sel] - d + jitter
                dev = self.torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
                self.refs[key] = (pts, dev, Ref(self.oracle, pts, leg, q))
        return self.refs[key]


@pytest.fixture(scope="module")
def clouds(lrm, oracle, torch_cuda):
    return Clouds(torch_cuda, lrm, oracle)


def windows(lrm, n):
    """indices compared in a cloud of n points: all of it up to FULL, else both ends and ROUND_WIN points around every round
    boundary k * stride of the table kernels' grids (LRM_MODE_TOL / LRM_MODE_FAST, LRM_MODE_TOL_REL) and of the kernel without one"""
    if n <= FULL:
        return None
    g = lrm.dbg_tol_grid(n)
    parts = [np.arange(0, END_WIN), np.arange(n - END_WIN, n)]
    for k in ("tab", "rel", "notab"):
        stride = g[k] * BLOCK
        for b in range(stride, n, stride):
            parts.append(np.arange(max(b - ROUND_WIN // 2, 0), min(b + ROUND_WIN // 2, n)))
    return np.unique(np.concatenate(parts))


def check_field(mode, pts, d, dref, leg, what):
    """the field contract of `mode` on matching rows of points, result and oracle"""
    d = np.asarray(d, np.float32)
    if mode in ("strict", "fast"):
        bad = ~bits_equal(d, dref).all(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} vectors differ from the oracle, first at row {int(np.argmax(bad))}"
    elif mode == "tol":
        e = field_error(pts, d, dref, leg)
        assert e["metric"].max(initial=0.0) <= TOL, f"{what}: distance error {e['metric'].max():.3e}"
    else:
        err = np.linalg.norm(d.astype(np.float64) - dref.astype(np.float64), axis=1)
        nref = np.linalg.norm(dref.astype(np.float64), axis=1)
        assert (err <= TOL * nref).all(), f"{what}: relative error {float((err / np.maximum(nref, 1e-300)).max()):.3e}"
        short = nref < SHORT_MM
        assert bits_equal(d[short], dref[short]).all(), f"{what}: a vector shorter than {SHORT_MM} mm is not bit-identical"


class Outputs:
    """device outputs of one size, each followed by guard words: the fused call's mask, bit words and three components, the
    distance-only call's validity bytes and three components"""

    def __init__(self, torch, n):
        self.torch, self.n, self.nw = torch, n, (n + 63) // 64
        f32 = dict(dtype=torch.float32, device="cuda")
        self.mask = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        self.valid = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        self.bits = torch.empty(self.nw + 2, dtype=torch.int64, device="cuda")
        self.d = [torch.empty(n + 16, **f32) for _ in range(3)]   # separately allocated: 16-byte aligned rows
        self.dv = [torch.empty(n + 16, **f32) for _ in range(3)]

    def fill(self):
        """guards everywhere, so that an output the call leaves unwritten shows too"""
        self.mask.fill_(MASK_GUARD)
        self.valid.fill_(MASK_GUARD)
        self.bits.fill_(BITS_GUARD)
        for c in self.d + self.dv:
            c.fill_(FIELD_GUARD)

    def guards_intact(self):
        n, nw = self.n, self.nw
        ok = bool((self.mask[n:] == MASK_GUARD).all()) and bool((self.valid[n:] == MASK_GUARD).all())
        ok &= bool((self.bits[nw:] == BITS_GUARD).all())
        return ok and all(bool((c[n:] == FIELD_GUARD).all()) for c in self.d + self.dv)

    def field(self, comps, idx):
        if idx is None:
            return self.torch.stack([c[:self.n] for c in comps]).cpu().numpy().T
        it = self.torch.from_numpy(idx).cuda()
        return self.torch.stack([c[it] for c in comps]).cpu().numpy().T


def run_device_calls(lrm, torch, x, y, z, n, leg, q, out):
    from lrm_amd import _capi
    legp, qp = np.ascontiguousarray(leg, np.float32), np.ascontiguousarray(q, np.float32)
    st = torch.cuda.current_stream().cuda_stream
    _capi.check(lrm.lib().lrm_reach_dist_bits_dev(x.data_ptr(), y.data_ptr(), z.data_ptr(), n, _capi._ptr(legp), _capi._ptr(qp),
                                                  out.mask.data_ptr(), out.bits.data_ptr(), out.d[0].data_ptr(), out.d[1].data_ptr(),
                                                  out.d[2].data_ptr(), st))
    _capi.check(lrm.lib().lrm_dist_dev(x.data_ptr(), y.data_ptr(), z.data_ptr(), n, _capi._ptr(legp), _capi._ptr(qp),
                                       out.dv[0].data_ptr(), out.dv[1].data_ptr(), out.dv[2].data_ptr(), out.valid.data_ptr(), st))


def run_host_float3(lrm, pts, leg, q):
    """lrm_reach_dist on host float3 arrays (the apply_kernel boundary: the AoS instantiation of the kernels), guards after both outputs"""
    from lrm_amd import _capi
    n = len(pts)
    mask = np.full(n + 64, MASK_GUARD, np.uint8)
    d = np.full((n + 16, 3), FIELD_GUARD, np.float32)
    ms = C.c_float(0)
    legp, qp = np.ascontiguousarray(leg, np.float32), np.ascontiguousarray(q, np.float32)
    _capi.check(lrm.lib().lrm_reach_dist(_capi._ptr(np.ascontiguousarray(pts)), n, _capi._ptr(legp), _capi._ptr(qp), _capi._ptr(mask),
                                         _capi._ptr(d), C.addressof(ms)))
    assert (mask[n:] == MASK_GUARD).all() and (d[n:] == FIELD_GUARD).all(), "lrm_reach_dist wrote past n"
    return mask[:n], d[:n]


def check_case(lrm, torch, clouds, i, n, mode_names, label):
    t0 = time.perf_counter()
    name, leg, q, boundary = clouds.case(i, n)
    pts, dev, ref = clouds.get(name, leg, q, boundary)
    ref.upto(n)
    t_ref = time.perf_counter() - t0
    x, y, z = dev[0, :n], dev[1, :n], dev[2, :n]
    want_m = torch.from_numpy(ref.m[:n]).cuda()
    want_v = torch.from_numpy(ref.v[:n]).cuda()
    want_b = torch.from_numpy(packed(ref.m[:n]).view(np.int64)).cuda()
    idx = windows(lrm, n)
    rows = slice(0, n) if idx is None else idx
    out = Outputs(torch, n)
    all_modes = modes(lrm)
    try:
        for mname in mode_names:
            lrm.set_mode(all_modes[mname])
            out.fill()
            run_device_calls(lrm, torch, x, y, z, n, leg, q, out)
            torch.cuda.synchronize()
            what = f"n = {n}, {mname}, {name}"
            assert out.guards_intact(), f"{what}: a call wrote past n"
            assert torch.equal(out.mask[:n], want_m), f"{what}: reach mask differs from the oracle"
            assert torch.equal(out.bits[:out.nw], want_b), f"{what}: bit words differ from the oracle's mask"
            assert torch.equal(out.valid[:n], want_v), f"{what}: validity bytes differ from the oracle"
            check_field(mname, pts[rows], out.field(out.d, idx), ref.d[rows], leg, what + " (fused)")
            check_field(mname, pts[rows], out.field(out.dv, idx), ref.d[rows], leg, what + " (distance only)")
            if n <= FULL:
                m_h, d_h = run_host_float3(lrm, pts[:n], leg, q)
                assert np.array_equal(m_h, ref.m[:n]), f"{what}: float3 entry, reach mask"
                check_field(mname, pts[:n], d_h, ref.d[:n], leg, what + " (float3)")
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    g = lrm.dbg_tol_grid(n)
    print(f"{label} n = {n} ({name}; grids tab {g['tab']} rel {g['rel']} notab {g['notab']} workgroups; "
          f"{'all' if idx is None else len(idx)} vectors compared): {time.perf_counter() - t0:.2f} s, {t_ref:.2f} s of it the oracle")


@pytest.mark.parametrize("n", SIZES)
def test_every_mode_at_the_grid_transitions(lrm, torch_cuda, clouds, n):
    """every mode, the device SoA fused call with bit words, the device distance-only call with validity bytes and (up to FULL)
    the host float3 call, at n_t, n_t + 1 and n_t - RAGGED of every grid transition, at the dispatch switch to the table kernels
    (2e5 +- 1) and past the rounds cap"""
    check_case(lrm, torch_cuda, clouds, SIZES.index(n), n, ("strict", "fast", "tol", "tol_rel"), "grid transition")


@pytest.mark.parametrize("n", NOTAB_SIZES)
def test_the_kernel_without_a_table_at_its_own_transitions(lrm, torch_cuda, clouds, n, monkeypatch):
    """LRM_TOL_TABLE=0: the tolerance kernel without a plane table (a leg whose table the builder declines runs it at every size)
    and the filtered bit-exact kernel, at the sizes where that grid changes shape"""
    monkeypatch.setenv("LRM_TOL_TABLE", "0")
    check_case(lrm, torch_cuda, clouds, NOTAB_SIZES.index(n) + 1, n, ("fast", "tol", "tol_rel"), "without a table,")


def test_fix_up_redoes_every_segment_of_a_multi_round_grid(lrm, torch_cuda, clouds, monkeypatch):
    """LRM_TOL_SELFTEST=1 queues every point: every segment overflows and the fix-up re-evaluates every workgroup's points over all
    its rounds (index = segment + round * stride).  At a ragged size of three table rounds, five LRM_MODE_TOL_REL rounds and two
    rounds of the kernel without a table, the outputs must equal LRM_MODE_FAST bit for bit."""
    torch = torch_cuda
    t = transitions(lrm)
    steps = sorted(k for k, v in t.items() if "tab" in v)
    n = steps[1] * BLOCK + BLOCK - RAGGED  # past the second round step of the table kernel: three rounds, ragged
    g = lrm.dbg_tol_grid(n)
    assert -(-n // (g["tab"] * BLOCK)) >= 3 and -(-n // (g["rel"] * BLOCK)) >= 3 and -(-n // (g["notab"] * BLOCK)) >= 2
    pts, dev, _ = clouds.get(*clouds.legs[0], False)
    name, leg, q = clouds.legs[0]
    x, y, z = dev[0, :n], dev[1, :n], dev[2, :n]
    t0 = time.perf_counter()
    ref = Outputs(torch, n)
    ref.fill()
    lrm.set_mode(lrm.MODE_FAST)
    monkeypatch.delenv("LRM_TOL_SELFTEST", raising=False)
    run_device_calls(lrm, torch, x, y, z, n, leg, q, ref)
    out = Outputs(torch, n)
    try:
        monkeypatch.setenv("LRM_TOL_SELFTEST", "1")
        for mode, table in ((lrm.MODE_TOL, "1"), (lrm.MODE_TOL_REL, "1"), (lrm.MODE_TOL, "0"), (lrm.MODE_TOL_REL, "0")):
            monkeypatch.setenv("LRM_TOL_TABLE", table)
            lrm.set_mode(mode)
            out.fill()
            run_device_calls(lrm, torch, x, y, z, n, leg, q, out)
            torch.cuda.synchronize()
            npts, nq, nover = lrm.dbg_tol_queue_counts()
            what = f"selftest, mode {mode}, LRM_TOL_TABLE={table}"
            assert npts == n and nover > 0, (what, npts, nq, nover)
            assert out.guards_intact(), what
            assert torch.equal(out.mask, ref.mask) and torch.equal(out.bits, ref.bits) and torch.equal(out.valid, ref.valid), what
            for a, b in zip(out.d + out.dv, ref.d + ref.dv):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    print(f"redo path, n = {n}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n_max", [3_670_017, 7_340_033, 22_020_097])
def test_prepare_then_capture_calls_on_every_smaller_cloud(lrm, torch_cuda, clouds, n_max):
    """lrm_tol_prepare(n_max) on a side stream, then -- in LRM_MODE_TOL, LRM_MODE_TOL_REL and LRM_MODE_FAST -- one graph (a single
    stream) of fused calls on views of one cloud at n_max, n_max - 1 (one workgroup less: a grid of twice the workgroups at the
    table kernel's round steps), both sides of the table dispatch, and 1 point.  Being launch-only, the calls capture, the device's
    free memory does not move, and the replayed outputs match the oracle."""
    torch = torch_cuda
    t0 = time.perf_counter()
    name, leg, q = clouds.legs[0]
    pts, dev, ref = clouds.get(name, leg, q, False)
    sizes = (n_max, n_max - 1, TOLTAB_MIN_POINTS, TOLTAB_MIN_POINTS - 1, 1)
    ref.upto(n_max)
    outs = {n: Outputs(torch, n) for n in sizes}
    lrm.release_workspaces()  # the queues are then exactly what lrm_tol_prepare reserves (streams come from a pool and recur)
    side = torch.cuda.Stream()
    lrm.tol_prepare(leg, q, n_max, side.cuda_stream)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    from lrm_amd import _capi
    legp, qp = np.ascontiguousarray(leg, np.float32), np.ascontiguousarray(q, np.float32)
    try:
        for mname, mode in (("tol", lrm.MODE_TOL), ("tol_rel", lrm.MODE_TOL_REL), ("fast", lrm.MODE_FAST)):
            lrm.set_mode(mode)
            for o in outs.values():
                o.fill()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for n, o in outs.items():
                        _capi.check(lrm.lib().lrm_reach_dist_bits_dev(dev[0, :n].data_ptr(), dev[1, :n].data_ptr(), dev[2, :n].data_ptr(), n,
                                                                      _capi._ptr(legp), _capi._ptr(qp), o.mask.data_ptr(), o.bits.data_ptr(),
                                                                      o.d[0].data_ptr(), o.d[1].data_ptr(), o.d[2].data_ptr(), side.cuda_stream))
                g.replay()
            torch.cuda.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
            assert free1 >= free0 - (8 << 20), f"{mname}: the captured calls allocated {(free0 - free1) >> 20} MiB"
            for n, o in outs.items():
                what = f"n_max = {n_max}, {mname}, n = {n}"
                assert torch.equal(o.mask[:n], torch.from_numpy(ref.m[:n]).cuda()), what
                assert torch.equal(o.bits[:o.nw], torch.from_numpy(packed(ref.m[:n]).view(np.int64)).cuda()), what
                assert bool((o.mask[n:] == MASK_GUARD).all()) and bool((o.bits[o.nw:] == BITS_GUARD).all()), what
                assert all(bool((c[n:] == FIELD_GUARD).all()) for c in o.d), what
                idx = windows(lrm, n)
                rows = slice(0, n) if idx is None else idx
                check_field(mname, pts[rows], o.field(o.d, idx), ref.d[rows], leg, what)
            del g
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    print(f"prepare + capture, n_max = {n_max}: {time.perf_counter() - t0:.2f} s")


def test_32_bit_point_indices(lrm, oracle, torch_cuda):
    """Clouds past 2^31 points: LRM_MODE_FAST and LRM_MODE_TOL run the table kernels with 32-bit indices beyond 2^31 (n = 2^31 +
    4161), LRM_MODE_TOL_REL takes its table kernel at 2^31 - 1 points, the most its flag bit leaves, and falls back to the bit-exact
    kernels at 2^31 + 4161 (its field equals LRM_MODE_FAST's bit for bit).  The oracle on 2^20-point windows at both ends, around
    index 2^31 and around the last round boundary; bit words against the mask bytes over the whole cloud."""
    torch = torch_cuda
    N = (1 << 31) + 4161
    # inputs and field 2 x 3 x 4 N bytes, two masks, bit words, and the doubt queues of the table kernels
    g = lrm.dbg_tol_grid(N)
    need = 24 * N + 2 * N + N // 8 + 4 * g["prepare_words"] * 5 // 4 + (2 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < max(need, 64 << 30):
        pytest.skip(f"needs about {max(need, 64 << 30) / 2**30:.0f} GiB of free device memory, {free / 2**30:.0f} GiB free")
    t0 = time.perf_counter()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2024)
    lo, hi = (-200.0, -500.0, -500.0), (700.0, 500.0, 300.0)
    X = []
    for k in range(3):  # separate allocations: 16-byte aligned rows whatever N
        t = torch.rand(N, device="cuda", generator=gen)
        X.append(t.mul_(hi[k] - lo[k]).add_(lo[k]))
    name, leg, q = "M2 0.3, unit quaternion", lrm.get_M2_leg(0.3), unit((0.9239, 0.0, 0.0, 0.3827))
    W = 1 << 20

    def wins(n):
        """2^20-point windows: both ends, around 2^31 and around the last round boundary of every grid"""
        gg = lrm.dbg_tol_grid(n)
        starts = {0, n - W, (1 << 31) - W // 2}
        for k in ("tab", "rel", "notab"):
            stride = gg[k] * BLOCK
            starts.add(((n - 1) // stride) * stride - W // 2)
        return np.unique(np.concatenate([np.arange(max(a, 0), min(a + W, n)) for a in starts]))

    idx_all = np.unique(np.concatenate([wins(N), wins((1 << 31) - 1)]))
    it_all = torch.from_numpy(idx_all).cuda()
    pts_all = torch.stack([c[it_all] for c in X]).cpu().numpy().T.copy()
    want_m, want_d = np.empty(len(idx_all), np.uint8), np.empty((len(idx_all), 3), np.float32)

    def part(a, b):
        want_m[a:b] = oracle.reach(pts_all[a:b], leg, q)
        want_d[a:b], _ = oracle.dist(pts_all[a:b], leg, q)
    pooled(part, len(idx_all), 1 << 18)

    mask = torch.empty(N, dtype=torch.uint8, device="cuda")
    mask0 = torch.empty(N, dtype=torch.uint8, device="cuda")
    nw = (N + 63) // 64
    bits = torch.empty(nw, dtype=torch.int64, device="cuda")
    F = [torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(3)]
    from lrm_amd import _capi
    legp, qp = np.ascontiguousarray(leg, np.float32), np.ascontiguousarray(q, np.float32)
    st = torch.cuda.current_stream().cuda_stream

    def call(n, m):
        _capi.check(lrm.lib().lrm_reach_dist_bits_dev(X[0].data_ptr(), X[1].data_ptr(), X[2].data_ptr(), n, _capi._ptr(legp), _capi._ptr(qp),
                                                      m.data_ptr(), bits.data_ptr(), F[0].data_ptr(), F[1].data_ptr(), F[2].data_ptr(), st))
        torch.cuda.synchronize()

    def bits_match_mask(n, m):
        """bit (i & 63) of word i >> 6 is mask byte i over the whole cloud, the bits past n zero"""
        shifts = torch.arange(64, device="cuda", dtype=torch.int64)
        words = (n + 63) // 64
        step = 1 << 20
        for a in range(0, words, step):
            b = min(a + step, words)
            unpacked = ((bits[a:b].unsqueeze(1) >> shifts) & 1).to(torch.uint8).flatten()
            lo_i, hi_i = a * 64, min(b * 64, n)
            if not torch.equal(unpacked[:hi_i - lo_i], m[lo_i:hi_i]) or bool(unpacked[hi_i - lo_i:].any()):
                return False
        return True

    def check_windows(n, mname, m):
        idx = wins(n)
        rows = np.searchsorted(idx_all, idx)
        it = torch.from_numpy(idx).cuda()
        got_m = m[it].cpu().numpy()
        assert np.array_equal(got_m, want_m[rows]), f"{mname}, n = {n}: reach mask differs from the oracle"
        got_d = torch.stack([c[it] for c in F]).cpu().numpy().T
        check_field(mname, pts_all[rows], got_d, want_d[rows], leg, f"{mname}, n = {n}")

    try:
        lrm.set_mode(lrm.MODE_FAST)
        call(N, mask0)
        assert bits_match_mask(N, mask0), "LRM_MODE_FAST: bit words"
        check_windows(N, "fast", mask0)
        lrm.set_mode(lrm.MODE_TOL)
        call(N, mask)
        assert torch.equal(mask, mask0) and bits_match_mask(N, mask), "LRM_MODE_TOL: masks"
        check_windows(N, "tol", mask)
        lrm.set_mode(lrm.MODE_TOL_REL)
        n1 = (1 << 31) - 1
        call(n1, mask)
        assert torch.equal(mask[:n1], mask0[:n1]) and bits_match_mask(n1, mask), "LRM_MODE_TOL_REL at 2^31 - 1: masks"
        check_windows(n1, "tol_rel", mask)
        call(N, mask)
        assert torch.equal(mask, mask0) and bits_match_mask(N, mask), "LRM_MODE_TOL_REL at 2^31 + 4161: masks"
        check_windows(N, "fast", mask)  # the bit-exact kernels: bit-identical to the oracle
        # ... and to LRM_MODE_FAST over the whole cloud, which is bit-exact at any size: compared a slice at a time
        lrm.set_mode(lrm.MODE_FAST)
        chunk = 1 << 27
        cm = torch.empty(chunk, dtype=torch.uint8, device="cuda")
        cd = [torch.empty(chunk, dtype=torch.float32, device="cuda") for _ in range(3)]
        for a in range(0, N, chunk):
            n = min(chunk, N - a)
            _capi.check(lrm.lib().lrm_reach_dist_dev(X[0][a:].data_ptr(), X[1][a:].data_ptr(), X[2][a:].data_ptr(), n, _capi._ptr(legp),
                                                     _capi._ptr(qp), cm.data_ptr(), cd[0].data_ptr(), cd[1].data_ptr(), cd[2].data_ptr(), st))
            torch.cuda.synchronize()
            assert torch.equal(cm[:n], mask[a:a + n])
            for c, f in zip(cd, F):
                assert torch.equal(c[:n].view(torch.int32), f[a:a + n].view(torch.int32)), f"LRM_MODE_TOL_REL past 2^31 differs from LRM_MODE_FAST in [{a}, {a + n})"
    finally:
        lrm.set_mode(lrm.MODE_FAST)
        lrm.release_workspaces()
    print(f"32-bit index edge, n = {N}: {time.perf_counter() - t0:.1f} s")
