"""The one-query-per-lane kernels across wave, block and grid-stride boundaries on the MI355X (run with -m gpu):
posed_kernel<reach, dist> (lrm_posed.hip), ik_kernel / fk_kernel (lrm_ik.hip), ik_posed_kernel / fk_posed_kernel
(lrm_ik_posed.hip).  Sizes are built around each kernel's own pass size S (query_cases.pass_sizes(), pinned by
tests/test_query_cases_cpu.py): past S a wave makes a second trip, and the per-wave table cache (`staged`) of
posed_kernel and ik_posed_kernel meets a sequence of records.  The index patterns of query_cases build those sequences
on purpose; every output of every query is compared bit for bit with the reference of its unique (pose, leg, pool
member) combination: the oracle for posed_kernel, the posed CPU calls for the IK and FK.  All outputs are prefilled with
sentinels (7.0, 9) and carry guard elements past n.

The kernels clamp every index before any load, so the out-of-range tests provoke no fault: they check that the clamp's
documented outputs appear, and that the lanes next to a clamped one keep their own record's answer."""
import numpy as np
import pytest

import query_cases as qc
from conftest import bits_equal

pytestmark = pytest.mark.gpu

GUARD = 5
NAN = np.float32(np.nan)
SMALL = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513]
SIZES = {"S-1": lambda S: S - 1, "S+1": lambda S: S + 1, "S+65": lambda S: S + 65, "2S+63": lambda S: 2 * S + 63,
         "3S+63": lambda S: 3 * S + 63}
# 3S+63 with echo: the only size here with many waves in a third trip (uniform on A, mixed, uniform on A again)
BOUNDARY = [(p, s) for p in ("runs", "echo", "interleaved") for s in ("S-1", "S+1", "S+65", "2S+63")] + [("shuffled", "2S+63")]
CACHED = BOUNDARY + [("echo", "3S+63")]
S_OF = qc.pass_sizes()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cs(lrm, oracle):
    return qc.cases(lrm, oracle)


@pytest.fixture(scope="module")
def ps(lrm, torch_cuda, cs):
    """workspaces sized exactly (nposes, nlegs): an unclamped index would leave them"""
    p = lrm.PoseSet(cs.legs, cs.P, ik=True).update(dev(torch_cuda, cs.quats), dev(torch_cuda, cs.body))
    assert p.workspace.numel() == cs.P * cs.L * 512 and p.ik_workspace.numel() == cs.P * cs.L * 128
    return p


def dev(torch, a, view=False):
    """a on the device; view: one element into a wider buffer (1-D), so only the element size aligns it"""
    a = np.ascontiguousarray(a)
    if not view:
        return torch.from_numpy(a).cuda()
    big = torch.zeros(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    big[1:] = torch.from_numpy(a).cuda()
    return big[1:]


def soa(torch, a, view=False):
    a = np.asarray(a, np.float32)
    if not view:
        t = dev(torch, a.T)
        return t[0], t[1], t[2]
    big = torch.zeros((3, len(a) + 1), dtype=torch.float32, device="cuda")
    big[:, 1:] = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    return big[0, 1:], big[1, 1:], big[2, 1:]


class Out:
    """sentinel-filled outputs with GUARD elements past n; view: offset views of wider buffers (3 floats / 1 byte in)"""

    def __init__(self, torch, n, view=False):
        self.n, self.off = n, (3, 1) if view else (0, 0)
        self.f_all = torch.full((3, n + GUARD + self.off[0]), 7.0, dtype=torch.float32, device="cuda")
        self.b_all = [torch.full((n + GUARD + self.off[1],), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.f = self.f_all[:, self.off[0]:]
        self.b = [b[self.off[1]:] for b in self.b_all]

    def floats(self, written=True):
        """the (n, 3) result; asserts the guards (and, when nothing was to be written, the whole buffer)"""
        a = self.f_all.cpu().numpy()
        lo = self.off[0]
        assert (a[:, :lo] == 7.0).all() and (a[:, lo + self.n:] == 7.0).all(), "float guard overwritten"
        assert written or (a == 7.0).all(), "a float buffer that was not passed was written"
        return np.ascontiguousarray(a[:, lo:lo + self.n].T)

    def bytes(self, k=0, written=True):
        a = self.b_all[k].cpu().numpy()
        lo = self.off[1]
        assert (a[:lo] == 9).all() and (a[lo + self.n:] == 9).all(), "byte guard overwritten"
        assert written or (a == 9).all(), "a byte buffer that was not passed was written"
        return a[lo:lo + self.n]


def same(got, want, what):
    ok = bits_equal(got, want) if want.dtype == np.float32 else got == want
    if not ok.all():
        bad = np.flatnonzero(~ok.reshape(len(want), -1).all(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} queries differ, first {bad[:8]}: got {got[bad[0]]} want {want[bad[0]]}")


def queries(cs, name, n, S, oob=False):
    """the index pattern, its out-of-range plants (or None), src into the unique combinations (-1: pose / leg out of
    range) and take, the pool entry whose target, seed and angles the query carries"""
    pose, leg = qc.pattern(name, n, cs.P, cs.L, S)
    o = qc.with_oob(pose, leg, S, cs.P, cs.L, cs.nu) if oob else None
    if o is not None:
        pose, leg = o.pose, o.leg
    k, src = qc.expand(pose, leg, cs.L, None if o is None else o.oob_pl)
    return pose, leg, o, src, np.where(src < 0, k, src)


def idx(torch, pose, leg, view=False, nulls=()):
    return (None if "pose" in nulls else dev(torch, pose, view)), (None if "leg" in nulls else dev(torch, leg, view))


def check_posed(torch, cs, ps, pose, leg, src, take, view=False, check=True, nulls=()):
    n = len(src)
    x, y, z = soa(torch, cs.xyz[take], view)
    pi, li = idx(torch, pose, leg, view, nulls)
    out = Out(torch, n, view)
    ps.reach_dist(x, y, z, pi, li, mask=out.b[0], out=out.f, valid=out.b[1], check=check)
    torch.cuda.synchronize()
    same(out.bytes(0), qc.gather(cs.mask, src, 0), "mask")
    same(out.bytes(1), qc.gather(cs.valid, src, 0), "valid")
    same(out.floats(), qc.gather(cs.field, src, NAN), "field")


def check_ik_posed(torch, cs, ps, pose, leg, src, take, o=None, view=False, check=True, nulls=(), forms=("indexed", "plain")):
    """indexed: targets through target_idx into the pool, with seeds; plain: the expanded targets, no seeds"""
    n = len(src)
    pi, li = idx(torch, pose, leg, view, nulls)
    for form in forms:
        out = Out(torch, n, view)
        if form == "indexed":
            ti, t_bad = take.astype(np.int32), np.zeros(n, bool)
            if o is not None:
                ti[o.t_at], t_bad[o.t_at] = o.t_val, True
            x, y, z = soa(torch, cs.xyz, view)
            ps.ik(x, y, z, pi, li, target_idx=dev(torch, ti, view), seed=soa(torch, cs.seed[take], view), out=out.f,
                  status=out.b[0], check=check)
            want_a, want_s = qc.gather(cs.iks_a, src, NAN, t_bad), qc.gather(cs.iks_s, src, 0, t_bad)
        else:
            x, y, z = soa(torch, cs.xyz[take], view)
            ps.ik(x, y, z, pi, li, out=out.f, status=out.b[0], check=check)
            want_a, want_s = qc.gather(cs.ik_a, src, NAN), qc.gather(cs.ik_s, src, 0)
        torch.cuda.synchronize()
        same(out.bytes(0), want_s, f"status ({form})")
        same(out.floats(), want_a, f"angles ({form})")
        out.bytes(1, written=False)


def check_fk_posed(torch, cs, ps, pose, leg, src, take, view=False, check=True, nulls=(), inputs=("ik", "raw")):
    """ik: the reference IK's angles (nan where it gave none); raw: the pool's angle grid; finite: raw made finite, so
    that a nan tip can only be the out-of-range rule"""
    n = len(src)
    pi, li = idx(torch, pose, leg, view, nulls)
    for inp in inputs:
        ang, want = {"ik": (cs.ik_a, cs.fk_ik), "raw": (cs.ang, cs.fk_raw), "finite": (cs.ang_finite, cs.fk_finite)}[inp]
        out = Out(torch, n, view)
        ps.fk(*soa(torch, ang[take], view), pi, li, out=out.f, check=check)
        torch.cuda.synchronize()
        same(out.floats(), qc.gather(want, src, NAN), f"tip ({inp})")


def check_ik_one(lrm, torch, cs, n, seeded):
    o, k = cs.one, qc.pick(n)
    out = Out(torch, n)
    lrm.device.ik(*soa(torch, o.xyz[k]), o.leg, o.quat, seed=soa(torch, o.seed[k]) if seeded else None, out=out.f, status=out.b[0])
    torch.cuda.synchronize()
    same(out.bytes(0), (o.iks_s if seeded else o.ik_s)[k], "status")
    same(out.floats(), (o.iks_a if seeded else o.ik_a)[k], "angles")


def check_fk_one(lrm, torch, cs, n, inp):
    o, k = cs.one, qc.pick(n)
    ang, want = {"ik": (o.ik_a, o.fk_ik), "raw": (o.ang, o.fk_raw)}[inp]
    out = Out(torch, n)
    lrm.device.fk(*soa(torch, ang[k]), o.leg, o.quat, out=out.f)
    torch.cuda.synchronize()
    same(out.floats(), want[k], "tip")


# ---- small sizes: one wave, two, a block, two blocks, and the partial last wave of each ---------------------------
@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_posed_kernel(torch_cuda, cs, ps, n):
    for name in ("runs", "shuffled"):
        pose, leg, _, src, take = queries(cs, name, n, S_OF["posed_kernel"])
        check_posed(torch_cuda, cs, ps, pose, leg, src, take)


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_ik_posed_kernel(torch_cuda, cs, ps, n):
    for name in ("runs", "shuffled"):
        pose, leg, _, src, take = queries(cs, name, n, S_OF["ik_posed_kernel"])
        check_ik_posed(torch_cuda, cs, ps, pose, leg, src, take)


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_fk_posed_kernel(torch_cuda, cs, ps, n):
    for name in ("runs", "shuffled"):
        pose, leg, _, src, take = queries(cs, name, n, S_OF["fk_posed_kernel"])
        check_fk_posed(torch_cuda, cs, ps, pose, leg, src, take)


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_ik_kernel(lrm, torch_cuda, cs, n):
    for seeded in (False, True):
        check_ik_one(lrm, torch_cuda, cs, n, seeded)


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_fk_kernel(lrm, torch_cuda, cs, n):
    for inp in ("ik", "raw"):
        check_fk_one(lrm, torch_cuda, cs, n, inp)


# ---- pass boundaries: the grid-stride loop's second (and third) trip -------------------------------------------------
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("size", ["S-1", "S+1", "S+65", "2S+63"])
def test_pass_boundaries_ik_kernel(lrm, torch_cuda, cs, size, seeded):
    check_ik_one(lrm, torch_cuda, cs, SIZES[size](S_OF["ik_kernel"]), seeded)


@pytest.mark.parametrize("inp", ["ik", "raw"])
@pytest.mark.parametrize("size", ["S-1", "S+1", "S+65", "2S+63"])
def test_pass_boundaries_fk_kernel(lrm, torch_cuda, cs, size, inp):
    check_fk_one(lrm, torch_cuda, cs, SIZES[size](S_OF["fk_kernel"]), inp)


@pytest.mark.parametrize("name,size", CACHED)
def test_pass_boundaries_posed_kernel(torch_cuda, cs, ps, name, size):
    S = S_OF["posed_kernel"]
    pose, leg, _, src, take = queries(cs, name, SIZES[size](S), S)
    check_posed(torch_cuda, cs, ps, pose, leg, src, take)


@pytest.mark.parametrize("name,size", CACHED)
def test_pass_boundaries_ik_posed_kernel(torch_cuda, cs, ps, name, size):
    S = S_OF["ik_posed_kernel"]
    pose, leg, _, src, take = queries(cs, name, SIZES[size](S), S)
    check_ik_posed(torch_cuda, cs, ps, pose, leg, src, take)


@pytest.mark.parametrize("name,size", BOUNDARY)
def test_pass_boundaries_fk_posed_kernel(torch_cuda, cs, ps, name, size):
    S = S_OF["fk_posed_kernel"]
    pose, leg, _, src, take = queries(cs, name, SIZES[size](S), S)
    check_fk_posed(torch_cuda, cs, ps, pose, leg, src, take)


# ---- out-of-range indices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["runs", "echo"])
@pytest.mark.parametrize("kernel", ["posed_kernel", "ik_posed_kernel", "fk_posed_kernel"])
def test_out_of_range_indices(torch_cuda, cs, ps, kernel, name):
    """the six placements of query_cases.with_oob at n = S + 65, check=False: mask 0, valid 0 and a nan field; status 0
    and nan angles; a nan tip; every other query, the lanes next to them included, has its own record's answer"""
    torch, S = torch_cuda, S_OF[kernel]
    pose, leg, o, src, take = queries(cs, name, S + 65, S, oob=True)
    assert (src[o.oob_pl] == -1).all() and (src[~o.oob_pl] >= 0).all()
    if kernel == "posed_kernel":
        with pytest.raises(ValueError):
            ps.reach_dist(*soa(torch, cs.xyz[take[:1000]]), dev(torch, np.full(1000, -1, np.int32)), dev(torch, leg[:1000]))
        check_posed(torch, cs, ps, pose, leg, src, take, check=False)
        want = qc.gather(cs.field, src, NAN)
        assert np.isnan(want[o.oob_pl]).all() and np.isfinite(want[~o.oob_pl]).any(1).mean() > 0.9
    elif kernel == "ik_posed_kernel":
        check_ik_posed(torch, cs, ps, pose, leg, src, take, o=o, check=False)
        bad = o.oob_pl | o.oob_t
        want = qc.gather(cs.iks_s, src, 0, o.oob_t)
        assert (want[bad] == 0).all() and (want[~bad] != 0).mean() > 0.9
    else:
        check_fk_posed(torch, cs, ps, pose, leg, src, take, check=False, inputs=("finite",))
        want = qc.gather(cs.fk_finite, src, NAN)
        assert np.isnan(want[o.oob_pl]).all() and np.isfinite(want[~o.oob_pl]).all()


# ---- the instantiations and NULL forms of lrm_reach_dist_posed_dev, through the C ABI -------------------------------------
@pytest.mark.parametrize("form", ["valid_field", "valid", "field", "mask", "mask_valid"])
def test_null_forms_of_the_posed_call(lrm, torch_cuda, cs, ps, form):
    """posed_kernel<false, true> (no mask), <true, false> (mask only) and <true, true> without a field; the buffers not
    passed keep their sentinel"""
    torch, S = torch_cuda, S_OF["posed_kernel"]
    pose, leg, _, src, take = queries(cs, "runs", S + 65, S)
    n = len(src)
    x, y, z = soa(torch, cs.xyz[take])
    pi, li = idx(torch, pose, leg)
    out = Out(torch, n)
    give = {"valid_field": (0, 1, 1), "valid": (0, 1, 0), "field": (0, 0, 1), "mask": (1, 0, 0), "mask_valid": (1, 1, 0)}[form]
    dp = lambda t, on: t.data_ptr() if on else None
    rc = lrm.load().lrm_reach_dist_posed_dev(x.data_ptr(), y.data_ptr(), z.data_ptr(), n, pi.data_ptr(), li.data_ptr(),
                                             ps.workspace.data_ptr(), cs.P, cs.L, dp(out.b[0], give[0]), dp(out.b[1], give[1]),
                                             dp(out.f[0], give[2]), dp(out.f[1], give[2]), dp(out.f[2], give[2]),
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    m, v, f = out.bytes(0, give[0]), out.bytes(1, give[1]), out.floats(give[2])
    if give[0]:
        same(m, qc.gather(cs.mask, src, 0), "mask")
    if give[1]:
        same(v, qc.gather(cs.valid, src, 0), "valid")
    if give[2]:
        same(f, qc.gather(cs.field, src, NAN), "field")


# ---- one index array NULL -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [("pose",), ("leg",), ("pose", "leg")])
@pytest.mark.parametrize("kernel", ["posed_kernel", "ik_posed_kernel", "fk_posed_kernel"])
def test_null_index_arrays(torch_cuda, cs, ps, kernel, nulls):
    """pose_idx NULL: pose 0 with a varying leg; leg_idx NULL: leg 0 with a varying pose; both: record (0, 0)"""
    S = S_OF[kernel]
    pose, leg = qc.pattern("single" if len(nulls) == 2 else "runs", S + 1, cs.P, cs.L, S)
    pose = np.zeros_like(pose) if "pose" in nulls else pose
    leg = np.zeros_like(leg) if "leg" in nulls else leg
    assert len(nulls) == 2 or len(np.unique(pose.astype(np.int64) * cs.L + leg)) >= min(cs.P, cs.L)
    k, src = qc.expand(pose, leg, cs.L)
    check = {"posed_kernel": check_posed, "ik_posed_kernel": check_ik_posed, "fk_posed_kernel": check_fk_posed}[kernel]
    check(torch_cuda, cs, ps, pose, leg, src, src, nulls=nulls)


# ---- views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["posed_kernel", "ik_posed_kernel", "fk_posed_kernel"])
def test_views_one_element_into_wider_buffers(torch_cuda, cs, ps, kernel):
    S = S_OF[kernel]
    pose, leg, _, src, take = queries(cs, "runs", S + 65, S)
    check = {"posed_kernel": check_posed, "ik_posed_kernel": check_ik_posed, "fk_posed_kernel": check_fk_posed}[kernel]
    check(torch_cuda, cs, ps, pose, leg, src, take, view=True)
