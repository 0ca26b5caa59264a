"""The device build of csrc/lrm_exact_math.h against its host build on EVERY float (run with -m gpu on an MI355X):
lrm_atanf, and the sine and the cosine of lrm_sincosf, as block checksums over all 2^32 bit patterns (csrc/lrm_dbg_math.h: 65536
sums per function, one launch per function), then the named switch patterns and the atan2f lattice of exact_math_cases through
the array calls.  The host build is held to glibc by tests/test_exact_math_cpu.py; the rule is device == host == glibc.
A differing pattern is a bug in lrm_exact_math.h or in how a file is compiled."""
import ctypes as C
import time

import numpy as np
import pytest

import exact_math_cases as E
from conftest import bits_equal

pytestmark = pytest.mark.gpu

FN_NAMES = ("lrm_atanf", "lrm_sincosf sine", "lrm_sincosf cosine")
P = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def host_sums(lrm):
    """The 3 x 65536 host checksums, computed once for this file (up to 16 threads)."""
    out = np.zeros((3, E.NBLOCKS), np.uint64)
    t0 = time.perf_counter()
    for fn in range(3):
        lrm._capi.check(lrm.lib().lrm_dbg_exact_math_sums_host(fn, 0, E.NBLOCKS, P(out[fn])))
    print(f"host checksums of 3 x 2^32 patterns: {time.perf_counter() - t0:.1f} s")
    out.setflags(write=False)
    return out


def both_builds(lrm, torch, a, b):
    """(atan2f(a, b), sin a, cos a) by the host build and by the device build."""
    a, b = np.array(a, np.float32), np.array(b, np.float32)  # writable copies: the cases are handed out read-only
    host = [np.empty_like(a) for _ in range(3)]
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_host(P(a), P(b), len(a), *[P(o) for o in host]))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dev = [torch.empty_like(ta) for _ in range(3)]
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_dev(ta.data_ptr(), tb.data_ptr(), len(a), *[o.data_ptr() for o in dev],
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return host, [d.cpu().numpy() for d in dev]


def assert_same(a, b, host, dev, what):
    for name, h, d in zip(("atan2f", "sin", "cos"), host, dev):
        bad = np.flatnonzero(~bits_equal(h, d))
        if len(bad):
            i = int(bad[0])
            pytest.fail(f"{what}: {name} differs on {len(bad)} of {len(h)}, first a = 0x{E.bits(a)[i]:08x} b = 0x{E.bits(b)[i]:08x}: "
                        f"device 0x{E.bits(d)[i]:08x}, host 0x{E.bits(h)[i]:08x}")


@pytest.mark.parametrize("fn", [0, 1, 2])
def test_device_equals_host_on_every_float(lrm, torch_cuda, host_sums, fn):
    """All 65536 block sums of one function, one launch: every one of the 2^32 results enters its block's sum with an odd weight."""
    torch = torch_cuda
    sums = torch.full((E.NBLOCKS,), -1, dtype=torch.int64, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_sums_dev(fn, 0, E.NBLOCKS, sums.data_ptr(), torch.cuda.current_stream().cuda_stream))
    stop.record()
    torch.cuda.synchronize()
    print(f"device checksums of {FN_NAMES[fn]} over 2^32 patterns: {start.elapsed_time(stop):.1f} ms")
    got = sums.cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != host_sums[fn])
    if len(bad) == 0:
        return
    # the first differing block, pattern by pattern through the array calls (atan2f(x, 1) is atanf(x))
    block = int(bad[0])
    x = E.block_patterns(block)
    host, dev = both_builds(lrm, torch, x, np.ones_like(x))
    h, d = host[fn], dev[fn]
    diff = np.flatnonzero(~bits_equal(h, d))
    where = (f"first pattern 0x{E.bits(x)[diff[0]]:08x}: device 0x{E.bits(d)[diff[0]]:08x}, host 0x{E.bits(h)[diff[0]]:08x}"
             if len(diff) else "the array calls agree on that block: the checksum kernel itself is suspect")
    pytest.fail(f"{FN_NAMES[fn]}: {len(bad)} of 65536 block sums differ, first block 0x{block:04x}; {where}")


def test_named_patterns_device_equals_host(lrm, torch_cuda):
    """Every range, threshold and quadrant switch with its +-8-ulp neighbours and the specials: as a with b = 1, and as b with a
    from a short list.  No |a| < 100 filter: values >= 120, inf and nan give nan on both sides."""
    p = E.named_patterns()
    host, dev = both_builds(lrm, torch_cuda, p, np.ones_like(p))
    assert_same(p, np.ones_like(p), host, dev, "pattern as a")
    out_of_range = ~(np.abs(p) < 120)
    assert out_of_range.sum() >= 2 * 9 + 3
    for k in (1, 2):
        assert np.isnan(host[k][out_of_range]).all() and np.isnan(dev[k][out_of_range]).all()
        assert not np.isnan(host[k][~out_of_range]).any() and not np.isnan(dev[k][~out_of_range]).any()
    short = np.array([1.0, -1.0, 0.0, -0.0, 0.4375, -2.4375, 3.0e-39, 1.0e-30, -1.0e30, np.inf, -np.inf, np.nan], np.float32)
    a, b = np.repeat(short, len(p)), np.tile(p, len(short))
    host, dev = both_builds(lrm, torch_cuda, a, b)
    assert_same(a, b, host, dev, "pattern as b")


def test_atan2_lattice_device_equals_host(lrm, torch_cuda):
    """All pairs of ~1000 values over the exponent range, around the k = +-60 / +-61 cuts and through the zero / inf / nan table;
    and the pairs whose quotient sits on and beside each of lrm_atanf's six switches."""
    y, x = E.atan2_pool()
    host, dev = both_builds(lrm, torch_cuda, y, x)
    assert_same(y, x, host, dev, "atan2 pool")
    y, x, _ = E.atan2_on_threshold()
    host, dev = both_builds(lrm, torch_cuda, y, x)
    assert_same(y, x, host, dev, "atan2 on threshold")


@pytest.mark.parametrize("first,n", [(0, 1), (65535, 1), (1, 3), (0, 0)])
def test_sums_kernel_launch_shapes_leave_their_sentinels(lrm, torch_cuda, first, n):
    """Only the asked sums are written, and each equals the host's sum of its block."""
    torch = torch_cuda
    sentinel = -0x0123456789ABCDEF
    for fn in range(3):
        want = np.zeros(n, np.uint64)
        lrm._capi.check(lrm.lib().lrm_dbg_exact_math_sums_host(fn, first, n, P(want)))
        buf = torch.full((n + 8,), sentinel, dtype=torch.int64, device="cuda")
        lrm._capi.check(lrm.lib().lrm_dbg_exact_math_sums_dev(fn, first, n, buf[4:].data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:4] == sentinel).all() and (got[4 + n:] == sentinel).all()
        assert np.array_equal(got[4:4 + n].view(np.uint64), want)
