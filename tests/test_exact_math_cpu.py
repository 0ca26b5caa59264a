"""csrc/lrm_exact_math.h on the CPU: the block checksums of lrm_dbg_exact_math_sums_host (csrc/lrm_dbg_math.h) against numpy,
and the host build against this machine's glibc on EVERY float, by tools/check_exact_math.cpp run from here:
  sincosf   every |x| < 120 (2 246 049 792 values, both results)
  atanf     the 2^31 non-negative patterns and every 257th negative one (lrm_atan2f only ever passes fabsf(y / x))
  atan2f    the lattice of exact_math_cases (all pairs of ~1000 values, pairs whose quotient sits on lrm_atanf's switches)
            and 1e8 pairs of the tool's random mode
The device build is held to the host build by tests/test_gpu_exact_math.py; together: device == host == glibc.
A mismatch here on a machine whose glibc differs from the one the header restates is a finding about that libm: report the
patterns the tool prints, do not loosen the test.  Measured: see DESIGN.md (the oracle and what parity means)."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import exact_math_cases as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
P = lambda a: a.ctypes.data_as(C.c_void_p)


def host_sums(lrm, fn, first_block, nblocks, out=None):
    out = np.zeros(nblocks, np.uint64) if out is None else out
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_sums_host(fn, first_block, nblocks, P(out)))
    return out


def array_results(lrm, x):
    """(atanf, sin, cos) of x through the array call: atan2f(x, 1) is atanf(x), in glibc and in lrm_atan2f."""
    outs = [np.empty_like(x) for _ in range(3)]
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_host(P(x), P(np.ones_like(x)), len(x), *[P(o) for o in outs]))
    return outs


def test_sums_entry_points_are_declared_and_exported(lrm):
    names = {"lrm_dbg_exact_math_sums_host", "lrm_dbg_exact_math_sums_dev"}
    assert names <= set(lrm.declared_symbols()) and names <= set(lrm.exported_symbols())


@pytest.fixture(scope="module")
def block_results(lrm):
    """The three functions on the eight blocks of E.SUM_BLOCKS, by the array call: [fn] -> (8, 65536) float32."""
    x = np.concatenate([E.block_patterns(b) for b in E.SUM_BLOCKS])
    res = [r.reshape(len(E.SUM_BLOCKS), E.BLOCK) for r in array_results(lrm, x)]
    for r in res:
        r.setflags(write=False)
    return res


@pytest.mark.parametrize("fn", [0, 1, 2])
def test_host_sums_match_numpy_on_eight_blocks(lrm, block_results, fn):
    """Block 0, a block of denormals, the blocks of 1.0 and 120.0, the last finite block, two negative blocks, the nan block."""
    x = E.block_patterns(0x3F80)
    assert x[0] == 1.0 and E.block_patterns(0x42F0)[0] == 120.0 and np.isnan(E.block_patterns(0x7FC0)).all()
    assert (E.block_patterns(0x0040) < np.finfo(np.float32).tiny).all() and (E.block_patterns(0xBF80) < 0).all()
    for k, b in enumerate(E.SUM_BLOCKS):
        got = int(host_sums(lrm, fn, b, 1)[0])
        assert got == E.sums_np(block_results[fn], k), f"fn {fn} block 0x{b:04x}"
    # sine and cosine of the nan block and of the 120.0 block are all nan: the canonical pattern times the sum of the weights
    if fn > 0:
        assert int(host_sums(lrm, fn, 0x42F0, 1)[0]) == (E.NAN_BITS * E.BLOCK * E.BLOCK) % 2**64


def test_checksum_sees_one_flipped_bit_and_one_swap(block_results):
    """What the checksum is there to see: one wrong result in a block (any single bit), or two results that changed places."""
    rng = np.random.default_rng(5)
    for fn in range(3):
        base = np.array(block_results[fn][2:3])  # the block of 1.0: finite, distinct results
        want = E.sums_np(base, 0)
        for bit in range(32):
            j = int(rng.integers(0, E.BLOCK))
            r = base.copy()
            r.view(np.uint32)[0, j] ^= np.uint32(1 << bit)
            if np.isnan(r[0, j]) and np.isnan(base[0, j]):
                continue  # nan payloads are not told apart, by design
            assert E.sums_np(r, 0) != want, (fn, bit, j)
        for _ in range(64):
            i, j = (int(v) for v in rng.integers(0, E.BLOCK, 2))
            if base.view(np.uint32)[0, i] == base.view(np.uint32)[0, j]:
                continue
            r = base.copy()
            r[0, [i, j]] = r[0, [j, i]]
            assert E.sums_np(r, 0) != want, (fn, i, j)


def test_host_sums_launch_shapes_threads_and_bad_arguments(lrm, monkeypatch):
    """(first_block, nblocks) = (0, 1), (65535, 1), (1, 3), (0, 0) into sentinel-filled outputs: only the asked sums are
    written, and they do not depend on the thread count."""
    sentinel = np.uint64(0xDEADBEEFDEADBEEF)
    ref = {}
    monkeypatch.setenv("LRM_DBG_MATH_THREADS", "1")
    for b in (0, 1, 2, 3, 65535):
        ref[b] = int(host_sums(lrm, 2, b, 1)[0])
    monkeypatch.setenv("LRM_DBG_MATH_THREADS", "3")
    for first, n in ((0, 1), (65535, 1), (1, 3), (0, 0)):
        out = np.full(n + 4, sentinel, np.uint64)
        host_sums(lrm, 2, first, n, out[2:])
        assert [int(v) for v in out[2:2 + n]] == [ref[first + k] for k in range(n)]
        assert (out[:2] == sentinel).all() and (out[2 + n:] == sentinel).all()
    L = lrm.lib()
    out = np.zeros(4, np.uint64)
    assert L.lrm_dbg_exact_math_sums_host(3, 0, 1, P(out)) == -1 and L.lrm_last_error()
    assert L.lrm_dbg_exact_math_sums_host(-1, 0, 1, P(out)) == -1
    assert L.lrm_dbg_exact_math_sums_host(0, 65535, 2, P(out)) == -1
    assert L.lrm_dbg_exact_math_sums_host(0, 65536, 1, P(out)) == -1
    assert L.lrm_dbg_exact_math_sums_host(0, 0, 1, None) == -1
    assert L.lrm_dbg_exact_math_sums_dev(3, 0, 1, P(out), None) == -1
    assert L.lrm_dbg_exact_math_sums_dev(0, 65535, 2, P(out), None) == -1
    assert L.lrm_dbg_exact_math_sums_dev(0, 0, 0, None, None) == 0  # nothing asked, nothing launched
    assert (out == 0).all()


def test_named_patterns_and_lattice_hold_what_they_promise():
    named = E.bits(E.named_patterns())
    for c in E.ATAN_THRESHOLDS + E.SINCOS_THRESHOLDS + tuple(int(q) for q in E.quadrant_patterns()):
        for d in (-8, -1, 0, 1, 8):
            assert c + d in named and ((c + d) | 0x80000000) in named
    assert set(E.bits(E.specials()).tolist()) <= set(named.tolist()) and len(E.specials()) == 13
    # between a quadrant pattern's neighbours the quadrant index of lrm_sincosf steps
    q = E.quadrant_patterns().astype(np.int64)
    n_of = lambda u: ((E.floats(u.astype(np.uint32)).astype(np.float64) * (2.0**24 * 2 / np.pi)).astype(np.int64) + 0x800000) >> 24
    assert (n_of(q + 8) - n_of(q - 8) == 1).all()
    v = E.atan2_values()
    assert 900 <= len(v) <= 1100 and len(np.unique(E.bits(v))) == len(v)
    y, x = E.atan2_pool()
    assert len(y) == len(v) ** 2
    # the exponent-gap cuts: k = (iy - ix) >> 23 takes every value from -62 to 62 around +-60 / +-61 among finite non-zero pairs
    iy, ix = (E.bits(a).astype(np.int64) & 0x7FFFFFFF for a in (y, x))
    ok = (iy > 0) & (ix > 0) & (iy < 0x7F800000) & (ix < 0x7F800000)
    ks = set(np.unique((iy[ok] - ix[ok]) >> 23).tolist())
    assert set(range(-63, -57)) | set(range(58, 64)) <= ks


def test_threshold_pairs_populate_both_sides_of_every_atanf_switch():
    y, x, t = E.atan2_on_threshold()
    assert len(y) == 6 * E.THRESHOLD_COORDS * 5 * 4
    for tau, (at, below) in zip(E.ATAN_THRESHOLDS, E.threshold_hits(y, x, t)):
        assert at >= 256 and below >= 256, (hex(tau), at, below)


# ---- the host build against glibc, exhaustively ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", CSRC, "check-exact-math"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "build", "check_exact_math")


def run_tool(tool, mode, *args):
    t0 = time.perf_counter()
    p = subprocess.run([tool, mode, *args], capture_output=True, text=True, timeout=1200)
    dt = time.perf_counter() - t0
    print(f"check_exact_math {mode} {' '.join(args)}: {dt:.1f} s\n{p.stdout}")
    return p, p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""


@pytest.mark.parametrize("mode,args,values", [
    ("sincos", (), 2 * 0x42F00000),                       # every |x| < 120: 2 246 049 792
    ("atanpos", (), 2**31 + (2**31 + 256) // 257),        # every non-negative pattern, every 257th negative one
    ("atan2", ("100000000",), 100_000_000),               # the random mode, cut to 1e8 pairs
])
def test_host_build_matches_glibc_on_every_float(tool, mode, args, values):
    p, last = run_tool(tool, mode, *args)
    assert last == f"{mode}: {values} values, 0 mismatches", p.stdout + p.stderr
    assert p.returncode == 0


def test_host_build_matches_glibc_on_the_atan2_lattice(tool, tmp_path):
    y, x = E.atan2_pool()
    ty, tx, _ = E.atan2_on_threshold()
    pairs = np.stack([np.concatenate([y, ty]), np.concatenate([x, tx])], axis=1).astype(np.float32)
    path = tmp_path / "pairs.bin"
    pairs.tofile(path)
    p, last = run_tool(tool, "pairs", str(path))
    assert last == f"pairs: {len(pairs)} values, 0 mismatches", p.stdout + p.stderr
    assert p.returncode == 0


def test_tool_reports_a_mismatch_count_and_takes_a_thread_count(tool, tmp_path):
    """The same pairs with 1 and with 3 threads: the same line; a malformed file or argument is refused."""
    ty, tx, _ = E.atan2_on_threshold()
    path = tmp_path / "pairs.bin"
    np.stack([ty, tx], axis=1).astype(np.float32).tofile(path)
    lines = {run_tool(tool, "pairs", str(path), n)[1] for n in ("1", "3")}
    assert lines == {f"pairs: {len(ty)} values, 0 mismatches"}
    (tmp_path / "odd.bin").write_bytes(b"\0" * 12)
    assert subprocess.run([tool, "pairs", str(tmp_path / "odd.bin")], capture_output=True).returncode == 2
    assert subprocess.run([tool, "pairs", str(path), "0"], capture_output=True).returncode == 2
    assert subprocess.run([tool, "nothing"], capture_output=True).returncode == 2
