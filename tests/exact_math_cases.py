"""Shared cases of the exact-math tests (test_exact_math_cpu.py, test_gpu_exact_math.py): the block checksum of
csrc/lrm_dbg_math.h restated in numpy, the single bit patterns at which csrc/lrm_exact_math.h switches from one
range, quadrant or table entry to the next, and a lattice of atan2f pairs built around them.  Everything here is
made once per process and handed out read-only."""
import functools

import numpy as np

from conftest import random_cloud

BLOCK = 65536            # patterns per checksum block: block b holds u = b * 65536 + j
NBLOCKS = 65536
NAN_BITS = 0x7FC00000    # what every nan counts as in a checksum

# lrm_atanf's range switches (ix = |x|'s bits): 2^-29, 0.4375, 0.6875, 1.1875, 2.4375, 2^25
ATAN_THRESHOLDS = (0x31000000, 0x3EE00000, 0x3F300000, 0x3F980000, 0x401C0000, 0x4C000000)
# lrm_sincosf's three `top` thresholds, their first patterns: 2^-12, 0.75, 120.0
SINCOS_THRESHOLDS = (0x39800000, 0x3F400000, 0x42F00000)
# lrm_atan2f's exponent-gap cuts: k = (iy - ix) >> 23 beyond +-60
ATAN2_K_CUT = 60

# the blocks the checksum code is checked on against numpy: block 0 (+0 and denormals), a block of denormals only, the block that
# holds 1.0, the block that holds 120.0, the last finite block, two blocks of negative values (-1.0's, -120.0's) and the nan block
SUM_BLOCKS = (0x0000, 0x0040, 0x3F80, 0x42F0, 0x7F7F, 0xBF80, 0xC2F0, 0x7FC0)


def _ro(a):
    a.setflags(write=False)
    return a


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def floats(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def block_patterns(block):
    """The 65536 floats of checksum block `block`, in the order of j."""
    return floats(np.uint32(block) * np.uint32(BLOCK) + np.arange(BLOCK, dtype=np.uint32))


def sums_np(fn_results, block):
    """The checksum of csrc/lrm_dbg_math.h in numpy uint64: fn_results holds the float32 results of whole blocks, one
    after the other ((k, 65536) or flat); this is the sum of the block at position `block` among them:
    sum_j r_j * (2 j + 1) mod 2^64 with r_j the result's bits, every nan counted as 0x7fc00000."""
    res = np.ascontiguousarray(fn_results, np.float32).reshape(-1, BLOCK)[block]
    r = bits(res).astype(np.uint64)
    r[np.isnan(res)] = NAN_BITS
    w = 2 * np.arange(BLOCK, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int((r * w).sum(dtype=np.uint64))  # uint64 arithmetic wraps: mod 2^64


def specials():
    """+-0, +-denormal min / max, +-FLT_MIN, +-FLT_MAX, +-inf, nan."""
    pos = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000], np.uint32)
    return floats(np.concatenate([pos, pos | np.uint32(0x80000000), np.array([NAN_BITS], np.uint32)]))


def quadrant_patterns():
    """The 76 floats nearest the odd multiples of pi / 4 below 120: between such a float and a neighbour,
    ((int32_t)r + 0x800000) >> 24 of lrm_sincosf steps to the next quadrant."""
    odd = np.arange(1, 153, 2, dtype=np.float64) * (np.pi / 4)
    odd = odd[odd < 120.0]
    assert len(odd) == 76
    return bits(odd.astype(np.float32))


@functools.lru_cache(maxsize=None)
def named_patterns():
    """Every pattern at which lrm_atanf or lrm_sincosf changes its path, each with its +-8-ulp neighbours and both
    signs, and the specials.  float32, unique bit patterns."""
    centres = np.concatenate([np.array(ATAN_THRESHOLDS + SINCOS_THRESHOLDS, np.uint32), quadrant_patterns()]).astype(np.int64)
    near = (centres[:, None] + np.arange(-8, 9, dtype=np.int64)[None, :]).ravel().astype(np.uint32)
    u = np.unique(np.concatenate([near, near | np.uint32(0x80000000), bits(specials())]))
    return _ro(floats(u))


def pool_exponents():
    e = set(range(-148, 128, 4)) | set(range(-3, 4))
    for k in (59, 60, 61, 62):
        e |= {k, -k}
    return sorted(e)


@functools.lru_cache(maxsize=None)
def atan2_values():
    """The specials and +-m * 2^e, m in {1, 1 + 2^-23, 1.375, 1.5 - 2^-23, 1.5, 2 - 2^-23}, e over every 4th exponent from
    -148 to 127, every e in [-3, 3] and +-59 .. +-62 (the denormal ones rounded to float32): about 1000 values."""
    m = np.array([1.0, 1.0 + 2.0**-23, 1.375, 1.5 - 2.0**-23, 1.5, 2.0 - 2.0**-23])
    e = np.array(pool_exponents(), np.float64)
    v = (m[None, :] * np.exp2(e)[:, None]).ravel()
    assert np.isfinite(v.astype(np.float32)).all()
    v = np.concatenate([v, -v]).astype(np.float32)
    return _ro(floats(np.unique(np.concatenate([bits(v), bits(specials())]))))


@functools.lru_cache(maxsize=None)
def atan2_pool():
    """All pairs (y, x) of atan2_values(): two float32 arrays of about 1e6 entries.  Exponent gaps of 56 .. 65 around the
    +-60 / +-61 cuts of k come from e = +-59 .. +-62 against e in [-3, 3]; every row and column of the zero / inf / nan
    table is there."""
    v = atan2_values()
    y = np.repeat(v, len(v))
    x = np.tile(v, len(v))
    return _ro(y), _ro(x)


THRESHOLD_COORDS = 512


@functools.lru_cache(maxsize=None)
def atan2_on_threshold():
    """Pairs whose quotient |y / x| sits on lrm_atanf's range switches, where lrm_atan2f meets them: for each of the six
    thresholds tau, 512 coordinates x drawn as random_cloud draws them, y = fl(tau * x) moved by -2 .. +2 ulps, both
    signs of y and of x.  Returns (y, x, tau_index), float32 / float32 / int."""
    ys, xs, ts = [], [], []
    for t, tau_bits in enumerate(ATAN_THRESHOLDS):
        tau = floats(np.array([tau_bits], np.uint32))[0]
        x = np.abs(random_cloud(THRESHOLD_COORDS, seed=1000 + t)[:, 0])
        y0 = bits(tau * x).astype(np.int64)  # positive: the bit pattern moves with the ulps
        for d in range(-2, 3):
            y = floats((y0 + d).astype(np.uint32))
            for sy in (1, -1):
                for sx in (1, -1):
                    ys.append(np.float32(sy) * y)
                    xs.append(np.float32(sx) * x)
                    ts.append(np.full(len(x), t))
    return _ro(np.concatenate(ys)), _ro(np.concatenate(xs)), _ro(np.concatenate(ts))


def threshold_hits(y, x, tau_index):
    """Per threshold: how many DISTINCT |x| have a pair with fl(|y / x|) exactly at the threshold pattern, and how many
    one with it one ulp below: [(at, below)] * 6.  Both sides of every switch must be populated."""
    with np.errstate(all="ignore"):
        q = bits(np.abs(y / x)).astype(np.int64)
    out = []
    for t, tau_bits in enumerate(ATAN_THRESHOLDS):
        sel = tau_index == t
        ax = bits(np.abs(x[sel]))
        out.append((len(np.unique(ax[q[sel] == tau_bits])), len(np.unique(ax[q[sel] == tau_bits - 1]))))
    return out
