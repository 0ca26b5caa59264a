"""Shared cases of the one-query-per-lane kernels (tests/test_query_cases_cpu.py, tests/test_gpu_query_shapes.py):
posed_kernel (lrm_posed.hip), ik_kernel / fk_kernel (lrm_ik.hip), ik_posed_kernel / fk_posed_kernel (lrm_ik_posed.hip).

 * pass_sizes(): the queries one pass of each kernel's grid covers, parsed from the three .hip files;
 * walk(): a model of the grid-stride wave walk and of the per-wave table cache (`staged`), loop structure only;
 * index patterns (runs, echo, interleaved, shuffled, single) and with_oob(), which plants out-of-range indices;
 * a pool of K targets, seeds and raw joint angles per (pose, leg), and expand() / gather(): query i takes pool member
   pick(i) of its (pose, leg), so the expected output of every one of n queries is the reference of one of the
   P * L * K unique combinations, gathered through src."""
import os
import re
from types import SimpleNamespace

import numpy as np

from ik_cases import BODY, BODY_ANGLE, COXA_PITCH, back_matrix, fk64, limits, unit
from posed_cases import leg_table, oracle_answer, pose_table

K = 128
INT32_MIN = np.iinfo(np.int32).min
RUN_LENGTHS = (1, 63, 64, 65, 128, 191, 256, 257, 1000)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")
KERNELS = ("posed_kernel", "ik_kernel", "fk_kernel", "ik_posed_kernel", "fk_posed_kernel")


# ---- the pass sizes, from the sources ---------------------------------------------------------
def pass_constants():
    """{kernel: (kBlock, block cap, the *_MIN_WAVES default or None)} as the launch functions compute them"""
    out = {}
    for fname in ("lrm_posed.hip", "lrm_ik.hip", "lrm_ik_posed.hip"):
        src = open(os.path.join(CSRC, fname)).read()
        block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
        macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (LRM_\w+_MIN_WAVES) (\d+)", src)}

        def product(expr):
            return int(np.prod([macros[t] if t in macros else int(t) for t in (s.strip() for s in expr.split("*"))]))

        bounds = {name: macros.get(macro) for macro, name in
                  re.findall(r"__launch_bounds__\(kBlock(?:, (\w+))?\)\s*void (\w+)\(", src)}
        if fname == "lrm_posed.hip":
            cap = product(re.search(r"const size_t cap = ([\d \*]+);", src).group(1))
            assert re.search(r"posed_kernel<true, true>\)?\), grid, dim3\(kBlock\)", src)
            out["posed_kernel"] = (block, cap, bounds["posed_kernel"])
        else:
            for name, expr in re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(grid_for\(n, ([\w \*]+)\)\), dim3\(kBlock\)", src):
                if name in KERNELS:
                    out[name] = (block, product(expr), bounds[name])
    assert set(out) == set(KERNELS), sorted(out)
    return out


def pass_sizes():
    """{kernel: S}, S = kBlock * block cap: a wave's next trip starts S queries after its last one once n > S"""
    return {k: b * cap for k, (b, cap, _) in pass_constants().items()}


# ---- the wave walk ----------------------------------------------------------------------------
def walk(n, S, rec, act_oob=None):
    """The kernels' loop: grid = min(ceil(n / 256), S / 256) blocks of 4 waves; wave w of block b visits i0 = b * 256 +
    w * 64 + k * grid * 256 in trip k.  One entry per 64-query chunk j (i0 = 64 j), visited by wave j % stride in trip
    j // stride.  rec: the (pose, leg) entry of each query; act_oob: queries whose pose or leg index is out of range
    (the clamp sends them to entry 0).  A wave is uniform when its active lanes share one entry; a uniform wave stages
    its entry's table unless `staged` already names it (hit); a mixed wave leaves `staged` alone."""
    rec = np.asarray(rec, np.int64)
    oob = np.zeros(n, bool) if act_oob is None else np.asarray(act_oob, bool)
    stride = min(-(-n // 256), S // 256) * 4
    nch = -(-n // 64)
    pad = nch * 64 - n
    r = np.pad(np.where(oob, 0, rec), (0, pad), mode="edge").reshape(nch, 64)
    active = (np.arange(nch * 64) < n).reshape(nch, 64)
    mixed = ((r != r[:, :1]) & active).any(1)
    hit, staged = np.zeros(nch, bool), np.full(stride, -1, np.int64)
    for k in range(-(-nch // stride)):
        j = np.arange(k * stride, min((k + 1) * stride, nch))
        uni = ~mixed[j]
        hit[j] = uni & (staged[: len(j)] == r[j, 0])
        staged[: len(j)] = np.where(uni, r[j, 0], staged[: len(j)])
    o = np.pad(oob, (0, pad)).reshape(nch, 64)
    return {"stride": stride, "trip": np.arange(nch) // stride, "rec0": r[:, 0], "mixed": mixed, "hit": hit,
            "miss": ~mixed & ~hit, "partial": ~active.all(1), "oob_in_uniform": ~mixed & o.any(1), "lane0_oob": o[:, 0]}


# ---- index patterns: (pose int32[n], leg uint8[n]) ---------------------------------------------
def _split(rec, L):
    return np.ascontiguousarray(rec // L, np.int32), np.ascontiguousarray(rec % L, np.uint8)


def runs(n, P, L, seed=3):
    """runs of one record, lengths cycling through RUN_LENGTHS, records in a shuffled order, every third run (0, 0)"""
    rng = np.random.default_rng(seed)
    nr = 9 * (n // sum(RUN_LENGTHS) + 1)
    rec = np.resize(rng.permutation(P * L), nr)
    rec[::3] = 0
    return _split(np.repeat(rec, np.resize(RUN_LENGTHS, nr))[:n], L)


def echo(n, P, L, S):
    """built from the pass size S (n > S: the stride of walk()): wave c of the grid meets, in trip k,
       c even: record A(c) in every trip (a staged hit from trip 1 on);
       c odd:  record B(c, k) != B(c, k - 1) (a staged miss in every trip);
       c % 5 == 0: record A5(c) in the even trips and, in the odd trips, a mixed wave whose lane 0 is still on A5(c):
                   uniform on A5, mixed, uniform on A5 again (a hit directly after the vector-load path)."""
    R, W = P * L, S // 64
    j = np.arange(-(-n // 64), dtype=np.int64)
    c, k = j % W, j // W
    rec = np.where(c % 2 == 0, (c // 2 * 5) % R, (c * 3 + k * 101 + 1) % R)
    rec = np.where(c % 5 == 0, (c // 5 * 11) % R, rec)
    q = np.repeat(rec, 64)[:n]
    lane = np.arange(n) % 64
    mix = np.repeat((c % 5 == 0) & (k % 2 == 1), 64)[:n]
    return _split(np.where(mix, (q + (lane % 3) * 7) % R, q), L)


def interleaved(n, P, L):
    i = np.arange(n, dtype=np.int64)
    return _split(((i // L) % P) * L + i % L, L)


def shuffled(n, P, L, seed=4):
    return _split(np.random.default_rng(seed).integers(0, P * L, n), L)


def single(n, P, L):
    return np.zeros(n, np.int32), np.zeros(n, np.uint8)


def pattern(name, n, P, L, S):
    return echo(n, P, L, S) if name == "echo" else {"runs": runs, "interleaved": interleaved, "shuffled": shuffled,
                                                    "single": single}[name](n, P, L)


PLACEMENTS = ("lane0", "lane63", "whole_wave", "lane_of_uniform_on_0", "lane_of_uniform_elsewhere", "last_query")


def with_oob(pose, leg, S, nposes, nlegs, nt, per=6):
    """Overwrite chosen queries with out-of-range pose, leg and target indices (the values of
    test_gpu_ik_posed.py::test_out_of_range_indices_on_the_device) at the six PLACEMENTS; the chunks next to a planted
    one stay as they were.  -> SimpleNamespace(pose, leg, t_at, t_val (target_idx[t_at] = t_val), oob_pl, oob_t (per
    query: pose / leg out of range, target out of range), places {placement: queries})"""
    n = len(pose)
    pose, leg = pose.copy(), leg.copy()
    w = walk(n, S, pose.astype(np.int64) * nlegs + leg)
    full, nch = ~w["partial"], len(w["mixed"])
    free = np.ones(nch, bool)  # neither planted nor next to a planted chunk
    free[max(nch - 2, 0):] = False  # the last query's chunk

    def some(sel):
        c, out = np.flatnonzero(sel), []
        for t in np.unique(np.linspace(0, len(c) - 1, per).astype(int)) if len(c) else []:
            cand = c[t:][free[c[t:]]]
            if len(cand):
                out.append(cand[0])
                free[max(cand[0] - 1, 0):cand[0] + 2] = False
        assert out, "with_oob: the pattern has no wave for a placement"
        return np.array(out)

    uni0 = some(full & ~w["mixed"] & (w["rec0"] == 0))
    uni_x = some(full & ~w["mixed"] & (w["rec0"] != 0))
    lane0, lane63, whole = some(full), some(full), some(full)
    places = {"lane0": lane0 * 64, "lane63": lane63 * 64 + 63, "whole_wave": (whole[:, None] * 64 + np.arange(64)).ravel(),
              "lane_of_uniform_on_0": uni0 * 64 + 17, "lane_of_uniform_elsewhere": uni_x * 64 + 41,
              "last_query": np.array([n - 1])}
    bad_pose = np.array([-1, nposes, 1000, INT32_MIN], np.int32)
    bad_leg = np.array([nlegs, 255], np.uint8)
    bad_t = np.array([-1, nt, INT32_MIN], np.int32)
    oob_pl, oob_t, t_at, t_val, m = np.zeros(n, bool), np.zeros(n, bool), [], [], 0
    for name in PLACEMENTS:
        for q in places[name]:
            kind = m % 3 if name in ("lane0", "lane63", "whole_wave") else m % 2  # the clamp placements: pose or leg
            if kind == 0:
                pose[q] = bad_pose[(m // 3) % 4]
            elif kind == 1:
                leg[q] = bad_leg[(m // 3) % 2]
            else:
                t_at.append(q)
                t_val.append(bad_t[(m // 3) % 3])
            (oob_t if kind == 2 else oob_pl)[q] = True
            m += 1
    return SimpleNamespace(pose=pose, leg=leg, t_at=np.array(t_at, np.int64), t_val=np.array(t_val, np.int32), oob_pl=oob_pl,
                           oob_t=oob_t, places=places)


# ---- the pool ---------------------------------------------------------------------------------
def coxa_frame(v, leg, quat):
    """points of the coxa joint's frame (z: the coxa axis, origin: the joint) in the caller's frame, float64: the chain
    of ik_cases.fk64 after the joint angles (coxa pitch, body offset, leg azimuth, body orientation)"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    leg = np.asarray(leg, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    cp, sp = np.cos(leg[COXA_PITCH]), np.sin(leg[COXA_PITCH])
    x, z = x * cp - z * sp + leg[BODY], x * sp + z * cp
    cb, sb = np.cos(leg[BODY_ANGLE]), np.sin(leg[BODY_ANGLE])
    x, y = x * cb - y * sb, x * sb + y * cb
    return np.stack([x, y, z], 1) @ back_matrix(quat).T


def bad_seeds(n, rng):
    """seeds() of test_gpu_ik_posed.py: finite, nan, inf, -inf, 1e20"""
    seed = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    seed[::7, 0] = np.nan
    seed[3::11] = np.inf
    seed[5::13, 2] = -np.inf
    seed[6::17] = 1e20
    return seed


def limit_grid(oracle, leg, quat):
    """27 joint-angle triples: lower limit, mid-range and upper limit of every joint (float32, after rotate_leg_data)"""
    lim = limits(oracle, leg, quat)
    axes = [np.array([lim[k][0], (np.float32(lim[k][0]) + np.float32(lim[k][1])) / np.float32(2), lim[k][1]], np.float32)
            for k in ("coxa", "femur", "tibia")]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(27, 3)


def pool_of(oracle, leg, quat, body, rng):
    """K body-relative targets (+ body, float32), K seeds, K raw joint-angle triples of one (pose, leg)"""
    grid = limit_grid(oracle, leg, quat)
    tips = fk64(grid, leg, quat)
    d = rng.standard_normal((27, 3))
    near = tips + 1e-3 * d / np.linalg.norm(d, axis=1, keepdims=True)
    s = np.array([-150.0, -20.0, 60.0, 250.0])
    on_axis = coxa_frame(np.stack([0 * s, 0 * s, s], 1), leg, quat)
    by_axis = coxa_frame(np.stack([1e-4 * np.cos(s), 1e-4 * np.sin(s), s], 1), leg, quat)
    joint = coxa_frame([[0, 0, 0]], leg, quat)
    far = 1e6 * d[:1] / np.linalg.norm(d[:1])
    special = np.array([[np.nan, 10, 10], [np.nan] * 3, [np.inf, 0, 0], [5, -np.inf, 5], [np.inf, np.inf, -np.inf]])
    fixed = np.concatenate([tips, near, on_axis, by_axis, joint, far, special])
    lo, hi = np.array([-450, -450, -400], np.float32), np.array([450, 450, 200], np.float32)
    rand = rng.random((K - len(fixed), 3), dtype=np.float32) * (hi - lo) + lo  # as posed_cases.queries
    rel = np.concatenate([fixed, rand]).astype(np.float32)
    ang = bad_seeds(K, rng) * np.float32(np.pi)
    ang[:27] = grid
    return (rel + body).astype(np.float32), bad_seeds(K, rng), ang


def pick(n):
    """the pool member of query i: a fixed hash of i, so neighbours and queries a pass apart take different members"""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(41)).astype(np.int64) % K


def expand(pose, leg, nlegs, oob_pl=None):
    """-> (k, src): the pool member of every query and its unique combination (pose * nlegs + leg) * K + k, -1 where the
    pose or leg index is out of range; such a query takes member k of entry 0, where the clamp sends it"""
    k = pick(len(pose))
    src = (pose.astype(np.int64) * nlegs + leg) * K + k
    return k, src if oob_pl is None else np.where(oob_pl, -1, src)


def gather(ref, src, fill, also=None):
    """the expected output of every query: ref[src], `fill` where src is -1 or `also` is set"""
    out = np.asarray(ref)[np.maximum(src, 0)]
    out[(src < 0) if also is None else ((src < 0) | also)] = fill
    return out


_CACHE = {}


def cases(lrm, oracle):
    """The tables (37 unit quaternions x 7 legs), the pool, its unique combinations U (pair-major) and their references,
    computed once per process: posed_kernel's from the oracle, the IK's and FK's from the posed CPU calls; `one`: the
    pool of one (pose, leg) as the single-pose calls see it, with lrm_ik_cpu / lrm_fk_cpu as the reference."""
    if "c" in _CACHE:
        return _CACHE["c"]
    quats, body = pose_table(lrm)
    quats = np.stack([unit(q) for q in quats])
    legs = leg_table(lrm)
    P, L = len(quats), len(legs)
    rng = np.random.default_rng(11)
    xyz, seed, ang = (np.zeros((P, L, K, 3), np.float32) for _ in range(3))
    for p in range(P):
        for l in range(L):
            xyz[p, l], seed[p, l], ang[p, l] = pool_of(oracle, legs[l], quats[p], body[p], rng)
    c = SimpleNamespace(quats=quats, body=body, legs=legs, P=P, L=L, nu=P * L * K, xyz=xyz.reshape(-1, 3), seed=seed.reshape(-1, 3),
                        ang=ang.reshape(-1, 3), pose=np.repeat(np.arange(P, dtype=np.int32), L * K),
                        leg=np.tile(np.repeat(np.arange(L, dtype=np.uint8), K), P))
    c.ang_finite = np.nan_to_num(np.clip(c.ang, -10, 10), nan=0.25)
    tab = (c.pose, c.leg, quats, body, legs)
    c.mask, c.valid, c.field = oracle_answer(oracle, c.xyz, *tab)
    c.ik_a, c.ik_s, _ = lrm.apply_ik_posed_cpu(c.xyz, *tab)
    c.iks_a, c.iks_s, _ = lrm.apply_ik_posed_cpu(c.xyz, *tab, seed=c.seed)
    c.fk_ik, _ = lrm.apply_fk_posed_cpu(c.ik_a, *tab)
    c.fk_raw, _ = lrm.apply_fk_posed_cpu(c.ang, *tab)
    c.fk_finite, _ = lrm.apply_fk_posed_cpu(c.ang_finite, *tab)
    sp, sl = 5, L - 1
    o = SimpleNamespace(leg=legs[sl], quat=quats[sp], seed=seed[sp, sl], ang=ang[sp, sl],
                        xyz=(xyz[sp, sl] - body[sp]).astype(np.float32))
    o.ik_a, o.ik_s, _ = lrm.apply_ik_cpu(o.xyz, o.leg, o.quat)
    o.iks_a, o.iks_s, _ = lrm.apply_ik_cpu(o.xyz, o.leg, o.quat, seed=o.seed)
    o.fk_ik, _ = lrm.apply_fk_cpu(o.ik_a, o.leg, o.quat)
    o.fk_raw, _ = lrm.apply_fk_cpu(o.ang, o.leg, o.quat)
    c.one = o
    _CACHE["c"] = c
    return c
