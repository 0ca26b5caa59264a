"""CPU-only checks of the product library: it loads, exports every symbol include/lrm.h
declares, its host-side leg compiler + strict per-point code (the same source the kernels
compile) reproduce the reference fixtures bit for bit through the explicit CPU entry points
(apply_reach_cpu / apply_dist_cpu mirrors), and the GPU entry points fail loudly, not
silently, when there is no device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, bits_equal, golden_cases, load_case, random_cloud


def test_library_exports_every_declared_symbol(lrm):
    declared = lrm.declared_symbols()
    exported = set(lrm.exported_symbols())
    assert len(declared) >= 25
    missing = [s for s in declared if s not in exported]
    assert not missing, missing


def test_leg_struct_layout_and_factories(lrm):
    legs = dict(np.load(os.path.join(GOLDEN, "legs.npz")))
    az = legs.pop("azimuths")
    for i, a in enumerate(az):
        assert lrm.get_M2_leg(float(a)).tobytes() == legs[f"m2_{i}"].tobytes()
        assert lrm.get_moonbot_leg(float(a)).tobytes() == legs[f"moonbot_{i}"].tobytes()
    tab = np.load(os.path.join(GOLDEN, "rotate_leg_data.npy"))
    for row in tab:
        assert lrm.rotate_leg_data(row[14:18], row[:14]).tobytes() == row[18:].tobytes()


@pytest.mark.parametrize("name", golden_cases())
def test_cpu_entry_points_match_reference_fixture(lrm, name):
    c = load_case(name)
    m, ms = lrm.apply_reach_cpu(c["points"], c["leg"], c["quat"])
    d, v, ms2 = lrm.apply_dist_cpu(c["points"], c["leg"], c["quat"])
    assert ms >= 0 and ms2 >= 0
    assert np.array_equal(m, c["mask"])
    assert np.array_equal(v, c["valid"])
    assert bits_equal(d, c["dist"]).all()


def test_cpu_entry_points_match_oracle_on_random_cloud(lrm, oracle):
    pts = random_cloud(200000, seed=123)
    for leg in (lrm.get_M2_leg(0.4), lrm.get_moonbot_leg(-1.0)):
        for q in (None, (0.97, 0.05, -0.2, 0.1)):
            qq = (1, 0, 0, 0) if q is None else q
            assert np.array_equal(lrm.apply_reach_cpu(pts, leg, q)[0], oracle.reach(pts, leg, qq))
            d, v, _ = lrm.apply_dist_cpu(pts, leg, q)
            d0, v0 = oracle.dist(pts, leg, qq)
            assert np.array_equal(v, v0) and bits_equal(d, d0).all()


def test_empty_and_null_arguments(lrm):
    L = lrm.lib()
    leg = lrm.get_M2_leg()
    m, _ = lrm.apply_reach_cpu(np.zeros((0, 3), np.float32), leg)
    assert m.shape == (0,)
    # null leg -> LRM_EINVAL with a message, no crash
    rc = L.lrm_reach_cpu(None, 4, None, None, None, None)
    assert rc == -1 and L.lrm_last_error()
    rc = L.lrm_reach_any_dev(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, None)
    assert rc == -1
    assert L.lrm_set_mode(7) == -1
    assert L.lrm_set_mode(3) == 0 and L.lrm_get_mode() == 3  # LRM_MODE_TOL_REL
    assert L.lrm_set_mode(0) == 0 and L.lrm_get_mode() == 0
    assert L.lrm_set_mode(1) == 0 and L.lrm_get_mode() == 1  # back to the default


def test_gpu_entry_points_fail_loudly_without_a_device(lrm):
    """No CPU fallback behind the GPU entry points."""
    if lrm.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(lrm.LrmError):
        lrm.apply_reach(np.zeros((8, 3), np.float32), lrm.get_M2_leg())
    with pytest.raises(lrm.LrmError):
        lrm.positionability(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32),
                            [lrm.get_M2_leg()], [(1, 0, 0, 0)])


def test_exact_math_host_matches_glibc(lrm):
    """csrc/lrm_exact_math.h (host build) == this machine's glibc atan2f / sincosf, bit for
    bit, on the value ranges the path produces (and well beyond for atan2f)."""
    rng = np.random.default_rng(0)
    n = 4_000_000
    a = np.concatenate([
        rng.uniform(-7, 7, n).astype(np.float32),                      # angles
        (rng.standard_normal(n) * 300).astype(np.float32),              # coordinates (mm)
        rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern
        np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-38, -1e-38, np.pi, -np.pi], np.float32),
    ])
    b = np.concatenate([
        (rng.standard_normal(n) * 300).astype(np.float32),
        (rng.standard_normal(n) * 300).astype(np.float32),
        rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32),
        np.array([1.0, 0.0, -0.0, 0.0, np.inf, np.inf, 1.0, -1e-38, 1e38, -1.0, -1.0], np.float32),
    ])
    at2 = np.empty_like(a)
    sn = np.empty_like(a)
    cs = np.empty_like(a)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lrm.lib().lrm_dbg_exact_math_host(P(a), P(b), len(a), P(at2), P(sn), P(cs)) == 0
    libm = C.CDLL("libm.so.6")
    libm.atan2f.restype = C.c_float
    libm.atan2f.argtypes = [C.c_float, C.c_float]
    # vectorised libm through numpy's float32 ufuncs would go through numpy's own SIMD
    # kernels, not glibc: call glibc directly on a subsample, and numpy on all as a second check
    idx = rng.integers(0, len(a), 200000)
    want = np.array([libm.atan2f(float(a[i]), float(b[i])) for i in idx], np.float32)
    assert bits_equal(at2[idx], want).all()
    s_ = C.c_float()
    c_ = C.c_float()
    libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    sel = idx[np.abs(a[idx]) < 100][:100000]
    ws = np.empty(len(sel), np.float32)
    wc = np.empty(len(sel), np.float32)
    for k, i in enumerate(sel):
        libm.sincosf(float(a[i]), C.byref(s_), C.byref(c_))
        ws[k], wc[k] = s_.value, c_.value
    assert bits_equal(sn[sel], ws).all() and bits_equal(cs[sel], wc).all()


@pytest.mark.parametrize("name", golden_cases())
def test_filtered_evaluation_on_host_matches_fixture(lrm, name):
    """csrc/lrm_point_fast.h (LRM_MODE_FAST) compiled for the host, without the caller-side
    fallback: the distance field and its validity byte are bit-identical on EVERY point (the
    filter resolves its doubts internally); the reach mask is identical wherever the filter does
    not raise its `uncertain` flag (flagged points are re-evaluated by the strict code)."""
    c = load_case(name)
    f = lrm.dbg_fast_host(c["points"], c["leg"], c["quat"])
    sure = f["mask_unc"] == 0
    assert np.array_equal(f["mask"][sure], c["mask"][sure])
    assert np.array_equal(f["valid"], c["valid"])
    assert bits_equal(f["dist"], c["dist"]).all()
    if name.startswith("cube"):
        assert 1 - sure.mean() < 1e-3  # the strict fallback is rare on ordinary clouds
    # the fused kernel's reach mask (a by-product of the distance evaluation, lrm_reach_from_dist)
    fm, fd = lrm.dbg_fused_reach_host(c["points"], c["leg"], c["quat"])
    assert np.array_equal(fm[fd == 0], c["mask"][fd == 0])
    if name.startswith("cube"):
        assert fd.mean() < 1e-3


def test_filtered_evaluation_random_legs_and_clouds(lrm):
    """Random legs (within the filter's eligibility) x orientations x clouds: filtered == strict."""
    rng = np.random.default_rng(2024)
    checked = 0
    for trial in range(12):
        leg = lrm.leg_factory(rng.uniform(-3, 3), rng.uniform(80, 250), rng.uniform(-60, 30), rng.uniform(30, 90),
                              rng.uniform(90, 160), rng.uniform(90, 170), rng.uniform(30, 80), rng.uniform(60, 100),
                              rng.uniform(90, 140), rng.uniform(-20, 10), rng.uniform(-20, 10))
        q = rng.normal(size=4).astype(np.float32)
        q[0] += 3.0
        pts = random_cloud(60000, seed=trial)
        try:
            f = lrm.dbg_fast_host(pts, leg, q)
        except lrm.LrmError:
            continue  # leg outside the filter's eligibility: the library uses the strict path
        m, _ = lrm.apply_reach_cpu(pts, leg, q)
        d, v, _ = lrm.apply_dist_cpu(pts, leg, q)
        sure = f["mask_unc"] == 0
        assert np.array_equal(f["mask"][sure], m[sure])
        assert np.array_equal(f["valid"], v) and bits_equal(f["dist"], d).all()
        fm, fd = lrm.dbg_fused_reach_host(pts, leg, q)
        assert np.array_equal(fm[fd == 0], m[fd == 0]) and fd.mean() < 2e-3
        checked += 1
    assert checked >= 8


def test_pair_bounding_sphere_contains_every_reachable_pair(lrm, oracle):
    """The per-leg sphere with which the pair kernels skip batches of footholds must contain every
    (foothold - body) the strict reachable_rotate_leg accepts: dense samples around the leg, the two
    committed legs at several mounts plus random legs, random body orientations."""
    rng = np.random.default_rng(77)
    legs = [lrm.get_M2_leg(a) for a in (0.0, 1.0471976, 2.0943952, 3.1415927, -1.0471976)]
    legs += [lrm.get_moonbot_leg(a) for a in (0.0, 1.5707964)]
    for _ in range(6):
        legs.append(lrm.leg_factory(rng.uniform(-3, 3), rng.uniform(80, 250), rng.uniform(-60, 30), rng.uniform(30, 90),
                                    rng.uniform(90, 160), rng.uniform(90, 170), rng.uniform(30, 80), rng.uniform(60, 100),
                                    rng.uniform(90, 140), rng.uniform(-20, 10), rng.uniform(-20, 10)))
    reachable_seen = 0
    for i, leg in enumerate(legs):
        q = np.array([1, 0, 0, 0], np.float32) if i % 2 == 0 else (rng.normal(size=4) + [3, 0, 0, 0]).astype(np.float32)
        centre, r2 = lrm.dbg_pair_sphere(leg, q)
        rel = rng.uniform(-700, 700, (150_000, 3)).astype(np.float32)
        # reach(body, target) depends on target - body only: one target at the origin, bodies at -rel
        hit = oracle.reach_any(-rel, np.zeros((1, 3), np.float32), [leg], q)[0].astype(bool)
        d2 = ((rel[hit].astype(np.float64) - centre) ** 2).sum(axis=1)
        assert (d2 <= r2).all(), (i, float(d2.max()), r2)
        reachable_seen += int(hit.sum())
        assert r2 < 0.75 * (float(leg[1]) + float(leg[3]) + float(leg[4]) + float(leg[5]) + 1) ** 2 or float(leg[3]) <= 0
    assert reachable_seen > 5000


def test_rbdl_equivalent_baseline(lrm):
    """lrm_rbdl_equiv_cpu = apply_RBDL's work (rbdl_benchmark.cpp:18-111) restated: PARITY UNPINNED (RBDL is absent
    and unpinned), so only sanity is checked: the chain has no joint limits, so nothing beyond its stretched length
    targets well inside its shell mostly converge within the 10 steps x 5 starts, and the call reports a time.
    (RBDL's second stopping rule, |dq| < step_tol, also "converges" on an unreachable target when the error is
    orthogonal to the Jacobian's range -- the stretched leg pointing at it: `valid` is not reachability.)"""
    pts = random_cloud(20000, seed=4)
    leg = lrm.get_M2_leg(0.0)
    ok, ms = lrm.apply_rbdl_equiv(pts, leg)
    assert ms > 0 and ok.dtype == np.uint8 and set(np.unique(ok)) <= {0, 1}
    # tip = (body,0,0) + Rz(q0)[(coxa,0,0) + ...]: |tip - (body,0,0)| <= coxa + femur + tibia
    d = np.linalg.norm(pts - np.array([leg[1], 0, 0], np.float32), axis=1)
    reach = leg[3] + leg[4] + leg[5]
    assert ok[d > reach + 1e-3].mean() < 0.05
    inside = (d < 0.8 * reach) & (d > 0.5 * reach)
    assert ok[inside].mean() > 0.5


def test_tolerance_kernels_keep_their_register_budget(lrm):
    """The headline kernel is built for 8 waves/SIMD (64 VGPRs) without scratch; the build writes the compiler's
    resource remarks next to the object (csrc/Makefile).  A change that spills shows up here, not as a slower bench."""
    import os
    import re
    path = os.path.join(os.path.dirname(lrm.LIB_PATH), "csrc", "build", "lrm_tol_kernels.resource.txt")
    if not os.path.exists(path):
        pytest.skip("resource remarks not present (library built elsewhere)")
    text = open(path).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if "dist_tol_staged_kernel" not in name:
            continue
        seen += 1
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) == 8, name
    assert seen == 4  # kOp 1 and 2, SoA and float3 layout


def test_shard_bounds_of_the_c_abi_equal_the_python_ones(lrm):
    """lrm_shard_bounds (the split lrm_reach_dist_multi uses) == lrm_amd.shard.shard_bounds (the torch.distributed
    drivers): both sides of a mixed deployment own identical slices; shards cover [0, n) and start on whole words."""
    from lrm_amd import shard
    for n in (0, 1, 63, 64, 65, 1000, 10**7 + 3, 10**8):
        for world in (1, 2, 3, 8):
            prev = 0
            for r in range(world):
                lo, hi = lrm.c_shard_bounds(n, world, r)
                assert (lo, hi) == shard.shard_bounds(n, world, r)
                assert lo == prev or lo == n
                assert lo % 64 == 0 or lo == n
                prev = hi
            assert prev == n
    with pytest.raises(lrm.LrmError):
        lrm.c_shard_bounds(10, 2, 2)
    with pytest.raises(lrm.LrmError):
        lrm.c_shard_bounds(10, 0, 0)


def test_multi_entry_fails_without_a_device(lrm):
    """no GPU in the build container: the multi-device entry reports LRM_ENODEV, it never computes on the CPU"""
    if lrm.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(lrm.LrmError):
        lrm.apply_reach_dist_multi(np.zeros((10, 3), np.float32), lrm.get_M2_leg(0.0), None, ndev=1)
