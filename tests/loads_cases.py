"""Shared cases of the stance loads tests (tests/test_stance_loads_cpu.py, tests/test_gpu_stance_loads.py): seeded corpora of
sets (a unit quaternion and three joint angles per leg, the feet spread below and around the body) and the host loop as a dict."""
import numpy as np

F = np.float32
TAU_MAX = np.array([np.inf, 120.0, 60.0], F)  # load x mm: the coxa never limits, femur and tibia do for stretched legs
COMS = ([0.0, 0.0, 0.0], [60.0, -40.0, 10.0], [-150.0, 90.0, -20.0])  # BODY frame, mm: centred, eccentric, near the rim
SLOPE = np.deg2rad(20.0)
PLANE_TILTED = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(SLOPE), np.sin(SLOPE)]], F)  # the plane normal to gravity on a 20 degree slope


def legs_n(lrm, n, moonbot_every=0):
    """n M2 legs evenly around the body; every moonbot_every-th one a moonbot leg"""
    az = 2 * np.pi * np.arange(n) / n
    return np.stack([(lrm.get_moonbot_leg if moonbot_every and l % moonbot_every == 1 else lrm.get_M2_leg)(float(az[l])) for l in range(n)]).astype(F)


def unit_quats(rng, n, tilt=0.25):
    """unit quaternions (w, x, y, z) within about `tilt` rad of the identity, any yaw"""
    yaw = rng.uniform(-np.pi, np.pi, n)
    q = np.column_stack([np.cos(yaw / 2), rng.uniform(-tilt, tilt, n) / 2, rng.uniform(-tilt, tilt, n) / 2, np.sin(yaw / 2)])
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def corpus(lrm, seed, ns=1500, nlegs=6, moonbot_every=0):
    """-> (legs [nlegs, 14], quats [ns, 4], angles [nlegs*ns, 3] at [l*ns + s]): every foot well below the coxa and out from
    the body, a fifth of the legs stretched nearly flat, a twentieth tucked under the body"""
    rng = np.random.default_rng(seed)
    legs = legs_n(lrm, nlegs, moonbot_every)
    quats = unit_quats(rng, ns)
    n = nlegs * ns
    a = np.column_stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.6, 0.5, n), rng.uniform(-2.2, -0.6, n)])
    flat = rng.random(n) < 0.2
    a[flat, 1] = rng.uniform(-0.1, 0.1, flat.sum())
    a[flat, 2] = rng.uniform(-0.3, 0.0, flat.sum())
    tucked = rng.random(n) < 0.05
    a[tucked, 1] = rng.uniform(0.6, 1.2, tucked.sum())
    a[tucked, 2] = rng.uniform(-2.8, -2.3, tucked.sum())
    return legs, quats, a.astype(F)


def host(lrm, quats, legs, angles, tau_max=TAU_MAX, pose_idx=None, com=None, plane=None, lift=None, live_in=None, **want):
    st, hold, peak, peak_at, load, tau, _ = lrm.stance_loads_posed_cpu(quats, legs, angles, tau_max, pose_idx, com, plane, lift, live_in,
                                                                      **want)
    return {"status": st, "holdable": hold, "peak": peak, "peak_at": peak_at, "load": load, "tau": tau}

