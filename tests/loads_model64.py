"""An independent float64 model of the foot loads and joint torques of stance_loads() (tests/test_stance_loads_cpu.py,
tests/test_gpu_stance_loads.py), written from the leg's geometry and from statics, not from the library: the joints are
leg_model64's (a yawing coxa, a femur and a tibia pitching in the plane through the yaw axis); a joint's axis is the normal of
the plane its link sweeps when that joint alone turns, taken from the model's own joints by a cross product -- NOT from a
Jacobian column; the torque about joint j is axis_j . ((P - J_j) x up); the loads are numpy.linalg.lstsq's minimum-norm
solution of (sum load = 1, both moments 0) on the feet the library reports as carrying (load > 0).

The model holds for unit quaternions (for others the frame change of the queries is no rotation and a cross product of
transformed vectors is no axis); the corpora here are unit.

The measured bands (measured by tests/test_stance_loads_cpu.py::test_the_band_is_measured on corpus(1), asserted
at four times the worst value seen, rounded up to one digit) live here so that the CPU and the GPU tests share them."""
import numpy as np

import leg_model64 as lm
import stance_model64 as sm

F = np.float32
D = np.float64

# What an answer may differ by grows with the conditioning of its carrying feet: every figure but "sum" is divided by
# cond(s) = the ratio of the largest to the smallest singular value of the 3 x k matrix [1, xi / LENGTH, eta / LENGTH] of the
# carrying feet, taken from the model's float64 feet (1 for a regular polygon about the centre of mass, some hundreds for feet
# nearly in line).  measured worst on corpus 1 -> asserted
LENGTH = 200.0  # mm: the scale of a stance
def band_of(measured):
    """four times the measured worst, rounded up to one digit (the project's convention)"""
    x = 4.0 * measured
    unit = 10.0 ** np.floor(np.log10(x))
    return float(np.ceil(x / unit * (1 - 1e-12)) * unit)


MEASURED = {"sum": 6.557e-07,     # |sum load - 1|
            "moment": 1.739e-04,  # |sum load xi64|, |sum load eta64| (mm) / cond
            "load": 2.765e-07,    # |load - load64| (fraction of the weight) / cond
            "tau": 5.486e-05}     # |tau - load64 arm64| (load x mm) / cond
BAND = {k: band_of(v) for k, v in MEASURED.items()}  # 3e-6, 7e-4 mm, 2e-6, 3e-4 mm
# b of the cross-check with stance_stability (mm): margin > b => status 1..3, and status 1..3 => margin >= -b
MEASURED_MARGIN = 3.003e-3
BAND_MARGIN = band_of(MEASURED_MARGIN)  # 0.02 mm
DELTA = 0.5         # rad: how far a joint turns to show the plane its link sweeps


def up_of(plane):
    """the direction the feet push along: +z without a plane, else u x v (not normalised, as the contract has it)"""
    if plane is None:
        return np.array([0.0, 0.0, 1.0])
    p = np.asarray(plane, F).astype(D).reshape(2, 3)
    return np.cross(p[0], p[1])


def project(q, plane):
    q = np.asarray(q, D)
    if plane is None:
        return q[..., :2]
    p = np.asarray(plane, F).astype(D).reshape(2, 3)
    return np.stack([q @ p[0], q @ p[1]], -1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def statics64(angles, legs, quats, pose_idx=None, com=None, plane=None):
    """angles float [nlegs*nsets, 3] at [l*nsets + s] -> dict: valid bool[nlegs, nsets] (finite joints), xi, eta [nlegs, nsets]
    (the foot's plane point minus the centre of mass), arm [nlegs, nsets, 3] (the torque about coxa, femur, tibia per unit
    load, in the angle's positive sense)"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    quats = np.asarray(quats, F).reshape(-1, 4)
    nl = len(legs)
    a = np.asarray(angles, F).astype(D).reshape(nl, -1, 3)
    ns = a.shape[1]
    pose_of = np.arange(ns) if pose_idx is None else np.asarray(pose_idx)
    up = up_of(plane)

    def joints(shift):
        return lm.joints64_posed((a + np.asarray(shift, D)).reshape(-1, 3), legs, quats, 0.0, pose_of)

    J = joints([0, 0, 0])
    turned = [joints([DELTA, 0, 0]), joints([0, DELTA, 0]), joints([0, 0, DELTA])]
    P = J[:, :, 3]
    arm = np.empty((nl, ns, 3), D)
    with np.errstate(invalid="ignore"):
        for j in range(3):  # joint j sits at J[j] and moves J[j + 1]
            axis = _unit(np.cross(J[:, :, j + 1] - J[:, :, j], turned[j][:, :, j + 1] - J[:, :, j]))
            arm[:, :, j] = (axis * np.cross(P - J[:, :, j], up)).sum(-1)
    com = np.zeros(3) if com is None else np.asarray(com, F).astype(D)
    c3 = np.stack([sm.rotation64(quats[p]) @ com for p in pose_of])
    f = project(P, plane) - project(c3, plane)[None]
    return {"valid": np.isfinite(J).all((2, 3)), "xi": f[..., 0], "eta": f[..., 1], "arm": arm}


def loads64(xi, eta, active):
    """the minimum-norm loads of the feet in `active` (bool[nlegs]) -> float64[nlegs], 0 elsewhere"""
    out = np.zeros(len(xi), D)
    k = np.flatnonzero(active)
    A = np.stack([np.ones(len(k)), xi[k], eta[k]])
    out[k] = np.linalg.lstsq(A, np.array([1.0, 0.0, 0.0]), rcond=None)[0]
    return out


def cond(xi, eta, active):
    k = np.flatnonzero(active)
    sv = np.linalg.svd(np.stack([np.ones(len(k)), xi[k] / LENGTH, eta[k] / LENGTH]), compute_uv=False)
    return float(sv[0] / sv[-1])


def measure(got, M, lift, measure_into=None):
    """The library's status, load [nmasks, nlegs, nsets] and tau [nmasks, nlegs, 3, nsets] against the model M = statics64(..)
    on every (lift set, set) with status 1..3 -> dict of the worst |sum load - 1| and, each divided by cond(), moment (mm),
    |load - load64| and |tau - load64 arm| (mm), and the number of answers compared.  Asserts what needs no band: loads >= 0, exactly +0 off the
    planted set, the carrying feet are planted and valid."""
    status, load, tau = got["status"], got["load"], got["tau"]
    nm, nl, ns = load.shape
    worst = {"sum": 0.0, "moment": 0.0, "load": 0.0, "tau": 0.0, "answers": 0}
    for m in range(nm):
        planted = M["valid"] & ~(((int(lift[m]) >> np.arange(nl)) & 1).astype(bool))[:, None]
        for s in np.flatnonzero((status[m] >= 1) & (status[m] <= 3)):
            w = load[m, :, s]
            assert (w >= 0).all() and not np.signbit(w).any(), (m, s, w)
            assert (w[~planted[:, s]] == 0).all() and (tau[m, ~planted[:, s], :, s] == 0).all(), (m, s)
            assert not np.signbit(tau[m, ~planted[:, s], :, s]).any()
            active = w > 0
            xi, eta = M["xi"][:, s], M["eta"][:, s]
            w64 = loads64(xi, eta, active)
            c = cond(xi, eta, active)
            worst["sum"] = max(worst["sum"], abs(float(w.astype(D).sum()) - 1.0))
            worst["moment"] = max(worst["moment"], abs(float(w @ xi)) / c, abs(float(w @ eta)) / c)
            worst["load"] = max(worst["load"], float(np.abs(w - w64).max()) / c)
            worst["tau"] = max(worst["tau"], float(np.abs(tau[m, :, :, s] - w64[:, None] * M["arm"][:, s]).max()) / c)
            worst["answers"] += 1
    if measure_into is not None:
        for k, v in worst.items():
            measure_into[k] = (measure_into.get(k, 0) + v) if k == "answers" else max(measure_into.get(k, 0.0), v)
    return worst
