"""Makes tests/golden/frozen/tab_point_frozen.npz (in a directory of its own: every .npz directly under tests/golden/ is taken
for a reference case by conftest.golden_cases): the outputs of the table evaluation of one point (csrc/lrm_point_tol.h,
lrm_tab_point) on the host, frozen bit for bit, for tests/test_tab_point_frozen_cpu.py.

Run it at the commit whose results are to be kept (it was run at the parent of the commit that cut lrm_tab_point's
instruction count, before any cut):  python tests/golden/make_tab_point_frozen.py

Per case (M2 and moonbot leg x the azimuths and the four QUATS of tests/test_tol_cpu.py) a seeded cloud that mixes
  * the config-2 box,
  * points within 1 mm of the coxa axis and of the two yaw-limit planes (a quarter of the latter ON the plane),
  * points beyond the inner grid (the outer-grid path of lrm_toltab_lookup2),
  * nan / inf / huge / zero coordinates,
  * points picked from a larger box cloud because the evaluation puts them in doubt, so many per LRM_TD_* kind, and
    because it evaluates their second yaw candidate (found by bisection on the `second_candidates` statistic).
Recorded: lrm_amd.dbg_toltab_host (the kInfo = false instance) and lrm_amd.dbg_replay_host (the kInfo = true instance and
the strict replay of its info word: a wrongly packed field shows as a different vector) as flag, doubt word and the
vector's raw uint32.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import lrm_amd  # noqa: E402

QUATS = [(1, 0, 0, 0), (0.9848, 0, 0.1736, 0), (0.9397, 0, 0, 0.342), (0.9, 0.1, 0.2, -0.3)]  # tests/test_tol_cpu.py
AZIMUTHS = [0.0, np.pi / 3, -2.0]
KINDS = {"yaw": 1, "region": 2, "clamp": 4, "tie": 8, "none": 16, "limit": 32, "pick": 64, "ambig": 0x100}
LO = np.array([-200, -500, -500], np.float32)
HI = np.array([700, 500, 300], np.float32)
SPECIAL = np.array([[np.nan, 0, 0], [0, np.nan, 5], [1, 2, np.nan], [np.inf, 1, 2], [-np.inf, 0, 0], [0, np.inf, 0], [3, 4, -np.inf],
                    [1e30, 1e30, -1e30], [3e38, 0, 0], [0, 0, 0], [-0.0, -0.0, -0.0], [1e-42, -1e-42, 1e-45],
                    [181.0, 0.0, 0.0], [181.0, 0.0, 50.0], [181.0, 0.0, -300.0], [181.0, 1e-30, 10.0]], np.float32)


def rot_q(q, sign):
    """v + 2 w (u x v) + 2 u x (u x v) as a matrix (no normalisation, as the library rotates); sign = -1: by the inverse
    quaternion, conjugate / |q|^2"""
    q = np.asarray(q, np.float64)
    if sign < 0:
        q = q * np.array([1, -1, -1, -1]) / (q @ q)
    w, u = float(q[0]), q[1:]
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + 2.0 * (w * K + K @ K)


def to_body(c, leg, q, conv):
    """coxa-frame points -> body frame: the inverse of  c = Rp (Rz (Rq p) - (body, 0, 0))  under sign convention conv"""
    sq, sz, sp = conv
    a, b = sz * float(leg[0]), sp * float(leg[2])
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rp = np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]])
    v = np.linalg.solve(Rp, np.asarray(c, np.float64).T).T + np.array([float(leg[1]), 0, 0])
    return np.linalg.solve(rot_q(q, sq) @ np.eye(3), np.linalg.solve(Rz, v.T)).T.astype(np.float32)


def axis_points(rng, n):
    rad, ang = rng.uniform(0, 1, n), rng.uniform(-np.pi, np.pi, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-400, 300, n)], 1)


def plane_points(rng, n, leg):
    """abscissa rho (either sign: the mirrored half too) along a yaw-limit direction, offset w across it"""
    lim = np.where(rng.random(n) < 0.5, float(leg[8]), float(leg[9]))
    rho = rng.uniform(-600, 600, n)
    w = np.where(np.arange(n) % 4 == 0, 0.0, rng.uniform(-1, 1, n))
    return np.stack([rho * np.cos(lim) - w * np.sin(lim), rho * np.sin(lim) + w * np.cos(lim), rng.uniform(-400, 300, n)], 1), w == 0.0


def convention(leg, q):
    """the sign convention under which points built ON the coxa axis and ON the yaw-limit planes are what the evaluation calls so
    (LRM_TD_YAW: r below LRM_TOL_RMIN, or a sector test inside its band)"""
    rng = np.random.default_rng(1)
    ax = axis_points(rng, 200)
    pl, on = plane_points(rng, 400, leg)
    best = None
    for conv in [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]:
        pts = np.concatenate([to_body(ax, leg, q, conv), to_body(pl[on], leg, q, conv)])
        _, _, doubt, _ = lrm_amd.dbg_toltab_host(pts, leg, q)
        score = float(((doubt & KINDS["yaw"]) != 0).mean())
        if best is None or score > best[0]:
            best = (score, conv)
    assert best[0] > 0.95, best
    return best[1]


def seconds(pts, leg, q):
    return lrm_amd.dbg_toltab_host(pts, leg, q)[3]["second_candidates"]


def find_seconds(pts, leg, q, want):
    """indices of points whose second candidate is evaluated: bisection on the statistic"""
    found, stack = [], [np.arange(len(pts))]
    while stack and len(found) < want:
        idx = stack.pop()
        if seconds(pts[idx], leg, q) == 0:
            continue
        if len(idx) == 1:
            found.append(int(idx[0]))
        else:
            stack += [idx[len(idx) // 2:], idx[:len(idx) // 2]]
    return found


def cloud(rng, leg, q):
    conv = convention(leg, q)
    box = (rng.random((260, 3), dtype=np.float32) * (HI - LO) + LO).astype(np.float32)
    axis = to_body(axis_points(rng, 80), leg, q, conv)
    planes = to_body(plane_points(rng, 160, leg)[0], leg, q, conv)
    far = (rng.random((100, 3), dtype=np.float32) * (HI - LO) + LO).astype(np.float32)
    far[:, 0] += rng.choice(np.array([900.0, 1500.0, 4000.0, 6000.0], np.float32), 100)
    far[::7, 1] *= np.float32(6.0)
    pool = (rng.random((60000, 3), dtype=np.float32) * (HI - LO) + LO).astype(np.float32)
    _, _, doubt, _ = lrm_amd.dbg_toltab_host(pool, leg, q)
    picked = []
    for bit in KINDS.values():
        picked += list(np.flatnonzero((doubt & bit) != 0)[:12])
    picked += find_seconds(pool, leg, q, 12)
    return np.concatenate([box, axis, planes, far, SPECIAL, pool[np.array(sorted(set(picked)), np.int64)]]).astype(np.float32)


def main():
    out = {}
    kinds_seen, n_second, n_pts = {k: 0 for k in KINDS}, 0, 0
    case = 0
    for legname, factory in (("m2", lrm_amd.get_M2_leg), ("moonbot", lrm_amd.get_moonbot_leg)):
        for ia, az in enumerate(AZIMUTHS):
            for iq, q in enumerate(QUATS):
                leg = factory(az)
                rng = np.random.default_rng(1000 + case)
                case += 1
                pts = cloud(rng, leg, q)
                key = f"{legname}_{ia}_{iq}"
                m, d, doubt, stats = lrm_amd.dbg_toltab_host(pts, leg, q)
                mr, dr, doubtr = lrm_amd.dbg_replay_host(pts, leg, q)
                out[key + "_points"] = pts.view(np.uint32)
                out[key + "_leg"] = np.asarray(leg, np.float32)
                out[key + "_quat"] = np.asarray(q, np.float32)
                out[key + "_tab_flag"], out[key + "_tab_doubt"], out[key + "_tab_vec"] = m, doubt, d.view(np.uint32)
                out[key + "_replay_flag"], out[key + "_replay_doubt"], out[key + "_replay_vec"] = mr, doubtr, dr.view(np.uint32)
                for k, bit in KINDS.items():
                    kinds_seen[k] += int(((doubt & bit) != 0).sum())
                n_second += stats["second_candidates"]
                n_pts += len(pts)
                assert all(((doubt & bit) != 0).any() for bit in KINDS.values()), (key, "a doubt kind is missing")
                assert stats["second_candidates"] > 0, (key, "no second-candidate point")
    path = os.path.join(ROOT, "tests", "golden", "frozen", "tab_point_frozen.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{case} cases, {n_pts} points, doubtful by kind {kinds_seen}, second candidates {n_second}, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
