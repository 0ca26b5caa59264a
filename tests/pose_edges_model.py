"""Two independent models of the pose-edge relation of include/lrm.h (lrm_pose_edges_cpu / _dev), in numpy alone.

edges32(): the relation in float32 in the stated operation order -- a brute force over every pair, a row at a time, that
produces counts, offsets and lists; the host loop must equal it bit for bit.
edges64(): the geometry the relation stands for, in float64: the true distance of the two bodies and the true angle between
the two rotation matrices (from the normalised quaternions, by atan2 of the sine and cosine of the relative rotation)."""
import numpy as np

F = np.float32


def valid32(quats, body, pose_live):
    """-> (valid bool [n], n_p float32 [n], body float32 [n, 3])"""
    q = np.ascontiguousarray(quats, F).reshape(-1, 4)
    n = len(q)
    b = np.zeros((n, 3), F) if body is None else np.ascontiguousarray(body, F).reshape(n, 3)
    with np.errstate(all="ignore"):
        norm = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        live = np.ones(n, bool) if pose_live is None else np.asarray(pose_live).reshape(n) != 0
        ok = live & np.isfinite(b).all(1) & np.isfinite(norm) & (norm > 0)
    assert norm.dtype == F
    return ok, norm, b


def edges32(quats, body, pose_live, max_step, min_dot, form):
    """-> dict(count int32 [n], offsets int64 [n + 1], edge_a, edge_b int32 [E], d2, cos2 float32 [E]); rows in ascending p,
    ascending q inside a row"""
    q = np.ascontiguousarray(quats, F).reshape(-1, 4)
    n = len(q)
    ok, norm, b = valid32(quats, body, pose_live)
    step2, dot2 = F(max_step) * F(max_step), F(min_dot) * F(min_dot)
    rows_a, rows_b, rows_d, rows_c = [], [], [], []
    count = np.zeros(n, np.int32)
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        for p in np.nonzero(ok)[0]:
            dx, dy, dz = b[:, 0] - b[p, 0], b[:, 1] - b[p, 1], b[:, 2] - b[p, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            c = ((q[p, 0] * q[:, 0] + q[p, 1] * q[:, 1]) + q[p, 2] * q[:, 2]) + q[p, 3] * q[:, 3]
            nn = norm[p] * norm
            near = ok & (d2 <= step2) & (c * c >= dot2 * nn) & ((idx != p) if form else (idx > p))
            assert d2.dtype == F and c.dtype == F and nn.dtype == F
            hit = np.nonzero(near)[0]
            count[p] = len(hit)
            rows_a.append(np.full(len(hit), p, np.int32))
            rows_b.append(hit.astype(np.int32))
            rows_d.append(d2[hit])
            rows_c.append((c[hit] * c[hit]) / nn[hit])
    cat = lambda rows, dt: np.concatenate(rows).astype(dt) if rows else np.zeros(0, dt)
    return {"count": count, "offsets": np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64),
            "edge_a": cat(rows_a, np.int32), "edge_b": cat(rows_b, np.int32), "d2": cat(rows_d, F), "cos2": cat(rows_c, F)}


def rotation64(q):
    """float64 rotation matrices [n, 3, 3] of the normalised quaternions (q[0] taken as the scalar part; the angle BETWEEN two
    rotations does not depend on which component is: the scalar part of conj(p) q is the 4-vector dot product either way)"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def pairs64(quats, body, p):
    """-> (distance [n], angle [n]) in float64 of pose p against every pose: |body_q - body_p| and the angle of R_p^T R_q"""
    b = np.asarray(body, np.float64)
    R = rotation64(quats)
    dist = np.sqrt(((b - b[p]) ** 2).sum(1))
    rel = np.einsum("ji,njk->nik", R[p], R)
    cos = (np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0
    sin = 0.5 * np.sqrt((rel[:, 2, 1] - rel[:, 1, 2]) ** 2 + (rel[:, 0, 2] - rel[:, 2, 0]) ** 2 + (rel[:, 1, 0] - rel[:, 0, 1]) ** 2)
    return dist, np.arctan2(sin, cos)
