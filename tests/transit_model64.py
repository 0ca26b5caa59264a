"""An independent float64 model of the PATH of the edge transit calls (include/lrm.h), and nothing else: given the two end
quaternions and bodies of an edge it says where sample s of S must be, and measures how far float32 samples are from it.

The model is geometric, not a restatement of the float32 recipe.  With e1 = qa / |qa| and e2 the unit vector of the part of
+-qb normal to qa (the sign that makes qa . +-qb >= 0), every interior sample must be

* unit:          | |q_s| - 1 |                                        (unit)
* on the arc:    the part of q_s outside span{e1, e2}                 (plane)
                 its angle theta_s = atan2(q_s . e2, q_s . e1) inside [0, Theta], Theta the angle of +-qb      (range)
                 and growing with s: max(0, theta_s - theta_(s+1))    (order)
* at the angle of the exact blend (1 - u) qa + u (+-qb), u = s / (S - 1) in float64: |theta_s - theta64_s|     (angle)

and each body_s must be on the segment from ba to bb: its distance from the line, and its parameter's excess over [0, 1],
both relative to max(|ba|, |bb|, 1) (segment), and its distance from ba + u (bb - ba) on the same scale (body)."""
import numpy as np

KEYS = ("unit", "plane", "range", "order", "angle", "segment", "body")


def random_edges(n, seed=0, max_body=4e6):
    """-> (qa, qb float32 [n, 4] unit, ba, bb float32 [n, 3]): the arc between qa and qb spans 0 to just under 90 degrees of
    quaternion angle (a rotation of 0 to just under 180 degrees), half of the qb are negated (the same rotation the long way
    round in quaternion space); bodies up to max_body mm, 0 to 2000 mm apart, some equal, some far apart"""
    rng = np.random.default_rng(seed)
    qa = rng.standard_normal((n, 4))
    qa /= np.linalg.norm(qa, axis=1, keepdims=True)
    t = rng.standard_normal((n, 4))
    t -= (t * qa).sum(1, keepdims=True) * qa
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    phi = rng.uniform(0.0, np.pi / 2, n) * rng.choice([1.0, 1.0, 1e-2, 1e-4, 0.999999], n)
    phi[::97] = 0.0
    qb = np.cos(phi)[:, None] * qa + np.sin(phi)[:, None] * t
    qb[rng.random(n) < 0.5] *= -1.0
    scale = 10.0 ** rng.uniform(0, np.log10(max_body), n)
    ba = rng.uniform(-1, 1, (n, 3)) * scale[:, None]
    step = rng.uniform(-1, 1, (n, 3)) * rng.choice([0.0, 1.0, 150.0, 2000.0, 1e5], n)[:, None]
    bb = ba + step
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(qa), f(qb), f(ba), f(bb)


def deviations(qa, qb, ba, bb, q32, b32):
    """qa, qb [n, 4], ba, bb [n, 3]: the ends as the call got them (float32); q32 [n, S, 4], b32 [n, S, 3]: the samples under
    test -> dict KEYS -> float64 [n]: the worst over the INTERIOR samples of each edge (the ends are the poses themselves)"""
    qa, qb, ba, bb = (np.asarray(a, np.float64) for a in (qa, qb, ba, bb))
    q, b = np.asarray(q32, np.float64), np.asarray(b32, np.float64)
    n, S = q.shape[:2]
    e1 = qa / np.linalg.norm(qa, axis=1, keepdims=True)
    qb = qb * np.where((qa * qb).sum(1, keepdims=True) < 0, -1.0, 1.0)
    perp = qb - (qb * e1).sum(1, keepdims=True) * e1
    pn = np.linalg.norm(perp, axis=1, keepdims=True)
    arc = pn > 1e-10  # below this the two ends are one direction up to float64 rounding: no plane, Theta = 0
    e2 = np.where(arc, perp / np.where(arc, pn, 1.0), 0.0)
    big = np.arctan2((qb * e2).sum(1), (qb * e1).sum(1))  # Theta
    c1, c2 = (q * e1[:, None, :]).sum(2), (q * e2[:, None, :]).sum(2)
    theta = np.arctan2(c2, c1)
    out = {}
    inner = slice(1, S - 1)
    zero = np.zeros(n)
    worst = lambda a: a[:, inner].max(1) if S > 2 else zero
    out["unit"] = worst(np.abs(np.linalg.norm(q, axis=2) - 1.0))
    out["plane"] = worst(np.linalg.norm(q - c1[..., None] * e1[:, None, :] - c2[..., None] * e2[:, None, :], axis=2))
    out["range"] = worst(np.maximum(0.0, np.maximum(-theta, theta - big[:, None])))
    # order: the ends count too (theta_0 = 0 and theta_(S-1) = Theta by construction of the model)
    th = theta.copy()
    th[:, 0], th[:, S - 1] = 0.0, big
    out["order"] = np.maximum(0.0, th[:, :-1] - th[:, 1:]).max(1)
    u = np.arange(S, dtype=np.float64) / (S - 1)
    m = (1.0 - u)[None, :, None] * qa[:, None, :] + u[None, :, None] * qb[:, None, :]
    theta64 = np.arctan2((m * e2[:, None, :]).sum(2), (m * e1[:, None, :]).sum(2))
    out["angle"] = worst(np.abs(theta - theta64))
    scale = np.maximum(1.0, np.maximum(np.linalg.norm(ba, axis=1), np.linalg.norm(bb, axis=1)))
    seg = bb - ba
    L2 = (seg * seg).sum(1)
    rel = b - ba[:, None, :]
    t = np.where(L2[:, None] > 0, (rel * seg[:, None, :]).sum(2) / np.where(L2 > 0, L2, 1.0)[:, None], 0.0)
    off = np.linalg.norm(rel - t[..., None] * seg[:, None, :], axis=2)
    past = np.maximum(0.0, np.maximum(-t, t - 1.0)) * np.sqrt(L2)[:, None]
    out["segment"] = worst(np.maximum(off, past) / scale[:, None])
    out["body"] = worst(np.linalg.norm(b - (ba[:, None, :] + u[None, :, None] * seg[:, None, :]), axis=2) / scale[:, None])
    return out


def table(edges, samples_of, S):
    """edges = random_edges(...); samples_of(quats, body, ea, eb, S) -> float32 [n, S, 7] (the host or the device build) -> dict
    KEYS -> the worst deviation over all edges"""
    qa, qb, ba, bb = edges
    n = len(qa)
    quats = np.ascontiguousarray(np.concatenate([qa, qb]))
    body = np.ascontiguousarray(np.concatenate([ba, bb]))
    ea, eb = np.arange(n, dtype=np.int32), (n + np.arange(n)).astype(np.int32)
    smp = np.asarray(samples_of(quats, body, ea, eb, S), np.float32).reshape(n, S, 7)
    # the ends are the table's own rows, bit for bit
    assert np.array_equal(smp[:, 0].view(np.uint32), np.concatenate([qa, ba], 1).view(np.uint32))
    assert np.array_equal(smp[:, S - 1].view(np.uint32), np.concatenate([qb, bb], 1).view(np.uint32))
    dev = deviations(qa, qb, ba, bb, smp[..., :4], smp[..., 4:])
    return {k: float(v.max()) for k, v in dev.items()}
