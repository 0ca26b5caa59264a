"""An independent float64 model of the FOOT PATH and of the point-to-polyline distance of the swing transit calls
(include/lrm.h), and nothing else: given the float32 inputs of a swinging (edge, leg) -- the two footholds, lift, up, the
sample count -- it says where the foot is at sample s and how far a terrain target is from the polyline through those points.

It shares no code with the library or with swing_cases.path_np: the path is the parabola A + u (B - A) + 4 lift u (1 - u) up
evaluated in float64 in the caller's frame (not about A), and the distance is the textbook projection onto each segment with
the parameter clipped to [0, 1]; a segment of zero length is a point."""
import numpy as np


def path64(A, B, S, lift, up=None):
    """A, B [n, 3] -> float64 [n, S, 3]: the foot at every sample, in the caller's frame"""
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    up = np.array([0.0, 0.0, 1.0]) if up is None else np.asarray(up, np.float64).reshape(3)
    u = np.arange(S, dtype=np.float64) / (S - 1)
    bump = 4.0 * float(lift) * u * (1.0 - u)
    return A[:, None, :] + u[None, :, None] * (B - A)[:, None, :] + bump[None, :, None] * up[None, None, :]


def segment_dist64(path, t):
    """path float64 [S, 3], t [m, 3] -> float64 [m, S - 1]: the distance of every target from every segment"""
    t = np.asarray(t, np.float64).reshape(-1, 3)
    p0, p1 = path[:-1], path[1:]
    d = p1 - p0
    len2 = (d * d).sum(1)
    rel = t[:, None, :] - p0[None, :, :]
    with np.errstate(all="ignore"):
        par = np.where(len2 > 0, (rel * d[None, :, :]).sum(2) / np.where(len2 > 0, len2, 1.0), 0.0)
    par = np.clip(par, 0.0, 1.0)
    foot = p0[None, :, :] + par[..., None] * d[None, :, :]
    return np.linalg.norm(t[:, None, :] - foot, axis=2)


def tested(S, skip):
    """the tested segments: range(skip, S - 1 - skip), empty when 2 * skip >= S - 1"""
    return range(0, 0) if 2 * skip >= S - 1 else range(skip, S - 1 - skip)


def entry64(targets, ifrom, ito, S, lift, up, skip):
    """-> float64 [nt, ntested]: the distances of one swinging entry, +inf in the rows of its own two footholds"""
    targets = np.asarray(targets, np.float64).reshape(-1, 3)
    ks = list(tested(S, skip))
    d = segment_dist64(path64(targets[ifrom], targets[ito], S, lift, up)[0], targets)[:, ks]
    d[[ifrom, ito]] = np.inf
    return d


def corpus(n, seed, max_coord=4e6):
    """n swinging entries with a probe target each -> (targets float32 [3n, 3]: from, to, probe per entry; lift; up): steps of
    0 to 600 mm (some of zero length), footholds up to max_coord mm from the origin, entries 5 m or more apart, probes 0 to
    120 mm from a random point of the path, some exactly on it"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(0, np.log10(max_coord), n)
    A = rng.uniform(-1, 1, (n, 3)) * scale[:, None] + np.arange(n)[:, None] * 5000.0
    step = rng.uniform(-1, 1, (n, 3)) * rng.choice([0.0, 1.0, 30.0, 150.0, 600.0], n)[:, None]
    step[:, 2] *= 0.2
    B = A + step
    lift = float(rng.choice([-40.0, 0.0, 20.0, 80.0, 250.0]))
    up = None if seed % 2 == 0 else np.array([0.1, -0.2, 0.97], np.float32)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    A, B = f(A), f(B)
    u = rng.uniform(0, 1, n)
    upv = np.array([0.0, 0.0, 1.0]) if up is None else up.astype(np.float64)
    on = A.astype(np.float64) + u[:, None] * (B.astype(np.float64) - A) + (4 * lift * u * (1 - u))[:, None] * upv[None, :]
    off = rng.standard_normal((n, 3))
    off *= (rng.uniform(0, 120, n) * rng.choice([0.0, 1.0, 1.0, 1.0], n) / np.linalg.norm(off, axis=1))[:, None]
    T = np.empty((3 * n, 3), np.float32)
    T[0::3], T[1::3], T[2::3] = A, B, f(on + off)
    return T, lift, up
