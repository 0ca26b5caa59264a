"""Shared scenes of the pose-edge tests (tests/test_pose_edges_cpu.py, tests/test_gpu_pose_edges.py): pose tables as dicts
{quats, body, pose_live, max_step, min_dot}, the host loop's answer as a dict, and the comparison helpers.  Everything is
generated from seeds; nothing here needs a GPU."""
import numpy as np

F = np.float32
KEYS = ("count", "offsets", "edge_a", "edge_b", "d2", "cos2")
PLACES = (0, 1, 31, 32, 62, 63)  # six places of a wave
PITCH = 50.0


def min_dot(max_turn):
    """float32(cos(max_turn / 2)), as device.pose_edges(max_turn=...) passes it; None = 0: no turn test"""
    return 0.0 if max_turn is None else float(F(np.cos(max_turn / 2.0)))


def case(quats, body, max_step, max_turn=None, pose_live=None):
    """max_turn in radians is what the device call takes, min_dot what the C ABI and the host loop take"""
    quats = np.ascontiguousarray(quats, F).reshape(-1, 4)
    return {"quats": quats, "body": None if body is None else np.ascontiguousarray(body, F).reshape(len(quats), 3),
            "pose_live": None if pose_live is None else np.ascontiguousarray(pose_live, np.uint8), "max_step": float(max_step),
            "max_turn": max_turn, "min_dot": min_dot(max_turn)}


def identity(n):
    q = np.zeros((n, 4), F)
    q[:, 0] = 1
    return q


def morton(ijk):
    """the Morton rank of integer lattice coordinates [n, 3] (10 bits each)"""
    key = np.zeros(len(ijk), np.int64)
    for bit in range(10):
        for ax in range(3):
            key |= ((ijk[:, ax].astype(np.int64) >> bit) & 1) << (3 * bit + ax)
    return np.argsort(key, kind="stable")


def lattice(nx, ny, nz, order="raster", origin=0.0, max_step=PITCH, seed=0):
    """a PITCH mm lattice: with max_step = PITCH the six axis neighbours lie at d2 == step2 bit-exactly (multiples of 50 up to
    2^22 are float32 numbers) and ARE neighbours; order "raster", "morton" or "shuffled" relabels the poses"""
    ijk = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    if order == "morton":
        ijk = ijk[morton(ijk)]
    elif order == "shuffled":
        ijk = ijk[np.random.default_rng(seed).permutation(len(ijk))]
    else:
        assert order == "raster"
    body = (ijk * PITCH + origin).astype(F)
    assert np.array_equal(body.astype(np.float64), ijk * PITCH + origin)
    return case(identity(len(body)), body, max_step)


def lattice_pairs(nx, ny, nz):
    """the unordered axis-neighbour pairs of an nx x ny x nz lattice"""
    return (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)


def yaw_quats(k, of):
    """unit quaternions of `of` equally spaced rotations about z, number k (q[0] the scalar part)"""
    a = 2 * np.pi * np.asarray(k) / of
    q = np.zeros((len(a), 4))
    q[:, 0], q[:, 3] = np.cos(a / 2), np.sin(a / 2)
    return q


def oriented(nx, ny, norient=8, seed=1, flip=True, scale=True):
    """norient yaw orientations per body of an nx x ny lattice, a turn limit of 1.01 steps of the yaw: a pose is linked to
    the adjacent orientations of its own body and of the axis neighbours.  flip: half of the quaternions negated (q and -q are
    one orientation); scale: non-unit quaternions, lengths 0.25 .. 4"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2)
    nb = len(ij)
    body = np.zeros((nb * norient, 3))
    body[:, :2] = np.repeat(ij, norient, axis=0) * PITCH
    q = yaw_quats(np.tile(np.arange(norient), nb), norient)
    if flip:
        q[rng.random(len(q)) < 0.5] *= -1
    if scale:
        q *= rng.uniform(0.25, 4.0, (len(q), 1))
    return case(q, body, PITCH, 1.01 * 2 * np.pi / norient)


def cloud(n, seed, box=600.0, max_step=90.0, max_turn=0.6, spread=0.5):
    """continuous random poses: bodies uniform in a box, orientations a random rotation of at most `spread` radians about a
    random axis, random quaternion lengths and signs"""
    rng = np.random.default_rng(seed)
    body = rng.uniform(0, box, (n, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, spread, n)
    q = np.column_stack([np.cos(ang / 2), axis * np.sin(ang / 2)[:, None]]) * rng.uniform(0.5, 2.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    return case(q, body, max_step, max_turn)


def with_threshold_pairs(c, m, seed):
    """c plus 2m poses that sit ON a threshold up to the rounding of their float32 coordinates, on either side of it: partners
    of poses 0 .. m-1 at max_step mm in a random direction with the same quaternion, and partners of poses m .. 2m-1 30 mm
    away, turned by 2 acos(min_dot) about a random axis (q[0] the scalar part; the angle does not depend on that)"""
    rng = np.random.default_rng(seed + 7000)
    q, b = c["quats"].astype(np.float64), c["body"].astype(np.float64)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    far = b[:m] + unit(rng.normal(size=(m, 3))) * c["max_step"]
    near = b[m:2 * m] + unit(rng.normal(size=(m, 3))) * 30.0
    t = 2.0 * np.arccos(np.float64(F(c["min_dot"])))
    r = np.column_stack([np.full(m, np.cos(t / 2)), unit(rng.normal(size=(m, 3))) * np.sin(t / 2)])
    p = q[m:2 * m]
    turned = np.column_stack([p[:, 0] * r[:, 0] - (p[:, 1:] * r[:, 1:]).sum(1),
                              p[:, :1] * r[:, 1:] + r[:, :1] * p[:, 1:] + np.cross(p[:, 1:], r[:, 1:])])
    return case(np.concatenate([q, q[:m], turned]), np.concatenate([b, far, near]), c["max_step"], c["max_turn"])


def hostile(n=200, seed=3):
    """a dense cloud with NaN / inf body and NaN / inf / zero quaternion at the six places of waves 0 and 1 (and of the last
    wave as far as it goes)"""
    c = cloud(n, seed, box=200.0, max_step=80.0, max_turn=0.8)
    bad_body = [np.nan, np.inf, -np.inf]
    bad_quat = [np.nan, np.inf, 0.0]
    k = 0
    for w in range(0, n, 64):
        for place in PLACES:
            p = w + place
            if p >= n:
                continue
            if k % 2 == 0:
                c["body"][p, k % 3] = bad_body[(k // 2) % 3]
            elif (k // 2) % 3 == 2:
                c["quats"][p] = 0.0
            else:
                c["quats"][p, k % 4] = bad_quat[(k // 2) % 3]
            k += 1
    return c


def dead_mask(n=300, seed=4):
    c = cloud(n, seed, box=250.0, max_step=80.0, max_turn=None)
    c["pose_live"] = (np.random.default_rng(seed).random(n) < 0.6).astype(np.uint8) * np.random.default_rng(seed + 1).choice([1, 255], n).astype(np.uint8)
    return c


def one_point(n=150):
    return case(identity(n), np.full((n, 3), 12.5), 0.0)


def no_body(n=130, seed=6):
    c = cloud(n, seed, max_turn=0.4, spread=1.5)
    c["body"] = None
    return c


SCENES = {
    "lattice_touching": lambda: lattice(7, 6, 5),
    "lattice_just_short": lambda: lattice(7, 6, 5, max_step=float(np.nextafter(F(PITCH), F(0)))),
    "lattice_far": lambda: lattice(7, 6, 5, origin=4.0e6),
    "lattice_morton": lambda: lattice(7, 6, 5, "morton"),
    "lattice_shuffled": lambda: lattice(7, 6, 5, "shuffled"),
    "lattice_diagonal": lambda: lattice(6, 5, 4, "morton", max_step=PITCH * 3 ** 0.5),
    "oriented": lambda: oriented(6, 5),
    "oriented_plain": lambda: oriented(5, 4, flip=False, scale=False),
    "cloud": lambda: cloud(500, 2),
    "hostile": hostile,
    "dead_mask": dead_mask,
    "one_point": one_point,
    "no_body": no_body,
    "all_steps": lambda: {**cloud(140, 7, max_turn=0.5), "max_step": float("inf")},
}


def host(lrm, c, form, **kw):
    """lrm_pose_edges_cpu (counts, then lists at the counts' offsets unless kw says otherwise) -> dict"""
    count, offsets, ea, eb, d2, cos2, written, _ = lrm.pose_edges_cpu(c["quats"], c["body"], c["max_step"], c["min_dot"], c["pose_live"], form, **kw)
    return {"count": count, "offsets": offsets, "edge_a": ea, "edge_b": eb, "d2": d2, "cos2": cos2, "written": written}


def assert_same(got, want, what="", keys=KEYS):
    """bit for bit: the floats compared as their 32-bit patterns"""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert not len(bad), (what, k, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def pair_set(ea, eb):
    return set(zip(np.asarray(ea).tolist(), np.asarray(eb).tolist()))


def permuted(c, perm):
    """the same poses relabelled: new pose i is old pose perm[i]"""
    return {**c, "quats": c["quats"][perm], "body": None if c["body"] is None else c["body"][perm],
            "pose_live": None if c["pose_live"] is None else c["pose_live"][perm]}


def hostile_offsets(count, seed):
    """offset arrays that are not the counts' scan -> list of (name, offsets, capacity).  Only "random" makes segments overlap
    (an overlap holds one of the rows that claim it: its contents are not compared)"""
    n = len(count)
    rng = np.random.default_rng(seed)
    good = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    total = int(good[-1])
    return [("good_cut", good, total // 2), ("good_cut_1", good, 1), ("good_over", good, total + 9),
            ("first_2", np.arange(n + 1, dtype=np.int64) * 2, 2 * n), ("first_2_cut", np.arange(n + 1, dtype=np.int64) * 2, n + 1),
            ("decreasing", good[::-1].copy(), total), ("negative", good - total // 3, total),
            ("random", rng.integers(-50, total + 50, n + 1).astype(np.int64), total),
            ("huge", np.where(np.arange(n + 1) % 2 == 0, np.int64(2) ** 62, -np.int64(2) ** 62), total),
            ("past_the_end", good + total, total), ("saturating", np.minimum(good, total // 4), total), ("zero_capacity", good, 0)]


def expect_rows(h, offsets, capacity, sent):
    """the documented segment rule applied to the whole answer h -> (edge_a, edge_b, d2, cos2 with `sent` outside the segments,
    written)"""
    ea, eb = np.full(capacity, sent, np.int32), np.full(capacity, sent, np.int32)
    d2, cos2 = np.full(capacity, sent, np.float32), np.full(capacity, sent, np.float32)
    written = np.zeros(len(h["count"]), np.int32)
    for p in range(len(h["count"])):
        base, end = int(offsets[p]), min(int(offsets[p + 1]), capacity)
        room = end - base if base >= 0 and end > base else 0
        w = min(int(h["count"][p]), room)
        s = slice(int(h["offsets"][p]), int(h["offsets"][p]) + w)
        ea[base:base + w], eb[base:base + w], d2[base:base + w], cos2[base:base + w] = h["edge_a"][s], h["edge_b"][s], h["d2"][s], h["cos2"][s]
        written[p] = w
    return ea, eb, d2, cos2, written
