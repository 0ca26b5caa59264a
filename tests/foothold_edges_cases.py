"""Shared cases of the pose-transition foothold tests (tests/test_foothold_edges_cpu.py, tests/test_gpu_foothold_edges.py):
pose tables in which every pose has a neighbour 50-150 mm away, edge lists over them, and a brute force that skips
nothing, built on the oracle's reachability_global alone: the masks of footholds_posed_cases.brute for the two poses of
an edge, ANDed, with count / argmin in numpy and d2 = d2_a + d2_b as one float32 add (no contraction, first occurrence of
the minimum among the common targets)."""
import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

MAX_TRIPLES = fc.MAX_TRIPLES  # per oracle brute force, counted over the poses the edges name


def with_neighbours(quats, body, seed, lo=50.0, hi=150.0):
    """-> (quats [2n, 4], body [2n, 3]): pose n + i is pose i moved by lo..hi mm (any horizontal direction, up to a fifth
    of that vertically).  Even i keep their quaternion, odd i take pose i + 1's: an edge (i, n + i) then joins two unit
    poses, a unit and a non-unit or nan one, or two non-unit ones, as the pool of footholds_posed_cases.pose_quats has it."""
    rng = np.random.default_rng(seed + 500)
    n = len(quats)
    ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(lo, hi, n)
    off = np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rad * rng.uniform(-0.2, 0.2, n)])
    q2 = quats.copy()
    q2[1::2] = np.roll(quats, -1, axis=0)[1::2]
    return (np.ascontiguousarray(np.concatenate([quats, q2]), np.float32),
            np.ascontiguousarray(np.concatenate([body, (body.astype(np.float64) + off).astype(np.float32)]), np.float32))


def edges_of(nbase, seed, extra=True):
    """(edge_a, edge_b) int32 over a table of with_neighbours: every pose to its neighbour; with extra also a tenth of
    them reversed, a few a == b edges on both halves, a few duplicates and a few random pairs (mostly far apart)"""
    rng = np.random.default_rng(seed + 900)
    a, b = np.arange(nbase), nbase + np.arange(nbase)
    if extra:
        k = max(1, nbase // 10)
        rev = rng.choice(nbase, k, replace=False)
        same = rng.integers(0, 2 * nbase, k)
        dup = rng.choice(nbase, k, replace=False)
        ra, rb = rng.integers(0, 2 * nbase, k), rng.integers(0, 2 * nbase, k)
        a = np.concatenate([a, nbase + rev, same, dup, ra])
        b = np.concatenate([b, rev, same, nbase + dup, rb])
    return np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)


def scene(lrm, nbase, nt, seed, kind="rough", extra=True):
    """(quats, body, targets, edge_a, edge_b): footholds_posed_cases.scene's poses and cloud, every pose with a neighbour"""
    quats, body, targets = fc.scene(lrm, nbase, nt, seed, kind)
    quats, body = with_neighbours(quats, body, seed)
    return (quats, body, targets) + edges_of(nbase, seed, extra)


def brute(oracle, targets, quats, body, legs, nominal_w, edge_a, edge_b):
    """-> dict(count, best int32[L, E], best_d2 float32[L, E], all_legs uint8[E]) from the oracle alone; nominal_w [P, L, 3]
    as the table holds it.  An edge with an index outside [0, P) gets 0, -1, +inf, 0."""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    ea, eb = np.asarray(edge_a, np.int64), np.asarray(edge_b, np.int64)
    nl, ne, nt, npz = len(legs), len(ea), len(targets), len(quats)
    valid = (ea >= 0) & (ea < npz) & (eb >= 0) & (eb < npz)
    used = np.unique(np.concatenate([ea[valid], eb[valid]]))
    assert nl * len(used) * nt <= MAX_TRIPLES, "brute force too large"
    count = np.zeros((nl, ne), np.int32)
    best = np.full((nl, ne), -1, np.int32)
    best_d2 = np.full((nl, ne), np.inf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        mask = {}
        for p in used:
            rel = (targets - body[p]).astype(np.float32)  # one f32 subtraction per component
            mask[p] = [oracle.reach(rel, legs[l], quats[p]).astype(bool) if nt else np.zeros(0, bool) for l in range(nl)]

        def d2_of(p, l, idx):
            c = (body[p] + nominal_w[p, l]).astype(np.float32)  # one f32 add per component
            d = (targets[idx] - c).astype(np.float32)
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

        for e in np.nonzero(valid)[0]:
            a, b = ea[e], eb[e]
            for l in range(nl):
                idx = np.nonzero(mask[a][l] & mask[b][l])[0]  # ascending
                count[l, e] = len(idx)
                if not len(idx):
                    continue
                d2 = (d2_of(a, l, idx) + d2_of(b, l, idx)).astype(np.float32)  # one f32 add
                mn = d2.min()
                best[l, e] = idx[np.argmax(d2 == mn)]  # the first common target at the minimum
                best_d2[l, e] = mn
    return {"count": count, "best": best, "best_d2": best_d2, "all_legs": ((count > 0).all(0) & valid).astype(np.uint8)}


def host(lrm, targets, quats, body, legs, nominal, edge_a, edge_b):
    count, best, best_d2, all_legs, _ = lrm.foothold_edges_posed_cpu(targets, quats, body, legs, edge_a, edge_b, nominal)
    return {"count": count, "best": best, "best_d2": best_d2, "all_legs": all_legs}


assert_same = fc.assert_same


def assert_not_vacuous(common, count_a, count_b, all_legs, share=0.25):
    """the inputs must make the intersection matter: at least `share` of the (edge, leg) entries hold a common set that is
    neither empty nor one pose's whole set, and the edges are neither all feasible nor all infeasible"""
    proper = (common > 0) & (common < np.minimum(count_a, count_b))
    assert proper.mean() >= share, float(proper.mean())
    assert (all_legs == 1).any() and (all_legs == 0).any()
