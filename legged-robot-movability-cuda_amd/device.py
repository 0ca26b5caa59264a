"""Device-resident entry points on torch CUDA(ROCm) tensors.  torch only owns the memory and
the stream; every computation is a liblrm.so kernel launched on torch's current stream."""
import math

import numpy as np

from . import _capi


def _torch():
    import torch
    return torch


def _dp(t):
    return None if t is None else t.data_ptr()


def _stream(ref=None):
    """torch's current stream ON THE DEVICE OF THE INPUTS (not on whatever device is current)"""
    torch = _torch()
    return torch.cuda.current_stream(ref.device if ref is not None else None).cuda_stream


def _check_f32(*ts):
    torch = _torch()
    n = ts[0].numel()
    dev = ts[0].device
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == dev):
            raise ValueError("expected contiguous float32 CUDA tensors of equal length on one device")
    return n


def _check_out(t, ref, dtype, numel, what):
    """Caller-supplied outputs go to the kernels as raw pointers: a short, strided, mistyped or other-device tensor
    would be an out-of-bounds device write."""
    if t is None:
        return
    if not (t.is_cuda and t.device == ref.device and t.dtype == dtype and t.is_contiguous() and t.numel() >= numel):
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of >= {numel} elements on {ref.device}")


def _check_field(out, ref, n):
    """(3, n) distance field whose three rows are each contiguous (row stride may exceed n: a view of a wider buffer)"""
    torch = _torch()
    if not (out.is_cuda and out.device == ref.device and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == 3
            and out.shape[1] >= n and (out.shape[1] <= 1 or out.stride(1) == 1)):
        raise ValueError(f"distance field: expected a float32 (3, >= {n}) tensor with contiguous rows on {ref.device}")


def _out(t, ref, shape, dtype, what, want=True):
    """An output: allocated next to ref when the caller gives none (left None with want=False: the kernel gets NULL),
    else checked as _check_out does -- at least prod(shape) elements, not that shape: callers pass longer buffers"""
    if t is None:
        return _torch().empty(shape, dtype=dtype, device=ref.device) if want else None
    _check_out(t, ref, dtype, shape if isinstance(shape, int) else math.prod(shape), what)
    return t


def _out_field(t, ref, n):
    """_out for a (3, n) float32 field"""
    if t is None:
        return _torch().empty((3, n), dtype=_torch().float32, device=ref.device)
    _check_field(t, ref, n)
    return t


def _check_in(t, ref, dtype, numel, what):
    """Optional device inputs (live_in, pose_live, pose_idx, leg_idx, edge_a, edge_b, count, target_idx) go to the kernels
    as raw pointers too: None, or on ref's device, of that dtype, contiguous, at least numel entries"""
    _check_out(t, ref, dtype, numel, what)


def _one_per(n, what, *ts):
    if any(t is not None and t.numel() != n for t in ts):
        raise ValueError(what)


def _launch(name, ref, *args):
    """One stream-ordered call of liblrm.so on ref's device: torch's current stream there is the last argument"""
    with _torch().cuda.device(ref.device):
        _capi.check(getattr(_capi.load(), name)(*args, _stream(ref)))


def _leg(leg):
    return np.ascontiguousarray(leg, dtype=np.float32).reshape(-1)


def _legs(legs):
    return np.ascontiguousarray(legs, dtype=np.float32).reshape(-1, 14)


def _q(quat):
    return None if quat is None else np.ascontiguousarray(quat, dtype=np.float32).reshape(4)


def _radius3(radius):
    radius = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
    if len(radius) != 3:
        raise ValueError("radius: three values (coxa, femur, tibia link)")
    return radius


def _check_poses(quats, body):
    """the tensors given to PoseSet.update(), as the calls without a table take them -> nposes"""
    torch = _torch()
    if not (quats.is_cuda and quats.dtype == torch.float32 and quats.dim() == 2 and quats.shape[1] == 4 and quats.is_contiguous()):
        raise ValueError("quats: expected a contiguous float32 CUDA tensor of shape (nposes, 4)")
    nposes = quats.shape[0]
    if body is not None and not (body.is_cuda and body.device == quats.device and body.dtype == torch.float32 and body.is_contiguous()
                                 and tuple(body.shape) == (nposes, 3)):
        raise ValueError("body: expected a contiguous float32 tensor of shape (nposes, 3) on the poses' device")
    return nposes


def _check_targets(nt, tx, ref):
    if nt and tx.device != ref.device:
        raise ValueError("targets and poses must live on one device")


def _check_edges(ref, edge_a, edge_b):
    """-> nedges"""
    ne = edge_a.numel()
    _check_in(edge_a, ref, _torch().int32, ne, "edge_a")
    _check_in(edge_b, ref, _torch().int32, ne, "edge_b")
    _one_per(ne, "edge_a / edge_b: one pose index each per edge", edge_b)
    return ne


def _check_feet(foot, ref, shape, what):
    """the int32 (nlegs, nedges) target indices of the transit calls"""
    if not (foot.is_cuda and foot.device == ref.device and foot.dtype == _torch().int32 and foot.dim() == 2 and foot.is_contiguous()
            and tuple(foot.shape) == shape):
        raise ValueError(f"{what}: expected a contiguous int32 tensor of shape ({shape[0]}, {shape[1]}) on the poses' device")


def _check_transit(tx, ty, tz, quats, body, legs, edge_a, edge_b):
    """what edge_transit() and swing_transit() take alike -> (nt, nposes, legs float32 (nlegs, 14), nedges)"""
    nt = _check_f32(tx, ty, tz)
    nposes = _check_poses(quats, body)
    _check_targets(nt, tx, quats)
    legs = _legs(legs)
    if not 1 <= len(legs) <= 8:
        raise ValueError("legs: 1 to 8 legs")
    return nt, nposes, legs, _check_edges(quats, edge_a, edge_b)


def reach(x, y, z, leg, quat=None, out=None, bits=None, want_bits=False):
    """mask[i] = reachability_global(point i) (one byte per point); optionally also the
    ballot bit mask (int64 words, bit i&63 of word i>>6)."""
    torch = _torch()
    n = _check_f32(x, y, z)
    out = _out(out, x, n, torch.uint8, "mask")
    bits = _out(bits, x, (n + 63) // 64, torch.int64, "bit words", want_bits)
    leg, q = _leg(leg), _q(quat)
    if bits is not None:
        _launch("lrm_reach_bits_dev", x, _dp(x), _dp(y), _dp(z), n, _capi._ptr(leg), _capi._ptr(q), _dp(out), _dp(bits))
        return out, bits
    _launch("lrm_reach_dev", x, _dp(x), _dp(y), _dp(z), n, _capi._ptr(leg), _capi._ptr(q), _dp(out))
    return out


def dist(x, y, z, leg, quat=None, out=None, valid=None, want_valid=True):
    n = _check_f32(x, y, z)
    out = _out_field(out, x, n)
    valid = _out(valid, x, n, _torch().uint8, "validity bytes", want_valid)
    leg, q = _leg(leg), _q(quat)
    _launch("lrm_dist_dev", x, _dp(x), _dp(y), _dp(z), n, _capi._ptr(leg), _capi._ptr(q), _dp(out[0]), _dp(out[1]), _dp(out[2]),
            _dp(valid))
    return out, valid


def reach_dist(x, y, z, leg, quat=None, mask=None, out=None, bits=None):
    """One launch: reach mask (bytes and/or ballot bit words) + distance field (3, n)."""
    torch = _torch()
    n = _check_f32(x, y, z)
    out = _out_field(out, x, n)
    mask = _out(mask, x, n, torch.uint8, "mask", want=bits is None)
    bits = _out(bits, x, (n + 63) // 64, torch.int64, "bit words", want=False)
    leg, q = _leg(leg), _q(quat)
    _launch("lrm_reach_dist_bits_dev", x, _dp(x), _dp(y), _dp(z), n, _capi._ptr(leg), _capi._ptr(q), _dp(mask), _dp(bits),
            _dp(out[0]), _dp(out[1]), _dp(out[2]))
    if bits is not None:
        return mask, out, bits
    return mask, out


def ik(x, y, z, leg, quat=None, seed=None, out=None, status=None):
    """Joint angles (coxa, femur, tibia) that put the tip on each point, or as near as the joint limits allow, and the
    LRM_IK_* status byte of each (include/lrm.h).  seed: None (mid-range of the limits) or three float32 tensors
    (coxa, femur, tibia) of the points' length.  -> (angles (3, n) float32, status uint8[n]); one launch."""
    n = _check_f32(x, y, z)
    if seed is not None:
        if len(seed) != 3:
            raise ValueError("seed: three tensors (coxa, femur, tibia) or None")
        if _check_f32(x, *seed) != n:
            raise ValueError("seed: one angle per point")
    out = _out_field(out, x, n)
    status = _out(status, x, n, _torch().uint8, "status")
    leg, q = _leg(leg), _q(quat)
    sc, sf, st = (None, None, None) if seed is None else seed
    _launch("lrm_ik_dev", x, _dp(x), _dp(y), _dp(z), n, _capi._ptr(leg), _capi._ptr(q), _dp(sc), _dp(sf), _dp(st), _dp(out[0]),
            _dp(out[1]), _dp(out[2]), _dp(status))
    return out, status


def fk(coxa, femur, tibia, leg, quat=None, out=None):
    """Tip positions (3, n) of joint angles, the inverse of the frame chain ik() solves in; one launch."""
    n = _check_f32(coxa, femur, tibia)
    out = _out_field(out, coxa, n)
    leg, q = _leg(leg), _q(quat)
    _launch("lrm_fk_dev", coxa, _dp(coxa), _dp(femur), _dp(tibia), n, _capi._ptr(leg), _capi._ptr(q), _dp(out[0]), _dp(out[1]),
            _dp(out[2]))
    return out


def reach_any(bx, by, bz, tx, ty, tz, legs, quat=None, out=None, all_legs=None):
    """out[l, b] = any target reachable by leg l from body b (legs used as given);
    all_legs[b] = AND over legs."""
    torch = _torch()
    nb = _check_f32(bx, by, bz)
    nt = _check_f32(tx, ty, tz)
    legs, q = _legs(legs), _q(quat)
    out = _out(out, bx, (len(legs), nb), torch.uint8, "per-leg results")
    all_legs = _out(all_legs, bx, nb, torch.uint8, "per-body results")
    if nt and tx.device != bx.device:
        raise ValueError("bodies and targets must live on one device")
    _launch("lrm_reach_any_dev", bx, _dp(bx), _dp(by), _dp(bz), nb, _dp(tx), _dp(ty), _dp(tz), nt, _capi._ptr(legs), len(legs),
            _capi._ptr(q), _dp(out), _dp(all_legs))
    return out, all_legs


def footholds(bx, by, bz, tx, ty, tz, legs, quat=None, nominal=None, count=None, best=None, best_d2=None):
    """lrm_footholds_dev: count[l, b] = targets leg l reaches from body b, best[l, b] = the reachable target nearest
    body b + nominal[l] (-1 if none), best_d2[l, b] = its squared distance (+inf if none); legs used as given,
    nominal (nlegs, 3) on the host or None = zero.  -> (count int32, best int32, best_d2 float32), each [nlegs, nb]"""
    torch = _torch()
    nb = _check_f32(bx, by, bz)
    nt = _check_f32(tx, ty, tz)
    legs, q = _legs(legs), _q(quat)
    nom = None if nominal is None else np.ascontiguousarray(nominal, dtype=np.float32).reshape(len(legs), 3)
    shape = (len(legs), nb)
    count = _out(count, bx, shape, torch.int32, "per-leg counts")
    best = _out(best, bx, shape, torch.int32, "per-leg choices")
    best_d2 = _out(best_d2, bx, shape, torch.float32, "per-leg squared distances")
    if nt and tx.device != bx.device:
        raise ValueError("bodies and targets must live on one device")
    _launch("lrm_footholds_dev", bx, _dp(bx), _dp(by), _dp(bz), nb, _dp(tx), _dp(ty), _dp(tz), nt, _capi._ptr(legs), len(legs),
            _capi._ptr(q), _capi._ptr(nom), _dp(count), _dp(best), _dp(best_d2))
    return count, best, best_d2


def foothold_offsets(count, out=None):
    """lrm_foothold_offsets_dev: the exclusive scan that turns the counts of footholds() into CSR offsets --
    out[0] = 0, out[k + 1] = out[k] + max(count.view(-1)[k], 0) -> int64 [count.numel() + 1].  One launch, no
    allocation inside, no host synchronisation."""
    torch = _torch()
    n = count.numel()
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()):
        raise ValueError("count: expected a contiguous int32 CUDA tensor")
    out = _out(out, count, n + 1, torch.int64, "offsets")
    _launch("lrm_foothold_offsets_dev", count, _dp(count) if n else None, n, _dp(out))
    return out


def footholds_layout(nb, nlegs, device):
    """(pose_idx int32, leg_idx uint8) of the [l*nb + b] order of both foothold calls with one pose per body: entry
    l*nb + b is (b, l), so that ps.ik(tx, ty, tz, *footholds_layout(nb, nlegs, dev), target_idx=best.view(-1)) solves
    every chosen foothold in one launch.  Two routes lead there:
      * PoseSet(legs, n, ik=True, footholds=True): ps.update(quats, body); ps.footholds(tx, ty, tz) -> best; ps.ik(...)
        on the SAME set.  Every body has its own quaternion, the legs are given unrotated, nominal is in the body frame.
      * footholds() (lrm_footholds_dev, reachable_rotate_leg's convention: one quaternion, legs used as given, measured
        in the clouds' frame): give a second PoseSet those same (already rotated) legs and, per body, the identity
        quaternion and the body position."""
    torch = _torch()
    pose = torch.arange(nb, dtype=torch.int32, device=device).repeat(nlegs)
    leg = torch.arange(nlegs, dtype=torch.uint8, device=device).repeat_interleave(nb)
    return pose, leg


def foothold_edges_layout(nedges, nlegs, device, edge_a, edge_b, which="a"):
    """(pose_idx int32, leg_idx uint8) of the [l*nedges + e] order of PoseSet.foothold_edges for ONE end of every edge:
    entry l*nedges + e is (edge_a[e] or edge_b[e], l), so that
    ps.ik(tx, ty, tz, *foothold_edges_layout(ne, nlegs, dev, ea, eb, "b"), target_idx=best.view(-1)) solves every chosen
    common foothold under the pose the body moves to ("a": the pose it leaves).  edge_a / edge_b: the int32 device tensors
    of the query; an edge whose best is -1 gets ik()'s status 0 (give ik() check=False if the edges hold bad indices)."""
    torch = _torch()
    if which not in ("a", "b"):
        raise ValueError('which: "a" or "b"')
    edge = edge_a if which == "a" else edge_b
    if not (edge.dtype == torch.int32 and edge.numel() == nedges):
        raise ValueError("edge_a / edge_b: int32 tensors of nedges pose indices")
    pose = edge.reshape(-1).to(device).repeat(nlegs)
    leg = torch.arange(nlegs, dtype=torch.uint8, device=device).repeat_interleave(nedges)
    return pose, leg


def foothold_support_layout(nt, nlegs, device, best_pose):
    """(target_idx int32, pose_idx int32, leg_idx uint8, valid bool) of the [l*nt + t] order of PoseSet.foothold_support:
    entry l*nt + t is (target t, pose best_pose[l, t], leg l), so that
    ps.ik(tx, ty, tz, pose_idx, leg_idx, target_idx=target_idx) solves every target under its best pose in one launch.
    Where best_pose is -1 (no pose reaches), valid is False, pose_idx is 0 and target_idx is -1, which ik() answers with
    status 0 and nan angles.  Only tensor operations: no host synchronisation."""
    torch = _torch()
    bp = best_pose.reshape(-1)
    if not (bp.dtype == torch.int32 and bp.numel() == nt * nlegs):
        raise ValueError("best_pose: an int32 tensor of nlegs * nt pose indices")
    bp = bp.to(device)
    valid = bp >= 0
    target = torch.arange(nt, dtype=torch.int32, device=device).repeat(nlegs)
    target = torch.where(valid, target, torch.full_like(target, -1))
    leg = torch.arange(nlegs, dtype=torch.uint8, device=device).repeat_interleave(nt)
    return target, bp.clamp(min=0), leg, valid


def positionability(bx, by, bz, tx, ty, tz, legs, quats, reference_culls=0, active=None, out=None):
    """lrm_positionability_dev: the orientation sweep of robot_full_struct on device-resident clouds and masks.
    reference_culls: 0 none, 2 the per-orientation cylinder culls.  -> (accepted uint8[nb] on the device, kernel ms)"""
    import ctypes as C
    torch = _torch()
    nb = _check_f32(bx, by, bz)
    nt = _check_f32(tx, ty, tz) if tx.numel() else 0
    legs = _legs(legs)
    quats = np.ascontiguousarray(quats, dtype=np.float32).reshape(-1, 4)
    out = _out(out, bx, nb, torch.uint8, "accepted bytes")
    _check_in(active, bx, torch.uint8, nb, "active bytes")
    ms = C.c_float(0)
    with torch.cuda.device(bx.device):
        torch.cuda.synchronize(bx.device)  # the library works on the null stream
        _capi.check(_capi.load().lrm_positionability_dev(_dp(bx), _dp(by), _dp(bz), nb, _dp(tx) if nt else None, _dp(ty) if nt else None,
                                                         _dp(tz) if nt else None, nt, _capi._ptr(legs), len(legs), _capi._ptr(quats),
                                                         len(quats), int(reference_culls), _dp(active), _dp(out), C.addressof(ms)))
    return out, ms.value


def any_in_sphere(cx, cy, cz, tx, ty, tz, radius, out=None):
    nc = _check_f32(cx, cy, cz)
    nt = _check_f32(tx, ty, tz)
    out = _out(out, cx, nc, _torch().uint8, "results")
    _launch("lrm_any_in_sphere_dev", cx, _dp(cx), _dp(cy), _dp(cz), nc, _dp(tx), _dp(ty), _dp(tz), nt, radius, _dp(out))
    return out


def any_in_cylinder(cx, cy, cz, tx, ty, tz, radius, plus_z, minus_z, out=None):
    nc = _check_f32(cx, cy, cz)
    nt = _check_f32(tx, ty, tz)
    out = _out(out, cx, nc, _torch().uint8, "results")
    _launch("lrm_any_in_cylinder_dev", cx, _dp(cx), _dp(cy), _dp(cz), nc, _dp(tx), _dp(ty), _dp(tz), nt, radius, plus_z, minus_z,
            _dp(out))
    return out


def apply_oct_partitioned(x, y, z, leg, settings, exchange):
    """apply_oct with THIS rank's part of the footholds on the device (lrm_apply_oct_partitioned_dev); `exchange` ORs the
    flag words over the ranks.  -> (centres float32[k, 3] on the host, kernel milliseconds)"""
    torch = _torch()
    n = _check_f32(x, y, z) if x.numel() else 0
    with torch.cuda.device(x.device):
        torch.cuda.synchronize(x.device)  # the library works on the null stream
        return _capi.apply_oct_partitioned_dev(_dp(x) if n else None, _dp(y) if n else None, _dp(z) if n else None, n, leg, settings, exchange)


def apply_oct(x, y, z, leg, settings=None, rank=0, world=1, exchange=None):
    """apply_oct on footholds that already live on the device (three float32 tensors); the level loop synchronises the
    device, so this is not a stream-ordered call.  -> (centres float32[k, 3] on the host, kernel milliseconds)"""
    torch = _torch()
    n = _check_f32(x, y, z)
    with torch.cuda.device(x.device):
        torch.cuda.synchronize(x.device)  # the library works on the null stream
        return _capi.apply_oct_dev(_dp(x), _dp(y), _dp(z), n, leg, settings, rank, world, exchange)


def stance_stability(tx, ty, tz, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0,
                     live_in=None, margin=None, edge=None, stable=None, feet=None):
    """lrm_stance_stability_dev: does the robot stand, and which legs can it lift.  A stance s is a pose (pose_idx[s], int32 on
    the device; None: pose s) and one target index per leg, foot int32 [nlegs, nstances]: PoseSet.footholds()'s best as it
    stands, or foothold_edges()'s best with pose_idx = edge_a or edge_b.  quats float32 (nposes, 4) and body float32
    (nposes, 3) or None are the tensors given to update().  com: the centre of mass in the BODY frame (3 host floats, None =
    the body origin); plane: None = gravity along -z of the caller's frame, else two host 3-vectors spanning the plane normal to
    gravity; lift: None = [0], "each" = [0, 1<<0, ..., 1<<(nlegs-1)], or 1 to 256 bit masks (bit l = leg l is in the air).
    margin[m, s] = the distance of the projected centre of mass from the nearest edge of the support polygon of the feet
    planted under lift set m (-inf: fewer than three, a degenerate polygon or a dead stance; negative: outside);
    edge[m, s] = that edge's code i*8 + j (255 with -inf); stable[m, s] = margin > min_margin; feet[s] = the valid feet.
    live_in: uint8 [nstances] on the device, 0 = dead.  -> (margin float32, edge uint8, stable uint8, each [nmasks,
    nstances]; feet uint8 [nstances]).  Every tensor must be contiguous.  stable[m] is directly the live_in / pose_live of the
    other posed calls.  One launch, no allocation beyond missing outputs, no shared buffer: it can be captured in a graph
    and may run next to anything."""
    torch = _torch()
    nt = _check_f32(tx, ty, tz)
    nposes = _check_poses(quats, body)
    _check_targets(nt, tx, quats)
    if not (foot.is_cuda and foot.device == quats.device and foot.dtype == torch.int32 and foot.dim() == 2 and foot.is_contiguous()
            and 1 <= foot.shape[0] <= 8):
        raise ValueError("foot: expected a contiguous int32 tensor of shape (nlegs, nstances), 1 to 8 legs, on the poses' device")
    nl, ns = foot.shape
    _check_in(pose_idx, quats, torch.int32, ns, "pose_idx")
    _check_in(live_in, quats, torch.uint8, ns, "live_in")
    _one_per(ns, "pose_idx / live_in: one entry per stance", pose_idx, live_in)
    if pose_idx is None and ns > nposes:
        raise ValueError("without pose_idx stance s takes pose s: nstances <= nposes")
    com, plane = _capi._stance_host(com, plane)
    lift = _capi.stance_lift(lift, nl)
    nm = len(lift)
    margin = _out(margin, quats, (nm, ns), torch.float32, "margins")
    edge = _out(edge, quats, (nm, ns), torch.uint8, "edge codes")
    stable = _out(stable, quats, (nm, ns), torch.uint8, "stable bytes")
    feet = _out(feet, quats, ns, torch.uint8, "per-stance feet")
    _launch("lrm_stance_stability_dev", quats, _dp(tx), _dp(ty), _dp(tz), nt, _dp(quats), _dp(body), nposes, _dp(pose_idx), _dp(foot),
            ns, nl, _capi._ptr(com), _capi._ptr(plane), _capi._ptr(lift), nm, float(min_margin), _dp(live_in), _dp(margin), _dp(edge),
            _dp(stable), _dp(feet))
    return margin, edge, stable, feet


def stance_loads(workspace, ik_workspace, quats, nlegs, angles, tau_max, pose_idx=None, com=None, plane=None, lift=None, live_in=None,
                 status=None, holdable=None, peak=None, peak_at=None, load=None, tau=None, want_peak_at=True, want_load=True,
                 want_tau=True):
    """lrm_stance_loads_posed_dev: what every planted foot carries and what the coxa, femur and tibia joints must hold, for
    every set and lift set.  workspace / ik_workspace: a PoseSet's pose and IK tables (uint8 tensors) compiled from quats
    float32 (nposes, 4) by update(); a set s is a pose (pose_idx[s], int32 on the device; None: pose s) and one angle triple per
    leg: angles is ik()'s (3, nlegs*nsets) tensor, entry l*nsets + s.  The model: frictionless point contacts that push along
    `up` (the normal u x v of plane, None: +z), massless legs, weight 1 -- loads are fractions of the robot's weight, torques
    load x mm.  com, plane and lift are stance_stability()'s; tau_max: three host floats (coxa, femur, tibia; > 0, inf allowed).
    status[m, s]: 0 dead set, 1 all planted feet carry, 2 some were dropped, 3 a tripod carries, 4 no equilibrium (loads and
    torques nan); holdable[m, s] = status 1..3 and every |tau| <= tau_max; peak[m, s] = the largest |tau| / tau_max (-inf if
    none); peak_at[m, s] = its code l*4 + j (255 if none); load[m, l, s]; tau[m, l, j, s].  Lifted legs and legs with nan
    angles get load 0 and tau 0.  live_in: uint8 [nsets] on the device, 0 = dead.
    -> (status uint8, holdable uint8, peak float32, peak_at uint8 or None, each [nmasks, nsets]; load float32 [nmasks, nlegs,
    nsets] or None; tau float32 [nmasks, nlegs, 3, nsets] or None); want_* False (and no tensor given) pass NULL.  Every tensor
    must be contiguous.  holdable[m] is directly the live_in of the other posed calls.  One launch, no allocation beyond missing
    outputs, no shared buffer: it can be captured in a graph and may run next to anything."""
    torch = _torch()
    nposes = _check_poses(quats, None)
    nl = int(nlegs)
    if not 1 <= nl <= 8:
        raise ValueError("nlegs: 1 to 8 legs")
    for ws, per, what in ((workspace, _capi.POSE_RECORD_BYTES, "workspace"), (ik_workspace, _capi.POSE_IK_RECORD_BYTES, "ik_workspace")):
        if ws is None or not (ws.is_cuda and ws.device == quats.device and ws.dtype == torch.uint8 and ws.is_contiguous()
                              and ws.numel() >= per * nposes * nl):
            raise ValueError(f"{what}: expected a contiguous uint8 tensor of >= {per} * nposes * nlegs bytes on the poses' device")
    if not (angles.is_cuda and angles.device == quats.device and angles.dtype == torch.float32 and angles.dim() == 2
            and angles.shape[0] == 3 and angles.shape[1] % nl == 0 and angles.is_contiguous()):
        raise ValueError(f"angles: expected ik()'s contiguous float32 (3, {nl} * nsets) tensor on {quats.device}")
    ns = angles.shape[1] // nl
    _check_in(pose_idx, quats, torch.int32, ns, "pose_idx")
    _check_in(live_in, quats, torch.uint8, ns, "live_in")
    _one_per(ns, "pose_idx / live_in: one entry per set", pose_idx, live_in)
    if pose_idx is None and ns > nposes:
        raise ValueError("without pose_idx set s takes pose s: nsets <= nposes")
    com, plane = _capi._stance_host(com, plane)
    lift = _capi.stance_lift(lift, nl)
    tau_max = _capi._tau_max(tau_max)
    nm = len(lift)
    status = _out(status, quats, (nm, ns), torch.uint8, "status bytes")
    holdable = _out(holdable, quats, (nm, ns), torch.uint8, "holdable bytes")
    peak = _out(peak, quats, (nm, ns), torch.float32, "peak ratios")
    peak_at = _out(peak_at, quats, (nm, ns), torch.uint8, "peak codes", want_peak_at)
    load = _out(load, quats, (nm, nl, ns), torch.float32, "loads", want_load)
    tau = _out(tau, quats, (nm, nl, 3, ns), torch.float32, "torques", want_tau)
    _launch("lrm_stance_loads_posed_dev", quats, _dp(workspace), _dp(ik_workspace), _dp(quats), nposes, nl, _dp(pose_idx), ns,
            _dp(angles[0]), _dp(angles[1]), _dp(angles[2]), _capi._ptr(com), _capi._ptr(plane), _capi._ptr(lift), nm, _capi._ptr(tau_max),
            _dp(live_in), _dp(status), _dp(holdable), _dp(peak), _dp(peak_at), _dp(load), _dp(tau))
    return status, holdable, peak, peak_at, load, tau


def pose_routes_workspace(nposes, rounds, device):
    """a workspace for pose_routes(): the 64-bit keys and one flag per launch (uint8 tensor; torch aligns it)"""
    nbytes = _capi.load().lrm_pose_routes_workspace_bytes(int(nposes), int(rounds))
    return _torch().empty(max(int(nbytes), 8), dtype=_torch().uint8, device=device)


def pose_routes(nposes, edge_a, edge_b, sources, edge_live=None, pose_live=None, edge_cost=None, direction=0, rounds=64, sync=True,
                workspace=None, cost=None, hops=None, pred_edge=None, pred_pose=None, reached=None, done=None, want_cost=True,
                want_hops=True, want_pred_edge=True, want_pred_pose=True, resume=False):
    """lrm_pose_routes_dev: shortest routes over the pose graph with integer costs -- which poses can be reached from `sources`,
    in how many steps, at what cost and through which transition.  edge_a / edge_b int32 device tensors (the arrays of the
    edge calls); sources int32 on the device; edge_live uint8 [nedges] (a clear or all_legs byte as it stands), pose_live uint8
    [nposes] (a free, stable or holdable row) and edge_cost int32 [nedges] on the device or None (no cost: 1 per edge, cost
    equals hops; a negative cost makes the edge dead); direction 0 an edge serves both ways, 1 a -> b only, 2 b -> a only (with
    the goal as source: the cost to go and the next edge towards the goal).  Any index is safe: an edge with an end out of range
    is dead, such a source is ignored.  cost[p] int64 and hops[p] int32 (-1 unreachable), pred_edge[p] int32 (the smallest usable
    edge with a tight arc into p; -1 for a source or an unreachable pose), pred_pose[p] int32 (that arc's other end, or -1);
    reached int32 [1] (poses with hops >= 0); done int32 [1] (>= 1: the fixed point was proven within `rounds` relaxation
    launches; -1: not yet, the per-pose outputs are unspecified and the workspace holds the state).
    sync=True: the call READS done ON THE HOST (one host synchronisation per call of the library) and calls again with resume = 1
    until the fixed point is proven; the answer is the same bits however the work was cut.  sync=False: ONE call of the library,
    no host synchronisation, done comes back as a tensor for the caller to look at: this form can be captured in a graph (a
    linear chain of init, seed, `rounds` relax and up to three finish launches; pass the workspace and the outputs; the number of
    launches a call needs varies from call to call, rounds >= the deepest route's hops + 1 always suffices, and done tells).  resume=True continues from the workspace's state (sync=False only needs
    it; every other argument as before).  workspace: a uint8 tensor of lrm_pose_routes_workspace_bytes(nposes, rounds) bytes
    (pose_routes_workspace()), allocated when None; calls on different streams need different workspaces and outputs.
    -> (cost, hops, pred_edge, pred_pose, reached, done); want_* False (and no tensor given) pass NULL, not all four.  Every
    tensor must be contiguous.  All atomics are integer min / add: bit-deterministic."""
    torch = _torch()
    nposes, rounds, direction = int(nposes), int(rounds), int(direction)
    if nposes < 0:
        raise ValueError("nposes: >= 0")
    if not 1 <= rounds <= 4096:
        raise ValueError("rounds: 1 to 4096 relaxation launches per call")
    if not edge_a.is_cuda:
        raise ValueError("edge_a: expected an int32 CUDA tensor")
    ref = edge_a
    ne = _check_edges(ref, edge_a, edge_b)
    ns = sources.numel()
    _check_in(sources, ref, torch.int32, ns, "sources")
    _check_in(edge_live, ref, torch.uint8, ne, "edge_live")
    _check_in(edge_cost, ref, torch.int32, ne, "edge_cost")
    _one_per(ne, "edge_live / edge_cost: one entry per edge", edge_live, edge_cost)
    _check_in(pose_live, ref, torch.uint8, nposes, "pose_live")
    _one_per(nposes, "pose_live: one byte per pose", pose_live)
    cost = _out(cost, ref, nposes, torch.int64, "route costs", want_cost)
    hops = _out(hops, ref, nposes, torch.int32, "route hops", want_hops)
    pred_edge = _out(pred_edge, ref, nposes, torch.int32, "predecessor edges", want_pred_edge)
    pred_pose = _out(pred_pose, ref, nposes, torch.int32, "predecessor poses", want_pred_pose)
    if cost is None and hops is None and pred_edge is None and pred_pose is None:
        raise ValueError("pose_routes: no output")
    reached = _out(reached, ref, 1, torch.int32, "reached count")
    done = _out(done, ref, 1, torch.int32, "done word")
    need = _capi.load().lrm_pose_routes_workspace_bytes(nposes, rounds)
    if workspace is None:
        workspace = pose_routes_workspace(nposes, rounds, ref.device)
    _check_out(workspace, ref, torch.uint8, need, "workspace")

    def call(resume):
        _launch("lrm_pose_routes_dev", ref, nposes, _dp(edge_a), _dp(edge_b), ne, _dp(edge_live), _dp(pose_live), _dp(edge_cost),
                _dp(sources), ns, direction, _dp(workspace), rounds, int(resume), _dp(cost), _dp(hops), _dp(pred_edge), _dp(pred_pose),
                _dp(reached), _dp(done))

    call(bool(resume))
    if sync:
        # after relax launch i every pose holds at most the best key over walks of i arcs: nposes launches reach the fixed
        # point and one more proves it
        for _ in range(nposes + 1):
            if int(done.item()) >= 1:
                break
            call(True)
        else:
            raise RuntimeError("pose_routes: no fixed point after nposes + 1 calls")
    return cost, hops, pred_edge, pred_pose, reached, done


def route_path(pred_pose, pred_edge, goal, hops=None):
    """The route to `goal` from pose_routes()'s predecessors, as host lists (poses from the source to the goal, the edges between
    them: len(poses) == len(edges) + 1).  Copies the arrays to the host (a synchronisation).  hops: pose_routes()'s hops; with
    it an unreached goal raises ValueError (the predecessors alone are -1 for a source and for an unreached pose alike, so
    without it a goal with no predecessor counts as a source) and the length is checked."""
    pp = pred_pose.detach().cpu().numpy() if hasattr(pred_pose, "detach") else np.asarray(pred_pose)
    pe = pred_edge.detach().cpu().numpy() if hasattr(pred_edge, "detach") else np.asarray(pred_edge)
    goal = int(goal)
    if not 0 <= goal < len(pp) or len(pe) != len(pp):
        raise ValueError("route_path: goal outside the poses, or predecessor arrays of different lengths")
    want = None
    if hops is not None:
        want = int(hops[goal].item() if hasattr(hops, "detach") else hops[goal])
        if want < 0:
            raise ValueError(f"route_path: pose {goal} is not reached")
    poses, edges, p = [goal], [], goal
    while pp[p] >= 0:
        if len(edges) >= len(pp):
            raise ValueError("route_path: the predecessors form a cycle (an unfinished answer?)")
        edges.append(int(pe[p]))
        p = int(pp[p])
        poses.append(p)
    if want is not None and want != len(edges):
        raise ValueError("route_path: the predecessors do not match hops (an unfinished answer?)")
    return poses[::-1], edges[::-1]


def pose_edges_workspace(nposes, device):
    """a workspace for pose_edge_counts() / pose_edges(): one bounding box per chunk of 64 poses and one per 64 chunks (uint8
    tensor; torch aligns it)"""
    nbytes = _capi.load().lrm_pose_edges_workspace_bytes(int(nposes))
    return _torch().empty(int(nbytes), dtype=_torch().uint8, device=device)


_EDGE_FORMS = {"upper": 0, "full": 1}


def _pose_edges_args(quats, body, max_step, max_turn, pose_live, form, workspace):
    """what pose_edge_counts() and pose_edges() take alike -> (nposes, max_step, min_dot, form 0 / 1, workspace)"""
    torch = _torch()
    nposes = _check_poses(quats, body)
    if form not in _EDGE_FORMS:
        raise ValueError('form: "upper" (q > p: every pair once) or "full" (q != p: an adjacency list)')
    max_step = float(max_step)
    if not max_step >= 0.0:
        raise ValueError("max_step: mm, >= 0 (inf allowed)")
    _check_in(pose_live, quats, torch.uint8, nposes, "pose_live")
    _one_per(nposes, "pose_live: one byte per pose", pose_live)
    need = _capi.load().lrm_pose_edges_workspace_bytes(nposes)
    if workspace is None:
        workspace = pose_edges_workspace(nposes, quats.device)
    _check_out(workspace, quats, torch.uint8, need, "workspace")
    return nposes, max_step, _capi.pose_edges_min_dot(max_turn), _EDGE_FORMS[form], workspace


def pose_edge_counts(quats, body, max_step, max_turn=None, pose_live=None, form="upper", workspace=None, count=None):
    """lrm_pose_edge_counts_dev: count[p] = the neighbour poses of pose p within a step and a turn (pose_edges() has the
    relation); form "upper" counts the neighbours q > p, "full" all q != p.  quats float32 (nposes, 4) and body float32
    (nposes, 3) or None on the device, as PoseSet.update() takes them; pose_live uint8 [nposes] or None.  Three launches (the
    chunk boxes, the group boxes, the walk), no allocation with a workspace and count given, no host synchronisation.  -> count int32 [nposes]"""
    torch = _torch()
    nposes, max_step, min_dot, form, workspace = _pose_edges_args(quats, body, max_step, max_turn, pose_live, form, workspace)
    count = _out(count, quats, nposes, torch.int32, "per-pose counts")
    _launch("lrm_pose_edge_counts_dev", quats, _dp(quats), _dp(body), nposes, _dp(pose_live), max_step, min_dot, form, _dp(workspace),
            _dp(count))
    return count


def pose_edges(quats, body, max_step, max_turn=None, pose_live=None, form="upper", count=None, offsets=None, capacity=None, workspace=None,
               edge_a=None, edge_b=None, d2=None, cos2=None, written=None, want_d2=True, want_cos2=True):
    """lrm_pose_edges_dev: which pose can step to which -- the edge_a / edge_b every edge call takes, built on the device from
    the poses alone, in CSR form.  Poses p != q are NEIGHBOURS iff both are valid (live, finite body, squared quaternion norm
    finite and > 0), their bodies are at most max_step mm apart and their orientations at most max_turn radians (None: no turn
    test; q and -q are one orientation); the float32 arithmetic is include/lrm.h's, symmetric bit for bit, and the answer is the
    host loop's bit for bit.  form "upper": row p holds the neighbours q > p, every unordered pair once (what routes() with
    direction = 0 wants); "full": all q != p, an adjacency list.  Row p lies at offsets[p] in ascending q, as far as
    min(offsets[p + 1], capacity) leaves room (foothold_lists()'s segment rule: any offsets are memory-safe, nothing outside a
    segment is written); edge_a = p, edge_b = q, d2 = the squared distance, cos2 = the squared cosine of half the turn,
    written[p] = the entries stored.  With offsets from the counts and room for all, the list is sorted by (a, b).
      * offsets=None: count=None runs pose_edge_counts() first, then foothold_offsets(count).
      * capacity=None and edge_a=None: offsets[-1] is read back to allocate exactly that -- ONE host synchronisation.
      * with a capacity (or a preallocated edge_a: capacity = its length) the call ONLY LAUNCHES, and an edge_a it allocates
        comes back prefilled with -1 beyond the written part: pass edge_a, edge_b and nedges = capacity to the edge calls, which
        treat an end outside [0, nposes) as a dead edge -- no read-back of offsets[-1], and counts -> offsets -> edges can be
        captured in a graph (pass the workspace and every output; prefill edge_a yourself).  A row that does not fit is cut short and written says so.
    Calls on different streams need different workspaces (pose_edges_workspace()).  Clouds in Morton order make the chunk boxes
    tight and the call fast; the answer does not depend on the order.
    -> (edge_a int32, edge_b int32, offsets int64 [nposes + 1], d2, cos2 float32 or None, written int32 [nposes])"""
    torch = _torch()
    form_name = form
    nposes, max_step, min_dot, form, workspace = _pose_edges_args(quats, body, max_step, max_turn, pose_live, form, workspace)
    if offsets is None:
        if count is None:
            count = pose_edge_counts(quats, body, max_step, max_turn, pose_live, form_name, workspace)
        _check_in(count, quats, torch.int32, nposes, "per-pose counts")
        offsets = foothold_offsets(count.view(-1)[:nposes])
    _check_in(offsets, quats, torch.int64, nposes + 1, "offsets")
    if capacity is None:
        capacity = edge_a.numel() if edge_a is not None else max(int(offsets[nposes].item()), 0)  # the one synchronisation
    capacity = int(capacity)
    if capacity < 0:
        raise ValueError("capacity >= 0")
    if edge_a is None:
        edge_a = torch.full((capacity,), -1, dtype=torch.int32, device=quats.device)
    _check_out(edge_a, quats, torch.int32, capacity, "edge_a")
    edge_b = _out(edge_b, quats, capacity, torch.int32, "edge_b")
    d2 = _out(d2, quats, capacity, torch.float32, "edge squared distances", want_d2)
    cos2 = _out(cos2, quats, capacity, torch.float32, "edge squared half-turn cosines", want_cos2)
    written = _out(written, quats, nposes, torch.int32, "per-pose written counts")
    # capacity 0: nothing but written is stored, but the C ABI refuses NULL lists first and an empty tensor has no address
    pa, pb = (_dp(edge_a), _dp(edge_b)) if capacity else (_dp(workspace), _dp(workspace))
    _launch("lrm_pose_edges_dev", quats, _dp(quats), _dp(body), nposes, _dp(pose_live), max_step, min_dot, form, _dp(workspace),
            _dp(offsets), capacity, pa, pb, _dp(d2), _dp(cos2), _dp(written))
    return edge_a, edge_b, offsets, d2, cos2, written


def edge_transit(tx, ty, tz, quats, body, legs, edge_a, edge_b, foot, nsamples=9, live_in=None, mask=None, reached=None,
                 first_miss=None, worst=None, worst_d2=None, planted=None, clear=None, advance=None):
    """lrm_edge_transit_posed_dev: does a planted foot stay reachable while the body moves from pose edge_a[e] to pose edge_b[e].
    foothold_edges() looks at the two ends of an edge only; this call samples nsamples poses between them, the ends included:
    the normalised linear blend of the two quaternions (the short way round: the great arc of slerp at another speed) and the
    linear blend of the bodies.  quats float32 (nposes, 4) and body float32 (nposes, 3) or None are the tensors given to
    update(); legs the host legs (1 to 8); edge_a / edge_b int32 device tensors; foot int32 [nlegs, nedges] on the device:
    foothold_edges()'s best as it stands (-1 = the leg is in the air).  No table is read or written.
    mask[l, e] (int64; bit s = sample s reaches), reached[l, e] (the number of bits; -1 when not planted), first_miss[l, e] (-1 if
    none), worst[l, e] (the unreachable sample with the largest squared distance vector; -1 if none), worst_d2[l, e] (0 if none);
    planted[e] (bit l = leg l is planted), clear[e] (1 iff live, both ends in range and every planted leg reaches at every
    sample), advance[e] (the number of leading samples at which every planted leg reaches; 0 for a dead edge).
    live_in: uint8 [nedges] on the device, 0 = dead.  Any index in edge_a, edge_b and foot is safe: one outside its range
    makes the edge dead or the leg unplanted.  -> (mask, reached, first_miss, worst, worst_d2, planted, clear, advance); clear
    is directly the live_in of the other posed calls.  Every tensor must be contiguous.  One launch, no allocation beyond
    missing outputs, no shared buffer: it can be captured in a graph and may run next to anything."""
    torch = _torch()
    nt, nposes, legs, ne = _check_transit(tx, ty, tz, quats, body, legs, edge_a, edge_b)
    shape = (len(legs), ne)
    _check_feet(foot, quats, shape, "foot")
    _check_in(live_in, quats, torch.uint8, ne, "live_in")
    _one_per(ne, "live_in: one byte per edge", live_in)
    nsamples = _capi._nsamples(nsamples)
    mask = _out(mask, quats, shape, torch.int64, "per-leg sample masks")
    reached = _out(reached, quats, shape, torch.int32, "per-leg reached counts")
    first_miss = _out(first_miss, quats, shape, torch.int32, "per-leg first misses")
    worst = _out(worst, quats, shape, torch.int32, "per-leg worst samples")
    worst_d2 = _out(worst_d2, quats, shape, torch.float32, "per-leg worst squared distances")
    planted = _out(planted, quats, ne, torch.uint8, "per-edge planted bits")
    clear = _out(clear, quats, ne, torch.uint8, "per-edge clear bytes")
    advance = _out(advance, quats, ne, torch.int32, "per-edge advances")
    _launch("lrm_edge_transit_posed_dev", quats, _dp(tx), _dp(ty), _dp(tz), nt, _dp(quats), _dp(body), nposes, _capi._ptr(legs),
            len(legs), _dp(edge_a), _dp(edge_b), ne, _dp(foot), nsamples, _dp(live_in), _dp(mask), _dp(reached), _dp(first_miss),
            _dp(worst), _dp(worst_d2), _dp(planted), _dp(clear), _dp(advance))
    return mask, reached, first_miss, worst, worst_d2, planted, clear, advance


def swing_layout(best, edge_a, edge_b, lift_mask):
    """(foot_from, foot_to) int32 [nlegs, nedges] for swing_transit() from PoseSet.footholds()'s best [nlegs, nposes]: leg l of
    edge e leaves best[l, edge_a[e]] and lands on best[l, edge_b[e]] where bit l of lift_mask[e] (uint8 device tensor, nedges)
    is set, and gets -1 / -1 (not swinging: a planted leg, edge_transit()'s business) where it is clear or where an end lies
    outside [0, nposes) (a dead edge).  edge_a / edge_b: int32 device tensors.  Only tensor operations: no host
    synchronisation."""
    torch = _torch()
    if not (best.dtype == torch.int32 and best.dim() == 2 and 1 <= best.shape[0] <= 8):
        raise ValueError("best: the int32 (nlegs, nposes) tensor of footholds()")
    nl, ne = best.shape[0], edge_a.numel()
    if not (edge_a.dtype == torch.int32 and edge_b.dtype == torch.int32 and edge_b.numel() == ne):
        raise ValueError("edge_a / edge_b: int32 tensors of nedges pose indices")
    if not (lift_mask.dtype == torch.uint8 and lift_mask.numel() == ne):
        raise ValueError("lift_mask: a uint8 tensor of nedges leg bit masks")
    dev = best.device
    lifted = (lift_mask.reshape(1, ne).to(dev).to(torch.int32) >> torch.arange(nl, dtype=torch.int32, device=dev).reshape(nl, 1)) & 1
    none = torch.full((nl, ne), -1, dtype=torch.int32, device=dev)
    a, b = edge_a.reshape(-1).to(dev).long(), edge_b.reshape(-1).to(dev).long()
    nposes = best.shape[1]
    take = (lifted != 0) & ((a >= 0) & (a < nposes) & (b >= 0) & (b < nposes)).reshape(1, ne)  # a bad end is a dead edge: nothing swings
    foot_from = torch.where(take, best[:, a.clamp(0, max(nposes - 1, 0))], none)
    foot_to = torch.where(take, best[:, b.clamp(0, max(nposes - 1, 0))], none)
    return foot_from.contiguous(), foot_to.contiguous()


def swing_transit(tx, ty, tz, quats, body, legs, edge_a, edge_b, foot_from, foot_to, nsamples=9, lift=0.0, up=None,
                  foot_radius=0.0, margin=0.0, skip=0, live_in=None, mask=None, reached=None, first_miss=None, worst=None,
                  worst_d2=None, hits=None, hit_seg=None, near=None, pen=None, swinging=None, clear=None):
    """lrm_swing_transit_posed_dev: can a LIFTED foot get from its foothold under pose edge_a[e] to its foothold under pose
    edge_b[e].  edge_transit() samples the move for the feet that stay planted; this call does it for the swinging foot, which
    travels from target foot_from[l, e] to target foot_to[l, e] along a straight line with a parabolic bump of height lift along
    up (3 host floats, None = (0, 0, 1), not normalised), at the same nsamples sampled poses.  foot_from / foot_to: int32
    [nlegs, nedges] on the device (swing_layout() builds them); a leg with either index outside the cloud (-1) is not swinging.
    Reach part: mask, reached, first_miss, worst, worst_d2 [l, e] as edge_transit()'s, for the moving foot.  Terrain part, only
    with foot_radius > 0: the path's segments skip .. nsamples-2-skip against every target but the two footholds: hits[l, e]
    (targets within foot_radius), hit_seg[l, e] (the first segment hit, -1), near[l, e] (the deepest target within foot_radius +
    margin, -1) and its pen[l, e] (foot_radius - distance; -inf).  swinging[e] (bit l), clear[e] (1 iff live, both ends in range,
    every swinging leg reaches at every sample and hits nothing): directly the live_in of the other posed calls.
    Any index is safe.  -> (mask, reached, first_miss, worst, worst_d2, hits, hit_seg, near, pen, swinging, clear).  Every tensor
    must be contiguous.  No table.  With foot_radius == 0 one launch and no shared buffer; with foot_radius > 0 and 4096 targets
    or more it uses the pair kernels' box buffer (their threading rules; graph capture after one call on the largest cloud)."""
    torch = _torch()
    nt, nposes, legs, ne = _check_transit(tx, ty, tz, quats, body, legs, edge_a, edge_b)
    shape = (len(legs), ne)
    _check_feet(foot_from, quats, shape, "foot_from")
    _check_feet(foot_to, quats, shape, "foot_to")
    _check_in(live_in, quats, torch.uint8, ne, "live_in")
    _one_per(ne, "live_in: one byte per edge", live_in)
    nsamples = _capi._nsamples(nsamples)
    lift, up, foot_radius, margin, skip = _capi._swing_scalars(lift, up, foot_radius, margin, skip)
    mask = _out(mask, quats, shape, torch.int64, "per-leg sample masks")
    reached = _out(reached, quats, shape, torch.int32, "per-leg reached counts")
    first_miss = _out(first_miss, quats, shape, torch.int32, "per-leg first misses")
    worst = _out(worst, quats, shape, torch.int32, "per-leg worst samples")
    worst_d2 = _out(worst_d2, quats, shape, torch.float32, "per-leg worst squared distances")
    hits = _out(hits, quats, shape, torch.int32, "per-leg hit counts")
    hit_seg = _out(hit_seg, quats, shape, torch.int32, "per-leg first hit segments")
    near = _out(near, quats, shape, torch.int32, "per-leg deepest near targets")
    pen = _out(pen, quats, shape, torch.float32, "per-leg penetrations")
    swinging = _out(swinging, quats, ne, torch.uint8, "per-edge swinging bits")
    clear = _out(clear, quats, ne, torch.uint8, "per-edge clear bytes")
    _launch("lrm_swing_transit_posed_dev", quats, _dp(tx), _dp(ty), _dp(tz), nt, _dp(quats), _dp(body), nposes, _capi._ptr(legs),
            len(legs), _dp(edge_a), _dp(edge_b), ne, _dp(foot_from), _dp(foot_to), nsamples, lift, _capi._ptr(up), foot_radius, margin,
            skip, _dp(live_in), _dp(mask), _dp(reached), _dp(first_miss), _dp(worst), _dp(worst_d2), _dp(hits), _dp(hit_seg), _dp(near),
            _dp(pen), _dp(swinging), _dp(clear))
    return mask, reached, first_miss, worst, worst_d2, hits, hit_seg, near, pen, swinging, clear


def dbg_edge_transit_samples(quats, body, edge_a, edge_b, nsamples):
    """lrm_dbg_edge_transit_samples_dev: the sampled path of edge_transit() -> float32 (nedges, nsamples, 7) on the device: the
    quaternion and the body position of every sample (nan for an edge with an end out of range); one sample per lane."""
    nposes = _check_poses(quats, body)
    ne = _check_edges(quats, edge_a, edge_b)
    nsamples = _capi._nsamples(nsamples)
    out = _torch().empty((ne, nsamples, 7), dtype=_torch().float32, device=quats.device)
    _launch("lrm_dbg_edge_transit_samples_dev", quats, _dp(quats), _dp(body), nposes, _dp(edge_a), _dp(edge_b), ne, nsamples, _dp(out))
    return out


def dbg_link_pair_dist(segs, out=None):
    """lrm_dbg_link_pair_dist_dev: the link-pair distance of self_clearance() on segment pairs, segs float32 (n, 12) =
    A1, B1, A2, B2 on the device -> float32 (n,); one pair per lane."""
    torch = _torch()
    if not (segs.is_cuda and segs.dtype == torch.float32 and segs.dim() == 2 and segs.shape[1] == 12 and segs.is_contiguous()):
        raise ValueError("segs: expected a contiguous float32 CUDA tensor of shape (n, 12)")
    n = segs.shape[0]
    out = _out(out, segs, n, torch.float32, "distances")
    _launch("lrm_dbg_link_pair_dist_dev", segs, _dp(segs), n, _dp(out))
    return out


def dbg_trunk_link_dist(segs, trunk_radius, plus_z, minus_z, out=None):
    """lrm_dbg_trunk_link_dist_dev: the link-to-cylinder distance of trunk_clearance() on links in the body frame, segs float32
    (n, 6) = A, B on the device -> float32 (n,); one link per lane."""
    torch = _torch()
    if not (segs.is_cuda and segs.dtype == torch.float32 and segs.dim() == 2 and segs.shape[1] == 6 and segs.is_contiguous()):
        raise ValueError("segs: expected a contiguous float32 CUDA tensor of shape (n, 6)")
    n = segs.shape[0]
    out = _out(out, segs, n, torch.float32, "distances")
    _launch("lrm_dbg_trunk_link_dist_dev", segs, _dp(segs), n, float(trunk_radius), float(plus_z), float(minus_z), _dp(out))
    return out


class PoseSet:
    """A pose table for batched multi-pose queries (lrm_pose_compile_dev / lrm_reach_dist_posed_dev).

    legs: up to 8 legs (14 floats each, used as given: the per-pose rotate_leg_data happens inside).  The workspace --
    one 512-byte record per (pose, leg) for up to nposes_max poses -- is a tensor this object owns.  update() compiles the
    records from device-resident quaternions (and body positions) on the current stream; reach_dist() answers queries
    (target, pose, leg).  Both only launch: with check=False, reach_dist can be captured in a graph next to update()
    and replayed after new poses were copied into the captured quaternion tensor.  The arithmetic is LRM_MODE_STRICT's,
    whatever set_mode says.  ik=True: the set also owns the table of IK constants (128 bytes per (pose, leg)), update()
    compiles it too on the same stream, and ik() / fk() answer joint-angle queries.  footholds=True: the set owns the
    foothold table as well (32 bytes per (pose, leg): bounding sphere and nominal point, nominal (nlegs, 3) on the host
    in the BODY frame or None = zero), update() compiles it on the same stream, and footholds() counts and chooses the
    reachable targets per (pose, leg); foothold_edges() does the same for the targets two poses have in common, and
    foothold_misses() finds, for a leg that reaches nothing, the nearest miss and the body shift that would reach it;
    foothold_support() turns the question round: per target and leg, how many poses reach it and which does it best;
    body_clearance() asks whether the trunk itself fits: terrain inside the body cylinder, the worst point and the lift;
    leg_clearance() (with ik=True) asks the same of the legs under ik()'s angles: terrain inside the coxa, femur and tibia
    links, and leg_joints() returns the joints it tests; stance_stability() asks whether the chosen footholds carry the
    centre of mass, and which legs can be lifted; self_clearance() (with ik=True) asks whether the legs fit next to each
    other under ik()'s angles: links of different legs against each other; trunk_clearance() (with ik=True) whether they
    stay out of the robot's own trunk: leg links against the body cylinder; swing_transit() whether a lifted foot gets from
    its old foothold to its new one; edge_transit() whether the feet that
    foothold_edges() plants stay reachable at sampled poses between the two ends of a transition."""

    def __init__(self, legs, nposes_max, device=None, ik=False, footholds=False, nominal=None):
        torch = _torch()
        self.legs = np.ascontiguousarray(legs, dtype=np.float32).reshape(-1, 14)
        if not 1 <= len(self.legs) <= 8:
            raise ValueError("PoseSet: 1 to 8 legs (LRM_MAX_LEGS)")
        self.nposes_max = int(nposes_max)
        if self.nposes_max < 1:
            raise ValueError("PoseSet: nposes_max >= 1")
        self.device = torch.device(device if device is not None else "cuda")
        nbytes = _capi.load().lrm_posed_workspace_bytes(self.nposes_max, len(self.legs))
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.ik_workspace = None
        if ik:
            nbytes = _capi.load().lrm_posed_ik_workspace_bytes(self.nposes_max, len(self.legs))
            self.ik_workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.fh_workspace = None
        self.nominal = None if nominal is None else np.ascontiguousarray(nominal, dtype=np.float32).reshape(len(self.legs), 3)
        if footholds:
            nbytes = _capi.load().lrm_posed_footholds_workspace_bytes(self.nposes_max, len(self.legs))
            self.fh_workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        elif nominal is not None:
            raise ValueError("PoseSet: nominal without footholds=True")
        self.support_workspace = None  # foothold_support(): grows with the largest cloud seen
        self.nposes = 0

    @property
    def nlegs(self):
        return len(self.legs)

    def _need(self, table=None):
        """ValueError unless the set owns that table ("footholds" or "ik") and update() has run"""
        if table is not None and (self.fh_workspace if table == "footholds" else self.ik_workspace) is None:
            raise ValueError(f"PoseSet: built without {table}=True")
        if self.nposes == 0:
            raise ValueError("PoseSet: update() before the first query")

    def _cloud(self, tx, ty, tz, table="footholds"):
        """the preamble of the calls that take a target cloud and read that table -> nt"""
        nt = _check_f32(tx, ty, tz)
        self._need(table)
        _check_targets(nt, tx, self.workspace)
        return nt

    def _check_edge_range(self, edge_a, edge_b, check):
        """check=True of the edge calls: the pose indices are read back (one host synchronisation)"""
        if check and edge_a.numel() and edge_a.numel() == edge_b.numel():
            lo = min(int(edge_a.min()), int(edge_b.min()))
            hi = max(int(edge_a.max()), int(edge_b.max()))
            if lo < 0 or hi >= self.nposes:
                raise ValueError(f"edge_a / edge_b outside [0, {self.nposes})")

    def _last_update(self, quats):
        """quats must be the tensor of the last update(): the set keeps compiled records, not the poses"""
        self._need()
        if quats.dim() != 2 or quats.shape[0] != self.nposes:
            raise ValueError(f"quats: the ({self.nposes}, 4) tensor of the last update()")
        if quats.device != self.workspace.device:
            raise ValueError("quats and poses must live on one device")

    def _sets(self, angles, radius, pose_idx, live_in):
        """the sets of self_clearance() and trunk_clearance() -> (nsets, radius float32[3])"""
        torch = _torch()
        self._need("ik")
        if not (angles.is_cuda and angles.device == self.workspace.device and angles.dtype == torch.float32 and angles.dim() == 2
                and angles.shape[0] == 3 and angles.shape[1] % self.nlegs == 0 and angles.is_contiguous()):
            raise ValueError(f"angles: expected ik()'s contiguous float32 (3, {self.nlegs} * nsets) tensor on {self.workspace.device}")
        ns = angles.shape[1] // self.nlegs
        radius = _radius3(radius)
        _check_in(pose_idx, self.workspace, torch.int32, ns, "pose_idx")
        _check_in(live_in, self.workspace, torch.uint8, ns, "live_in")
        _one_per(ns, "pose_idx / live_in: one entry per set", pose_idx, live_in)
        if pose_idx is None and ns > self.nposes:
            raise ValueError("without pose_idx set s takes pose s: nsets <= nposes")
        return ns, radius

    def update(self, quats, body=None):
        """(Re)compile the records of poses 0 .. len(quats) - 1 from quats (float32 [nposes, 4], the quat convention
        of the single-pose calls) and body (float32 [nposes, 3] or None: no offset), both on this set's device."""
        torch = _torch()
        if quats.dim() != 2 or quats.shape[1] != 4:
            raise ValueError("quats: expected a float32 tensor of shape (nposes, 4)")
        nposes = quats.shape[0]
        if not 1 <= nposes <= self.nposes_max:
            raise ValueError(f"quats: 1 to {self.nposes_max} poses")
        ws = self.workspace
        _check_in(quats, ws, torch.float32, 4 * nposes, "quats")
        _check_in(body, ws, torch.float32, 3 * nposes, "body")
        if body is not None and tuple(body.shape) != (nposes, 3):
            raise ValueError("body: expected a float32 tensor of shape (nposes, 3)")
        _launch("lrm_pose_compile_dev", ws, _dp(quats), _dp(body), nposes, _capi._ptr(self.legs), self.nlegs, _dp(ws))
        if self.ik_workspace is not None:
            _launch("lrm_pose_ik_compile_dev", ws, _dp(quats), nposes, _capi._ptr(self.legs), self.nlegs, _dp(self.ik_workspace))
        if self.fh_workspace is not None:
            _launch("lrm_pose_footholds_compile_dev", ws, _dp(quats), nposes, _capi._ptr(self.legs), self.nlegs,
                    _capi._ptr(self.nominal), _dp(self.fh_workspace))
        self.nposes = nposes
        return self

    def footholds(self, tx, ty, tz, count=None, best=None, best_d2=None, all_legs=None):
        """lrm_footholds_posed_dev: count[l, p] = targets leg l reaches under pose p (reachability_global on
        target - body[p]), best[l, p] = the reachable target nearest body[p] + the leg's nominal point rotated by the
        pose (-1 if none), best_d2[l, p] = its squared distance (+inf if none), all_legs[p] = 1 iff every leg has one.
        -> (count int32, best int32, best_d2 float32, each [nlegs, nposes]; all_legs uint8[nposes]).  One launch behind
        the cloud's bounding boxes; best.view(-1) is ik()'s target_idx with footholds_layout(nposes, nlegs, device)."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        ws, shape = self.workspace, (self.nlegs, self.nposes)
        count = _out(count, ws, shape, torch.int32, "per-leg counts")
        best = _out(best, ws, shape, torch.int32, "per-leg choices")
        best_d2 = _out(best_d2, ws, shape, torch.float32, "per-leg squared distances")
        all_legs = _out(all_legs, ws, self.nposes, torch.uint8, "per-pose bytes")
        _launch("lrm_footholds_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes, self.nlegs,
                _dp(count), _dp(best), _dp(best_d2), _dp(all_legs))
        return count, best, best_d2, all_legs

    def foothold_lists(self, tx, ty, tz, count=None, offsets=None, capacity=None, idx=None, d2=None, written=None, want_d2=True):
        """lrm_foothold_lists_posed_dev: the reachable targets of every (pose, leg) in CSR form.  Segment o = l*nposes + p
        of idx holds the targets leg l reaches under pose p in ascending index, from offsets[o] on, as far as
        min(offsets[o + 1], capacity) leaves room; d2 holds, at the same positions, the squared distance to the leg's
        nominal point that footholds() minimises; written[l, p] = the entries stored.  Nothing else in idx / d2 is
        touched, whatever offsets holds (include/lrm.h).  -> (offsets int64[nlegs*nposes + 1], idx int32[capacity],
        d2 float32[capacity] or None with want_d2=False, written int32[nlegs, nposes]).
          * count=None and offsets=None: footholds() runs first; offsets=None: foothold_offsets(count).
          * capacity=None and idx=None: offsets[-1] is read back to allocate exactly that -- ONE host synchronisation.
            With capacity or a preallocated idx (capacity = its length) the call only launches, so update -> footholds
            -> foothold_offsets -> foothold_lists can be captured in a graph after one warm call on the largest cloud;
            a list that does not fit is cut short and written says so."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        ws, n = self.workspace, self.nlegs * self.nposes
        if offsets is None:
            if count is None:
                count = self.footholds(tx, ty, tz)[0]
            _check_in(count, ws, torch.int32, n, "per-leg counts")
            offsets = foothold_offsets(count.view(-1)[:n])
        _check_in(offsets, ws, torch.int64, n + 1, "offsets")
        if capacity is None:
            capacity = idx.numel() if idx is not None else max(int(offsets[n].item()), 0)  # the one synchronisation
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity >= 0")
        idx = _out(idx, ws, capacity, torch.int32, "list indices")
        d2 = _out(d2, ws, capacity, torch.float32, "list squared distances", want_d2)
        written = _out(written, ws, (self.nlegs, self.nposes), torch.int32, "per-leg written counts")
        _launch("lrm_foothold_lists_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes,
                self.nlegs, _dp(offsets), capacity, _dp(idx), _dp(d2) if want_d2 else None, _dp(written))
        return offsets, idx, d2 if want_d2 else None, written

    def foothold_edges(self, tx, ty, tz, edge_a, edge_b, count=None, best=None, best_d2=None, all_legs=None, check=True):
        """lrm_foothold_edges_posed_dev: per pose transition e = (edge_a[e], edge_b[e]) (int32 device tensors of pose
        indices) and leg l, the targets leg l reaches under BOTH poses, i.e. the footholds a stance foot can keep during
        the move.  count[l, e] = how many, best[l, e] = the common target with the smallest sum of footholds()'s two d2
        (-1 if none), best_d2[l, e] = that sum (+inf if none), all_legs[e] = 1 iff every leg has one.
        -> (count int32, best int32, best_d2 float32, each [nlegs, nedges]; all_legs uint8[nedges]).  check=True
        validates the indices on the host (one synchronisation); check=False leaves an index outside [0, nposes) to the
        kernel (count 0, best -1, +inf, all_legs 0): the form for graph capture.  One launch behind the cloud's bounding
        boxes; best.view(-1) is ik()'s target_idx with foothold_edges_layout() for either end of the edges."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        ws = self.workspace
        ne = _check_edges(ws, edge_a, edge_b)
        self._check_edge_range(edge_a, edge_b, check)
        shape = (self.nlegs, ne)
        count = _out(count, ws, shape, torch.int32, "per-leg counts")
        best = _out(best, ws, shape, torch.int32, "per-leg choices")
        best_d2 = _out(best_d2, ws, shape, torch.float32, "per-leg squared distances")
        all_legs = _out(all_legs, ws, ne, torch.uint8, "per-edge bytes")
        _launch("lrm_foothold_edges_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes,
                self.nlegs, _dp(edge_a), _dp(edge_b), ne, _dp(count), _dp(best), _dp(best_d2), _dp(all_legs))
        return count, best, best_d2, all_legs

    def foothold_misses(self, tx, ty, tz, margin, count=None, miss=None, m2=None, shift=None, near=None, want_shift=True):
        """lrm_foothold_misses_posed_dev: for every (pose, leg) that count does not skip, the target closest to being
        reachable.  Candidates are the targets inside the leg's bounding sphere widened by margin (mm, >= 0 or +inf);
        among the unreachable ones, miss[l, p] = the target whose distance_global vector is the shortest (-1 if none),
        m2[l, p] = its squared length (+inf if none), shift[:, l, p] = the vector -- translating the body by it at fixed
        orientation puts the target on the workspace boundary (nan if none) -- and near[l, p] = the number of unreachable
        candidates.  count: int32 [nlegs, nposes] or None; wherever count > 0 the entry is skipped and gets the empty
        answer: pass footholds()'s count so that only footless legs cost anything.
        -> (miss int32, m2 float32, each [nlegs, nposes]; shift float32 [3, nlegs, nposes] or None with
        want_shift=False; near int32 [nlegs, nposes]).  One launch behind the cloud's bounding boxes; it only launches,
        so update -> footholds -> foothold_misses can be captured in a graph after one warm call on the largest cloud.
        reach_dist on (miss, p, l) returns mask 0 and exactly the shift bits."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        margin = float(margin)
        if not margin >= 0.0:
            raise ValueError("margin: >= 0 or +inf")
        ws, shape, n = self.workspace, (self.nlegs, self.nposes), self.nlegs * self.nposes
        _check_in(count, ws, torch.int32, n, "per-leg counts")
        miss = _out(miss, ws, shape, torch.int32, "per-leg misses")
        m2 = _out(m2, ws, shape, torch.float32, "per-leg squared distances")
        near = _out(near, ws, shape, torch.int32, "per-leg miss counts")
        sx = sy = sz = None
        if want_shift:
            shift = _out(shift, ws, (3,) + shape, torch.float32, "per-leg shift vectors")
            sv = shift.view(-1)
            sx, sy, sz = sv[:n], sv[n:2 * n], sv[2 * n:3 * n]
        _launch("lrm_foothold_misses_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes,
                self.nlegs, margin, _dp(count), _dp(miss), _dp(m2), _dp(sx), _dp(sy), _dp(sz), _dp(near))
        return miss, m2, shift if want_shift else None, near

    def foothold_support(self, tx, ty, tz, pose_live=None, count=None, best_pose=None, best_d2=None, legs_mask=None):
        """lrm_foothold_support_posed_dev: the per-TARGET view of footholds().  count[l, t] = the live poses under which leg l
        reaches target t (reachability_global on target - body[p]; pose_live: uint8 [nposes] on the device, 0 = the pose
        does not count, None = every pose), best_pose[l, t] = the reaching pose whose nominal point of leg l lies nearest
        the target (footholds()'s d2 of that triple, ties to the smaller pose; -1 if none), best_d2[l, t] = that d2
        (+inf if none), legs_mask[t] = bit l set iff count[l, t] > 0.
        -> (count int32, best_pose int32, best_d2 float32, each [nlegs, nt]; legs_mask uint8[nt]).  pose_live and given
        outputs must be contiguous.  The set keeps a support workspace sized for the largest cloud seen: a first or larger
        call allocates it (through torch), every other call only launches, so update -> footholds ->
        foothold_support(pose_live=all_legs) can be captured in a graph after one call on a cloud of the largest size.
        It does not use the pair kernels' box buffer.  foothold_support_layout() turns best_pose into ik()'s indices."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        ws, shape = self.workspace, (self.nlegs, nt)
        _check_in(pose_live, ws, torch.uint8, self.nposes, "pose_live")
        count = _out(count, ws, shape, torch.int32, "per-leg counts")
        best_pose = _out(best_pose, ws, shape, torch.int32, "per-leg best poses")
        best_d2 = _out(best_d2, ws, shape, torch.float32, "per-leg squared distances")
        legs_mask = _out(legs_mask, ws, nt, torch.uint8, "per-target leg masks")
        if nt == 0:
            return count, best_pose, best_d2, legs_mask
        need = _capi.load().lrm_foothold_support_workspace_bytes(self.nposes_max, self.nlegs, nt)
        if self.support_workspace is None or self.support_workspace.numel() < need:
            self.support_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        _launch("lrm_foothold_support_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes,
                self.nlegs, _dp(pose_live), _dp(self.support_workspace), _dp(count), _dp(best_pose), _dp(best_d2), _dp(legs_mask))
        return count, best_pose, best_d2, legs_mask

    def body_clearance(self, tx, ty, tz, radius, plus_z, minus_z, floor_z=None, live_in=None, hits=None, top=None, height=None,
                       free=None):
        """lrm_body_clearance_posed_dev: does the trunk of every pose fit over the terrain.  The body volume is a cylinder
        in the BODY frame about the body's z axis through the body origin: radius, top plus_z, belly plane minus_z (mm).
        hits[p] = the targets inside it; top[p] = the target of the column under the body (the same cylinder down to
        floor_z; None = minus_z) that stands highest over the belly plane (-1 if none); height[p] = its vz - minus_z
        (-inf if none): > 0 is the lift along the body's z that clears the pose, <= 0 the ground clearance left;
        free[p] = 1 iff the pose is live and hits[p] == 0.  live_in: uint8 [nposes] on the device, 0 = the pose is skipped
        (0, -1, -inf, free 0), None = every pose; pass footholds()'s all_legs.
        -> (hits int32, top int32, height float32, free uint8, each [nposes]).  live_in and given outputs must be
        contiguous.  free is directly foothold_support()'s pose_live.  One launch behind the cloud's bounding boxes; it
        only launches, so update -> footholds -> body_clearance can be captured in a graph after one warm call on the
        largest cloud."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz)
        radius, plus_z, minus_z = float(radius), float(plus_z), float(minus_z)
        floor_z = minus_z if floor_z is None else float(floor_z)
        ws, n = self.workspace, self.nposes
        _check_in(live_in, ws, torch.uint8, n, "live_in")
        hits = _out(hits, ws, n, torch.int32, "per-pose hit counts")
        top = _out(top, ws, n, torch.int32, "per-pose top targets")
        height = _out(height, ws, n, torch.float32, "per-pose heights")
        free = _out(free, ws, n, torch.uint8, "per-pose free bytes")
        _launch("lrm_body_clearance_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.fh_workspace), self.nposes,
                self.nlegs, radius, plus_z, minus_z, floor_z, _dp(live_in), _dp(hits), _dp(top), _dp(height), _dp(free))
        return hits, top, height, free

    def stance_stability(self, tx, ty, tz, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0,
                         live_in=None, margin=None, edge=None, stable=None, feet=None):
        """device.stance_stability() on this set's poses: quats (and body) are the tensors of the last update() -- the set keeps
        compiled records, not the poses -- so their pose count must be the set's, foot is [nlegs, nstances] with the set's
        legs, and everything lives on the set's device.  foot = footholds()'s best (a stance per pose), or foothold_edges()'s
        best with pose_idx = edge_a or edge_b.  -> (margin, edge, stable [nmasks, nstances]; feet [nstances]); stable[0] is
        body_clearance()'s live_in.  It only launches: update -> footholds -> stance_stability can be captured in a graph."""
        self._last_update(quats)
        if foot.dim() != 2 or foot.shape[0] != self.nlegs:
            raise ValueError(f"foot: expected an int32 tensor of shape ({self.nlegs}, nstances)")
        return stance_stability(tx, ty, tz, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in, margin, edge, stable,
                                feet)

    def edge_transit(self, tx, ty, tz, quats, body, edge_a, edge_b, foot, nsamples=9, live_in=None, mask=None, reached=None,
                     first_miss=None, worst=None, worst_d2=None, planted=None, clear=None, advance=None, check=True):
        """device.edge_transit() with this set's legs: quats (and body) are the tensors of the last update() -- the set keeps
        compiled records, not the poses, and the call compiles the poses in between itself -- so their pose count must be the
        set's; foot is foothold_edges()'s best [nlegs, nedges].  check=True validates edge_a / edge_b on the host (one
        synchronisation), as foothold_edges() does; check=False leaves an index outside [0, nposes) to the kernel (a dead edge):
        the form for graph capture.  -> (mask, reached, first_miss, worst, worst_d2 [nlegs, nedges]; planted, clear, advance
        [nedges]); clear is the live_in of ik()'s callers and of stance_stability():
        update -> footholds -> foothold_edges -> edge_transit -> ik / stance_stability(live_in = clear)."""
        self._last_update(quats)
        self._check_edge_range(edge_a, edge_b, check)
        return edge_transit(tx, ty, tz, quats, body, self.legs, edge_a, edge_b, foot, nsamples, live_in, mask, reached, first_miss,
                            worst, worst_d2, planted, clear, advance)

    def swing_transit(self, tx, ty, tz, quats, body, edge_a, edge_b, foot_from, foot_to, nsamples=9, lift=0.0, up=None,
                      foot_radius=0.0, margin=0.0, skip=0, live_in=None, mask=None, reached=None, first_miss=None, worst=None,
                      worst_d2=None, hits=None, hit_seg=None, near=None, pen=None, swinging=None, clear=None, check=True):
        """device.swing_transit() with this set's legs: quats (and body) are the tensors of the last update(), so their pose
        count must be the set's; foot_from / foot_to [nlegs, nedges] come from swing_layout(footholds()'s best, edge_a, edge_b,
        lift_mask).  check=True validates edge_a / edge_b on the host (one synchronisation), as edge_transit() does; check=False
        leaves an index outside [0, nposes) to the kernel (a dead edge): the form for graph capture.  -> (mask, reached,
        first_miss, worst, worst_d2, hits, hit_seg, near, pen [nlegs, nedges]; swinging, clear [nedges]); give edge_transit()'s
        clear as live_in, and this clear to what follows:
        update -> footholds -> foothold_edges -> edge_transit -> swing_transit(live_in = clear) -> ik / stance_stability."""
        self._last_update(quats)
        self._check_edge_range(edge_a, edge_b, check)
        return swing_transit(tx, ty, tz, quats, body, self.legs, edge_a, edge_b, foot_from, foot_to, nsamples, lift, up, foot_radius,
                             margin, skip, live_in, mask, reached, first_miss, worst, worst_d2, hits, hit_seg, near, pen, swinging,
                             clear)

    def routes(self, edge_a, edge_b, sources, **kw):
        """device.pose_routes() over the poses of the last update(): nposes is this set's, every other argument is that
        call's (edge_live, pose_live, edge_cost, direction, rounds, sync, workspace, the outputs).  No table is read: the call
        composes the bytes of the other calls -- the capstone of the chain
        update -> footholds -> foothold_edges -> edge_transit -> swing_transit -> routes(edge_live = clear, pose_live = all_legs).
        -> (cost, hops, pred_edge, pred_pose, reached, done)"""
        self._need()
        if edge_a.device != self.workspace.device:
            raise ValueError("edges and poses must live on one device")
        return pose_routes(self.nposes, edge_a, edge_b, sources, **kw)

    def edges(self, quats, body, max_step, max_turn=None, **kw):
        """device.pose_edges() on the poses of the last update(): quats (and body) must be that call's tensors, every other
        argument is pose_edges()'s (pose_live, form, count, offsets, capacity, workspace, the outputs).  No table is read: the
        call builds the edge_a / edge_b the edge calls take -- the first link of the chain
        update -> edges -> footholds -> foothold_edges -> edge_transit -> swing_transit -> routes.
        -> (edge_a, edge_b, offsets, d2, cos2, written)"""
        self._last_update(quats)
        return pose_edges(quats, body, max_step, max_turn, **kw)

    def _check_angles(self, angles):
        torch = _torch()
        self._need("ik")
        n = self.nlegs * self.nposes
        if not (angles.is_cuda and angles.device == self.workspace.device and angles.dtype == torch.float32 and angles.dim() == 2
                and tuple(angles.shape) == (3, n) and angles.is_contiguous()):
            raise ValueError(f"angles: expected ik()'s contiguous float32 (3, {n}) tensor on {self.workspace.device}")

    def leg_clearance(self, tx, ty, tz, angles, radius, margin=0.0, tip_clear=0.0, live_in=None, hits=None, links=None, worst=None,
                      pen=None, free=None):
        """lrm_leg_clearance_posed_dev: do the legs themselves fit over the terrain under the given joint angles.
        angles: ik()'s (3, nlegs*nposes) tensor under footholds_layout (entry l*nposes + p).  radius: three capsule radii
        (coxa, femur, tibia link; 0 = the link is not tested), margin: how far outside a link a target still counts as
        near, tip_clear: how far short of the foot the tibia link stops (mm).  hits[l, p] = the targets inside a link;
        links[l, p] = bit k set iff link k is hit; worst[l, p] = the near target that stands deepest (-1 if none);
        pen[l, p] = its radius - distance (-inf if none): > 0 an intrusion, <= 0 the clearance left within the margin;
        free[p] = 1 iff the pose is live and no leg is hit.  A leg with nan angles is skipped (all empty) and does not block
        free.  live_in: uint8 [nposes] on the device, 0 = the pose is skipped (0, 0, -1, -inf, free 0), None = every pose.
        -> (hits int32, links uint8, worst int32, pen float32, each [nlegs, nposes]; free uint8[nposes]).  live_in and
        given outputs must be contiguous.  One launch behind the cloud's bounding boxes; it only launches, so
        update -> footholds -> ik -> leg_clearance can be captured in a graph after one warm call on the largest cloud."""
        torch = _torch()
        nt = self._cloud(tx, ty, tz, "ik")
        self._check_angles(angles)
        radius = _radius3(radius)
        ws, shape = self.workspace, (self.nlegs, self.nposes)
        _check_in(live_in, ws, torch.uint8, self.nposes, "live_in")
        hits = _out(hits, ws, shape, torch.int32, "per-leg hit counts")
        links = _out(links, ws, shape, torch.uint8, "per-leg link masks")
        worst = _out(worst, ws, shape, torch.int32, "per-leg worst targets")
        pen = _out(pen, ws, shape, torch.float32, "per-leg penetrations")
        free = _out(free, ws, self.nposes, torch.uint8, "per-pose free bytes")
        _launch("lrm_leg_clearance_posed_dev", ws, _dp(tx), _dp(ty), _dp(tz), nt, _dp(ws), _dp(self.ik_workspace), self.nposes,
                self.nlegs, _dp(angles[0]), _dp(angles[1]), _dp(angles[2]), _capi._ptr(radius), float(margin), float(tip_clear),
                _dp(live_in), _dp(hits), _dp(links), _dp(worst), _dp(pen), _dp(free))
        return hits, links, worst, pen, free

    def self_clearance(self, angles, radius, margin=0.0, tip_clear=0.0, pose_idx=None, live_in=None, hits=None, with_=None, links=None,
                       worst=None, pen=None, free=None):
        """lrm_self_clearance_posed_dev: do the legs fit next to each other under the given joint angles.  A set s is a pose
        (pose_idx[s], int32 on the device; None: pose s) and one angle triple per leg: angles is ik()'s (3, nlegs*nsets)
        tensor, entry l*nsets + s -- under footholds_layout a set per pose, under foothold_edges_layout a set per edge
        with pose_idx = edge_a or edge_b.  radius, margin and tip_clear are leg_clearance()'s.  Every link of a leg is tested
        against every link of every OTHER leg: hits[l, s] = the link pairs that hit; with_[l, s] = bit j set iff leg j is hit;
        links[l, s] = bit k set iff the own link k is in a hit; worst[l, s] = the pair within margin that stands deepest, as
        code j*9 + own_link*3 + other_link (255 if none); pen[l, s] = its radius sum - distance (-inf if none); free[s] = 1 iff
        the set is live and no leg is hit.  A leg with nan angles takes part in no pair and does not block free.  live_in: uint8
        [nsets] on the device, 0 = dead (0, 0, 0, 255, -inf, free 0), as is a pose index outside the set's poses.
        -> (hits int32, with_ uint8, links uint8, worst uint8, pen float32, each [nlegs, nsets]; free uint8[nsets]); free is
        leg_clearance()'s live_in.  pose_idx, live_in and given outputs must be contiguous.  One launch, no allocation beyond
        missing outputs, no shared buffer: update -> footholds -> ik -> self_clearance -> leg_clearance can be captured in a
        graph, and the call may run next to anything."""
        torch = _torch()
        ns, radius = self._sets(angles, radius, pose_idx, live_in)
        ws, shape = self.workspace, (self.nlegs, ns)
        hits = _out(hits, ws, shape, torch.int32, "per-leg hit counts")
        with_ = _out(with_, ws, shape, torch.uint8, "per-leg leg masks")
        links = _out(links, ws, shape, torch.uint8, "per-leg link masks")
        worst = _out(worst, ws, shape, torch.uint8, "per-leg worst pairs")
        pen = _out(pen, ws, shape, torch.float32, "per-leg penetrations")
        free = _out(free, ws, ns, torch.uint8, "per-set free bytes")
        _launch("lrm_self_clearance_posed_dev", ws, _dp(ws), _dp(self.ik_workspace), self.nposes, self.nlegs, _dp(pose_idx), ns,
                _dp(angles[0]), _dp(angles[1]), _dp(angles[2]), _capi._ptr(radius), float(margin), float(tip_clear), _dp(live_in),
                _dp(hits), _dp(with_), _dp(links), _dp(worst), _dp(pen), _dp(free))
        return hits, with_, links, worst, pen, free

    def stance_loads(self, angles, quats, tau_max, pose_idx=None, com=None, plane=None, lift=None, live_in=None, status=None,
                     holdable=None, peak=None, peak_at=None, load=None, tau=None, want_peak_at=True, want_load=True, want_tau=True):
        """device.stance_loads() on this set's tables (built with ik=True): quats is the tensor of the last update() -- the set
        keeps compiled records, not the poses, and the centre of mass needs the quaternion -- so its pose count must be the
        set's.  angles: ik()'s (3, nlegs*nsets) tensor, entry l*nsets + s, under footholds_layout a set per pose, under
        foothold_edges_layout a set per edge with pose_idx = edge_a or edge_b.
        -> (status, holdable, peak, peak_at [nmasks, nsets]; load [nmasks, nlegs, nsets]; tau [nmasks, nlegs, 3, nsets]);
        holdable[m] is the live_in of stance_stability(), self_clearance() and the other posed calls.  It only launches:
        update -> footholds -> ik -> stance_loads -> stance_stability(live_in = holdable[0]) can be captured in a graph."""
        self._need("ik")
        self._last_update(quats)
        return stance_loads(self.workspace, self.ik_workspace, quats, self.nlegs, angles, tau_max, pose_idx, com, plane, lift, live_in,
                            status, holdable, peak, peak_at, load, tau, want_peak_at, want_load, want_tau)

    def trunk_clearance(self, angles, radius, trunk_radius, plus_z, minus_z, margin=0.0, tip_clear=0.0, links=0b110, pose_idx=None,
                        live_in=None, hit=None, worst=None, pen=None, free=None):
        """lrm_trunk_clearance_posed_dev: do the legs stay out of the robot's own trunk under the given joint angles.  Sets,
        angles (ik()'s (3, nlegs*nsets) tensor, entry l*nsets + s), radius, margin, tip_clear, pose_idx and live_in are
        self_clearance()'s.  The trunk is body_clearance()'s cylinder: trunk_radius, plus_z, minus_z in the body frame, axis z,
        about the body origin.  links: bit k set = link k (0 coxa, 1 femur, 2 tibia) is tested; the coxa link starts at its
        mount on the trunk, hence 0b110; a link with radius 0 is not tested either.  hit[l, s] = bit k set iff link k of leg l
        hits the trunk; worst[l, s] = the link within margin that stands deepest (255 if none); pen[l, s] = its radius -
        distance (-inf if none); free[s] = 1 iff the set is live and no leg hits.  A leg with nan angles gets the empty answer
        and does not block free.  live_in: uint8[nsets] on the device, 0 = dead (0, 255, -inf, free 0), as is a pose index
        outside the set's poses.
        -> (hit uint8, worst uint8, pen float32, each [nlegs, nsets]; free uint8[nsets]); free is self_clearance()'s and
        leg_clearance()'s live_in.  pose_idx, live_in and given outputs must be contiguous.  One launch, no allocation beyond
        missing outputs, no shared buffer: update -> footholds -> ik -> trunk_clearance -> self_clearance -> leg_clearance can
        be captured in a graph, and the call may run next to anything."""
        torch = _torch()
        ns, radius = self._sets(angles, radius, pose_idx, live_in)
        links = _capi._links_mask(links)
        ws, shape = self.workspace, (self.nlegs, ns)
        hit = _out(hit, ws, shape, torch.uint8, "per-leg link masks")
        worst = _out(worst, ws, shape, torch.uint8, "per-leg worst links")
        pen = _out(pen, ws, shape, torch.float32, "per-leg penetrations")
        free = _out(free, ws, ns, torch.uint8, "per-set free bytes")
        _launch("lrm_trunk_clearance_posed_dev", ws, _dp(ws), _dp(self.ik_workspace), self.nposes, self.nlegs, _dp(pose_idx), ns,
                _dp(angles[0]), _dp(angles[1]), _dp(angles[2]), _capi._ptr(radius), float(margin), float(tip_clear),
                float(trunk_radius), float(plus_z), float(minus_z), links, _dp(live_in), _dp(hit), _dp(worst), _dp(pen), _dp(free))
        return hit, worst, pen, free

    def leg_joints(self, angles, tip_clear=0.0, out=None):
        """lrm_leg_joints_posed_dev: the four joints of every (leg, pose) under angles (ik()'s (3, nlegs*nposes) tensor under
        footholds_layout): coxa joint, femur joint, knee and the tibia's end tip_clear short of the foot, body position
        added -> float32 (nlegs, nposes, 4, 3).  One launch."""
        self._check_angles(angles)
        ws = self.workspace
        out = _out(out, ws, (self.nlegs, self.nposes, 4, 3), _torch().float32, "joints")
        _launch("lrm_leg_joints_posed_dev", ws, _dp(angles[0]), _dp(angles[1]), _dp(angles[2]), self.nposes, self.nlegs, _dp(ws),
                _dp(self.ik_workspace), float(tip_clear), _dp(out))
        return out

    def _check_indices(self, ref, n, pose_idx, leg_idx, check):
        torch = _torch()
        self._need()
        if ref.device != self.workspace.device:
            raise ValueError("queries and poses must live on one device")
        _check_in(pose_idx, ref, torch.int32, n, "pose_idx")
        _check_in(leg_idx, ref, torch.uint8, n, "leg_idx")
        _one_per(n, "pose_idx / leg_idx: one index per query", pose_idx, leg_idx)
        if check and n:
            if pose_idx is not None:
                lo, hi = torch.aminmax(pose_idx)
                if int(lo) < 0 or int(hi) >= self.nposes:
                    raise ValueError(f"pose_idx outside [0, {self.nposes})")
            if leg_idx is not None and int(leg_idx.max()) >= self.nlegs:
                raise ValueError(f"leg_idx outside [0, {self.nlegs})")

    def ik(self, x, y, z, pose_idx=None, leg_idx=None, target_idx=None, seed=None, out=None, status=None, check=True):
        """lrm_ik_posed_dev.  Query i takes target target_idx[i] (int32) of (x, y, z), or target i without target_idx,
        minus the body position of pose pose_idx[i], and solves leg leg_idx[i] under that pose's quaternion.  seed:
        None or three float32 tensors, one angle per query.  -> (angles float32 (3, n), status uint8[n]).  check=True
        validates pose_idx and leg_idx on the host (one synchronisation); target_idx is never validated: an index
        outside [0, len(x)), the -1 of footholds() included, gives status 0 and nan angles.  One launch."""
        torch = _torch()
        nt = _check_f32(x, y, z)
        if self.ik_workspace is None:
            raise ValueError("PoseSet: built without ik=True")
        if target_idx is not None:
            n = target_idx.numel()
            _check_in(target_idx, x, torch.int32, n, "target_idx")
        else:
            n = nt
        self._check_indices(x, n, pose_idx, leg_idx, check)
        if seed is not None:
            if len(seed) != 3:
                raise ValueError("seed: three tensors (coxa, femur, tibia) or None")
            if _check_f32(*seed) != n or seed[0].device != x.device:
                raise ValueError("seed: one angle per query, on the queries' device")
        out = _out_field(out, x, n)
        status = _out(status, x, n, torch.uint8, "status")
        sc, sf, st = (None, None, None) if seed is None else seed
        _launch("lrm_ik_posed_dev", x, _dp(x), _dp(y), _dp(z), nt, _dp(target_idx), n, _dp(pose_idx), _dp(leg_idx), _dp(self.workspace),
                _dp(self.ik_workspace), self.nposes, self.nlegs, _dp(sc), _dp(sf), _dp(st), _dp(out[0]), _dp(out[1]), _dp(out[2]),
                _dp(status))
        return out, status

    def fk(self, coxa, femur, tibia, pose_idx=None, leg_idx=None, out=None, check=True):
        """lrm_fk_posed_dev: the tip of angles i for leg leg_idx[i] under pose pose_idx[i], plus that pose's body
        position -> float32 (3, n).  One launch."""
        n = _check_f32(coxa, femur, tibia)
        if self.ik_workspace is None:
            raise ValueError("PoseSet: built without ik=True")
        self._check_indices(coxa, n, pose_idx, leg_idx, check)
        out = _out_field(out, coxa, n)
        _launch("lrm_fk_posed_dev", coxa, _dp(coxa), _dp(femur), _dp(tibia), n, _dp(pose_idx), _dp(leg_idx), _dp(self.workspace),
                _dp(self.ik_workspace), self.nposes, self.nlegs, _dp(out[0]), _dp(out[1]), _dp(out[2]))
        return out

    def reach_dist(self, x, y, z, pose_idx=None, leg_idx=None, mask=None, out=None, valid=None, want_dist=True, check=True):
        """Query i = (x[i], y[i], z[i]) for pose pose_idx[i] (int32; None: pose 0) and leg leg_idx[i] (uint8; None:
        leg 0) -> (mask uint8[n], field float32 (3, n), valid uint8[n]); with want_dist=False only the mask (field and
        valid None).  check=True validates the indices on the host (one synchronisation); check=False leaves an
        out-of-range index to the kernel (mask 0, valid 0, nan field): the form for graph capture."""
        torch = _torch()
        n = _check_f32(x, y, z)
        self._check_indices(x, n, pose_idx, leg_idx, check)
        mask = _out(mask, x, n, torch.uint8, "mask")
        if want_dist:
            out = _out_field(out, x, n)
            valid = _out(valid, x, n, torch.uint8, "validity bytes")
        else:
            out = valid = None
        f = (None, None, None) if out is None else (_dp(out[0]), _dp(out[1]), _dp(out[2]))
        _launch("lrm_reach_dist_posed_dev", x, _dp(x), _dp(y), _dp(z), n, _dp(pose_idx), _dp(leg_idx), _dp(self.workspace), self.nposes,
                self.nlegs, _dp(mask), _dp(valid), *f)
        return mask, out, valid
