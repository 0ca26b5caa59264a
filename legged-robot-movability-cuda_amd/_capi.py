"""ctypes binding of liblrm.so (include/lrm.h).  No compute happens in Python, and there
is no fallback: if the shared library is missing, load() raises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LRM_LIB_PATH: load another build of the same library (A/B runs of kernel variants)
LIB_PATH = os.environ.get("LRM_LIB_PATH") or os.path.join(_HERE, "liblrm.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lrm.h")
MODE_STRICT, MODE_FAST, MODE_TOL, MODE_TOL_REL = 0, 1, 2, 3
_lib = None


class LrmError(RuntimeError):
    pass


def build(verbose=False):
    """Compile csrc/ into liblrm.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_C_SCALARS = {"size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "int": C.c_int, "int32_t": C.c_int32,
              "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_C_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "void": None, "const char*": C.c_char_p}
_signatures = None  # parse_header(include/lrm.h), read once


def parse_header(text):
    """{name: (restype, [argtypes])} of every lrm_* prototype in header text: the only source of the ctypes signatures.
    A pointer, an array or the LrmOctExchange callback is a c_void_p, a scalar by value its own ctypes type; a type that is
    not listed above raises LrmError (never a guess)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([^;{}()]*?)\b(lrm_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _C_RETURNS:
            raise LrmError(f"{name}: unknown return type '{ret}'")
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            if "*" in p or "[" in p or words[:1] == ["LrmOctExchange"]:
                argtypes.append(C.c_void_p)
            elif len(words) in (1, 2) and words[0] in _C_SCALARS:
                argtypes.append(_C_SCALARS[words[0]])
            else:
                raise LrmError(f"{name}: unknown parameter type '{' '.join(p.split())}'")
        out[name] = (_C_RETURNS[ret], argtypes)
    return out


def signatures():
    """parse_header() of include/lrm.h"""
    global _signatures
    if _signatures is None:
        try:
            text = open(HEADER_PATH).read()
        except OSError as e:
            raise LrmError(f"{HEADER_PATH} is missing: the ctypes signatures come from it ({e})")
        _signatures = parse_header(text)
    return _signatures


def declared_symbols():
    """Every function name declared in include/lrm.h."""
    return sorted(signatures())


def exported_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LrmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the HIP path)")
    try:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7; importing it
        # first makes liblrm.so bind to that copy, so torch's device pointers and streams are
        # valid in our launches.  Without torch the library binds to /opt/rocm's runtime.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in signatures().items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if name.startswith("lrm_dbg_") or (os.environ.get("LRM_LIB_PATH") and name.startswith(("lrm_foothold_", "lrm_body_clearance_", "lrm_leg_", "lrm_stance_", "lrm_self_", "lrm_trunk_", "lrm_edge_", "lrm_pose_routes_", "lrm_pose_edge"))):
                continue  # an older library variant in an A/B run (LRM_LIB_PATH): diagnostics and the newest calls may be missing
            raise
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


def lib():
    return load()


def check(rc):
    if rc != 0:
        raise LrmError(f"liblrm error {rc}: {load().lrm_last_error().decode()}")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def _quat(q):
    return None if q is None else _f32(q, (4,))


def _nominal(nominal, nlegs):
    return None if nominal is None else _f32(nominal, (nlegs, 3))


def _u8_per(a, n, what):
    """an optional byte per pose, stance, set or edge (live_in, pose_live); what: the complaint about another length"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.uint8).reshape(-1)
    if len(a) != n:
        raise ValueError(what)
    return a


def _edges(edge_a, edge_b):
    edge_a = np.ascontiguousarray(edge_a, np.int32).reshape(-1)
    edge_b = np.ascontiguousarray(edge_b, np.int32).reshape(-1)
    if len(edge_a) != len(edge_b):
        raise ValueError("edge_a / edge_b: one pose index each per edge")
    return edge_a, edge_b


def _posed_indices(n, pose_idx, leg_idx):
    pi = None if pose_idx is None else np.ascontiguousarray(pose_idx, np.int32).reshape(n)
    li = None if leg_idx is None else np.ascontiguousarray(leg_idx, np.uint8).reshape(n)
    return pi, li


def device_count():
    return load().lrm_device_count()


def set_mode(mode):
    check(load().lrm_set_mode(mode))


def get_mode():
    return load().lrm_get_mode()


# ---- leg factories (static_variables.cpp:6-93) -------------------------------------------
def leg_factory(azimut, body2coxa, coxa_pitch_deg, coxa2tibia, tibia2femur, femur2tip,
                coxa_angle_deg, femur_angle_deg, tibia_angle_deg, tib_abs_pos, tib_abs_neg):
    out = np.zeros(14, np.float32)
    load().lrm_leg_factory(azimut, body2coxa, coxa_pitch_deg, coxa2tibia, tibia2femur, femur2tip,
                           coxa_angle_deg, femur_angle_deg, tibia_angle_deg, tib_abs_pos, tib_abs_neg,
                           _ptr(out))
    return out


def get_M2_leg(azimut=0.0):
    out = np.zeros(14, np.float32)
    load().lrm_get_M2_leg(azimut, _ptr(out))
    return out


def get_moonbot_leg(azimut=0.0):
    out = np.zeros(14, np.float32)
    load().lrm_get_moonbot_leg(azimut, _ptr(out))
    return out


def rotate_leg_data(quat, leg):
    out = np.zeros(14, np.float32)
    load().lrm_rotate_leg_data(_ptr(_f32(quat, (4,))), _ptr(_f32(leg, (14,))), _ptr(out))
    return out


# ---- host-buffer drop-ins (apply_kernel, cross_compiled.cu:33-79) -------------------------
def apply_reach(xyz, leg, quat=None):
    """-> (mask uint8[n], kernel milliseconds); GPU."""
    xyz = _f32(xyz, (-1, 3))
    mask = np.zeros(len(xyz), np.uint8)
    ms = C.c_float(0)
    check(load().lrm_reach(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask),
                           C.addressof(ms)))
    return mask, ms.value


def apply_dist(xyz, leg, quat=None):
    """-> (distance float32[n,3], validity uint8[n], kernel milliseconds); GPU."""
    xyz = _f32(xyz, (-1, 3))
    d = np.zeros_like(xyz)
    v = np.zeros(len(xyz), np.uint8)
    ms = C.c_float(0)
    check(load().lrm_dist(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(d), _ptr(v),
                          C.addressof(ms)))
    return d, v, ms.value


def apply_reach_dist(xyz, leg, quat=None):
    xyz = _f32(xyz, (-1, 3))
    d = np.zeros_like(xyz)
    m = np.zeros(len(xyz), np.uint8)
    ms = C.c_float(0)
    check(load().lrm_reach_dist(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(m), _ptr(d),
                                C.addressof(ms)))
    return m, d, ms.value


def tol_prepare(leg, quat=None, n_max=0, stream=None):
    """lrm_tol_prepare: LRM_MODE_TOL's tables and queues for (leg, orientation) and clouds of up to n_max points, ahead of time"""
    check(load().lrm_tol_prepare(_ptr(_f32(leg, (14,))), _ptr(_quat(quat)), n_max, stream))


def last_table_build_ms():
    """milliseconds the most recent plane-table build took (-1.0: none yet)"""
    ms = C.c_float(0)
    check(load().lrm_tol_table_build_ms(C.byref(ms)))
    return float(ms.value)


def release_workspaces():
    load().lrm_release_workspaces()


def shard_bounds(n, world, rank, align=64):
    """lrm_shard_bounds: the C ABI's shard arithmetic (equal to lrm_amd.shard.shard_bounds)"""
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    check(load().lrm_shard_bounds(n, world, rank, align, C.addressof(lo), C.addressof(hi)))
    return int(lo.value), int(hi.value)


def apply_reach_dist_multi(xyz, leg, quat=None, ndev=1, devices=None, want_bits=True):
    """lrm_reach_dist_multi: the fused kernels over ndev devices of this process + RCCL gather of the bit words
    -> (mask, vectors, gathered words or None, kernel ms per device)"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    d = np.zeros_like(xyz)
    m = np.zeros(n, np.uint8)
    bits = np.zeros((n + 63) // 64, np.uint64) if want_bits else None
    ms = np.zeros(ndev, np.float32)
    devs = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
    check(load().lrm_reach_dist_multi(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), ndev,
                                      None if devs is None else _ptr(devs), _ptr(m), _ptr(d),
                                      None if bits is None else _ptr(bits), _ptr(ms)))
    return m, d, bits, ms


# ---- CPU entry points (apply_reach_cpu / apply_dist_cpu, cross_compiled.cu:163-181) --------
def apply_reach_cpu(xyz, leg, quat=None):
    xyz = _f32(xyz, (-1, 3))
    mask = np.zeros(len(xyz), np.uint8)
    ms = C.c_double(0)
    check(load().lrm_reach_cpu(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask),
                               C.addressof(ms)))
    return mask, ms.value


def apply_dist_cpu(xyz, leg, quat=None):
    xyz = _f32(xyz, (-1, 3))
    d = np.zeros_like(xyz)
    v = np.zeros(len(xyz), np.uint8)
    ms = C.c_double(0)
    check(load().lrm_dist_cpu(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(d), _ptr(v),
                              C.addressof(ms)))
    return d, v, ms.value


POSE_RECORD_BYTES = 512  # lrm_posed_workspace_bytes(1, 1)


def _posed_tables(quats, body, legs):
    quats = _f32(quats).reshape(-1, 4)
    body = None if body is None else _f32(body).reshape(-1, 3)
    if body is not None and len(body) != len(quats):
        raise ValueError("body: one position per pose")
    return quats, body, _f32(legs).reshape(-1, 14)


def apply_reach_dist_posed_cpu(xyz, pose_idx, leg_idx, quats, body, legs):
    """lrm_reach_dist_posed_cpu: query i = (xyz[i], pose pose_idx[i], leg leg_idx[i]) on the host; pose_idx (int32) /
    leg_idx (uint8) None = pose 0 / leg 0 for all -> (mask uint8[n], valid uint8[n], field float32[n, 3], ms)"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    quats, body, legs = _posed_tables(quats, body, legs)
    pi, li = _posed_indices(n, pose_idx, leg_idx)
    m, v, d = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros_like(xyz)
    ms = C.c_double(0)
    check(load().lrm_reach_dist_posed_cpu(_ptr(xyz), n, _ptr(pi), _ptr(li), _ptr(quats), _ptr(body), len(quats), _ptr(legs),
                                          len(legs), _ptr(m), _ptr(v), _ptr(d), C.addressof(ms)))
    return m, v, d, ms.value


def dbg_pose_compile_host(quats, body, legs):
    """the pose records the host compiler makes -> uint8[nposes, nlegs, POSE_RECORD_BYTES]"""
    quats, body, legs = _posed_tables(quats, body, legs)
    out = np.zeros((len(quats), len(legs), POSE_RECORD_BYTES), np.uint8)
    check(load().lrm_dbg_pose_compile_host(_ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs), _ptr(out)))
    return out


def dbg_compile_leg_head(leg, quat=None):
    """the first 480 bytes of lrm_compile_leg(leg, quat, 1) -> uint8[480]"""
    out = np.zeros(480, np.uint8)
    check(load().lrm_dbg_compile_leg_head(_ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(out)))
    return out


# ---- joint angles (lrm_ik_*, lrm_fk_*) ------------------------------------------------------
IK_NONE, IK_REACHED, IK_NEAREST, IK_MODEL_GAP, IK_FAR_GAP = 0, 1, 2, 3, 4  # LRM_IK_* status bytes


def apply_ik_cpu(xyz, leg, quat=None, seed=None):
    """lrm_ik_cpu: joint angles that put the tip on each point, or as near as the limits allow
    -> (angles float32[n, 3] {coxa, femur, tibia}, status uint8[n] LRM_IK_*, ms); seed None = mid-range of the limits"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    if seed is not None:
        seed = _f32(seed)
        if seed.shape != (n, 3):
            raise ValueError("seed: one (coxa, femur, tibia) triple per point")
    ang = np.zeros((n, 3), np.float32)
    st = np.zeros(n, np.uint8)
    ms = C.c_double(0)
    check(load().lrm_ik_cpu(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(seed), _ptr(ang), _ptr(st),
                            C.addressof(ms)))
    return ang, st, ms.value


def apply_fk_cpu(angles, leg, quat=None):
    """lrm_fk_cpu: tip positions of joint angles (float32[n, 3] {coxa, femur, tibia}) -> (xyz float32[n, 3], ms)"""
    ang = _f32(angles, (-1, 3))
    xyz = np.zeros_like(ang)
    ms = C.c_double(0)
    check(load().lrm_fk_cpu(_ptr(ang), len(ang), _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(xyz), C.addressof(ms)))
    return xyz, ms.value


POSE_IK_RECORD_BYTES = 128  # lrm_posed_ik_workspace_bytes(1, 1)


def apply_ik_posed_cpu(xyz, pose_idx, leg_idx, quats, body, legs, target_idx=None, seed=None):
    """lrm_ik_posed_cpu: query i = (target target_idx[i] of xyz, or target i; pose pose_idx[i]; leg leg_idx[i]) on the
    host, p = target - body[pose]; indices None = target i / pose 0 / leg 0; seed None or float32[n, 3] per query
    -> (angles float32[n, 3], status uint8[n], ms); out-of-range indices (target_idx -1 included): status 0, nan"""
    xyz = _f32(xyz, (-1, 3))
    ti = None if target_idx is None else np.ascontiguousarray(target_idx, np.int32).reshape(-1)
    n = len(xyz) if ti is None else len(ti)
    quats, body, legs = _posed_tables(quats, body, legs)
    pi, li = _posed_indices(n, pose_idx, leg_idx)
    if seed is not None:
        seed = _f32(seed)
        if seed.shape != (n, 3):
            raise ValueError("seed: one (coxa, femur, tibia) triple per query")
    ang, st = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    ms = C.c_double(0)
    check(load().lrm_ik_posed_cpu(_ptr(xyz), len(xyz), _ptr(ti), n, _ptr(pi), _ptr(li), _ptr(quats), _ptr(body), len(quats),
                                  _ptr(legs), len(legs), _ptr(seed), _ptr(ang), _ptr(st), C.addressof(ms)))
    return ang, st, ms.value


def apply_fk_posed_cpu(angles, pose_idx, leg_idx, quats, body, legs):
    """lrm_fk_posed_cpu: tip of angles[i] for (legs[leg_idx[i]], quats[pose_idx[i]]) + body[pose] -> (xyz float32[n, 3], ms)"""
    ang = _f32(angles, (-1, 3))
    n = len(ang)
    quats, body, legs = _posed_tables(quats, body, legs)
    pi, li = _posed_indices(n, pose_idx, leg_idx)
    xyz = np.zeros_like(ang)
    ms = C.c_double(0)
    check(load().lrm_fk_posed_cpu(_ptr(ang), n, _ptr(pi), _ptr(li), _ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs),
                                  _ptr(xyz), C.addressof(ms)))
    return xyz, ms.value


def dbg_pose_ik_compile_host(quats, legs):
    """the IK table the host makes -> uint8[nposes, nlegs, POSE_IK_RECORD_BYTES]"""
    quats, _, legs = _posed_tables(quats, None, legs)
    out = np.zeros((len(quats), len(legs), POSE_IK_RECORD_BYTES), np.uint8)
    check(load().lrm_dbg_pose_ik_compile_host(_ptr(quats), len(quats), _ptr(legs), len(legs), _ptr(out)))
    return out


POSE_FOOTHOLD_BYTES = 32  # lrm_posed_footholds_workspace_bytes(1, 1)


def dbg_pose_footholds_compile_host(quats, legs, nominal=None):
    """the foothold table the host makes -> float32[nposes, nlegs, 8]: {cull_center[3], cull_r2, nominal_w[3], pad}"""
    quats, _, legs = _posed_tables(quats, None, legs)
    nom = _nominal(nominal, len(legs))
    out = np.zeros((len(quats), len(legs), POSE_FOOTHOLD_BYTES // 4), np.float32)
    check(load().lrm_dbg_pose_footholds_compile_host(_ptr(quats), len(quats), _ptr(legs), len(legs), _ptr(nom), _ptr(out)))
    return out


def footholds_posed_cpu(targets, quats, body, legs, nominal=None):
    """lrm_footholds_posed_cpu: per (leg, pose) the number of targets with reachability_global(t - body[pose], legs[leg],
    quats[pose]), the index of the reachable target nearest body[pose] + nominal_w (nominal (nlegs, 3) in the BODY frame,
    None = zero; -1 if none), its squared distance (+inf if none), and per pose whether every leg has one; serial host
    loop, no culling -> (count int32[nlegs, nposes], best int32[nlegs, nposes], best_d2 float32[nlegs, nposes],
    all_legs uint8[nposes], ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nom = _nominal(nominal, len(legs))
    shape = (len(legs), len(quats))
    count, best, best_d2 = np.zeros(shape, np.int32), np.zeros(shape, np.int32), np.zeros(shape, np.float32)
    all_legs = np.zeros(len(quats), np.uint8)
    ms = C.c_double(0)
    check(load().lrm_footholds_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs),
                                         _ptr(nom), _ptr(count), _ptr(best), _ptr(best_d2), _ptr(all_legs), C.addressof(ms)))
    return count, best, best_d2, all_legs, ms.value


def foothold_lists_posed_cpu(targets, quats, body, legs, offsets, capacity=None, nominal=None, idx=None, d2=None, written=None,
                             want_d2=True, want_written=True):
    """lrm_foothold_lists_posed_cpu: per (leg, pose) segment o = l*nposes + p of offsets (int64[nlegs*nposes + 1], any
    values) the reachable targets in ascending index, as far as the segment has room (include/lrm.h); serial host loop,
    no culling.  capacity None = len(idx), or offsets[-1] without idx.  idx / d2 / written given are written in place
    (whatever else they hold survives); want_d2 / want_written False pass NULL.
    -> (idx int32[capacity], d2 float32[capacity] or None, written int32[nlegs, nposes] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nom = _nominal(nominal, len(legs))
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    if len(offsets) != len(legs) * len(quats) + 1:
        raise ValueError("offsets: nlegs * nposes + 1 entries")
    if capacity is None:
        capacity = len(idx) if idx is not None else max(int(offsets[-1]), 0)
    if idx is None:
        idx = np.zeros(capacity, np.int32)
    if d2 is None and want_d2:
        d2 = np.zeros(capacity, np.float32)
    if written is None and want_written:
        written = np.zeros((len(legs), len(quats)), np.int32)
    for a, dt, n, what in ((idx, np.int32, capacity, "idx"), (d2, np.float32, capacity, "d2"),
                           (written, np.int32, len(legs) * len(quats), "written")):
        if a is not None and not (a.dtype == dt and a.flags.c_contiguous and a.size >= n):
            raise ValueError(f"{what}: expected a contiguous {np.dtype(dt)} array of >= {n} elements")
    ms = C.c_double(0)
    check(load().lrm_foothold_lists_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs),
                                              len(legs), _ptr(nom), _ptr(offsets), capacity, _ptr(idx),
                                              _ptr(d2) if want_d2 else None, _ptr(written) if want_written else None,
                                              C.addressof(ms)))
    return idx, d2 if want_d2 else None, written if want_written else None, ms.value


def foothold_edges_posed_cpu(targets, quats, body, legs, edge_a, edge_b, nominal=None, want_d2=True, want_all_legs=True):
    """lrm_foothold_edges_posed_cpu: per (leg, edge) the number of targets leg reaches under pose edge_a[e] AND under pose
    edge_b[e], the common target with the smallest d2_a + d2_b (one float32 add of footholds_posed_cpu's two d2; -1 if
    none), that sum (+inf if none), and per edge whether every leg has one.  An edge with an index outside
    [0, nposes) gives 0, -1, +inf, 0.  Serial host loop, no culling; want_d2 / want_all_legs False pass NULL.
    -> (count int32[nlegs, nedges], best int32[nlegs, nedges], best_d2 float32[nlegs, nedges] or None,
    all_legs uint8[nedges] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nom = _nominal(nominal, len(legs))
    edge_a, edge_b = _edges(edge_a, edge_b)
    shape = (len(legs), len(edge_a))
    count, best = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    best_d2 = np.zeros(shape, np.float32) if want_d2 else None
    all_legs = np.zeros(len(edge_a), np.uint8) if want_all_legs else None
    ms = C.c_double(0)
    check(load().lrm_foothold_edges_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs),
                                              _ptr(nom), _ptr(edge_a), _ptr(edge_b), len(edge_a), _ptr(count), _ptr(best),
                                              _ptr(best_d2), _ptr(all_legs), C.addressof(ms)))
    return count, best, best_d2, all_legs, ms.value


def foothold_misses_posed_cpu(targets, quats, body, legs, margin, count_in=None, want_m2=True, want_shift=True, want_near=True):
    """lrm_foothold_misses_posed_cpu: per (leg, pose) not skipped by count_in (int32[nlegs, nposes] or None; > 0 skips) the
    unreachable target inside the entry's sphere widened by margin (mm, >= 0 or +inf) whose distance_global vector is the
    shortest (-1 if none), that squared length m2 (+inf if none), the vector itself -- the body translation that puts the
    target on the workspace boundary (nan if none) -- and the number of unreachable candidates.  Serial host loop, no box
    culling; want_* False pass NULL.
    -> (miss int32[nlegs, nposes], m2 float32[nlegs, nposes] or None, shift float32[3, nlegs, nposes] or None,
    near int32[nlegs, nposes] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    shape = (len(legs), len(quats))
    if count_in is not None:
        count_in = np.ascontiguousarray(count_in, np.int32)
        if count_in.size != shape[0] * shape[1]:
            raise ValueError("count_in: nlegs * nposes entries")
    miss = np.zeros(shape, np.int32)
    m2 = np.zeros(shape, np.float32) if want_m2 else None
    shift = np.zeros((3,) + shape, np.float32) if want_shift else None
    near = np.zeros(shape, np.int32) if want_near else None
    ms = C.c_double(0)
    check(load().lrm_foothold_misses_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs),
                                               float(margin), _ptr(count_in), _ptr(miss), _ptr(m2),
                                               _ptr(shift[0]) if want_shift else None, _ptr(shift[1]) if want_shift else None,
                                               _ptr(shift[2]) if want_shift else None, _ptr(near), C.addressof(ms)))
    return miss, m2, shift, near, ms.value


def foothold_support_posed_cpu(targets, quats, body, legs, nominal=None, pose_live=None, want_d2=True, want_mask=True):
    """lrm_foothold_support_posed_cpu: per (leg, target) the number of live poses p (pose_live uint8[nposes] or None = all)
    with reachability_global(t - body[p], legs[leg], quats[p]), the reaching pose with the smallest footholds_posed_cpu d2
    of that triple (ties: the smaller pose; -1 if none), that d2 (+inf if none), and per target the bit mask of the legs
    with a reaching pose.  Serial host loop over every (target, leg, pose), no culling; want_* False pass NULL.
    -> (count int32[nlegs, nt], best_pose int32[nlegs, nt], best_d2 float32[nlegs, nt] or None, legs_mask uint8[nt] or
    None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nom = _nominal(nominal, len(legs))
    pose_live = _u8_per(pose_live, len(quats), "pose_live: one byte per pose")
    shape = (len(legs), len(targets))
    count, best = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    best_d2 = np.zeros(shape, np.float32) if want_d2 else None
    mask = np.zeros(len(targets), np.uint8) if want_mask else None
    ms = C.c_double(0)
    check(load().lrm_foothold_support_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), len(legs),
                                                _ptr(nom), _ptr(pose_live), _ptr(count), _ptr(best), _ptr(best_d2), _ptr(mask),
                                                C.addressof(ms)))
    return count, best, best_d2, mask, ms.value


def dbg_foothold_support_grid(nt, nposes):
    """lrm_dbg_foothold_support_grid: the launch shape of the per-target support call for nt targets and nposes poses --
    dict with the poses per pose chunk, the slices of the pose range per 64-target chunk, the most poses one slice walks
    (slice s takes the pose chunks c with c % slices == s) and the workgroups of the traversal.  Host only."""
    out = np.zeros(4, np.uint64)
    check(load().lrm_dbg_foothold_support_grid(int(nt), int(nposes), _ptr(out)))
    return {"pose_chunk": int(out[0]), "slices": int(out[1]), "poses_per_slice": int(out[2]), "blocks": int(out[3])}


def body_clearance_posed_cpu(targets, quats, body, legs, radius, plus_z, minus_z, floor_z=None, live_in=None, want_height=True,
                              want_free=True):
    """lrm_body_clearance_posed_cpu: per pose not skipped by live_in (uint8[nposes] or None; 0 skips) the number of targets
    inside the body cylinder (radius, plus_z, minus_z) in the BODY frame, the target of the column (radius, plus_z, floor_z;
    floor_z None = minus_z) that stands highest over the belly plane (-1 if none), that height vz - minus_z (-inf if none),
    and whether the pose is live and free of hits.  Serial host loop over every (pose, target), no culling; want_* False
    pass NULL.  -> (hits int32[nposes], top int32[nposes], height float32[nposes] or None, free uint8[nposes] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    live_in = _u8_per(live_in, len(quats), "live_in: one byte per pose")
    n = len(quats)
    hits, top = np.zeros(n, np.int32), np.zeros(n, np.int32)
    height = np.zeros(n, np.float32) if want_height else None
    free = np.zeros(n, np.uint8) if want_free else None
    ms = C.c_double(0)
    check(load().lrm_body_clearance_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), n, _ptr(legs), len(legs),
                                              float(radius), float(plus_z), float(minus_z),
                                              float(minus_z if floor_z is None else floor_z), _ptr(live_in), _ptr(hits), _ptr(top),
                                              _ptr(height), _ptr(free), C.addressof(ms)))
    return hits, top, height, free, ms.value


def _leg_angles(angles, nlegs, nposes):
    angles = _f32(angles)
    if angles.size != nlegs * nposes * 3:
        raise ValueError("angles: one (coxa, femur, tibia) triple per (leg, pose), at [l*nposes + p]")
    return angles.reshape(nlegs * nposes, 3)


def leg_clearance_posed_cpu(targets, quats, body, legs, angles, radius, margin=0.0, tip_clear=0.0, live_in=None, want_pen=True,
                            want_free=True):
    """lrm_leg_clearance_posed_cpu: per (leg, pose) not skipped by live_in (uint8[nposes] or None; 0 skips) the number of
    targets inside one of the leg's three links (capsules of radius[k] about coxa, femur, tibia under angles[l*nposes + p] =
    (coxa, femur, tibia), the tibia ending tip_clear short of the foot), the bit mask of the links hit, the target within
    margin of a link that stands deepest (-1 if none), its pen = radius - distance (-inf if none), and per pose whether it is
    live and no leg is hit.  angles: float32 [nlegs*nposes, 3], apply_ik_posed_cpu's output under the [l*nposes + p] layout.
    Serial host loop over every (pose, leg, target), no culling; want_* False pass NULL.
    -> (hits int32[nlegs, nposes], links uint8[nlegs, nposes], worst int32[nlegs, nposes], pen float32[nlegs, nposes] or None,
    free uint8[nposes] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    n, nl = len(quats), len(legs)
    angles = _leg_angles(angles, nl, n)
    radius = _f32(radius, (3,))
    live_in = _u8_per(live_in, n, "live_in: one byte per pose")
    hits, links, worst = np.zeros((nl, n), np.int32), np.zeros((nl, n), np.uint8), np.zeros((nl, n), np.int32)
    pen = np.zeros((nl, n), np.float32) if want_pen else None
    free = np.zeros(n, np.uint8) if want_free else None
    ms = C.c_double(0)
    check(load().lrm_leg_clearance_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), n, _ptr(legs), nl, _ptr(angles),
                                             _ptr(radius), float(margin), float(tip_clear), _ptr(live_in), _ptr(hits), _ptr(links),
                                             _ptr(worst), _ptr(pen), _ptr(free), C.addressof(ms)))
    return hits, links, worst, pen, free, ms.value


def leg_joints_posed_cpu(angles, quats, body, legs, tip_clear=0.0):
    """lrm_leg_joints_posed_cpu: the four joints (coxa joint, femur joint, knee, tibia end tip_clear short of the foot) of
    every (leg, pose) under angles[l*nposes + p], body[p] added -> (joints float32[nlegs, nposes, 4, 3], ms)"""
    quats, body, legs = _posed_tables(quats, body, legs)
    n, nl = len(quats), len(legs)
    angles = _leg_angles(angles, nl, n)
    out = np.zeros((nl, n, 4, 3), np.float32)
    ms = C.c_double(0)
    check(load().lrm_leg_joints_posed_cpu(_ptr(angles), _ptr(quats), _ptr(body), n, _ptr(legs), nl, float(tip_clear), _ptr(out),
                                          C.addressof(ms)))
    return out, ms.value


def stance_lift(lift, nlegs):
    """The lift sets of the stance stability calls as uint8: None = [0] (every foot planted), "each" = [0, 1<<0, ...,
    1<<(nlegs-1)] (nothing lifted, then each leg alone), otherwise 1 to 256 bit masks (bit l = leg l is in the air)."""
    if lift is None:
        return np.zeros(1, np.uint8)
    if isinstance(lift, str):
        if lift != "each":
            raise ValueError('lift: None, "each" or 1 to 256 bit masks')
        return np.array([0] + [1 << l for l in range(nlegs)], np.uint8)
    a = np.asarray(lift)
    if a.ndim != 1 or not 1 <= a.size <= 256 or a.dtype.kind not in "iub" or (a.size and (a.min() < 0 or a.max() > 255)):
        raise ValueError('lift: None, "each" or 1 to 256 bit masks in 0..255')
    return np.ascontiguousarray(a, np.uint8)


def _stance_host(com, plane):
    com = None if com is None else _f32(com, (3,))
    plane = None if plane is None else _f32(plane, (6,))
    return com, plane


def stance_stability_cpu(targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0,
                         live_in=None, want_edge=True, want_feet=True):
    """lrm_stance_stability_cpu: per stance s (pose pose_idx[s], or pose s with pose_idx None; one target index per leg,
    foot int32[nlegs, nstances]: footholds_posed_cpu's best) and per lift set m (stance_lift), the distance of the centre of
    mass (com, BODY frame, rotated by the pose; None = the body origin) from the nearest edge of the support polygon of the
    planted feet, in the plane normal to gravity (plane None: the caller's x, y; else two 3-vectors spanning it): margin
    (-inf: fewer than three planted feet, a degenerate polygon or a dead stance), the edge's code i*8 + j (255 with -inf),
    stable = margin > min_margin, and per stance the bit mask of the valid feet.  live_in: uint8[nstances] or None; 0 = dead.
    Serial host loop over every (stance, lift set); want_* False pass NULL.
    -> (margin float32[nmasks, nstances], edge uint8[nmasks, nstances] or None, stable uint8[nmasks, nstances],
    feet uint8[nstances] or None, ms)"""
    targets = _f32(targets, (-1, 3))
    quats = _f32(quats, (-1, 4))
    n = len(quats)
    body = None if body is None else _f32(body, (n, 3))
    foot = np.ascontiguousarray(foot, np.int32)
    if foot.ndim != 2:
        raise ValueError("foot: int32 [nlegs, nstances]")
    nl, ns = foot.shape
    if pose_idx is not None:
        pose_idx = np.ascontiguousarray(pose_idx, np.int32).reshape(-1)
        if len(pose_idx) != ns:
            raise ValueError("pose_idx: one pose per stance")
    live_in = _u8_per(live_in, ns, "live_in: one byte per stance")
    com, plane = _stance_host(com, plane)
    lift = stance_lift(lift, nl)
    nm = len(lift)
    margin, stable = np.zeros((nm, ns), np.float32), np.zeros((nm, ns), np.uint8)
    edge = np.zeros((nm, ns), np.uint8) if want_edge else None
    feet = np.zeros(ns, np.uint8) if want_feet else None
    ms = C.c_double(0)
    check(load().lrm_stance_stability_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), n, _ptr(pose_idx), _ptr(foot), ns, nl,
                                          _ptr(com), _ptr(plane), _ptr(lift), nm, float(min_margin), _ptr(live_in), _ptr(margin),
                                          _ptr(edge), _ptr(stable), _ptr(feet), C.addressof(ms)))
    return margin, edge, stable, feet, ms.value


def self_clearance_posed_cpu(quats, legs, angles, radius, margin=0.0, tip_clear=0.0, pose_idx=None, live_in=None, want_pen=True,
                             want_free=True):
    """lrm_self_clearance_posed_cpu: do the legs fit next to each other.  A set s is a pose (pose_idx[s], or pose s with
    pose_idx None) and one (coxa, femur, tibia) triple per leg, angles float32 [nlegs*nsets, 3] at [l*nsets + s]:
    apply_ik_posed_cpu's output under the [l*nposes + p] layout.  Every link of a leg (capsules of radius[k] about coxa,
    femur, tibia, the tibia ending tip_clear short of the foot; radius 0 = not tested) is tested against every link of every
    OTHER leg: per (leg, set) the number of link pairs that hit, the bit mask of the legs hit, the bit mask of the own links
    in a hit, the pair within margin that stands deepest as code other*9 + own_link*3 + other_link (255 if none) and its
    pen = radius sum - distance (-inf if none); per set whether it is live and no leg is hit.  live_in: uint8[nsets] or None;
    0 = dead, as is a pose index outside the poses.  Serial host loop over every (set, pair); want_* False pass NULL.
    -> (hits int32, with_ uint8, links uint8, worst uint8, pen float32 or None, each [nlegs, nsets]; free uint8[nsets] or
    None; ms)"""
    quats = _f32(quats, (-1, 4))
    legs = _f32(legs, (-1, 14))
    n, nl = len(quats), len(legs)
    angles = _f32(angles)
    if nl == 0 or angles.size % (3 * nl):
        raise ValueError("angles: one (coxa, femur, tibia) triple per (leg, set), at [l*nsets + s]")
    ns = angles.size // (3 * nl)
    angles = angles.reshape(nl * ns, 3)
    radius = _f32(radius, (3,))
    if pose_idx is not None:
        pose_idx = np.ascontiguousarray(pose_idx, np.int32).reshape(-1)
        if len(pose_idx) != ns:
            raise ValueError("pose_idx: one pose per set")
    live_in = _u8_per(live_in, ns, "live_in: one byte per set")
    hits = np.zeros((nl, ns), np.int32)
    with_, links, worst = (np.zeros((nl, ns), np.uint8) for _ in range(3))
    pen = np.zeros((nl, ns), np.float32) if want_pen else None
    free = np.zeros(ns, np.uint8) if want_free else None
    ms = C.c_double(0)
    check(load().lrm_self_clearance_posed_cpu(_ptr(quats), n, _ptr(legs), nl, _ptr(pose_idx), ns, _ptr(angles), _ptr(radius),
                                              float(margin), float(tip_clear), _ptr(live_in), _ptr(hits), _ptr(with_), _ptr(links),
                                              _ptr(worst), _ptr(pen), _ptr(free), C.addressof(ms)))
    return hits, with_, links, worst, pen, free, ms.value


def _tau_max(tau_max):
    tau_max = _f32(tau_max).reshape(-1)
    if len(tau_max) != 3:
        raise ValueError("tau_max: three values (coxa, femur, tibia joint), each > 0, inf allowed")
    return tau_max


LOADS_DEAD, LOADS_ALL, LOADS_DROPPED, LOADS_TRIPOD, LOADS_NONE = range(5)


def stance_loads_posed_cpu(quats, legs, angles, tau_max, pose_idx=None, com=None, plane=None, lift=None, live_in=None,
                           want_peak_at=True, want_load=True, want_tau=True):
    """lrm_stance_loads_posed_cpu: what every planted foot carries and what the joints must hold.  A set s is a pose
    (pose_idx[s], or pose s with pose_idx None) and one (coxa, femur, tibia) triple per leg, angles float32 [nlegs*nsets, 3]
    at [l*nsets + s]: apply_ik_posed_cpu's output in that layout.  Frictionless point contacts pushing along `up` (the normal
    of `plane`, None: +z), massless legs, weight 1: loads are fractions of the weight, torques load x mm.  com, plane and lift
    are stance_stability_cpu's; tau_max: three limits (coxa, femur, tibia; > 0, inf allowed) in the torques' unit.  Per
    (lift set, set): status (LOADS_DEAD, _ALL, _DROPPED, _TRIPOD, _NONE), holdable = status 1..3 and every |tau| <= tau_max,
    peak = the largest |tau| / tau_max (-inf if none), peak_at = its code l*4 + j (255 if none); per (lift set, leg, set) the
    load; per (lift set, leg, joint, set) the torque.  live_in: uint8[nsets] or None; 0 = dead, as is a pose index outside the
    poses.  Serial host loop; want_* False pass NULL.
    -> (status uint8[nmasks, nsets], holdable uint8[nmasks, nsets], peak float32[nmasks, nsets], peak_at uint8[nmasks, nsets] or
    None, load float32[nmasks, nlegs, nsets] or None, tau float32[nmasks, nlegs, 3, nsets] or None, ms)"""
    quats = _f32(quats, (-1, 4))
    legs = _f32(legs, (-1, 14))
    n, nl = len(quats), len(legs)
    angles = _f32(angles)
    if nl == 0 or angles.size % (3 * nl):
        raise ValueError("angles: one (coxa, femur, tibia) triple per (leg, set), at [l*nsets + s]")
    ns = angles.size // (3 * nl)
    angles = angles.reshape(nl * ns, 3)
    if pose_idx is not None:
        pose_idx = np.ascontiguousarray(pose_idx, np.int32).reshape(-1)
        if len(pose_idx) != ns:
            raise ValueError("pose_idx: one pose per set")
    live_in = _u8_per(live_in, ns, "live_in: one byte per set")
    com, plane = _stance_host(com, plane)
    lift = stance_lift(lift, nl)
    tau_max = _tau_max(tau_max)
    nm = len(lift)
    status, holdable, peak = np.zeros((nm, ns), np.uint8), np.zeros((nm, ns), np.uint8), np.zeros((nm, ns), np.float32)
    peak_at = np.zeros((nm, ns), np.uint8) if want_peak_at else None
    load = np.zeros((nm, nl, ns), np.float32) if want_load else None
    tau = np.zeros((nm, nl, 3, ns), np.float32) if want_tau else None
    ms = C.c_double(0)
    check(lib().lrm_stance_loads_posed_cpu(_ptr(quats), n, _ptr(legs), nl, _ptr(pose_idx), ns, _ptr(angles), _ptr(com), _ptr(plane),
                                                _ptr(lift), nm, _ptr(tau_max), _ptr(live_in), _ptr(status), _ptr(holdable), _ptr(peak),
                                                _ptr(peak_at), _ptr(load), _ptr(tau), C.addressof(ms)))
    return status, holdable, peak, peak_at, load, tau, ms.value


def _links_mask(links):
    links = int(links)
    if not 0 <= links <= 255:
        raise ValueError("links: a bit mask of the links to test (bit 0 coxa, 1 femur, 2 tibia)")
    return links


def trunk_clearance_posed_cpu(quats, legs, angles, radius, trunk_radius, plus_z, minus_z, margin=0.0, tip_clear=0.0, links=0b110,
                              pose_idx=None, live_in=None, want_pen=True, want_free=True):
    """lrm_trunk_clearance_posed_cpu: do the legs stay out of the robot's own trunk.  Sets, angles float32 [nlegs*nsets, 3] at
    [l*nsets + s], radius, margin, tip_clear, pose_idx and live_in are self_clearance_posed_cpu's.  The trunk is
    body_clearance_posed_cpu's cylinder (trunk_radius, plus_z, minus_z; body frame, axis z, about the body origin).  links: bit k
    set = link k (0 coxa, 1 femur, 2 tibia) is tested; the coxa link starts at its mount on the trunk, hence 0b110.  Per
    (leg, set): the bit mask of the links that hit the trunk, the link within margin that stands deepest (255 if none) and its
    pen = radius - distance (-inf if none); per set whether it is live and no leg hits.  Serial host loop; want_* False pass NULL.
    -> (links uint8, worst uint8, pen float32 or None, each [nlegs, nsets]; free uint8[nsets] or None; ms)"""
    quats = _f32(quats, (-1, 4))
    legs = _f32(legs, (-1, 14))
    n, nl = len(quats), len(legs)
    angles = _f32(angles)
    if nl == 0 or angles.size % (3 * nl):
        raise ValueError("angles: one (coxa, femur, tibia) triple per (leg, set), at [l*nsets + s]")
    ns = angles.size // (3 * nl)
    angles = angles.reshape(nl * ns, 3)
    radius = _f32(radius, (3,))
    if pose_idx is not None:
        pose_idx = np.ascontiguousarray(pose_idx, np.int32).reshape(-1)
        if len(pose_idx) != ns:
            raise ValueError("pose_idx: one pose per set")
    live_in = _u8_per(live_in, ns, "live_in: one byte per set")
    hit, worst = (np.zeros((nl, ns), np.uint8) for _ in range(2))
    pen = np.zeros((nl, ns), np.float32) if want_pen else None
    free = np.zeros(ns, np.uint8) if want_free else None
    ms = C.c_double(0)
    check(load().lrm_trunk_clearance_posed_cpu(_ptr(quats), n, _ptr(legs), nl, _ptr(pose_idx), ns, _ptr(angles), _ptr(radius),
                                               float(margin), float(tip_clear), float(trunk_radius), float(plus_z), float(minus_z),
                                               _links_mask(links), _ptr(live_in), _ptr(hit), _ptr(worst), _ptr(pen), _ptr(free),
                                               C.addressof(ms)))
    return hit, worst, pen, free, ms.value


def _nsamples(nsamples):
    nsamples = int(nsamples)
    if nsamples < 0:
        raise ValueError("nsamples: 2 to 64 poses per edge, the ends included")
    return nsamples


def edge_transit_posed_cpu(targets, quats, body, legs, edge_a, edge_b, foot, nsamples=9, live_in=None, want_mask=True,
                           want_worst=True, want_edge=True):
    """lrm_edge_transit_posed_cpu: does a planted foot stay reachable while the body moves from pose edge_a[e] to pose edge_b[e].
    foot int32 [nlegs, nedges] = foothold_edges_posed_cpu's best as it stands (-1: the leg is in the air); nsamples poses per
    edge, the ends included: the normalised linear blend of the two quaternions (the short way round; the great arc of slerp at
    another speed) and the linear blend of the bodies; the ends are the poses themselves.  Per (leg, edge): mask (bit s = sample
    s reaches), reached (the number of bits; -1 when not planted), first_miss (the first sample that does not reach; -1 if none),
    worst (the unreachable sample with the largest squared distance_global vector; -1 if none) and that worst_d2 (0 if none);
    per edge: planted (bit l = leg l is planted), clear (live, both ends in range and every planted leg reaches at every sample)
    and advance (the number of leading samples at which every planted leg reaches; 0 for a dead edge).  Serial host loop;
    want_* False pass NULL.
    -> (mask uint64 or None, reached int32, first_miss int32, worst int32 or None, worst_d2 float32 or None, each [nlegs, nedges];
    planted uint8, clear uint8, advance int32, each [nedges] or None; ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nl = len(legs)
    edge_a, edge_b = _edges(edge_a, edge_b)
    ne = len(edge_a)
    foot = np.ascontiguousarray(foot, np.int32)
    if foot.size != nl * ne:
        raise ValueError("foot: one target index per (leg, edge), at [l*nedges + e]")
    live_in = _u8_per(live_in, ne, "live_in: one byte per edge")
    shape = (nl, ne)
    mask = np.zeros(shape, np.uint64) if want_mask else None
    reached, first_miss = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    worst = np.zeros(shape, np.int32) if want_worst else None
    worst_d2 = np.zeros(shape, np.float32) if want_worst else None
    planted = np.zeros(ne, np.uint8) if want_edge else None
    clear = np.zeros(ne, np.uint8) if want_edge else None
    advance = np.zeros(ne, np.int32) if want_edge else None
    ms = C.c_double(0)
    check(load().lrm_edge_transit_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), nl,
                                            _ptr(edge_a), _ptr(edge_b), ne, _ptr(foot), _nsamples(nsamples), _ptr(live_in), _ptr(mask),
                                            _ptr(reached), _ptr(first_miss), _ptr(worst), _ptr(worst_d2), _ptr(planted), _ptr(clear),
                                            _ptr(advance), C.addressof(ms)))
    return mask, reached, first_miss, worst, worst_d2, planted, clear, advance, ms.value


def _routes_host(nposes, edge_a, edge_b, sources, edge_live, pose_live, edge_cost):
    """the host inputs of pose_routes_cpu -> (nposes, edge_a, edge_b, sources, edge_live, pose_live, edge_cost)"""
    nposes = int(nposes)
    edge_a, edge_b = _edges(edge_a, edge_b)
    ne = len(edge_a)
    sources = np.ascontiguousarray(sources, np.int32).reshape(-1)
    edge_live = _u8_per(edge_live, ne, "edge_live: one byte per edge")
    pose_live = _u8_per(pose_live, nposes, "pose_live: one byte per pose")
    if edge_cost is not None:
        edge_cost = np.ascontiguousarray(edge_cost, np.int32).reshape(-1)
        if len(edge_cost) != ne:
            raise ValueError("edge_cost: one int32 per edge")
    return nposes, edge_a, edge_b, sources, edge_live, pose_live, edge_cost


def pose_routes_cpu(nposes, edge_a, edge_b, sources, edge_live=None, pose_live=None, edge_cost=None, direction=0, want_cost=True,
                    want_hops=True, want_pred_edge=True, want_pred_pose=True):
    """lrm_pose_routes_cpu: shortest routes over the pose graph with integer costs, from the poses in `sources`.  edge_a / edge_b
    int32 [nedges]; edge_live uint8 [nedges] and pose_live uint8 [nposes] or None (0 = dead); edge_cost int32 [nedges] or None
    (1 per edge: cost equals hops; a negative cost makes the edge dead); direction 0 both ways, 1 a -> b, 2 b -> a.  An edge is
    usable iff it is live, both ends are live poses in range and its cost is >= 0; a source counts iff it is in range and live.
    The key of a pose is the lexicographic minimum of (sum of costs, number of arcs) over the walks from a source whose sum of
    costs is <= 4 294 967 294.  cost (-1 unreachable), hops (-1 unreachable), pred_edge (the smallest usable edge with a tight
    arc into the pose; -1 for a source or an unreachable pose), pred_pose (that arc's tail, or -1).  A binary-heap Dijkstra;
    want_* False pass NULL (not all four).  -> (cost int64, hops int32, pred_edge int32, pred_pose int32, each [nposes] or None;
    reached int; ms)"""
    nposes, edge_a, edge_b, sources, edge_live, pose_live, edge_cost = _routes_host(nposes, edge_a, edge_b, sources, edge_live, pose_live,
                                                                                    edge_cost)
    cost = np.zeros(nposes, np.int64) if want_cost else None
    hops = np.zeros(nposes, np.int32) if want_hops else None
    pred_edge = np.zeros(nposes, np.int32) if want_pred_edge else None
    pred_pose = np.zeros(nposes, np.int32) if want_pred_pose else None
    reached, ms = C.c_int32(0), C.c_double(0)
    check(load().lrm_pose_routes_cpu(nposes, _ptr(edge_a), _ptr(edge_b), len(edge_a), _ptr(edge_live), _ptr(pose_live), _ptr(edge_cost),
                                     _ptr(sources), len(sources), int(direction), _ptr(cost), _ptr(hops), _ptr(pred_edge), _ptr(pred_pose),
                                     C.addressof(reached), C.addressof(ms)))
    return cost, hops, pred_edge, pred_pose, int(reached.value), ms.value


def dbg_pose_routes_plan(nedges):
    """lrm_dbg_pose_routes_plan: the launch arithmetic of a relax launch of lrm_pose_routes_dev on nedges edges.  Host only."""
    out = np.zeros(4, np.uint64)
    check(load().lrm_dbg_pose_routes_plan(int(nedges), _ptr(out)))
    return dict(zip(("chunk", "grid_cap", "sweeps", "workgroups"), (int(v) for v in out)))


def pose_edges_min_dot(max_turn):
    """min_dot of the pose edge calls from the largest turn in radians: float32(cos(max_turn / 2)); None = 0, no turn test"""
    if max_turn is None:
        return 0.0
    max_turn = float(max_turn)
    if not 0.0 <= max_turn <= np.pi:
        raise ValueError("max_turn: radians in [0, pi] (None: no turn test)")
    return float(np.float32(max(np.cos(max_turn / 2.0), 0.0)))


def pose_edges_cpu(quats, body, max_step, min_dot=0.0, pose_live=None, form=0, offsets=None, capacity=None, edge_a=None, edge_b=None,
                   d2=None, cos2=None, written=None, want_d2=True, want_cos2=True, counts_only=False):
    """lrm_pose_edges_cpu: which pose can step to which, as counts and as a CSR edge list.  quats float32 [nposes, 4] in storage
    order, body float32 [nposes, 3] or None (0), pose_live uint8 [nposes] or None; max_step in mm (>= 0, inf allowed), min_dot
    in [0, 1] (pose_edges_min_dot(max_turn); 0: no turn test); form 0: row p holds the neighbours q > p, 1: all q != p.  Poses
    p != q are neighbours iff both are valid (live, finite body, squared quaternion norm finite and > 0),
    d2 = (dx*dx + dy*dy) + dz*dz <= max_step*max_step and c*c >= min_dot*min_dot * (n_p*n_q), all in float32 (include/lrm.h).
    offsets=None: the counts are taken first and offsets = their exclusive sum, capacity = offsets[-1] unless given; with
    offsets (int64 [nposes + 1], any contents) the segment rule of foothold_lists applies.  edge_a / edge_b / d2 / cos2 /
    written: buffers to write into (views of longer ones are fine), allocated when None.  A serial loop over every pair.
    -> (count int32 [nposes], offsets int64 [nposes + 1], edge_a, edge_b int32 [capacity], d2, cos2 float32 [capacity] or
    None, written int32 [nposes], ms); counts_only=True -> (count, ms)."""
    quats = _f32(quats).reshape(-1, 4)
    nposes = len(quats)
    body = None if body is None else _f32(body, (nposes, 3))
    pose_live = _u8_per(pose_live, nposes, "pose_live: one byte per pose")
    count = np.zeros(nposes, np.int32)
    ms = C.c_double(0)
    fn = load().lrm_pose_edges_cpu
    if counts_only or offsets is None:
        check(fn(_ptr(quats), _ptr(body), nposes, _ptr(pose_live), float(max_step), float(min_dot), int(form), _ptr(count), None, 0, None,
                 None, None, None, None, C.addressof(ms)))
        if counts_only:
            return count, ms.value
        offsets = np.concatenate([[0], np.cumsum(np.maximum(count, 0), dtype=np.int64)]).astype(np.int64)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    if len(offsets) != nposes + 1:
        raise ValueError("offsets: nposes + 1 entries")
    capacity = max(int(offsets[-1]), 0) if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("capacity >= 0")

    def buf(a, dtype, n, want=True):
        if a is None:
            return np.zeros(n, dtype) if want else None
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 1 and a.flags.c_contiguous and len(a) >= n):
            raise ValueError(f"expected a contiguous {np.dtype(dtype).name} array of >= {n} entries")
        return a

    edge_a, edge_b = buf(edge_a, np.int32, capacity), buf(edge_b, np.int32, capacity)
    d2, cos2 = buf(d2, np.float32, capacity, want_d2), buf(cos2, np.float32, capacity, want_cos2)
    written = buf(written, np.int32, nposes)
    check(fn(_ptr(quats), _ptr(body), nposes, _ptr(pose_live), float(max_step), float(min_dot), int(form), _ptr(count), _ptr(offsets),
             capacity, _ptr(edge_a), _ptr(edge_b), _ptr(d2), _ptr(cos2), _ptr(written), C.addressof(ms)))
    return count, offsets, edge_a, edge_b, d2, cos2, written, ms.value


def dbg_pose_edges_plan(nposes):
    """lrm_dbg_pose_edges_plan: the launch arithmetic of the pose edge kernels on nposes poses.  Host only."""
    out = np.zeros(4, np.uint64)
    check(load().lrm_dbg_pose_edges_plan(int(nposes), _ptr(out)))
    return dict(zip(("chunk", "round", "workgroups", "block"), (int(v) for v in out)))


def _swing_scalars(lift, up, foot_radius, margin, skip):
    """the host scalars of the swing transit calls: (lift, up float32[3] or None, foot_radius, margin, skip); the library
    checks their values"""
    if up is not None:
        up = np.ascontiguousarray(up, np.float32).reshape(-1)
        if len(up) != 3:
            raise ValueError("up: three floats, or None for (0, 0, 1)")
    skip = int(skip)
    if not 0 <= skip <= 63:
        raise ValueError("skip: 0 to 63 segments at either end of the path")
    return float(lift), up, float(foot_radius), float(margin), skip


def swing_transit_posed_cpu(targets, quats, body, legs, edge_a, edge_b, foot_from, foot_to, nsamples=9, lift=0.0, up=None,
                            foot_radius=0.0, margin=0.0, skip=0, live_in=None, want_mask=True, want_worst=True, want_pen=True,
                            want_edge=True):
    """lrm_swing_transit_posed_cpu: can a LIFTED foot get from target foot_from[l, e] (under pose edge_a[e]) to target
    foot_to[l, e] (under pose edge_b[e]): along a straight line with a parabolic bump of height lift along up, at nsamples
    sampled poses (edge_transit_posed_cpu's), is the moving foot reachable, and do terrain targets stand within foot_radius of
    the polyline (segments skip .. nsamples-2-skip; the two footholds themselves are never tested; foot_radius 0: no terrain
    test).  A leg with either index outside the cloud (-1) is not swinging.  Per (leg, edge): mask, reached, first_miss, worst,
    worst_d2 as edge_transit_posed_cpu's; hits (targets hit), hit_seg (the first segment hit, -1), near (the deepest target
    within foot_radius + margin, -1) and its pen (-inf); per edge: swinging (bit l) and clear (live, every swinging leg reaches at
    every sample and hits nothing).  Serial host loop without any cull; want_* False pass NULL.
    -> (mask uint64 or None, reached, first_miss int32, worst int32 or None, worst_d2 float32 or None, hits, hit_seg, near int32,
    pen float32 or None, each [nlegs, nedges]; swinging, clear uint8 [nedges] or None; ms)"""
    targets = _f32(targets, (-1, 3))
    quats, body, legs = _posed_tables(quats, body, legs)
    nl = len(legs)
    edge_a, edge_b = _edges(edge_a, edge_b)
    ne = len(edge_a)
    foot_from = np.ascontiguousarray(foot_from, np.int32)
    foot_to = np.ascontiguousarray(foot_to, np.int32)
    if foot_from.size != nl * ne or foot_to.size != nl * ne:
        raise ValueError("foot_from / foot_to: one target index per (leg, edge), at [l*nedges + e]")
    live_in = _u8_per(live_in, ne, "live_in: one byte per edge")
    lift, up, foot_radius, margin, skip = _swing_scalars(lift, up, foot_radius, margin, skip)
    shape = (nl, ne)
    mask = np.zeros(shape, np.uint64) if want_mask else None
    reached, first_miss = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    worst = np.zeros(shape, np.int32) if want_worst else None
    worst_d2 = np.zeros(shape, np.float32) if want_worst else None
    hits, hit_seg, near = np.zeros(shape, np.int32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    pen = np.zeros(shape, np.float32) if want_pen else None
    swinging = np.zeros(ne, np.uint8) if want_edge else None
    clear = np.zeros(ne, np.uint8) if want_edge else None
    ms = C.c_double(0)
    check(load().lrm_swing_transit_posed_cpu(_ptr(targets), len(targets), _ptr(quats), _ptr(body), len(quats), _ptr(legs), nl,
                                             _ptr(edge_a), _ptr(edge_b), ne, _ptr(foot_from), _ptr(foot_to), _nsamples(nsamples), lift,
                                             _ptr(up), foot_radius, margin, skip, _ptr(live_in), _ptr(mask), _ptr(reached),
                                             _ptr(first_miss), _ptr(worst), _ptr(worst_d2), _ptr(hits), _ptr(hit_seg), _ptr(near),
                                             _ptr(pen), _ptr(swinging), _ptr(clear), C.addressof(ms)))
    return mask, reached, first_miss, worst, worst_d2, hits, hit_seg, near, pen, swinging, clear, ms.value


def dbg_edge_transit_samples_host(quats, body, edge_a, edge_b, nsamples):
    """lrm_dbg_edge_transit_samples_host: the sampled path of the edge transit calls -> float32 [nedges, nsamples, 7] = the
    quaternion and the body position of every sample (nan for an edge with an end out of range)"""
    quats = _f32(quats).reshape(-1, 4)
    body = None if body is None else _f32(body).reshape(-1, 3)
    edge_a = np.ascontiguousarray(edge_a, np.int32).reshape(-1)
    edge_b = np.ascontiguousarray(edge_b, np.int32).reshape(-1)
    if len(edge_a) != len(edge_b) or (body is not None and len(body) != len(quats)):
        raise ValueError("edge_a / edge_b: one pose index each per edge; body: one position per pose")
    out = np.zeros((len(edge_a), _nsamples(nsamples), 7), np.float32)
    check(load().lrm_dbg_edge_transit_samples_host(_ptr(quats), _ptr(body), len(quats), _ptr(edge_a), _ptr(edge_b), len(edge_a),
                                                   _nsamples(nsamples), _ptr(out)))
    return out


def dbg_trunk_link_dist_host(segs, trunk_radius, plus_z, minus_z):
    """lrm_dbg_trunk_link_dist_host: the link-to-cylinder distance of the trunk clearance calls on hand-made links in the body
    frame, segs float32 [n, 6] = A, B -> float32[n]"""
    segs = _f32(segs, (-1, 6))
    out = np.zeros(len(segs), np.float32)
    check(load().lrm_dbg_trunk_link_dist_host(_ptr(segs), len(segs), float(trunk_radius), float(plus_z), float(minus_z), _ptr(out)))
    return out


def dbg_link_pair_dist_host(segs):
    """lrm_dbg_link_pair_dist_host: the link-pair distance of the self clearance calls on hand-made segment pairs, segs
    float32 [n, 12] = A1, B1, A2, B2 -> float32[n]"""
    segs = _f32(segs, (-1, 12))
    out = np.zeros(len(segs), np.float32)
    check(load().lrm_dbg_link_pair_dist_host(_ptr(segs), len(segs), _ptr(out)))
    return out


def apply_rbdl_equiv(xyz, leg):
    """apply_RBDL's work restated (RBDL-equivalent LM position IK, parity unpinned) -> (converged uint8[n], ms); CPU."""
    xyz = _f32(xyz, (-1, 3))
    mask = np.zeros(len(xyz), np.uint8)
    ms = C.c_double(0)
    check(load().lrm_rbdl_equiv_cpu(_ptr(xyz), len(xyz), _ptr(_f32(leg, (14,))), _ptr(mask), C.addressof(ms)))
    return mask, ms.value


def morton_order(points):
    """Indices that put an (n,3) cloud in Morton order (compact tiles for the pair kernels)."""
    points = _f32(points, (-1, 3))
    out = np.zeros(len(points), np.uint64)
    check(load().lrm_morton_order(_ptr(points), len(points), _ptr(out)))
    return out.astype(np.int64)


class OctreeSettings(C.Structure):
    """LrmOctreeSettings (include/lrm.h): the octree knobs of settings.h:15-46."""
    _fields_ = [("box_center", C.c_float * 3), ("box_size", C.c_float * 3), ("min_box", C.c_float),
                ("enable_rot_below", C.c_float), ("convex_radius", C.c_float), ("angle_sample", C.c_int32 * 3),
                ("angle_minmax", C.c_float * 6), ("leg_count", C.c_int32), ("leg_mount", C.c_float * 8),
                ("leg_number_for_stab", C.c_int32), ("max_depth", C.c_int32)]


def octree_default_settings():
    s = OctreeSettings()
    load().lrm_octree_default_settings(C.addressof(s))
    return s


def apply_oct(footholds, leg, settings=None, capacity=None):
    """apply_oct (several_leg_octree.cu:391-488) -> (centres float32[k,3], kernel ms); GPU."""
    footholds = _f32(footholds, (-1, 3))
    cap = capacity if capacity is not None else 65536  # valid leaves; a larger tree makes the call run twice
    while True:
        out = np.zeros((max(cap, 1), 3), np.float32)
        n_out = C.c_size_t(0)
        ms = C.c_float(0)
        rc = load().lrm_apply_oct(_ptr(footholds), len(footholds), _ptr(_f32(leg, (14,))),
                                  None if settings is None else C.addressof(settings), _ptr(out), cap,
                                  C.addressof(n_out), C.addressof(ms))
        if rc == -1 and n_out.value > cap and capacity is None:
            cap = n_out.value
            continue
        if rc != 0:
            raise LrmError(f"liblrm error {rc}: {load().lrm_octree_last_error().decode()}")
        return out[: n_out.value].copy(), ms.value


OCT_EXCHANGE = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p)


def _oct_call(fn, head_args, leg, settings, tail_args, exchange, capacity):
    """One of the lrm_apply_oct* entry points with an optional exchange callback.  `exchange(flags: np.ndarray[uint32])`
    must replace the array, in place, by its element-wise bitwise OR over all ranks.  An exception raised inside it is
    kept, turned into a non-zero return (the library then fails the call instead of going on with flags that were never
    combined) and re-raised here."""
    cap = capacity if capacity is not None else 65536  # valid leaves; a larger tree makes the call run twice
    raised = []

    def _cb(ptr, m, _user):
        try:
            exchange(np.ctypeslib.as_array(ptr, shape=(m,)))
            return 0
        except BaseException as e:  # noqa: BLE001 -- must not propagate through the C frames
            raised.append(e)
            return 1

    cb = OCT_EXCHANGE(_cb) if exchange is not None else None
    cb_arg = [C.cast(cb, C.c_void_p) if cb is not None else None, None]
    while True:
        out = np.zeros((max(cap, 1), 3), np.float32)
        n_out = C.c_size_t(0)
        ms = C.c_float(0)
        rc = fn(*head_args, _ptr(_f32(leg, (14,))), None if settings is None else C.addressof(settings), _ptr(out), cap,
                C.addressof(n_out), C.addressof(ms), *tail_args, *(cb_arg if (exchange is not None or tail_args) else []))
        if raised:
            raise raised[0]
        if rc == -1 and n_out.value > cap and capacity is None:
            cap = n_out.value  # every rank sees the same count and retries together
            continue
        if rc != 0:
            raise LrmError(f"liblrm error {rc}: {load().lrm_octree_last_error().decode()}")
        return out[: n_out.value].copy(), ms.value


def apply_oct_dev(x_ptr, y_ptr, z_ptr, n, leg, settings=None, rank=0, world=1, exchange=None, capacity=None):
    """lrm_apply_oct_dev: the footholds as three device arrays (raw pointers) -> (centres float32[k,3], kernel ms)."""
    return _oct_call(load().lrm_apply_oct_dev, (x_ptr, y_ptr, z_ptr, n), leg, settings, (rank, world), exchange, capacity)


def apply_oct_sharded(footholds, leg, settings, rank, world, exchange, capacity=None):
    """lrm_apply_oct_sharded (every rank holds all footholds, the children of a level are dealt round-robin)
    -> (centres float32[k,3], kernel ms); GPU."""
    footholds = _f32(footholds, (-1, 3))
    return _oct_call(load().lrm_apply_oct_sharded, (_ptr(footholds), len(footholds)), leg, settings, (rank, world), exchange, capacity)


def apply_oct_partitioned(local_footholds, leg, settings, exchange, capacity=None):
    """lrm_apply_oct_partitioned (every rank holds ITS part of the footholds, host array (n, 3)) -> (centres, kernel ms)"""
    f = _f32(local_footholds, (-1, 3))
    return _oct_call(load().lrm_apply_oct_partitioned, (_ptr(f), len(f)), leg, settings, (), exchange, capacity)


def apply_oct_partitioned_dev(x_ptr, y_ptr, z_ptr, n, leg, settings, exchange, capacity=None):
    """lrm_apply_oct_partitioned_dev: this rank's part of the footholds as three device arrays (raw pointers)"""
    return _oct_call(load().lrm_apply_oct_partitioned_dev, (x_ptr, y_ptr, z_ptr, n), leg, settings, (), exchange, capacity)


def dbg_sqrt_check_dev():
    """lrm_sqrtf vs the compiler's IEEE sqrtf on all 2^32 bit patterns, on the device -> (mismatches, first_bad)."""
    bad = C.c_uint64(0)
    first = C.c_uint32(0)
    check(load().lrm_dbg_sqrt_check_dev(C.byref(bad), C.byref(first)))
    return int(bad.value), int(first.value)


def dbg_fast_host(xyz, leg, quat=None):
    """Filtered evaluation on the host without fallback -> dict(mask, mask_unc, dist, valid, dist_unc)."""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    out = dict(mask=np.zeros(n, np.uint8), mask_unc=np.zeros(n, np.uint8), dist=np.zeros_like(xyz),
               valid=np.zeros(n, np.uint8), dist_unc=np.zeros(n, np.uint8))
    check(load().lrm_dbg_fast_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(out["mask"]),
                                   _ptr(out["mask_unc"]), _ptr(out["dist"]), _ptr(out["valid"]),
                                   _ptr(out["dist_unc"])))
    return out


def dbg_tol_host(xyz, leg, quat=None):
    """Contract-tolerance evaluation on the host, no re-evaluation -> (mask, dist, doubt bits uint32)."""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    mask, d, doubt = np.zeros(n, np.uint8), np.zeros_like(xyz), np.zeros(n, np.uint32)
    check(load().lrm_dbg_tol_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask), _ptr(d),
                                  _ptr(doubt)))
    return mask, d, doubt


def dbg_toltab_host(xyz, leg, quat=None):
    """LRM_MODE_TOL on the host with the plane table with deferred decisions -> (mask, vectors, doubt bits, table stats)"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    mask, d, doubt = np.zeros(n, np.uint8), np.zeros_like(xyz), np.zeros(n, np.uint32)
    stats = np.zeros(5, np.uint32)
    check(load().lrm_dbg_toltab_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask), _ptr(d),
                                     _ptr(doubt), _ptr(stats)))
    return mask, d, doubt, dict(rows=int(stats[0]), vrows=int(stats[1]), refined=int(stats[2]), bytes=int(stats[3]),
                                second_candidates=int(stats[4]))


def dbg_xtab_host(xyz, leg, quat=None):
    """the bit-exact table-guided evaluation (csrc/lrm_point_xtab.h) on the host, no re-evaluation of its doubtful
    points -> (mask, vectors, doubt bits, dict(second_chains, bytes))"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    mask, d, doubt = np.zeros(n, np.uint8), np.zeros_like(xyz), np.zeros(n, np.uint32)
    stats = np.zeros(2, np.uint32)
    check(load().lrm_dbg_xtab_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask), _ptr(d),
                                   _ptr(doubt), _ptr(stats)))
    return mask, d, doubt, dict(second_chains=int(stats[0]), bytes=int(stats[1]))


def dbg_replay_host(xyz, leg, quat=None):
    """the tolerance evaluation with the plane table + the strict replay of its decisions (LRM_MODE_TOL_REL's short-vector path)
    on the host -> (mask, vectors, doubt bits); vectors of points without doubt are the bit-exact ones"""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    mask, d, doubt = np.zeros(n, np.uint8), np.zeros_like(xyz), np.zeros(n, np.uint32)
    check(load().lrm_dbg_replay_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask), _ptr(d), _ptr(doubt)))
    return mask, d, doubt


def dbg_toltab_build(leg, quat=None, device=False):
    """the plane table of (leg, quat) from the host builder or the device builder -> (bytes as uint8 array, build milliseconds)"""
    size, ms = C.c_size_t(0), C.c_float(0)
    legp, q = _f32(leg, (14,)), _quat(quat)
    buf = np.zeros(24 << 20, np.uint8)
    check(load().lrm_dbg_toltab_build(_ptr(legp), _ptr(q), 1 if device else 0, _ptr(buf), buf.size, C.byref(size), C.byref(ms)))
    assert size.value <= buf.size
    return buf[:size.value].copy(), float(ms.value)


def dbg_toltab_bounds(xz, leg, quat=None):
    """the plane table's lower bound at plane points (abscissa - coxa_length, z) -> (bound, distance of the full plane
    evaluation, its validity, its doubt bits)"""
    xz = _f32(xz, (-1, 2))
    n = len(xz)
    lb, dist = np.zeros(n, np.float32), np.zeros(n, np.float32)
    valid, doubt = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    check(load().lrm_dbg_toltab_bounds(_ptr(xz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(lb), _ptr(dist),
                                       _ptr(valid), _ptr(doubt)))
    return lb, dist, valid, doubt


def dbg_oct_trace(enable):
    check(load().lrm_dbg_oct_trace(1 if enable else 0))


def dbg_oct_trace_read():
    """records of the traced octree calls: float32[n, 12] = c[3], h[3], parent h[3], flag bits, parent_valid + 2 rot + 4 skip, depth"""
    n = C.c_size_t(0)
    check(load().lrm_dbg_oct_trace_read(None, 0, C.addressof(n)))
    out = np.zeros((int(n.value), 12), np.float32)
    check(load().lrm_dbg_oct_trace_read(_ptr(out), int(n.value), C.addressof(n)))
    return out


def dbg_oct_plan(nc, nf):
    """lrm_dbg_oct_plan: what an octree call launches for a level of nc children on nf footholds under the LRM_OCT_* switches
    of the environment (deferred: as when the plane tables and the queue exist).  Host only."""
    out = np.zeros(8, np.uint64)
    check(load().lrm_dbg_oct_plan(int(nc), int(nf), _ptr(out)))
    names = ("kernel", "grid_x", "grid_y", "tpr", "splits", "deferred", "ntiles", "block")
    return {**dict(zip(names, (int(v) for v in out))), "kernel": "chunked" if out[0] else "every", "deferred": bool(out[5])}


def dbg_pair_counts():
    """counting build only: (full evaluations, leg-sphere tests, footholds inside a reach sphere, footholds loaded) since the last call"""
    out = np.zeros(4, np.uint64)
    check(load().lrm_dbg_pair_counts(_ptr(out)))
    return [int(v) for v in out]


def dbg_tol_queue_counts():
    """(points, queued for the bit-exact fix-up, overflowed workgroup segments) of the last tolerance-mode call on device buffers"""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(load().lrm_dbg_tol_queue_counts(C.addressof(a), C.addressof(b), C.addressof(c)))
    return int(a.value), int(b.value), int(c.value)


def dbg_tol_grid(n):
    """lrm_dbg_tol_grid: the launch grids and queue words for n points -- dict with the workgroups of the table kernels of
    LRM_MODE_TOL / LRM_MODE_FAST ("tab") and of LRM_MODE_TOL_REL ("rel"), of the kernel without a table ("notab"), the queue
    words a call with / without the table requests ("tab_words", "notab_words") and those lrm_tol_prepare(n) reserves ("prepare_words")"""
    out = np.zeros(6, np.uint64)
    check(load().lrm_dbg_tol_grid(n, _ptr(out)))
    return dict(zip(("tab", "rel", "notab", "tab_words", "notab_words", "prepare_words"), (int(v) for v in out)))


def dbg_tol_ok(leg, quat=None):
    return bool(load().lrm_dbg_tol_ok(_ptr(_f32(leg, (14,))), _ptr(_quat(quat))))


def dbg_pair_sphere(leg, quat=None):
    """Bounding sphere of the pair test of one leg -> (centre[3] relative to the body position, r^2)."""
    out = np.zeros(4, np.float32)
    check(load().lrm_dbg_pair_sphere(_ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(out)))
    return out[:3].copy(), float(out[3])


def dbg_fused_reach_host(xyz, leg, quat=None):
    """The fused kernel's reach-from-distance by-product on the host, no fallback -> (mask, doubt)."""
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    mask, doubt = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    check(load().lrm_dbg_fused_reach_host(_ptr(xyz), n, _ptr(_f32(leg, (14,))), _ptr(_quat(quat)), _ptr(mask),
                                          _ptr(doubt)))
    return mask, doubt


def positionability(bodies, targets, legs, quats, reference_culls=False):
    """robot_full_struct's pipeline as a mask (several_leg.cu:326-877) -> (uint8[nb], ms); GPU."""
    bodies = _f32(bodies, (-1, 3))
    targets = _f32(targets, (-1, 3))
    legs = _f32(legs).reshape(-1, 14)
    quats = _f32(quats).reshape(-1, 4)
    out = np.zeros(len(bodies), np.uint8)
    ms = C.c_float(0)
    check(load().lrm_positionability(_ptr(bodies), len(bodies), _ptr(targets), len(targets), _ptr(legs),
                                     len(legs), _ptr(quats), len(quats), int(reference_culls), _ptr(out),
                                     C.addressof(ms)))
    return out, ms.value


def footholds_cpu(bodies, targets, legs, quat=None, nominal=None):
    """lrm_footholds_cpu: per (leg, body) the number of reachable targets, the index of the reachable target nearest the
    leg's nominal point (body + nominal[l], nominal None = zero; -1 if none) and its squared distance (+inf if none);
    serial host loop -> (count int32[nlegs, nb], best int32[nlegs, nb], best_d2 float32[nlegs, nb], ms)"""
    bodies = _f32(bodies, (-1, 3))
    targets = _f32(targets, (-1, 3))
    legs = _f32(legs).reshape(-1, 14)
    nom = _nominal(nominal, len(legs))
    count = np.zeros((len(legs), len(bodies)), np.int32)
    best = np.zeros((len(legs), len(bodies)), np.int32)
    best_d2 = np.zeros((len(legs), len(bodies)), np.float32)
    ms = C.c_double(0)
    check(load().lrm_footholds_cpu(_ptr(bodies), len(bodies), _ptr(targets), len(targets), _ptr(legs), len(legs),
                                   _ptr(_quat(quat)), _ptr(nom), _ptr(count), _ptr(best), _ptr(best_d2), C.addressof(ms)))
    return count, best, best_d2, ms.value
