"""Calls that overlap (include/lrm.h, "Threading"; run with -m gpu on an MI355X).

Every other GPU test runs one call, synchronises, then runs the next.  Here work is queued on several streams with no
synchronise until the end, past the library's cache sizes (16 doubt-queue workspaces, 64 plane tables, 16 leg slots of the
pair kernels), and issued from several host threads at once.  Every answer must equal, bit for bit and guard words
included, the same call run alone on one stream with a synchronise after it; a 2^16-point sample of those serial answers
is checked against the oracle, so the module stands on its own.

  A  every mode and every distance / fused entry point on 4 streams, first-use table builds and queue growth included
  B  70 (leg, orientation) pairs on 20 streams: tables and queue workspaces are evicted (hipFree) under queued work
  C  24 pair-kernel launches on 4 streams: more launches than leg slots
  D  posed queries and IK -> FK, one pose workspace per stream
  E  8 host threads: device table builds, first-use fused calls and octree calls with tables, all building tables at once
  G  host-buffer calls from 6 threads, through the host pipeline (LRM_HOST_PIPELINE=1) and without it
  F  lrm_release_workspaces gives back what the library cached on the device, and the calls after it give the same bits"""
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import bits_equal, random_cloud
from grid_cases import BLOCK, TOLTAB_MIN_POINTS, transitions
from ik_cases import check_contract, fixture_quats, fk64, unit
from octree_oracle import apply_oct as oracle_apply_oct
from posed_cases import leg_table, oracle_answer, pose_table, queries
from tolcheck import TOL, field_error

pytestmark = pytest.mark.gpu

SAMPLE = 1 << 16      # points of every serial answer checked against the oracle
SHORT_MM = 16.0       # LRM_MODE_TOL_REL: vectors shorter than this are bit-identical to the oracle
MASK_GUARD, FIELD_GUARD, BITS_GUARD = 7, -777.0, -1
POOL = 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


def capi():
    from lrm_amd import _capi
    return _capi


def hp(a):
    """a host array the call only reads, kept alive by the caller"""
    return capi()._ptr(a)


def modes(lrm):
    return {"strict": lrm.MODE_STRICT, "fast": lrm.MODE_FAST, "tol": lrm.MODE_TOL, "tol_rel": lrm.MODE_TOL_REL}


def sample_rows(n, seed):
    if n <= SAMPLE:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, SAMPLE, replace=False))


def check_oracle(oracle, mode, pts, leg, q, mask=None, valid=None, field=None, what=""):
    """the contract of `mode` on matching rows: masks and validity bytes bit-identical; the field bit-identical (strict, fast),
    within tests/tolcheck.py's TOL (tol), within 1e-5 relative and bit-identical below SHORT_MM (tol_rel)"""
    want_m = oracle.reach(pts, leg, q)
    want_d, want_v = oracle.dist(pts, leg, q)
    if mask is not None:
        assert np.array_equal(mask, want_m), f"{what}: reach mask differs from the oracle"
    if valid is not None:
        assert np.array_equal(valid, want_v), f"{what}: validity bytes differ from the oracle"
    if field is None:
        return
    if mode in ("strict", "fast"):
        assert bits_equal(field, want_d).all(), f"{what}: field differs from the oracle"
    elif mode == "tol":
        e = field_error(pts, field, want_d, leg)
        assert e["metric"].max(initial=0.0) <= TOL, f"{what}: distance error {e['metric'].max():.3e}"
    else:
        err = np.linalg.norm(field.astype(np.float64) - want_d.astype(np.float64), axis=1)
        nref = np.linalg.norm(want_d.astype(np.float64), axis=1)
        assert (err <= TOL * nref).all(), f"{what}: relative error above {TOL}"
        short = nref < SHORT_MM
        assert bits_equal(field[short], want_d[short]).all(), f"{what}: a vector shorter than {SHORT_MM} mm is not bit-identical"


def pooled(fns):
    """run the oracle checks on POOL threads (its C calls drop the GIL); the first failure is raised"""
    with ThreadPoolExecutor(POOL) as ex:
        for f in [ex.submit(fn) for fn in fns]:
            f.result()


class Buffers:
    """device outputs of one job, each followed by guard words; fill() writes guards everywhere, so that an output the call
    leaves unwritten shows too"""

    GUARD = {"mask": MASK_GUARD, "valid": MASK_GUARD, "status": MASK_GUARD, "bits": BITS_GUARD}

    def __init__(self, torch, n, names):
        self.torch, self.n, self.nw = torch, n, (n + 63) // 64
        self.t = {}
        for name in names:
            if name in ("mask", "valid", "status"):
                self.t[name] = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
            elif name == "bits":
                self.t[name] = torch.empty(self.nw + 2, dtype=torch.int64, device="cuda")
            elif name == "aos":
                self.t[name] = torch.empty(3 * n + 16, dtype=torch.float32, device="cuda")
            else:  # a field component or an angle: its own allocation (16-byte aligned)
                self.t[name] = torch.empty(n + 16, dtype=torch.float32, device="cuda")

    def used(self, name):
        return self.nw if name == "bits" else 3 * self.n if name == "aos" else self.n

    def fill(self):
        for name, t in self.t.items():
            t.fill_(self.GUARD.get(name, FIELD_GUARD))

    def p(self, name):
        return self.t[name].data_ptr()

    def host(self):
        """name -> the whole buffer, guards included, as raw bits"""
        out = {}
        for name, t in self.t.items():
            a = t.cpu().numpy()
            out[name] = a.view(np.uint32) if a.dtype == np.float32 else a
        return out

    def guards_intact(self, snap):
        for name, a in snap.items():
            g = np.array(self.GUARD[name], a.dtype) if name in self.GUARD else np.float32(FIELD_GUARD).view(np.uint32)
            if not (a[self.used(name):] == g).all():
                return False
        return True


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def field_of(snap, n, names=("dx", "dy", "dz")):
    return np.stack([snap[k][:n].view(np.float32) for k in names], axis=1)


# ---- A: several streams, every mode, every entry point -----------------------------------------------------------------------

ENTRIES = ("bits", "dist", "fused", "aos")


def table_size(lrm):
    """one size where the table kernels' grid changes shape (tests/grid_cases.py): the first point past the first transition
    above the dispatch switch"""
    t = min(t for t in transitions(lrm) if t * BLOCK > TOLTAB_MIN_POINTS + 1)
    return t * BLOCK + 1


def standard_legs(lrm):
    fq = [unit(q) for q in fixture_quats()]
    return [(f"M2 {a:+.2f}", lrm.get_M2_leg(a), fq[k % len(fq)]) if k % 2 == 0 else
            (f"moonbot {a:+.2f}", lrm.get_moonbot_leg(a), fq[k % len(fq)])
            for k, a in enumerate((0.3, -1.1, 2.0, 0.0, -2.6, 1.4))]


def enqueue(lrm, entry, cloud, aos, n, leg, q, buf, stream):
    """one job's calls on `stream`"""
    L, legp, qp = lrm.lib(), np.ascontiguousarray(leg, np.float32), np.ascontiguousarray(q, np.float32)
    x, y, z = (cloud[i].data_ptr() for i in range(3))
    ck, p = capi().check, buf.p
    if entry == "bits":
        ck(L.lrm_reach_bits_dev(x, y, z, n, hp(legp), hp(qp), p("mask"), p("bits"), stream))
    elif entry == "dist":
        ck(L.lrm_dist_dev(x, y, z, n, hp(legp), hp(qp), p("dx"), p("dy"), p("dz"), p("valid"), stream))
    elif entry == "fused":
        ck(L.lrm_reach_dist_bits_dev(x, y, z, n, hp(legp), hp(qp), p("mask"), p("bits"), p("dx"), p("dy"), p("dz"), stream))
    else:
        ck(L.lrm_reach_aos_dev(aos.data_ptr(), n, hp(legp), hp(qp), p("mask"), stream))
        ck(L.lrm_dist_aos_dev(aos.data_ptr(), n, hp(legp), hp(qp), p("aos"), p("valid"), stream))


ENTRY_OUTPUTS = {"bits": ("mask", "bits"), "dist": ("dx", "dy", "dz", "valid"), "fused": ("mask", "bits", "dx", "dy", "dz"),
                 "aos": ("mask", "aos", "valid")}


def check_job_oracle(oracle, entry, mname, pts, n, leg, q, snap, seed, what):
    rows = sample_rows(n, seed)
    p = np.ascontiguousarray(pts[rows])
    mask = snap["mask"][rows] if "mask" in snap else None
    valid = snap["valid"][rows] if "valid" in snap else None
    if entry == "aos":
        field = snap["aos"][:3 * n].view(np.float32).reshape(n, 3)[rows]
    elif "dx" in snap:
        field = field_of(snap, n)[rows]
    else:
        field = None
    check_oracle(oracle, mname, p, leg, q, mask, valid, field, what)
    if "bits" in snap:
        want = np.packbits(np.pad(snap["mask"][:n], (0, (-n) % 64)), bitorder="little").view(np.int64)
        assert np.array_equal(snap["bits"][:len(want)], want), f"{what}: bit words differ from the mask"


def test_every_mode_and_entry_point_on_four_streams(lrm, oracle, torch_cuda):
    torch = torch_cuda
    sizes = [1_003, TOLTAB_MIN_POINTS - 1, TOLTAB_MIN_POINTS + 1, 1_000_003, table_size(lrm)]
    nmax = max(sizes)
    pts = random_cloud((nmax + 63) // 64 * 64, seed=7)
    cloud = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    aos = torch.from_numpy(np.ascontiguousarray(pts)).cuda().reshape(-1)
    legs = standard_legs(lrm)
    mnames = list(modes(lrm))
    jobs = []
    for i in range(24):  # jobs 0-15 take each (mode, entry point) once
        mname, entry = mnames[i % 4], ENTRIES[(i + i // 4) % 4]
        name, leg, q = legs[i % len(legs)]
        n = sizes[i % len(sizes)]
        jobs.append(dict(mode=mname, entry=entry, leg=leg, q=q, n=n, what=f"job {i}: {mname}, {entry}, n = {n}, {name}",
                         buf=Buffers(torch, n, ENTRY_OUTPUTS[entry])))
    streams = [torch.cuda.Stream() for _ in range(4)]
    all_modes = modes(lrm)
    t0 = time.perf_counter()
    try:
        for j in jobs:
            j["buf"].fill()
        torch.cuda.synchronize()
        lrm.release_workspaces()  # first-use table builds, queue allocation and growth happen below, with work queued
        for i, j in enumerate(jobs):
            lrm.set_mode(all_modes[j["mode"]])  # read at call time
            enqueue(lrm, j["entry"], cloud, aos, j["n"], j["leg"], j["q"], j["buf"], streams[i % 4].cuda_stream)
        torch.cuda.synchronize()
        for j in jobs:
            j["got"] = j["buf"].host()
        t1 = time.perf_counter()
        lrm.release_workspaces()  # the serial calls build their own tables
        serial = torch.cuda.current_stream().cuda_stream
        for j in jobs:
            lrm.set_mode(all_modes[j["mode"]])
            j["buf"].fill()
            enqueue(lrm, j["entry"], cloud, aos, j["n"], j["leg"], j["q"], j["buf"], serial)
            torch.cuda.synchronize()
            j["want"] = j["buf"].host()
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    for j in jobs:
        assert j["buf"].guards_intact(j["got"]), f"{j['what']}: a call on 4 streams wrote past n"
        assert j["buf"].guards_intact(j["want"]), f"{j['what']}: a serial call wrote past n"
        assert same_bits(j["got"], j["want"]), f"{j['what']}: 4 streams and a serial call differ"
    pooled([lambda k=k, j=j: check_job_oracle(oracle, j["entry"], j["mode"], pts, j["n"], j["leg"], j["q"], j["want"], k, j["what"])
            for k, j in enumerate(jobs)])
    print(f"\n24 jobs on 4 streams: {t1 - t0:.2f} s enqueue + run, sizes {sizes}")


# ---- B: eviction of tables and queue workspaces under queued work ------------------------------------------------------------

def many_pairs(lrm, count, offset=0.0):
    """`count` distinct (leg, orientation) pairs that take the table-guided modes"""
    fq = [unit(q) for q in fixture_quats()]
    out = []
    k = 0
    while len(out) < count:
        a = -3.0 + offset + 0.0853 * k
        leg = lrm.get_M2_leg(a) if k % 2 == 0 else lrm.get_moonbot_leg(a)
        q = fq[k % len(fq)]
        if lrm.dbg_tol_ok(leg, q):
            out.append((f"{'M2' if k % 2 == 0 else 'moonbot'} {a:+.4f} q{k % len(fq)}", leg, q))
        k += 1
        assert k < 20 * count, "too few legs take the table-guided modes"
    return out


def test_tables_and_workspaces_evicted_under_queued_work(lrm, oracle, torch_cuda):
    """20 streams (16 queue workspaces), 70 pairs (64 cached tables) in LRM_MODE_TOL_REL at 250 000 points: every call builds a
    table, the 65th and later evict the least recently used one and the 17th stream evicts a workspace, each with hipFree while
    other streams still hold queued kernels that read them (hipFree waits for the device)"""
    torch = torch_cuda
    n = 250_000
    pts = random_cloud(n, seed=19)
    cloud = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    pairs = many_pairs(lrm, 70)
    bufs = [Buffers(torch, n, ENTRY_OUTPUTS["fused"]) for _ in pairs]
    streams = [torch.cuda.Stream() for _ in range(20)]
    assert len({s.cuda_stream for s in streams}) == 20
    lrm.set_mode(lrm.MODE_TOL_REL)
    try:
        for b in bufs:
            b.fill()
        torch.cuda.synchronize()
        lrm.release_workspaces()
        t0 = time.perf_counter()
        for i, ((_, leg, q), b) in enumerate(zip(pairs, bufs)):
            enqueue(lrm, "fused", cloud, None, n, leg, q, b, streams[i % 20].cuda_stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = [b.host() for b in bufs]
        lrm.release_workspaces()  # the serial calls build their own tables
        serial = torch.cuda.current_stream().cuda_stream
        want = []
        for (_, leg, q), b in zip(pairs, bufs):
            b.fill()
            enqueue(lrm, "fused", cloud, None, n, leg, q, b, serial)
            torch.cuda.synchronize()
            want.append(b.host())
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    for (name, _, _), b, g, w in zip(pairs, bufs, got, want):
        assert b.guards_intact(g) and b.guards_intact(w), f"{name}: a call wrote past n"
        assert same_bits(g, w), f"{name}: 20 streams and a serial call differ"
    per = SAMPLE // len(pairs) + 1  # 2^16 points in all

    def check(k):
        (name, leg, q), w = pairs[k], want[k]
        r = np.sort(np.random.default_rng(k).choice(n, per, replace=False))
        check_oracle(oracle, "tol_rel", pts[r], leg, q, w["mask"][r], None, field_of(w, n)[r], name)

    pooled([lambda k=k: check(k) for k in range(len(pairs))])
    print(f"\n70 pairs on 20 streams: {t1 - t0:.2f} s")


# ---- C: leg slots of the pair kernels ----------------------------------------------------------------------------------------

def pair_scene(nb, nt, seed):
    rng = np.random.default_rng(seed)
    txy = rng.uniform(-900, 900, (nt, 2))
    tz = 40 * np.sin(txy[:, 0] / 150) + 30 * np.cos(txy[:, 1] / 110) + rng.normal(0, 5, nt)
    bxy = rng.uniform(-700, 700, (nb, 2))
    bz = rng.uniform(60, 330, nb)
    return np.column_stack([bxy, bz]).astype(np.float32), np.column_stack([txy, tz]).astype(np.float32)


def pair_jobs(lrm, oracle, count):
    """`count` launches, each with its own leg set (1 to 6 legs) and quaternion"""
    jobs = []
    for i in range(count):
        axis = np.array([np.sin(i), np.cos(i), 1.0]) / np.sqrt(2.0)
        q = np.asarray(oracle.quat_from_vect_angle(axis, 0.05 * (i % 7)), np.float32)
        nlegs = 1 + i % 6
        base = lrm.get_M2_leg if i % 2 == 0 else lrm.get_moonbot_leg
        legs = np.stack([lrm.rotate_leg_data(q, base(2 * np.pi * k / nlegs + 0.1 * i)) for k in range(nlegs)])
        jobs.append(dict(q=q, legs=legs, scene=i % 2))
    return jobs


def test_pair_kernels_on_four_streams_past_the_leg_slots(lrm, oracle, torch_cuda):
    """24 lrm_reach_any_dev launches (16 leg slots) on 4 streams, fewer than 4096 targets each (the per-device box buffer stays
    unused: its one-cloud-at-a-time rule is documented); the serial answers against the brute-force oracle"""
    torch = torch_cuda
    nb = 97
    scenes = [pair_scene(nb, 2003, 41), pair_scene(nb, 3001, 42)]
    dev = [[torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in s] for s in scenes]
    jobs = pair_jobs(lrm, oracle, 24)
    for j in jobs:
        j["out"] = torch.empty(len(j["legs"]) * nb + 64, dtype=torch.uint8, device="cuda")
        j["all"] = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(4)]
    L = lrm.lib()

    def launch(j, stream):
        (b, t) = dev[j["scene"]]
        nt = t.shape[1]
        legs = np.ascontiguousarray(j["legs"], np.float32)
        capi().check(L.lrm_reach_any_dev(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), nb, t[0].data_ptr(), t[1].data_ptr(),
                                         t[2].data_ptr(), nt, hp(legs), len(legs), hp(j["q"]), j["out"].data_ptr(),
                                         j["all"].data_ptr(), stream))

    def snap(j):
        return j["out"].cpu().numpy(), j["all"].cpu().numpy()

    def fill():
        for j in jobs:
            j["out"].fill_(MASK_GUARD)
            j["all"].fill_(MASK_GUARD)
        torch.cuda.synchronize()

    try:
        fill()
        lrm.release_workspaces()
        for i, j in enumerate(jobs):
            lrm.set_mode(lrm.MODE_STRICT if i % 3 == 0 else lrm.MODE_FAST)  # the kernels' fast flag is read at call time
            launch(j, streams[i % 4].cuda_stream)
        torch.cuda.synchronize()
        got = [snap(j) for j in jobs]
        fill()
        want = []
        for i, j in enumerate(jobs):
            lrm.set_mode(lrm.MODE_STRICT if i % 3 == 0 else lrm.MODE_FAST)
            launch(j, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            want.append(snap(j))
    finally:
        lrm.set_mode(lrm.MODE_FAST)

    def check(i):
        j, (go, ga), (wo, wa) = jobs[i], got[i], want[i]
        m = len(j["legs"]) * nb
        assert (go[m:] == MASK_GUARD).all() and (ga[nb:] == MASK_GUARD).all(), f"launch {i}: wrote past its outputs"
        assert np.array_equal(go, wo) and np.array_equal(ga, wa), f"launch {i}: 4 streams and a serial launch differ"
        bodies, targets = scenes[j["scene"]]
        o = oracle.reach_any(bodies, targets, j["legs"], j["q"])
        assert np.array_equal(wo[:m].reshape(len(j["legs"]), nb), o), f"launch {i}: differs from the brute-force oracle"
        assert np.array_equal(wa[:nb], o.min(axis=0)), f"launch {i}: per-body AND differs from the oracle"

    pooled([lambda i=i: check(i) for i in range(len(jobs))])
    w = np.concatenate([w[0][:len(j["legs"]) * nb] for j, w in zip(jobs, want)])
    assert 0.02 < w.mean() < 0.98  # both outcomes exercised


# ---- D: posed queries and IK / FK on several streams -------------------------------------------------------------------------

def test_posed_and_ik_fk_on_four_streams(lrm, oracle, torch_cuda):
    """each stream compiles its own pose workspace, answers posed queries in it, and runs IK then FK on its own leg"""
    torch = torch_cuda
    ns = 4
    legs = leg_table(lrm)
    std = standard_legs(lrm)
    work = []
    for s in range(ns):
        quats, body = pose_table(lrm, n=29 + s, seed=60 + s)
        xyz, pose, li = queries(len(quats), len(legs), body, 173, np.random.default_rng(70 + s), "shuffled")
        n = len(xyz) - 13 * s
        xyz, pose, li = xyz[:n], pose[:n], li[:n]
        ik_pts = random_cloud(300_007 + 1_000 * s, seed=80 + s)
        w = dict(quats=quats, body=body, xyz=xyz, pose=pose, li=li, n=n, ik_pts=ik_pts, leg=std[s][1], q=std[s][2],
                 ps=lrm.PoseSet(legs, len(quats)),
                 d_quats=torch.from_numpy(quats).cuda(), d_body=torch.from_numpy(body).cuda(),
                 d_xyz=torch.from_numpy(np.ascontiguousarray(xyz.T)).cuda(), d_pose=torch.from_numpy(pose).cuda(),
                 d_li=torch.from_numpy(li).cuda(), d_ik=torch.from_numpy(np.ascontiguousarray(ik_pts.T)).cuda(),
                 pb=Buffers(torch, n, ("mask", "valid")), pf=torch.empty((3, n + 16), dtype=torch.float32, device="cuda"),
                 ib=Buffers(torch, len(ik_pts), ("status",)),
                 ia=torch.empty((3, len(ik_pts) + 16), dtype=torch.float32, device="cuda"),
                 fx=torch.empty((3, len(ik_pts) + 16), dtype=torch.float32, device="cuda"))
        work.append(w)

    def fill():
        for w in work:
            w["pb"].fill()
            w["ib"].fill()
            for t in (w["pf"], w["ia"], w["fx"]):
                t.fill_(FIELD_GUARD)
            w["ps"].workspace.fill_(0)
        torch.cuda.synchronize()

    def run(w):
        """on torch's current stream"""
        m = len(w["ik_pts"])
        w["ps"].update(w["d_quats"], w["d_body"])
        x = w["d_xyz"]
        w["ps"].reach_dist(x[0], x[1], x[2], w["d_pose"], w["d_li"], mask=w["pb"].t["mask"], out=w["pf"],
                           valid=w["pb"].t["valid"], check=False)
        p = w["d_ik"]
        lrm.device.ik(p[0], p[1], p[2], w["leg"], w["q"], out=w["ia"], status=w["ib"].t["status"])
        lrm.device.fk(w["ia"][0, :m], w["ia"][1, :m], w["ia"][2, :m], w["leg"], w["q"], out=w["fx"])

    def snap(w):
        s = w["pb"].host()
        s.update(w["ib"].host())
        for k in ("pf", "ia", "fx"):
            s[k] = w[k].cpu().numpy().view(np.uint32)
        s["records"] = w["ps"].workspace.cpu().numpy()
        return s

    fill()
    streams = [torch.cuda.Stream() for _ in range(ns)]
    for w, st in zip(work, streams):
        with torch.cuda.stream(st):
            run(w)
    torch.cuda.synchronize()
    got = [snap(w) for w in work]
    fill()
    for w in work:
        run(w)
        torch.cuda.synchronize()
    want = [snap(w) for w in work]
    g32 = np.float32(FIELD_GUARD).view(np.uint32)
    for s, (w, g, wt) in enumerate(zip(work, got, want)):
        n, m = w["n"], len(w["ik_pts"])
        assert w["pb"].guards_intact({k: g[k] for k in ("mask", "valid")}) and w["ib"].guards_intact({"status": g["status"]})
        assert (g["pf"][:, n:] == g32).all() and (g["ia"][:, m:] == g32).all() and (g["fx"][:, m:] == g32).all(), f"stream {s}"
        assert same_bits(g, wt), f"stream {s}: 4 streams and a serial run differ in " + \
            ", ".join(k for k in g if not np.array_equal(g[k], wt[k]))

    def check(s):
        w, wt = work[s], want[s]
        rows = sample_rows(w["n"], s)
        wm, wv, wd = oracle_answer(oracle, w["xyz"][rows], w["pose"][rows], w["li"][rows], w["quats"], w["body"], legs)
        assert np.array_equal(wt["mask"][rows], wm) and np.array_equal(wt["valid"][rows], wv), f"stream {s}: posed mask / validity"
        assert bits_equal(wt["pf"][:, :w["n"]].view(np.float32).T[rows], wd).all(), f"stream {s}: posed field"
        # IK: the contract of lrm_ik_* against the oracle (statuses = reach mask, limits, the tip on p or at p - d); FK: the
        # tip of those angles by an independent float64 forward kinematics
        m = len(w["ik_pts"])
        rows = sample_rows(m, 10 + s)
        ang = wt["ia"][:, :m].view(np.float32).T[rows]
        check_contract(oracle, np.ascontiguousarray(w["ik_pts"][rows]), w["leg"], w["q"], ang, wt["status"][rows], clean=False)
        tip = wt["fx"][:, :m].view(np.float32).T[rows].astype(np.float64)
        assert np.linalg.norm(tip - fk64(ang, w["leg"], w["q"]), axis=1).max() <= 1e-3, f"stream {s}: FK against float64 kinematics"

    pooled([lambda s=s: check(s) for s in range(ns)])


# ---- E: several host threads -------------------------------------------------------------------------------------------------

def oct_footholds(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-600, 600, (n, 2))
    z = 20 * np.sin(xy[:, 0] / 120) + rng.normal(0, 4, n) - 150
    return np.column_stack([xy, z]).astype(np.float32)


def oct_settings(lrm, shift):
    """a small root box with the 27 orientation samples active from the first level; `shift` moves the sampled angles, so
    every call meets 27 x 4 (orientation, leg) pairs no earlier call met"""
    st = lrm.octree_default_settings()
    for i in range(3):
        st.box_size[i] = 300.0
    st.max_depth = 3
    st.leg_number_for_stab = 1
    st.enable_rot_below = 400.0
    for i in range(6):
        st.angle_minmax[i] = st.angle_minmax[i] + shift
    return st


def host_tables(lrm, cands, want):
    """the first `want` candidate pairs the host builder makes a table for -> [(leg, q, table)]"""
    out = []
    for leg, q in cands:
        try:
            tab, _ = lrm.dbg_toltab_build(leg, q, device=False)
        except lrm.LrmError:
            continue
        out.append((leg, q, tab))
        if len(out) == want:
            return out
    raise AssertionError("too few candidate legs have a table")


def test_eight_host_threads_build_tables_at_once(lrm, oracle, torch_cuda, monkeypatch):
    """8 threads released together by a barrier, each on its own stream and its own new pairs: 3 build tables with the device
    builder (lrm_dbg_toltab_build: no lock of the library's own), 3 make first-use LRM_MODE_TOL fused calls on 400 000 points
    (table builds under the cache lock), 2 run lrm_apply_oct with tolerance blocks and tables (builds under the octree's lock).
    The device builder shares one scratch set per device between all three, so builds that interleaved would mix one leg's
    cells with another's layout.  Device-built tables must equal the host builder's, fused outputs a serial rerun on host-built
    tables, octree leaves a serial call.  Three rounds."""
    torch = torch_cuda
    n = 400_000
    pts = random_cloud(n, seed=23)
    cloud = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    f = oct_footholds(160, seed=404)
    dim = lrm.get_M2_leg(0.0)
    monkeypatch.setenv("LRM_OCT_TOL", "1")
    monkeypatch.setenv("LRM_OCT_TAB", "1")
    monkeypatch.delenv("LRM_OCT_DEFER", raising=False)
    monkeypatch.delenv("LRM_TOLTAB_HOST", raising=False)
    monkeypatch.delenv("LRM_TOL_TABLE", raising=False)
    L = lrm.lib()
    t_all = time.perf_counter()
    for rnd in range(3):
        fq = [unit(q) for q in fixture_quats()]
        cands = [((lrm.get_M2_leg if k % 2 else lrm.get_moonbot_leg)(0.05 + 0.113 * k + 0.031 * rnd), fq[(k + rnd) % len(fq)])
                 for k in range(60)]
        builds = host_tables(lrm, cands[:40], 18)
        fused = [(leg, q) for leg, q in cands[40:] if lrm.dbg_tol_ok(leg, q)][:6]
        assert len(fused) == 6
        shifts = [0.0101 * (1 + 2 * rnd + t) for t in range(2)]
        bufs = [Buffers(torch, n, ENTRY_OUTPUTS["fused"]) for _ in fused]
        for b in bufs:
            b.fill()
        streams = [torch.cuda.Stream() for _ in range(8)]
        torch.cuda.synchronize()
        lrm.release_workspaces()  # the octree's cache and the library's tables are empty: every pair below is built now
        lrm.set_mode(lrm.MODE_TOL)
        barrier = threading.Barrier(8)
        res, errs = {}, []

        def builder(t):
            barrier.wait()  # (the builder works on the null stream)
            res[("tab", t)] = [lrm.dbg_toltab_build(leg, q, device=True)[0] for leg, q, _ in builds[6 * t:6 * t + 6]]

        def caller(t):
            barrier.wait()
            for k in (2 * t, 2 * t + 1):
                leg, q = fused[k]
                enqueue(lrm, "fused", cloud, None, n, leg, q, bufs[k], streams[3 + t].cuda_stream)
            streams[3 + t].synchronize()

        def octree(t):
            barrier.wait()
            res[("oct", t)] = lrm.apply_oct(f, dim, oct_settings(lrm, shifts[t]))[0]

        def guarded(fn, t):
            try:
                fn(t)
            except BaseException as e:  # noqa: BLE001 -- re-raised on the main thread
                errs.append(e)
                barrier.abort()

        roles = [(builder, t) for t in range(3)] + [(caller, t) for t in range(3)] + [(octree, t) for t in range(2)]
        ths = [threading.Thread(target=guarded, args=r) for r in roles]
        try:
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            torch.cuda.synchronize()
        finally:
            lrm.set_mode(lrm.MODE_FAST)
        if errs:
            raise errs[0]
        got = [b.host() for b in bufs]
        # serial reruns: the fused calls on host-built tables, the octree calls alone
        lrm.release_workspaces()
        lrm.set_mode(lrm.MODE_TOL)
        monkeypatch.setenv("LRM_TOLTAB_HOST", "1")
        try:
            want = []
            for (leg, q), b in zip(fused, bufs):
                b.fill()
                enqueue(lrm, "fused", cloud, None, n, leg, q, b, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                want.append(b.host())
        finally:
            monkeypatch.delenv("LRM_TOLTAB_HOST")
            lrm.set_mode(lrm.MODE_FAST)
        lrm.release_workspaces()
        lrm.set_mode(lrm.MODE_TOL)
        try:
            oct_want = [lrm.apply_oct(f, dim, oct_settings(lrm, s))[0] for s in shifts]
        finally:
            lrm.set_mode(lrm.MODE_FAST)
        for t in range(3):
            for k, (tab, (_, _, host)) in enumerate(zip(res[("tab", t)], builds[6 * t:6 * t + 6])):
                assert tab.size == host.size and np.array_equal(tab, host), f"round {rnd}, builder {t}, pair {k}: table differs"
        for k, (b, g, w) in enumerate(zip(bufs, got, want)):
            assert b.guards_intact(g), f"round {rnd}, fused call {k}: wrote past n"
            assert same_bits(g, w), f"round {rnd}, fused call {k}: differs from the serial call on a host-built table"
        for t in range(2):
            assert np.array_equal(res[("oct", t)].view(np.uint32), oct_want[t].view(np.uint32)), f"round {rnd}, octree {t}"
        rows = sample_rows(n, rnd)
        pooled([lambda k=k, w=w: check_oracle(oracle, "tol", pts[rows], fused[k][0], fused[k][1], w["mask"][rows], None,
                                              field_of(w, n)[rows], f"round {rnd}, fused call {k}")
                for k, w in enumerate(want)])
    lrm.release_workspaces()
    want0, _ = oracle_apply_oct(oracle, f, dim, oct_settings(lrm, shifts[0]))
    assert np.array_equal(oct_want[0].view(np.uint32), want0.view(np.uint32)), "octree: the serial call differs from the oracle"
    print(f"\n3 rounds of 8 threads: {time.perf_counter() - t_all:.2f} s")


# ---- G: host-buffer calls from several threads -------------------------------------------------------------------------------

def test_host_buffer_calls_from_six_threads(lrm, oracle, torch_cuda, monkeypatch):
    """lrm_reach_dist on host arrays from 6 threads at once, in LRM_MODE_FAST and LRM_MODE_TOL, with LRM_HOST_PIPELINE=1: the
    clouds of 3 threads are long enough for the pipeline (its device buffers, pinned slots, streams and events are one set per
    device, and they grow with the cloud), the other 3 take the direct path.  Each answer must equal the same call made alone."""
    monkeypatch.setenv("LRM_HOST_PIPELINE", "1")
    monkeypatch.delenv("LRM_HOST_PIPELINE_CHUNK", raising=False)
    sizes = [1_100_003, 1_300_001, 2_200_007, 300_001, 250_003, 1_003]  # the pipeline from 2 * 2^19 points on
    pts = random_cloud(max(sizes), seed=37)
    legs = standard_legs(lrm)
    for mode, mname in ((lrm.MODE_FAST, "fast"), (lrm.MODE_TOL, "tol")):
        lrm.release_workspaces()  # the pipeline's buffers grow inside the concurrent phase
        lrm.set_mode(mode)
        try:
            barrier = threading.Barrier(len(sizes))
            got, errs = [None] * len(sizes), []

            def body(k):
                try:
                    barrier.wait()
                    got[k] = lrm.apply_reach_dist(pts[:sizes[k]], legs[k][1], legs[k][2])[:2]
                except BaseException as e:  # noqa: BLE001 -- re-raised on the main thread
                    errs.append(e)
                    barrier.abort()

            ths = [threading.Thread(target=body, args=(k,)) for k in range(len(sizes))]
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            if errs:
                raise errs[0]
            lrm.release_workspaces()
            want = [lrm.apply_reach_dist(pts[:n], leg, q)[:2] for n, (_, leg, q) in zip(sizes, legs)]
        finally:
            lrm.set_mode(lrm.MODE_FAST)
        for k, ((gm, gd), (wm, wd)) in enumerate(zip(got, want)):
            what = f"{mname}, thread {k}, n = {sizes[k]}, {legs[k][0]}"
            assert np.array_equal(gm, wm) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), \
                f"{what}: differs from the same call made alone"

        def check(k, mname=mname, want=want):
            rows = sample_rows(sizes[k], 40 + k)
            wm, wd = want[k]
            check_oracle(oracle, mname, pts[rows], legs[k][1], legs[k][2], wm[rows], None, wd[rows], f"{mname}, thread {k}")

        pooled([lambda k=k: check(k) for k in range(len(sizes))])
    lrm.release_workspaces()


# ---- F: lrm_release_workspaces frees what the library cached -----------------------------------------------------------------

def test_release_workspaces_frees_every_cached_buffer(lrm, oracle, torch_cuda, monkeypatch):
    """the octree's table cache, the pair kernels' boxes and leg slots, tables and queues of 3 streams, the builder's scratch:
    after lrm_release_workspaces the device's free memory is back within 16 MiB of where it was, and one more call of each
    kind gives the bits it gave before.  The octree's tables alone are well over 16 MiB; the pair kernels' pools are not (their
    release is measured on its own below).  Free memory is the whole device's: another process on the GPU would move it."""
    torch = torch_cuda
    monkeypatch.setenv("LRM_OCT_TOL", "1")
    monkeypatch.setenv("LRM_OCT_TAB", "1")
    monkeypatch.delenv("LRM_TOLTAB_HOST", raising=False)
    n = 300_000
    pts = random_cloud(n, seed=29)
    cloud = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    bodies, _ = pair_scene(32, 16, 51)
    _, targets = pair_scene(1, 2_000_000, 52)
    d_b = torch.from_numpy(np.ascontiguousarray(bodies.T)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(targets.T)).cuda()
    pair_legs = np.stack([lrm.get_moonbot_leg(k * np.pi / 2) for k in range(4)])
    f = oct_footholds(160, seed=405)
    dim = lrm.get_moonbot_leg(0.0)
    st_many = oct_settings(lrm, 0.0)
    for i in range(3):
        st_many.angle_sample[i] = 5  # 125 orientations x 4 legs: 500 tables
    quats, body = pose_table(lrm, n=17, seed=3)
    plegs = leg_table(lrm)
    xyz, pose, li = queries(len(quats), len(plegs), body, 101, np.random.default_rng(3), "shuffled")
    d_q, d_body = torch.from_numpy(quats).cuda(), torch.from_numpy(body).cuda()
    d_xyz, d_pose, d_li = torch.from_numpy(np.ascontiguousarray(xyz.T)).cuda(), torch.from_numpy(pose).cuda(), torch.from_numpy(li).cuda()
    tol_pairs = many_pairs(lrm, 3, offset=0.6)
    streams = [torch.cuda.Stream() for _ in range(3)]

    def run_all(st_oct):
        """one call of each kind -> host copies of the results (the device outputs are dropped)"""
        out = {}
        lrm.set_mode(lrm.MODE_TOL)
        try:
            out["oct"] = lrm.apply_oct(f, dim, st_oct)[0]
            for k, ((_, leg, q), s) in enumerate(zip(tol_pairs, streams)):
                with torch.cuda.stream(s):
                    m, d = lrm.device.reach_dist(cloud[0], cloud[1], cloud[2], leg, q)
                torch.cuda.synchronize()
                out[f"tol{k}"] = (m.cpu().numpy(), d.cpu().numpy().view(np.uint32))
                del m, d
        finally:
            lrm.set_mode(lrm.MODE_FAST)
        o, a = lrm.device.reach_any(d_b[0], d_b[1], d_b[2], d_t[0], d_t[1], d_t[2], pair_legs)
        torch.cuda.synchronize()
        out["pair"] = (o.cpu().numpy(), a.cpu().numpy())
        ps = lrm.PoseSet(plegs, len(quats)).update(d_q, d_body)
        m, d, v = ps.reach_dist(d_xyz[0], d_xyz[1], d_xyz[2], d_pose, d_li)
        torch.cuda.synchronize()
        out["posed"] = (m.cpu().numpy(), d.cpu().numpy().view(np.uint32), v.cpu().numpy())
        del o, a, ps, m, d, v
        return out

    small = oct_settings(lrm, 0.5)
    run_all(small)  # warm-up: code objects, streams, the runtime's own first-use allocations
    lrm.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    before = run_all(st_many)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_mid, _ = torch.cuda.mem_get_info()
    tab_bytes = lrm.dbg_toltab_build(dim, None, device=False)[0].size
    lrm.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    print(f"\ncached before the release: {(free0 - free_mid) / 2**20:.1f} MiB (estimate for the octree's tables, 500 times the host "
          f"table of one pair: {500 * tab_bytes / 2**20:.0f} MiB); left after it: {(free0 - free1) / 2**20:.1f} MiB")
    assert free0 - free_mid > 16 << 20, "the calls cached less than the test is meant to catch"
    assert free0 - free1 <= 16 << 20, f"{(free0 - free1) / 2**20:.1f} MiB still held after lrm_release_workspaces"
    after = run_all(st_many)
    assert np.array_equal(before["oct"].view(np.uint32), after["oct"].view(np.uint32)), "octree after the release"
    for k in before:
        if k != "oct":
            assert all(np.array_equal(a, b) for a, b in zip(before[k], after[k])), f"{k} after the release"
    lrm.release_workspaces()
    rows = sample_rows(n, 5)
    for k, (_, leg, q) in enumerate(tol_pairs):
        m, d = after[f"tol{k}"]
        check_oracle(oracle, "tol", pts[rows], leg, q, m[rows], None, d.view(np.float32).T[rows], f"TOL call {k}")
    wm, wv, wd = oracle_answer(oracle, xyz, pose, li, quats, body, plegs)
    m, d, v = after["posed"]
    assert np.array_equal(m, wm) and np.array_equal(v, wv) and bits_equal(d.view(np.float32).T, wd).all(), "posed call"


def test_release_workspaces_frees_the_pair_kernels_pools(lrm, torch_cuda):
    """the pair kernels' per-device boxes and leg slots, measured on their own: a target cloud of 3 * 2^24 points makes the
    boxes (6 floats per 1024-target tile and per 64-target chunk, with room to grow) about 29 MiB; lrm_release_workspaces must
    give back all but 4 MiB of what the launch left cached, and the launch after it must give the same bits"""
    torch = torch_cuda
    nt = 3 << 24
    bodies, _ = pair_scene(8, 16, 61)
    _, targets = pair_scene(1, nt, 62)
    d_b = torch.from_numpy(np.ascontiguousarray(bodies.T)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(targets.T)).cuda()
    del targets
    legs = np.stack([lrm.get_M2_leg(k * np.pi) for k in range(2)])

    def launch(t):
        o, a = lrm.device.reach_any(d_b[0], d_b[1], d_b[2], t[0], t[1], t[2], legs)
        torch.cuda.synchronize()
        out = (o.cpu().numpy(), a.cpu().numpy())
        del o, a
        return out

    launch(d_t[:, :8192].contiguous())  # warm-up: code objects, the first pool allocations
    lrm.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    before = launch(d_t)
    torch.cuda.empty_cache()
    free_mid, _ = torch.cuda.mem_get_info()
    lrm.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    print(f"\npair kernels: {(free0 - free_mid) / 2**20:.1f} MiB cached, {(free0 - free1) / 2**20:.1f} MiB left after the release")
    assert free0 - free_mid >= 24 << 20, "the launch cached less than its boxes"
    assert free0 - free1 <= 4 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of the pair kernels' pools still held after the release"
    after = launch(d_t)
    lrm.release_workspaces()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "pair launch after the release"
    assert 0 < before[0].mean() <= 1  # some body reaches some target
