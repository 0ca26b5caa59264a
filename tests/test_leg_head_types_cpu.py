"""The strict per-point layer is declared on LrmLegHead, the base of LrmCompiledLeg (csrc/lrm_types.h): it takes the head of
a pose record and a whole compiled leg alike, and code that reads the tail (csrc/lrm_point_fast.h) does not take a bare head.
Two snippets, syntax-checked as host C++ with the Makefile's compiler; nothing is run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged-robot-movability-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

STRICT = """
#include "lrm_leg_clearance.h" // lrm_ik.h, lrm_compile_head.h and lrm_point.h with it
void strict(const LrmLegHead& H, const LrmIkLeg& K, LrmVec3 p) {
    LrmVec3 J[4];
    (void)lrm_reach_global(H, &H.lists[0][0], p);
    (void)lrm_dist_global(H, &H.lists[0][0], p);
    (void)lrm_fk_point(H, K, 0.f, 0.f, 0.f);
    lrm_leg_joints(H, K, 0.f, 0.f, 0.f, 0.f, J);
}
void on_record(const LrmPoseRecord& R, const LrmIkLeg& K, LrmVec3 p) {
    LrmVec3 J[4];
    (void)lrm_reach_global(R.head, &R.head.lists[0][0], p);
    (void)lrm_dist_global(R.head, &R.head.lists[0][0], p);
    (void)lrm_fk_point(R.head, K, 0.f, 0.f, 0.f);
    lrm_leg_joints(R.head, K, 0.f, 0.f, 0.f, 0.f, J);
}
void on_leg(const LrmCompiledLeg& L, const LrmIkLeg& K, LrmVec3 p) {
    LrmVec3 J[4];
    (void)lrm_reach_global(L, &L.lists[0][0], p);
    (void)lrm_dist_global(L, &L.lists[0][0], p);
    (void)lrm_fk_point(L, K, 0.f, 0.f, 0.f);
    lrm_leg_joints(L, K, 0.f, 0.f, 0.f, 0.f, J);
}
"""

# LEG names what stands for the leg: a whole compiled leg compiles, the head of a record must not
FAST = """
#include "lrm_compile_head.h"
#include "lrm_point_fast.h"
bool fast(const LrmCompiledLeg& L, const LrmPoseRecord& R, LrmVec3 p) {
    uint32_t unc = 0;
    return lrm_reach_global_fast(LEG, &L.lean[0][0], p, unc);
}
"""


def syntax_check(tmp_path, text, *flags):
    src = tmp_path / "snippet.cpp"
    src.write_text(text)
    return subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", CSRC, *flags, str(src)],
                          capture_output=True, text=True, timeout=300)


def test_strict_layer_takes_a_record_head_and_tail_readers_refuse_it(tmp_path):
    r = syntax_check(tmp_path, STRICT)
    assert r.returncode == 0, r.stderr[-3000:]
    r = syntax_check(tmp_path, FAST, "-DLEG=L")
    assert r.returncode == 0, r.stderr[-3000:]  # the snippet is sound: only the head argument can make it fail
    r = syntax_check(tmp_path, FAST, "-DLEG=R.head")
    assert r.returncode != 0, "lrm_reach_global_fast reads the tail and accepted an LrmLegHead"
    assert "lrm_reach_global_fast" in r.stderr and "LrmLegHead" in r.stderr, r.stderr[-3000:]
