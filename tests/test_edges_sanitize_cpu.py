"""The pose edges HOST loop under AddressSanitizer and UndefinedBehaviorSanitizer (no GPU): `make -C csrc sanitize-edges`
builds the stand-alone driver tests/host_sanitize/san_edges_main.cpp against the sanitized host objects of
tests/test_host_sanitize_cpu.py's build; the program runs lrm_pose_edges_cpu on a hostile corpus (NaN, inf, FLT_MAX, denormal
and zero bodies and quaternions; live bytes of 0, 1 and 255; NULL body and pose_live; steps of 0, inf and FLT_MAX; capacity 0
and 1; offsets that decrease, are negative, overlap, lie past the end or hold INT64_MIN / INT64_MAX; the optional pointers NULL;
every refusal in its order, the device forms' included, which come before any device is touched).  The host loop is the
bit-exact reference of the GPU tests and shares its arithmetic header with the kernels.

The program is an ordinary executable with a main of its own: nothing is preloaded and nothing loaded into Python runs under a
sanitizer.  It belongs on a CPU machine: where a GPU is present (/dev/kfd) the test skips, as it does without hipcc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged-robot-movability-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REPORTS = ("Sanitizer", "runtime error:", "SUMMARY:")

pytestmark = [
    pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc: the sanitizer builds need the compiler"),
    pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU machine: sanitizer builds run on the CPU machine only"),
]


def test_address_and_undefined_behaviour():
    r = subprocess.run(["make", "-C", CSRC, "-j", str(min(4, os.cpu_count() or 1)), "sanitize-edges"], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    path = os.path.join(CSRC, "build", "asan", "san_edges_main")
    env = dict(os.environ)  # the inherited environment, plus the sanitizers' own options
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([path], env=env, capture_output=True, text=True, timeout=900)
    text = r.stdout + r.stderr
    print(text[-2000:])
    assert r.returncode == 0, text[-6000:]
    assert not any(w in text for w in REPORTS), text[-6000:]
    assert "san_edges_main: every call returned as documented" in r.stdout
