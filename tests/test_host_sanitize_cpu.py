"""The library's HOST code under sanitizers (no GPU): `make -C csrc sanitize` rebuilds the four host translation units and the
stand-alone driver tests/host_sanitize/san_main.cpp with -fsanitize=address,undefined and with -fsanitize=thread; the two
programs run the single-leg entries, the debug twins of the table code and every posed *_cpu loop on a hostile corpus (nan, inf,
denormals, 1e30 and 2^31 in coordinates, quaternions, bodies and angles; indices and CSR offsets out of range; the optional
pointers NULL) and, on eight threads, the host table builder, the loops, the mode switch and the last error.  The host loops
are the bit-exact reference of every posed GPU test and share their arithmetic headers with the kernels, so this is the
out-of-bounds and undefined-behaviour check that arithmetic gets.

The programs are ordinary executables with a main of their own: nothing is preloaded and nothing loaded into Python runs under
a sanitizer.  They belong on a CPU machine: where a GPU is present (/dev/kfd) the test skips, as it does without hipcc."""
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


@pytest.fixture(scope="module")
def programs():
    """both programs, built once in a subprocess"""
    r = subprocess.run(["make", "-C", CSRC, "-j", str(min(4, os.cpu_count() or 1)), "sanitize"], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = {k: os.path.join(CSRC, "build", k, "san_main") for k in ("asan", "tsan")}
    assert all(os.path.exists(p) for p in out.values())
    return out


def run(path, *args):
    env = dict(os.environ)  # the inherited environment, plus the sanitizers' own options
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0")
    r = subprocess.run([path, *args], env=env, capture_output=True, text=True, timeout=900)
    text = r.stdout + r.stderr
    print(text[-2000:])
    assert r.returncode == 0, text[-6000:]
    assert not any(w in text for w in REPORTS), text[-6000:]
    assert "san_main: every call returned as documented" in r.stdout


def test_address_and_undefined_behaviour(programs):
    """the whole corpus, the thread section included"""
    run(programs["asan"])


def test_threads(programs):
    """eight threads: table builds of the same and of different (leg, quaternion), the loops, lrm_set_mode / lrm_get_mode,
    lrm_last_error"""
    run(programs["tsan"], "--threads-only")
