"""lrm_norm_sums_less (csrc/lrm_point.h): the pick of two strict norms from their sums of squares, against the comparison of the
two correctly rounded roots it replaces, on the host build, by tools/check_norm_pick.cpp run from here.  Both rewritten picks
are this one function: the yaw-limit alternative `norm(p) > norm(lim)` (lrm_xtab_chain, lrm_finish_closest_fast; arguments
swapped) and the fix-up's `norm(a) < norm(b)` of the two yaw candidates (lrm_redo_pair).  The twin picks keep their roots.

  constructed   equal sums; the four neighbouring floats on either side; every sum above A that shares A's root and the first one
                that does not; 65 floats around A * (1 - 2^-20) and around A / (1 - 2^-20), the two sides of the gap; over all
                exponents, at both edges of [2^-96, 2^96), on denormals and the largest floats; zeros, denormals, inf, nan and
                negative values in all pairs.  Every pair both ways round.
  random        1e7 pairs: half log-uniform and independent, half a few ulps to a few thousand ulps apart.
Any pair that the sums decide differently from the roots fails."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", CSRC, "check-norm-pick"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "build", "check_norm_pick")


def run(tool, *args):
    p = subprocess.run([tool, *args], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    return p, p.stdout.strip().splitlines()


def test_constructed_pairs(tool):
    p, lines = run(tool, "constructed")
    assert p.returncode == 0, p.stdout + p.stderr
    assert lines[-1].startswith("constructed: ") and lines[-1].endswith(" pairs, 0 mismatches")
    counts = dict(item.rsplit(" ", 1) for item in lines[0].split(", "))
    assert set(counts) == {"equal", "neighbours", "same root", "around the gap", "specials"}
    assert all(int(v) > 0 for v in counts.values()) and int(counts["specials"]) == 14 * 14
    # both ways of deciding were exercised, and sums that differ although their roots do not were among the pairs
    by = lines[-2].replace(",", "").split()
    assert int(by[4]) > 0 and int(by[8]) > 0 and int(by[-1]) > 0, lines[-2]


def test_1e7_random_pairs(tool):
    p, lines = run(tool, "random", "10000000", "42")
    assert p.returncode == 0, p.stdout + p.stderr
    assert lines[-1] == "random: 10000000 pairs, 0 mismatches"


def test_tool_refuses_what_it_does_not_know(tool):
    assert subprocess.run([tool], capture_output=True).returncode == 2
    assert subprocess.run([tool, "nothing"], capture_output=True).returncode == 2
