"""The table evaluation of one point (csrc/lrm_point_tol.h: lrm_tab_point, both instances) reproduces, bit for bit, what it
gave before its instruction count was cut: tests/golden/frozen/tab_point_frozen.npz was recorded by
tests/golden/make_tab_point_frozen.py at the commit before the first cut.  Flags, the doubt SET (doubt != 0 as a boolean: which
bits name a doubt is a host statistic) and every float of every vector, raw uint32 -- those of doubtful and non-finite points
included, and, through the strict replay of the info word (dbg_replay_host), every field of the word the kInfo instance packs."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

KINDS = {"yaw": 1, "region": 2, "clamp": 4, "tie": 8, "none": 16, "limit": 32, "pick": 64, "ambig": 0x100}
FROZEN = dict(np.load(os.path.join(GOLDEN, "frozen", "tab_point_frozen.npz")))
CASES = sorted(k[:-len("_points")] for k in FROZEN if k.endswith("_points"))


def test_fixture_covers_what_it_must():
    """24 cases (2 legs x 3 azimuths x 4 orientations); in each: every kind of doubt the host build distinguishes, points beyond
    the inner grid, non-finite points, and doubt-free points for the replay to work on"""
    assert len(CASES) == 24
    for key in CASES:
        doubt = FROZEN[key + "_tab_doubt"]
        for name, bit in KINDS.items():
            assert ((doubt & bit) != 0).any(), (key, name)
        pts = FROZEN[key + "_points"].view(np.float32)
        assert (~np.isfinite(pts)).any() and (np.abs(pts[np.isfinite(pts).all(axis=1)]).max() > 2000.0)
        assert (doubt == 0).mean() > 0.3


@pytest.mark.parametrize("key", CASES)
def test_tab_point_reproduces_the_frozen_outputs(lrm, key):
    pts = FROZEN[key + "_points"].view(np.float32)
    leg, q = FROZEN[key + "_leg"], FROZEN[key + "_quat"]
    m, d, doubt, stats = lrm.dbg_toltab_host(pts, leg, q)
    assert stats["second_candidates"] > 0, "the cloud holds points whose second yaw candidate is evaluated"
    assert np.array_equal(m, FROZEN[key + "_tab_flag"])
    assert np.array_equal(doubt != 0, FROZEN[key + "_tab_doubt"] != 0)
    assert np.array_equal(d.view(np.uint32), FROZEN[key + "_tab_vec"])
    m, d, doubt = lrm.dbg_replay_host(pts, leg, q)
    assert np.array_equal(m, FROZEN[key + "_replay_flag"])
    assert np.array_equal(doubt != 0, FROZEN[key + "_replay_doubt"] != 0)
    assert np.array_equal(d.view(np.uint32), FROZEN[key + "_replay_vec"])
