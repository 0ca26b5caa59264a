"""lrm_footholds_cpu (include/lrm.h) against a brute force over the oracle's reachable_rotate_leg, with the count, the
argmin and d2 recomputed in numpy float32; its edge cases and argument checks (also those of lrm_footholds_dev, which
run before any device work)."""
import ctypes as C

import numpy as np
import pytest

from footholds_cases import QUATS, bits, expected, legs_for, nominal_for, oracle_reachable, scene

LRM_EINVAL = -1


@pytest.mark.parametrize("nlegs,qname", [(4, "identity"), (6, "identity"), (4, "tilted"), (6, "tilted")])
def test_footholds_cpu_matches_oracle_bruteforce(lrm, oracle, nlegs, qname):
    quat = QUATS[qname]
    bodies, targets = scene(48, 1500, seed=nlegs)
    legs = legs_for(lrm, nlegs, quat)
    reach = oracle_reachable(oracle, bodies, targets, legs, quat)
    assert 0.05 < (reach.sum(-1) > 0).mean() < 1.0 and reach.sum(-1).max() > 2  # empty and crowded (leg, body) pairs
    for nominal in (None, nominal_for(nlegs)):
        want = expected(reach, bodies, targets, nominal)
        count, best, best_d2, ms = lrm.footholds_cpu(bodies, targets, legs, quat, nominal)
        assert count.shape == best.shape == best_d2.shape == (nlegs, len(bodies)) and ms >= 0
        assert np.array_equal(count, want[0])
        assert np.array_equal(best, want[1])
        assert np.array_equal(bits(best_d2), bits(want[2]))


def test_footholds_cpu_edge_cases(lrm):
    bodies, targets = scene(40, 1200, seed=11)
    legs = legs_for(lrm, 4, QUATS["identity"])
    nominal = nominal_for(4)
    count, best, best_d2, _ = lrm.footholds_cpu(bodies, targets, legs, None, nominal)
    assert (count > 0).any() and (count == 0).any()
    # no targets: count 0, best -1, +inf everywhere
    c0, b0, d0, _ = lrm.footholds_cpu(bodies, np.zeros((0, 3), np.float32), legs, None, nominal)
    assert (c0 == 0).all() and (b0 == -1).all() and np.isposinf(d0).all()
    # the cloud twice: twice the count, the choice stays in the first copy
    c2, b2, d2, _ = lrm.footholds_cpu(bodies, np.concatenate([targets, targets]), legs, None, nominal)
    assert np.array_equal(c2, 2 * count) and np.array_equal(b2, best) and np.array_equal(bits(d2), bits(best_d2))
    # a NaN target in front: never counted, never chosen
    nan_first = np.concatenate([np.full((1, 3), np.nan, np.float32), targets])
    cn, bn, dn, _ = lrm.footholds_cpu(bodies, nan_first, legs, None, nominal)
    assert np.array_equal(cn, count) and np.array_equal(bn, np.where(best >= 0, best + 1, -1))
    assert np.array_equal(bits(dn), bits(best_d2))


def test_footholds_argument_checks(lrm):
    """nt > INT32_MAX and nlegs outside 1..LRM_MAX_LEGS are refused before the nb == 0 early return, so no buffer is read"""
    L = lrm.load()
    legs = legs_for(lrm, 8, QUATS["identity"])
    f = np.zeros(16, np.float32)
    i = np.zeros(16, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for nt, nlegs in ((2 ** 31, 6), (100, 0), (100, 9)):
        assert L.lrm_footholds_cpu(p(f), 0, p(f), nt, p(legs), nlegs, None, None, p(i), p(i), p(f), None) == LRM_EINVAL
        assert L.lrm_footholds_dev(p(f), p(f), p(f), 0, p(f), p(f), p(f), nt, p(legs), nlegs, None, None, p(i), p(i),
                                   p(f), None) == LRM_EINVAL
    assert L.lrm_footholds_cpu(p(f), 0, p(f), 2 ** 31 - 1, p(legs), 6, None, None, p(i), p(i), p(f), None) == 0
    with pytest.raises(ValueError):
        lrm.footholds_cpu(np.zeros((2, 3)), np.zeros((5, 3)), legs[:2], None, np.zeros((3, 3)))
