"""The launch grids of the distance / fused calls (include/lrm.h: lrm_dbg_tol_grid) and the cloud sizes at which they change
shape, shared by tests/test_grid_cpu.py (the sizing invariant of lrm_tol_prepare) and tests/test_gpu_shapes.py (the kernels
at those sizes).  Every size comes from the library's own grid functions, so the tests keep aiming at the transitions if a
grid constant changes."""
import functools

import numpy as np

BLOCK = 256                        # threads (points per round) of a workgroup
KERNELS = ("tab", "rel", "notab")  # table kernels of LRM_MODE_TOL / LRM_MODE_FAST, of LRM_MODE_TOL_REL, the kernel without a table
SCAN_NEED = 1 << 17                # transitions are looked for among clouds of up to 2^17 workgroups (33.5 M points)
FIXED_RUN = 64                     # a grid whose workgroup count stood still for this many workgroups of cloud is at a fixed count
TOLTAB_MIN_POINTS = 200_000        # the size from which the calls take the plane-table kernels (csrc/lrm_capi.cpp)
RAGGED = 69                        # n_t - RAGGED: n % 64 != 0 and n % 4 != 0, on the near side of a transition


def grid_table(lrm, need_max):
    """workgroups of every kernel and the words a call requests, for clouds of 256 * need points, need = 0 .. need_max"""
    out = {k: np.zeros(need_max + 1, np.int64) for k in KERNELS + ("tab_words", "notab_words", "prepare_words")}
    for need in range(need_max + 1):
        g = lrm.dbg_tol_grid(need * BLOCK)
        for k, v in g.items():
            out[k][need] = v
    return out


@functools.lru_cache(maxsize=None)
def transitions(lrm, need_max=SCAN_NEED):
    """{need t: what changes shape between clouds of t and t + 1 workgroups}, t < need_max.  A grid changes shape where its
    rounds per workgroup, ceil(need / workgroups), change, and where its workgroup count starts to grow again after standing
    at a fixed count (a floor or a ceiling of the grid); the queue words a call requests change shape where they start to
    grow again after standing still."""
    g = grid_table(lrm, need_max)
    need = np.arange(need_max + 1)
    out = {}
    for k in KERNELS + ("tab_words", "notab_words"):
        v = g[k]
        rounds = -(-need // np.maximum(v, 1)) if k in KERNELS else np.zeros_like(need)
        for t in range(1, need_max):
            change = rounds[t + 1] != rounds[t]
            change |= t >= FIXED_RUN and v[t + 1] > v[t] == v[t - FIXED_RUN]
            if change:
                out.setdefault(t, []).append(k)
    return out


def gpu_sizes(lrm):
    """the sizes tests/test_gpu_shapes.py runs: for every transition t (workgroups) n_t = 256 t, n_t + 1 (the first point of
    the next grid) and n_t - RAGGED (a ragged last wave on the near side); the dispatch switch to the table kernels; one size
    well past the rounds cap (about 5e7 points, ragged)"""
    sizes = set()
    for t in transitions(lrm):
        n_t = t * BLOCK
        sizes.update((n_t, n_t + 1, n_t - RAGGED))
    sizes.update((TOLTAB_MIN_POINTS - 1, TOLTAB_MIN_POINTS, TOLTAB_MIN_POINTS + 1))
    sizes.add(50_000_003)
    return sorted(sizes)
