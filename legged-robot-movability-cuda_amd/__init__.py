"""MI355X-native reach / distance / positionability path (drop-in for the hot path of
2lian/Legged-Robot-Movability-Cuda).  The product is csrc/ -> liblrm.so (HIP kernels + the
C ABI of include/lrm.h); this package is the Python binding used by tests and bench.py.
The C++ mirror of the reference's host interface is include/lrm_compat.hpp.
"""
from ._capi import (  # noqa: F401
    LIB_PATH, LrmError, MODE_FAST, MODE_STRICT, MODE_TOL, MODE_TOL_REL, build, lib, load, leg_factory, get_M2_leg,
    get_moonbot_leg, rotate_leg_data, apply_reach, apply_dist, apply_reach_dist,
    apply_reach_cpu, apply_dist_cpu, apply_rbdl_equiv, positionability, set_mode, get_mode, device_count,
    exported_symbols, declared_symbols, dbg_fast_host, dbg_fused_reach_host, dbg_tol_host, dbg_tol_ok, dbg_toltab_host, dbg_toltab_bounds, dbg_xtab_host, dbg_replay_host, dbg_toltab_build, shard_bounds as c_shard_bounds, apply_reach_dist_multi, tol_prepare, last_table_build_ms, release_workspaces, dbg_tol_queue_counts, dbg_tol_grid, dbg_pair_counts, dbg_oct_trace, dbg_oct_trace_read, dbg_oct_plan, dbg_pair_sphere, apply_oct, apply_oct_sharded, apply_oct_partitioned, octree_default_settings,
    OctreeSettings, morton_order, apply_reach_dist_posed_cpu, dbg_pose_compile_host, dbg_compile_leg_head,
    POSE_RECORD_BYTES, apply_ik_cpu, apply_fk_cpu, IK_NONE, IK_REACHED, IK_NEAREST, IK_MODEL_GAP, IK_FAR_GAP, footholds_cpu,
    apply_ik_posed_cpu, apply_fk_posed_cpu, dbg_pose_ik_compile_host, POSE_IK_RECORD_BYTES,
    footholds_posed_cpu, dbg_pose_footholds_compile_host, POSE_FOOTHOLD_BYTES, foothold_lists_posed_cpu,
    foothold_edges_posed_cpu,
    foothold_misses_posed_cpu,
    foothold_support_posed_cpu, dbg_foothold_support_grid,
    body_clearance_posed_cpu,
    leg_clearance_posed_cpu, leg_joints_posed_cpu,
    stance_stability_cpu, stance_lift,
    stance_loads_posed_cpu, LOADS_DEAD, LOADS_ALL, LOADS_DROPPED, LOADS_TRIPOD, LOADS_NONE,
    pose_routes_cpu, dbg_pose_routes_plan,
    pose_edges_cpu, pose_edges_min_dot, dbg_pose_edges_plan,
    self_clearance_posed_cpu, trunk_clearance_posed_cpu, edge_transit_posed_cpu, swing_transit_posed_cpu, dbg_link_pair_dist_host, dbg_trunk_link_dist_host, dbg_edge_transit_samples_host,
)
from . import device  # noqa: F401
from .device import PoseSet, ik, fk, edge_transit, swing_transit, stance_loads, pose_routes, route_path, pose_edges, pose_edge_counts, pose_edges_workspace, swing_layout, foothold_offsets, foothold_edges_layout, foothold_support_layout, dbg_link_pair_dist, dbg_trunk_link_dist, dbg_edge_transit_samples  # noqa: F401
from . import shard  # noqa: F401
