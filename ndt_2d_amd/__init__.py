"""ndt_2d_amd -- MI355X-native NDT scan-matching hot path of ndt_2d.

Host-side handles over libndt2d_hip.so (include/ndt2d_hip.h).  The package holds
only what the hot path needs: csrc/ (HIP kernels + C-ABI), the Python mirror of
the reference's ScanMatcher plugin interface, the synthetic workload generator
and the multi-GPU sharding helper.
"""
from ._capi import LIB_PATH, Ndt2dError  # noqa: F401
from .occupancy_map import OccupancyMap  # noqa: F401
from .particle_filter import MotionModel, ParticleFilter, RecoveryAverages  # noqa: F401
from .pose_graph import PoseGraph, closure_constraints, closure_distance, make_constraint, relative_covariance  # noqa: F401
from .seeder import Seeder  # noqa: F401
from .clearance import ClearanceMap  # noqa: F401
from .clusters import Clusterer, PoseCluster  # noqa: F401
from .wide_search import WideSearch  # noqa: F401
from .scan_matcher import (DEFAULT_PARAMS, Resampler, ScanMatcherNDT, close_loops, heading_fan,  # noqa: F401
                           explained_mask, host_build_grid, loop_closure_window, pf_measure, pf_update, refine_covariance, refine_matches,
                           relocalize, search_offsets, track_scans)

__all__ = ["ScanMatcherNDT", "Resampler", "ParticleFilter", "MotionModel", "pf_measure", "pf_update",
           "search_offsets", "host_build_grid", "DEFAULT_PARAMS", "Ndt2dError", "LIB_PATH", "OccupancyMap",
           "close_loops", "loop_closure_window", "relocalize", "heading_fan", "track_scans", "refine_matches", "refine_covariance", "explained_mask",
           "PoseGraph", "make_constraint", "closure_constraints", "relative_covariance", "closure_distance",
           "Seeder", "ClearanceMap", "RecoveryAverages", "Clusterer", "PoseCluster"]
