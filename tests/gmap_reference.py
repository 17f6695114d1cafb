"""numpy restatement of the loop-corrected global map (publishGlobalMap, global_fusion/poseGraphOptimization.cpp:310-336), from the statement of the semantics in
include/vilfusion.h: every selected key-frame cloud under its own pose, concatenated in key-frame order, pcl::VoxelGrid. Built from icp_reference's pose_matrix,
transform and voxel_grid, which the sub-map tests already pin against the oracle."""
import numpy as np

import icp_reference as R


def selected(first, count, skip):
    return range(first, first + count, skip)


def concatenation(clouds, poses6, first, count, skip):
    parts = [R.transform(R.pose_matrix(poses6[k]), R.xyzi(clouds[k])) for k in selected(first, count, skip)]
    parts = [q for q in parts if len(q)]
    return np.concatenate(parts) if parts else np.zeros((0, 4), dtype=R.F)


def global_map(clouds, poses6, first, count, skip, leaf):
    """clouds first, first + skip, ... (< first + count), each under its own pose -> (n, 4) float32 in ascending leaf index"""
    return R.voxel_grid(concatenation(clouds, poses6, first, count, skip), leaf)
