"""The parts of core/pcdet/utils/box_utils.py the Det6D target assignment needs, on the device.

`points_in_boxes3d` (:336-350) is a host-side hull test in the reference (scipy Delaunay, box by box); here it is one HIP
kernel (csrc/ext/box_targets.hip) with the same result convention: the index of the box a point lies in, -1 outside every
box, the highest index where boxes overlap, nothing inside a box without a positive size (the zero rows padding gt_boxes)."""
import torch

from ...ops import box_targets


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """(N, 6 + C) [x, y, z, dx, dy, dz, ...] -> a copy with extra_width added to dx, dy, dz (:180-193)"""
    large_boxes3d = boxes3d.clone()
    large_boxes3d[:, 3:6] += boxes3d.new_tensor(extra_width)[None, :]
    return large_boxes3d


def points_in_boxes3d(points, boxes3d):
    """points (n, 3+), boxes3d (m, 9) [x, y, z, dx, dy, dz, rz, ry, rx], device tensors of one scene -> (n,) int64 on the
    points' device: the index of the box each point lies in, -1 if none"""
    assert boxes3d.shape[-1] == 9
    pts = points[:, :3].contiguous().unsqueeze(0)
    return box_targets.points_in_boxes9(pts, boxes3d.contiguous().unsqueeze(0)).long()
