"""Python API of core/pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py:28-41 over libdet6d_hip_ext: the yaw-only
point-in-box test PointSASALoss labels its points with (csrc/ext/sasa_loss.hip).  points_in_boxes_cpu and the RoI-aware
pooling layer are not on the Det6D path and raise."""
from ...ops_backend import sasa_loss


def points_in_boxes_cpu(points, boxes):
    raise NotImplementedError("roiaware_pool3d_utils.points_in_boxes_cpu is not implemented (no CPU path; points_in_boxes_gpu)")


def points_in_boxes_gpu(points, boxes):
    """
    :param points: (B, M, 3)
    :param boxes: (B, T, 7), num_valid_boxes <= T
    :return box_idxs_of_pts: (B, M) int32, the FIRST box that holds the point, default background = -1
    """
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    batch_size, num_points, _ = points.shape
    return sasa_loss.points_in_boxes7(points.contiguous(), boxes.contiguous()).view(batch_size, num_points)


class RoIAwarePool3d(object):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("RoIAwarePool3d is not implemented (the RoI-aware pooling layer is not on the Det6D path)")
