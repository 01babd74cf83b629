"""Tensor wrappers of the target-assignment entries of libdet6d_hip_ext.so (include/det6d_ext.h): which full-pose box each
point lies in, and the class / box labels the vote head derives from it.  Asynchronous on the current stream; nothing here
reads a result on the host, so all of it can be captured into a graph."""
import torch

from .. import _lib as L


def _layout(points, boxes, xyz_col, bs_col, extra_width, n_per_scene):
    """shared argument checks -> (n_points, ld_points, n_per_scene, b, m, ld_boxes, extra tensor or None)"""
    L.require_cuda(points, boxes)
    if points.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise L.Det6dError("box targets need float32 points and boxes (got %s, %s)" % (points.dtype, boxes.dtype))
    if boxes.dim() != 3:
        raise L.Det6dError("boxes must be (B, M, >= 9), got %s" % (tuple(boxes.shape),))
    b, m, ld_boxes = boxes.shape
    if points.dim() == 3:                       # dense (B, N, ld): scene = row // N
        if bs_col >= 0:
            raise L.Det6dError("a dense (B, N, ld) point tensor carries no scene column")
        if points.shape[0] != b:
            raise L.Det6dError("points of %d scenes, boxes of %d" % (points.shape[0], b))
        n_per_scene, n_points = max(points.shape[1], 1), points.shape[0] * points.shape[1]
    elif points.dim() == 2:                     # stacked (N1 + N2 + ..., ld) with the scene in column bs_col, or dense rows
        if bs_col < 0 and (n_per_scene is None or n_per_scene < 1):
            raise L.Det6dError("(N, ld) points need the column of the scene index (bs_col) or the rows per scene (n_per_scene)")
        n_per_scene, n_points = (1 if bs_col >= 0 else n_per_scene), points.shape[0]
    else:
        raise L.Det6dError("points must be (N, ld) or (B, N, ld), got %s" % (tuple(points.shape),))
    extra = None
    if extra_width is not None:
        if torch.is_tensor(extra_width):
            extra = extra_width.to(device=points.device, dtype=torch.float32).contiguous()
        else:
            extra = torch.tensor([float(v) for v in extra_width], dtype=torch.float32, device=points.device)
        if extra.numel() != 3:
            raise L.Det6dError("extra_width must hold 3 values")
    return n_points, points.shape[-1], n_per_scene, b, m, ld_boxes, extra


def points_in_boxes9(points, boxes, extra_width=None, xyz_col=None, bs_col=None, n_per_scene=None):
    """Index of the box [x, y, z, dx, dy, dz, rz, ry, rx] each point lies in: (n_points,) int32, -1 outside every box of the
    point's scene, the HIGHEST index where boxes overlap.  points: stacked (N, ld) rows with the scene index in column bs_col
    (default 0, coordinates from column 1), dense (B, N, ld) (coordinates from column 0), or (N, ld) with bs_col=-1 and
    n_per_scene consecutive rows per scene; boxes (B, M, >= 9); extra_width:
    3 values added to dx, dy, dz.  Boxes whose enlarged size is not positive in all three axes contain nothing."""
    stacked = points.dim() == 2
    bs_col = (0 if stacked else -1) if bs_col is None else bs_col
    xyz_col = (1 if stacked else 0) if xyz_col is None else xyz_col
    n_points, ld, n_per_scene, b, m, ld_boxes, extra = _layout(points, boxes, xyz_col, bs_col, extra_width, n_per_scene)
    box_idx = torch.full((n_points,), -1, dtype=torch.int32, device=points.device)
    L.call_ext("det6d_ext_points_in_boxes9", n_points, L.ptr(points), ld, xyz_col, bs_col, n_per_scene, b, m, L.ptr(boxes),
               ld_boxes, L.ptr(extra), L.ptr(box_idx), L.stream_ptr())
    return box_idx


def assign_targets9(points, boxes, extra_width=None, class_col=-1, num_class=1, central_radius=0.0, n_cols=3, xyz_col=None,
                    bs_col=None, n_per_scene=None):
    """points_in_boxes9 plus the labels of the head in the same launch -> (box_idx (n,) int32, cls_labels (n,) int64,
    box_labels (n, n_cols) float32).  cls_labels: 0 outside every box, -1 inside a box but not closer than central_radius
    to its centre (central_radius <= 0: no such constraint), otherwise 1 when num_class == 1 or class_col < 0, else the
    box's column class_col.  box_labels: the first n_cols columns of the box for the points labelled foreground, else 0."""
    stacked = points.dim() == 2
    bs_col = (0 if stacked else -1) if bs_col is None else bs_col
    xyz_col = (1 if stacked else 0) if xyz_col is None else xyz_col
    n_points, ld, n_per_scene, b, m, ld_boxes, extra = _layout(points, boxes, xyz_col, bs_col, extra_width, n_per_scene)
    dev = points.device
    box_idx = torch.full((n_points,), -1, dtype=torch.int32, device=dev)
    cls_labels = torch.zeros((n_points,), dtype=torch.int64, device=dev)
    box_labels = torch.zeros((n_points, n_cols), dtype=torch.float32, device=dev)
    L.call_ext("det6d_ext_assign_targets9", n_points, L.ptr(points), ld, xyz_col, bs_col, n_per_scene, b, m, L.ptr(boxes),
               ld_boxes, L.ptr(extra), class_col, num_class, float(central_radius), L.ptr(box_idx), L.ptr(cls_labels),
               L.ptr(box_labels), n_cols, n_cols, L.stream_ptr())
    return box_idx, cls_labels, box_labels
