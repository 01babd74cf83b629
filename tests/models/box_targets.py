"""Executable CPU model of the target-assignment entries (de6d_amd/csrc/ext/box_targets.hip, include/det6d_ext.h) — TEST
INFRASTRUCTURE ONLY.

The reference's box_utils.points_in_boxes3d (box_utils.py:336-350) tests every point against the Delaunay hull of the float64
corners of every box; the engine tests fp32 local coordinates against the half extents, with an arithmetic fixed in the header:
  * per box: sin / cos of rz, ry, rx from d6_sincosf (oracle.ops.math_fn); the nine entries of R = Rx Ry Rz from singly rounded
    fp32 products and one rounded add / subtract each (rotations, below); half = 0.5f * (dims + extra); a box takes part only
    if all three dims + extra are > 0;
  * per pair: d = p - c in fp32, l_k = fmaf(d_z, R2k, fmaf(d_y, R1k, d_x * R0k)) — NumPy has no fmaf and emulating one in
    float64 rounds twice, so l = oracle.ops.linear(d, R), which is exactly that ascending chain from 0; inside iff
    |l_k| <= half_k for all k;
  * boxes in ascending order, a later box overwrites (= the kernel's scan from the top to the first hit);
  * ball: float64 ((dx*dx + dy*dy) + dz*dz) < r*r on the fp32 differences of the winning box (each product exact in float64).
"""
import numpy as np

from oracle import ops

F32 = np.float32


def rotations(angles):
    """(m, 3) [rz, ry, rx] -> (m, 3, 3) fp32 R = Rx(rx) Ry(ry) Rz(rz), entry by entry as det6d_ext.h spells them"""
    a = np.ascontiguousarray(angles, F32).reshape(-1, 3)
    sz, cz = ops.math_fn("sin", a[:, 0].copy()), ops.math_fn("cos", a[:, 0].copy())
    sy, cy = ops.math_fn("sin", a[:, 1].copy()), ops.math_fn("cos", a[:, 1].copy())
    sx, cx = ops.math_fn("sin", a[:, 2].copy()), ops.math_fn("cos", a[:, 2].copy())
    t, u = sx * sy, cx * sy                                   # float32 arrays: every operation rounds once
    r = np.empty((len(a), 3, 3), F32)
    r[:, 0, 0], r[:, 0, 1], r[:, 0, 2] = cy * cz, -(cy * sz), sy
    r[:, 1, 0], r[:, 1, 1], r[:, 1, 2] = cx * sz + t * cz, cx * cz - t * sz, -(sx * cy)
    r[:, 2, 0], r[:, 2, 1], r[:, 2, 2] = sx * sz - u * cz, sx * cz + u * sz, cx * cy
    return r


def local_coordinates(points, box, rot):
    """(n, 3) fp32 points, one box row, its (3, 3) rotation -> (d, l): d = p - c, l = R^T d by the fmaf chain"""
    d = (np.asarray(points, F32) - np.asarray(box[:3], F32)[None, :]).astype(F32)
    with np.errstate(invalid='ignore', over='ignore'):
        return d, ops.linear(np.ascontiguousarray(d), np.ascontiguousarray(rot))


def half_extents(boxes, extra_width=None):
    """(m, >= 9) -> ((m, 3) fp32 half extents, (m,) bool: the box takes part)"""
    e = np.zeros(3, F32) if extra_width is None else np.asarray(extra_width, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        w = (np.asarray(boxes, F32)[:, 3:6] + e[None, :]).astype(F32)
        return (F32(0.5) * w).astype(F32), (w > 0).all(1)


def points_in_boxes9_scene(points, boxes, extra_width=None):
    """one scene: points (n, 3), boxes (m, >= 9) -> (box_idx (n,) int32, d (n, 3) fp32 = p - centre of the winner, 0 if none)"""
    points = np.ascontiguousarray(points, F32)
    boxes = np.ascontiguousarray(boxes, F32)
    idx = np.full(len(points), -1, np.int32)
    dwin = np.zeros((len(points), 3), F32)
    if len(points) == 0 or len(boxes) == 0:
        return idx, dwin
    rot = rotations(boxes[:, 6:9])
    half, live = half_extents(boxes, extra_width)
    for i in range(len(boxes)):
        if not live[i]:
            continue
        d, l = local_coordinates(points, boxes[i], rot[i])
        with np.errstate(invalid='ignore'):
            inside = (np.abs(l) <= half[i][None, :]).all(1)
        idx[inside] = i
        dwin[inside] = d[inside]
    return idx, dwin


def scenes_of(points, bs_col, n_per_scene, b):
    """(n_points,) scene of every row, -1 = background"""
    n = len(points)
    if bs_col >= 0:
        s = np.asarray(points, F32)[:, bs_col]
        with np.errstate(invalid='ignore'):
            ok = (s >= 0) & (s < F32(b))
        return np.where(ok, np.where(ok, s, 0).astype(np.int64), -1)
    s = np.arange(n, dtype=np.int64) // n_per_scene
    return np.where(s < b, s, -1)


def assign_targets9(points, boxes, xyz_col=0, bs_col=-1, n_per_scene=1, extra_width=None, class_col=-1, num_class=1,
                    central_radius=0.0, n_cols=3):
    """det6d_ext_assign_targets9: points (n_points, ld), boxes (b, m, ld_boxes) -> box_idx int32, cls_labels int64,
    box_labels (n_points, n_cols) fp32"""
    points = np.asarray(points, F32)
    boxes = np.asarray(boxes, F32)
    b, m = boxes.shape[:2]
    n = len(points)
    idx = np.full(n, -1, np.int32)
    cls = np.zeros(n, np.int64)
    lab = np.zeros((n, n_cols), F32)
    scene = scenes_of(points, bs_col, n_per_scene, b)
    radius = F32(central_radius)
    for s in range(b):
        rows = np.nonzero(scene == s)[0]
        if len(rows) == 0 or m == 0:
            continue
        i, d = points_in_boxes9_scene(points[rows, xyz_col:xyz_col + 3], boxes[s], extra_width)
        inside = i >= 0
        near = np.ones(len(rows), bool)
        if radius > 0:
            d64 = d.astype(np.float64)
            near = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2] < np.float64(radius) * np.float64(radius)
        fg = inside & near
        win = boxes[s][np.maximum(i, 0)]
        label = np.ones(len(rows), np.int64) if (num_class == 1 or class_col < 0) else win[:, class_col].astype(np.int64)
        idx[rows] = i
        cls[rows] = np.where(fg, label, np.where(inside, -1, 0))
        lab[rows] = np.where(fg[:, None], win[:, :n_cols], F32(0))
    return idx, cls, lab


def points_in_boxes9(points, boxes, xyz_col=0, bs_col=-1, n_per_scene=1, extra_width=None):
    """det6d_ext_points_in_boxes9 -> box_idx (n_points,) int32"""
    return assign_targets9(points, boxes, xyz_col, bs_col, n_per_scene, extra_width, n_cols=0)[0]
