"""Tensor wrappers of the SASA entries of libdet6d_hip_ext.so (include/det6d_ext.h): the yaw-only point-in-box test, the
layer-wise segmentation labels of PointSASALoss, its loss and the gradient with respect to the confidence scores.  Asynchronous
on the current stream; nothing here reads a result on the host (the upstream gradient stays on the device too), so labels,
forward and backward can be captured into a graph."""
import torch

from .. import _lib as L
from .box_targets import _layout

BCE, FOCAL = 0, 1
FUNCS = {'BCE': BCE, 'Focal': FOCAL}
MAX_SEGMENTS = 8
IGNORE, LABELS_GIVEN = 1, 2
#: entries of a layer's four floats in `sums`; the total follows the last layer
LOSS, NORM, N_POS, N_IGNORE = range(4)


def points_in_boxes7(points, boxes, extra_width=None, xyz_col=None, bs_col=None, n_per_scene=None):
    """Index of the yaw-only box [x, y, z, dx, dy, dz, rz] each point lies in: (n_points,) int32, -1 outside every box of the
    point's scene, the LOWEST index where boxes overlap (points_in_boxes9 takes the highest).  The point layouts are those of
    points_in_boxes9; boxes (B, M, >= 7), columns beyond rz are not read; extra_width: 3 values added to dx, dy, dz.  Zero-sized
    boxes are boxes (the margin of the reference's test makes them 2e-5 wide)."""
    stacked = points.dim() == 2
    bs_col = (0 if stacked else -1) if bs_col is None else bs_col
    xyz_col = (1 if stacked else 0) if xyz_col is None else xyz_col
    n_points, ld, n_per_scene, b, m, ld_boxes, extra = _layout(points, boxes, xyz_col, bs_col, extra_width, n_per_scene)
    box_idx = torch.full((n_points,), -1, dtype=torch.int32, device=points.device)
    L.call_ext("det6d_ext_points_in_boxes7", n_points, L.ptr(points), ld, xyz_col, bs_col, n_per_scene, b, m, L.ptr(boxes),
               ld_boxes, L.ptr(extra), L.ptr(box_idx), L.stream_ptr())
    return box_idx


class SasaSpec(object):
    """the scalars of one LOSS_SASA_CONFIG.  extra_width is uploaded once per device (an upload cannot be captured)"""

    def __init__(self, func, layer_weights, extra_width=None, set_ignore_flag=False, alpha=0.25, gamma=2.0):
        if func not in FUNCS:
            raise NotImplementedError("PointSASALoss func: %s (BCE, Focal)" % (func,))
        if layer_weights is None or len(layer_weights) > MAX_SEGMENTS:
            raise ValueError("layer_weights must list at most %d layers, got %r" % (MAX_SEGMENTS, layer_weights))
        assert not set_ignore_flag or extra_width is not None, "set_ignore_flag needs extra_width"
        if extra_width is not None and len(extra_width) != 3:
            raise ValueError("extra_width must hold 3 values")
        self.func = FUNCS[func]
        self.layer_weights = [float(w) for w in layer_weights]
        self.extra_width = None if extra_width is None else tuple(float(v) for v in extra_width)
        self.set_ignore_flag = bool(set_ignore_flag)
        self.alpha, self.gamma = float(alpha), float(gamma)
        self._extra = {}

    def extra(self, device):
        if self.extra_width is None:
            return None
        if device not in self._extra:
            self._extra[device] = torch.tensor(self.extra_width, dtype=torch.float32, device=device)
        return self._extra[device]

    def skipped(self, i, scores_list):
        """the reference's rule (loss_utils.py:506): no scores at this level, or a weight of 0"""
        return i >= len(scores_list) or scores_list[i] is None or self.layer_weights[i] == 0


def _segments(spec, coords_list, scores_list, gt_boxes, labels=None, d_scores=None):
    """argument checks -> (SasaSegment array, b, the tensors it points into).  coords: dense (B, M, >= 3) with the coordinates
    in columns 0..2, or the (B * M, 4) [batch index, x, y, z] rows of point_coords_list — every scene holding M consecutive
    rows, as everywhere in this project (the batch index column is not read); scores (B * M, 1) or (B * M,).  A level whose
    coords is None is one scene of as many rows as it has scores: for labels the caller holds (gt_boxes (1, 0, 7))"""
    n = len(spec.layer_weights)
    L.require_cuda(gt_boxes)
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] < 7:
        raise L.Det6dError("the SASA loss needs float32 gt_boxes (B, M, >= 7), got %s %s" % (tuple(gt_boxes.shape), gt_boxes.dtype))
    if len(coords_list) < n:
        raise L.Det6dError("%d layer weights, coordinates of %d levels" % (n, len(coords_list)))
    b = gt_boxes.shape[0]
    segs = (L.SasaSegment * max(n, 1))()
    keep = []
    for i in range(n):
        segs[i].ld, segs[i].weight = 3, spec.layer_weights[i]
        if spec.skipped(i, scores_list):
            continue
        coords, scores = coords_list[i], scores_list[i]
        L.require_cuda(coords, scores)
        if (coords is not None and coords.dtype != torch.float32) or scores.dtype != torch.float32:
            raise L.Det6dError("the SASA loss needs float32 coordinates and scores")
        if coords is None:
            if b != 1 or labels is None or labels[i] is None:
                raise L.Det6dError("level %d: no coordinates and no labels" % i)
            m, xyz_col = scores.numel(), 0
        elif coords.dim() == 3 and coords.shape[0] == b and coords.shape[2] >= 3:
            m, xyz_col = coords.shape[1], 0
        elif coords.dim() == 2 and coords.shape[1] == 4 and b > 0 and coords.shape[0] % b == 0:
            m, xyz_col = coords.shape[0] // b, 1
        else:
            raise L.Det6dError("level %d: coordinates must be (%d, M, >= 3) or (%d * M, 4), got %s" % (i, b, b, tuple(coords.shape)))
        if scores.numel() != b * m or scores.dim() > 2:
            raise L.Det6dError("level %d: %d scores for %d points" % (i, scores.numel(), b * m))
        if coords is not None:
            segs[i].coords, segs[i].ld = coords.data_ptr(), coords.shape[-1]
        segs[i].m, segs[i].xyz_col = m, xyz_col
        segs[i].scores = scores.data_ptr()
        keep += [coords, scores]
        for field, tensors in (('labels', labels), ('d_scores', d_scores)):
            if tensors is not None and tensors[i] is not None:
                L.require_cuda(tensors[i])
                if tensors[i].numel() != b * m or tensors[i].dtype != (torch.int64 if field == 'labels' else torch.float32):
                    raise L.Det6dError("level %d: %s must hold %d values" % (i, field, b * m))
                setattr(segs[i], field, tensors[i].data_ptr())
                keep.append(tensors[i])
    return segs, b, keep


def _call(name, spec, segs, b, gt_boxes, given, *tail):
    n = len(spec.layer_weights)
    flags = (IGNORE if spec.set_ignore_flag else 0) | (LABELS_GIVEN if given else 0)
    L.call_ext(name, n, segs, b, gt_boxes.shape[1], L.ptr(gt_boxes) if gt_boxes.numel() else None, gt_boxes.shape[2],
               L.ptr(spec.extra(gt_boxes.device)), flags, spec.func, spec.alpha, spec.gamma, *tail, L.stream_ptr())


def forward(spec, coords_list, scores_list, gt_boxes, labels=False, given_labels=None):
    """-> sums (4 L + 1,) float32: per layer [weight * loss sum / max(norm, 1), norm = #(label >= 0), #(label > 0),
    #(label < 0)], then the total; with labels=True also the list of int64 labels per layer (None for a skipped layer: no
    scores, or a weight of 0 — its four sums are zero).  given_labels: a list of (N_i,) int64 labels to READ instead of
    testing the points (PointSASALoss.loss_forward); coordinates and boxes are then not read"""
    n = len(spec.layer_weights)
    dev = gt_boxes.device
    out = given_labels
    if labels and given_labels is None:
        out = [None if spec.skipped(i, scores_list) else torch.empty((scores_list[i].numel(),), dtype=torch.int64, device=dev)
               for i in range(n)]
    segs, b, keep = _segments(spec, coords_list, scores_list, gt_boxes, labels=out)
    ws_bytes = L.ext_lib().det6d_ext_sasa_workspace_bytes(n, segs, b)
    if ws_bytes < 0:
        raise L.Det6dError("the SASA loss: the sizes are out of range (include/det6d_ext.h)")
    # the final launch writes every element of sums; without rows nothing is launched and the sums are zero
    sums = (torch.empty if ws_bytes > 0 else torch.zeros)((4 * n + 1,), dtype=torch.float32, device=dev)
    workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _call("det6d_ext_sasa_forward", spec, segs, b, gt_boxes, given_labels is not None, L.ptr(workspace), ws_bytes, L.ptr(sums))
    return (sums, out) if labels else sums


def assign(spec, coords_list, scores_list, gt_boxes):
    """PointSASALoss.forward: the list of labels (N_i,) int64 — 1 foreground, 0 background, -1 ignored — or None per layer"""
    return forward(spec, coords_list, scores_list, gt_boxes, labels=True)[1]


def backward(spec, sums, grad, coords_list, scores_list, gt_boxes, labels=None, grad_stride=0):
    """grad: one float32 on the device, the upstream gradient of the total — or, with grad_stride > 0, one per layer,
    grad_stride floats apart (4: a gradient shaped like sums) -> the list of d_scores, shaped like the scores (None for a
    skipped layer).  labels: what forward(labels=True) returned, read instead of testing the points again"""
    n = len(spec.layer_weights)
    L.require_cuda(sums, grad)
    if sums.dtype != torch.float32 or sums.numel() != 4 * n + 1 or grad.dtype != torch.float32 \
            or grad.numel() < 1 + grad_stride * max(n - 1, 0):
        raise L.Det6dError("the SASA backward needs the forward's sums and the float32 upstream gradient on the device")
    d_scores = [None if spec.skipped(i, scores_list) else torch.empty_like(scores_list[i]) for i in range(n)]   # every row is written
    segs, b, keep = _segments(spec, coords_list, scores_list, gt_boxes, labels=labels, d_scores=d_scores)
    _call("det6d_ext_sasa_backward", spec, segs, b, gt_boxes, False, L.ptr(sums), L.ptr(grad), grad_stride)
    return d_scores


class SasaLoss(torch.autograd.Function):
    """loss, sums = SasaLoss.apply(spec, gt_boxes, coords_list, labels_list, *scores): one entry of `scores` per layer weight
    (None where the level has no confidence layer).  labels_list: None — the points are tested against gt_boxes — or the labels
    assign() returned, which are then read (gt_boxes and coords_list may be None).  loss is a 0-d view of sums (its last
    element); coordinates, boxes and labels are constants."""

    @staticmethod
    def forward(ctx, spec, gt_boxes, coords_list, labels_list, *scores):
        n = len(spec.layer_weights)
        scores = [None if s is None else s.detach().contiguous() for s in scores]
        if labels_list is None:
            gt_boxes = gt_boxes.detach().contiguous()
            coords = [None if spec.skipped(i, scores) else coords_list[i].detach().contiguous() for i in range(n)]
            sums, labels = forward(spec, coords, scores, gt_boxes, labels=True)
        else:
            gt_boxes = next(s for s in scores if s is not None).new_zeros((1, 0, 7))
            labels = [None if spec.skipped(i, scores) else labels_list[i].detach().contiguous().view(-1) for i in range(n)]
            sums = forward(spec, [None] * n, scores, gt_boxes, given_labels=labels)
        ctx.spec, ctx.scores, ctx.labels, ctx.boxes = spec, scores, labels, gt_boxes
        ctx.save_for_backward(sums)
        ctx.mark_non_differentiable(sums)
        return sums[-1], sums

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums):
        sums, = ctx.saved_tensors
        n = len(ctx.spec.layer_weights)
        grad_loss = grad_loss.detach().to(torch.float32).contiguous()
        d_scores = backward(ctx.spec, sums, grad_loss, [None] * n, ctx.scores, ctx.boxes[:1, :0], labels=ctx.labels)
        return (None,) * 4 + tuple(d_scores[i] if i < n and ctx.needs_input_grad[4 + i] else None for i in range(len(ctx.scores)))


class SasaLayerLosses(torch.autograd.Function):
    """sums = SasaLayerLosses.apply(spec, labels_list, *scores): the loss against labels the caller holds (PointSASALoss.
    loss_forward).  The layers' losses are sums[4 i]; each passes its own upstream gradient to its scores."""

    @staticmethod
    def forward(ctx, spec, labels_list, *scores):
        n = len(spec.layer_weights)
        scores = [None if s is None else s.detach().contiguous() for s in scores]
        labels = [None if spec.skipped(i, scores) else labels_list[i].detach().contiguous().view(-1) for i in range(n)]
        boxes = next(s for s in scores if s is not None).new_zeros((1, 0, 7))
        sums = forward(spec, [None] * n, scores, boxes, given_labels=labels)
        ctx.spec, ctx.scores, ctx.labels, ctx.boxes = spec, scores, labels, boxes
        ctx.save_for_backward(sums)
        return sums

    @staticmethod
    def backward(ctx, grad_sums):
        sums, = ctx.saved_tensors
        n = len(ctx.spec.layer_weights)
        grad = grad_sums.detach().to(torch.float32).contiguous()
        d_scores = backward(ctx.spec, sums, grad, [None] * n, ctx.scores, ctx.boxes, labels=ctx.labels, grad_stride=4)
        return (None, None) + tuple(d_scores[i] if i < n and ctx.needs_input_grad[2 + i] else None for i in range(len(ctx.scores)))
