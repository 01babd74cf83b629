"""Tensor wrappers of the training-loss entries of libdet6d_hip_ext.so (include/det6d_ext.h): the loss of PointHeadBox6DVote
and its gradient with respect to the predictions.  Asynchronous on the current stream; nothing here reads a result on the
host (the upstream gradient stays on the device too), so forward and backward can be captured into a graph."""
import ctypes

import torch

from .. import _lib as L

GROUND_AWARE, CENTERNESS, CORNER = 1, 2, 4
NCFG, NSUMS = 16, 16
#: index of each entry of `sums`
TOTAL, VOTE, CLS, BOX, N_VOTE_POS, N_POS, N_PITCH_POS, N_VALID, INV_VOTE, INV_CLS, INV_BOX, PITCH_SCALE = range(12)
WEIGHT_KEYS = ('vote_reg_weight', 'point_cls_weight', 'point_offset_reg_weight', 'point_angle_cls_weight',
               'point_angle_reg_weight', 'point_pitch_cls_weight', 'point_pitch_reg_weight', 'point_corner_weight')


class LossSpec(object):
    """the scalars of one loss configuration, kept as the small HOST array the entry points read (no per-call upload)"""

    def __init__(self, num_class, angle_bin_num, ground_aware=True, centerness=True, corner=True, weights=None, beta=1.0 / 9.0,
                 centerness_min=0.0, centerness_max=1.0):
        weights = weights or {}
        self.num_class, self.angle_bin_num = int(num_class), int(angle_bin_num)
        self.flags = (GROUND_AWARE if ground_aware else 0) | (CENTERNESS if centerness else 0) | (CORNER if corner else 0)
        self.code_size = 6 + 2 * self.angle_bin_num + (2 if ground_aware else 1)
        values = [float(weights.get(k, 0.0 if k == 'point_corner_weight' and not corner else 1.0)) for k in WEIGHT_KEYS]
        values += [float(beta), float(centerness_min), float(centerness_max)]
        self.cfg = (ctypes.c_float * NCFG)(*(values + [0.0] * (NCFG - len(values))))


def _inputs(spec, vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels, reg_preds, reg_labels, box_labels):
    floats = (vote_preds, vote_reg_labels, cls_preds, reg_preds, reg_labels, box_labels)
    L.require_cuda(*floats, vote_cls_labels, cls_labels)
    if any(t.dtype != torch.float32 for t in floats) or vote_cls_labels.dtype != torch.int64 or cls_labels.dtype != torch.int64:
        raise L.Det6dError("the head loss needs float32 predictions and labels and int64 class labels")
    n = vote_preds.shape[0]
    shapes = ((vote_preds, (n, 3)), (vote_reg_labels, (n, 3)), (vote_cls_labels, (n,)), (cls_preds, (n, spec.num_class)),
              (cls_labels, (n,)), (reg_preds, (n, spec.code_size)), (reg_labels, (n, spec.code_size)))
    for t, want in shapes:
        if tuple(t.shape) != want:
            raise L.Det6dError("the head loss got a tensor of shape %s where %s is expected" % (tuple(t.shape), want))
    if box_labels.dim() != 2 or box_labels.shape[0] != n or box_labels.shape[1] < 7:
        raise L.Det6dError("box_labels must be (%d, >= 7), got %s" % (n, tuple(box_labels.shape)))
    return n


def _pointers(tensors):
    return [L.ptr(t) for t in tensors]


def forward(spec, vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels, reg_preds, reg_labels, box_labels,
            per_point=False):
    """-> sums (16,) float32 (the total at TOTAL, the three losses, the counts and the normalisers of the backward) and, with
    per_point=True, the vectors (loss_cls, loss_box, centerness), each (n,)"""
    tensors = (vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels, reg_preds, reg_labels, box_labels)
    n = _inputs(spec, *tensors)
    dev = vote_preds.device
    make = torch.empty if n > 0 else torch.zeros              # every output element is written by the launches: no fill
    sums = make((NSUMS,), dtype=torch.float32, device=dev)
    ws_bytes = L.ext_lib().det6d_ext_head_loss_workspace_bytes(n)
    workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    vectors = tuple(make((n,), dtype=torch.float32, device=dev) for _ in range(3)) if per_point else (None, None, None)
    L.call_ext("det6d_ext_head_loss_forward", n, spec.num_class, spec.angle_bin_num, spec.flags, spec.cfg, *_pointers(tensors),
               box_labels.shape[1], L.ptr(workspace), ws_bytes, L.ptr(sums), *_pointers(vectors), L.stream_ptr())
    return (sums, vectors) if per_point else sums


def backward(spec, sums, grad_loss, vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels, reg_preds, reg_labels,
             box_labels, need=(True, True, True)):
    """grad_loss: one float32 on the device -> (d_vote, d_cls, d_reg), None where need[i] is false"""
    tensors = (vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels, reg_preds, reg_labels, box_labels)
    n = _inputs(spec, *tensors)
    L.require_cuda(sums, grad_loss)
    if sums.dtype != torch.float32 or sums.numel() != NSUMS or grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
        raise L.Det6dError("the head loss backward needs the forward's sums and one float32 upstream gradient on the device")
    if not any(need):
        return None, None, None
    like = (vote_preds, cls_preds, reg_preds)
    grads = tuple(torch.empty_like(t) if wanted else None for t, wanted in zip(like, need))    # every row is written
    L.call_ext("det6d_ext_head_loss_backward", n, spec.num_class, spec.angle_bin_num, spec.flags, spec.cfg, *_pointers(tensors),
               box_labels.shape[1], L.ptr(sums), L.ptr(grad_loss), *_pointers(grads), L.stream_ptr())
    return grads


def centerness_labels(points, box_labels, pos_mask):
    """generate_centerness_label: points (n, 3), box_labels (n, >= 7), pos_mask (n,) bool -> (n,) float32, 0 where the mask is
    false.  The frame is turned about z by the LAST column of box_labels, as in the reference."""
    L.require_cuda(points, box_labels, pos_mask)
    n = points.shape[0]
    if points.dtype != torch.float32 or box_labels.dtype != torch.float32 or pos_mask.dtype != torch.bool:
        raise L.Det6dError("centerness_labels needs float32 points and box labels and a bool mask")
    if tuple(points.shape) != (n, 3) or box_labels.dim() != 2 or box_labels.shape[0] != n or tuple(pos_mask.shape) != (n,):
        raise L.Det6dError("centerness_labels: points (n, 3), box_labels (n, >= 7), pos_mask (n,)")
    out = torch.empty((n,), dtype=torch.float32, device=points.device)
    L.call_ext("det6d_ext_centerness_labels", n, L.ptr(points), L.ptr(box_labels), box_labels.shape[1], L.ptr(pos_mask), L.ptr(out),
               L.stream_ptr())
    return out


def corner_loss(pred_boxes, gt_boxes):
    """get_corner_loss_lidar: (n, >= 7) and (n, >= 7) boxes [x, y, z, dx, dy, dz, rz, ...] -> (n,) float32"""
    L.require_cuda(pred_boxes, gt_boxes)
    if pred_boxes.dtype != torch.float32 or gt_boxes.dtype != torch.float32 or pred_boxes.dim() != 2 or gt_boxes.dim() != 2 \
            or pred_boxes.shape[0] != gt_boxes.shape[0]:
        raise L.Det6dError("corner_loss needs two float32 (n, >= 7) box tensors")
    n = pred_boxes.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=pred_boxes.device)
    L.call_ext("det6d_ext_corner_loss", n, L.ptr(pred_boxes), pred_boxes.shape[1], L.ptr(gt_boxes), gt_boxes.shape[1], L.ptr(out),
               L.stream_ptr())
    return out


class HeadLoss(torch.autograd.Function):
    """loss, sums = HeadLoss.apply(spec, vote_preds, cls_preds, reg_preds, vote_reg_labels, vote_cls_labels, cls_labels,
    reg_labels, box_labels).  loss is a 0-d view of sums; the labels are constants."""

    @staticmethod
    def forward(ctx, spec, vote_preds, cls_preds, reg_preds, vote_reg_labels, vote_cls_labels, cls_labels, reg_labels, box_labels):
        tensors = tuple(t.detach().contiguous() for t in (vote_preds, vote_reg_labels, vote_cls_labels, cls_preds, cls_labels,
                                                          reg_preds, reg_labels, box_labels))
        sums = forward(spec, *tensors)
        ctx.spec = spec
        ctx.save_for_backward(sums, *tensors)
        ctx.mark_non_differentiable(sums)
        return sums[TOTAL], sums

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums):
        sums, *tensors = ctx.saved_tensors
        grad_loss = grad_loss.detach().to(torch.float32).contiguous()
        d_vote, d_cls, d_reg = backward(ctx.spec, sums, grad_loss, *tensors, need=tuple(ctx.needs_input_grad[1:4]))
        return None, d_vote, d_cls, d_reg, None, None, None, None, None
