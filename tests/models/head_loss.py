"""Executable CPU model of det6d_ext_head_loss_forward / _backward (include/det6d_ext.h): the training loss of
PointHeadBox6DVote and its analytic gradient, in NumPy float64, written from the formulas the header states.  It is the truth
the GPU kernels (de6d_amd/csrc/ext/head_loss.hip) are compared against; tests/golden/head_loss_ref.npz holds what the
reference computes in fp32 on the same inputs.

    cfg = config(num_class=1, angle_bin_num=12, ground_aware=True, centerness=True, corner=True, weights={...})
    out = evaluate(inputs, cfg)          # inputs: dict of arrays, see INPUT_KEYS
"""
import json

import numpy as np

INPUT_KEYS = ('vote_preds', 'vote_reg_labels', 'vote_cls_labels', 'cls_preds', 'cls_labels', 'reg_preds', 'reg_labels',
              'box_labels')
WEIGHT_KEYS = ('vote_reg_weight', 'point_cls_weight', 'point_offset_reg_weight', 'point_angle_cls_weight',
               'point_angle_reg_weight', 'point_pitch_cls_weight', 'point_pitch_reg_weight', 'point_corner_weight')
DEFAULT_WEIGHTS = {'vote_reg_weight': 1.0, 'point_cls_weight': 1.0, 'point_offset_reg_weight': 1.0,
                   'point_angle_cls_weight': 0.2, 'point_angle_reg_weight': 1.0, 'point_pitch_cls_weight': 0.2,
                   'point_pitch_reg_weight': 1.0, 'point_corner_weight': 1.0}
FOCAL_ALPHA, FOCAL_GAMMA = 0.25, 2.0
#: corner j of a box = centre + Rz(yaw) (size * TEMPLATE[j])
TEMPLATE = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]],
                    np.float64) / 2
#: the floor of every fp32 bound: 16 roundings of 2^-24 (the longest per-element chain: exp, log1p, pow, sincos, divide)
FLOOR = 16 * 2.0 ** -24


def config(num_class=1, angle_bin_num=12, ground_aware=True, centerness=True, corner=True, weights=None, beta=1.0 / 9.0,
           centerness_min=0.0, centerness_max=1.0):
    w = dict(DEFAULT_WEIGHTS)
    w.update(weights or {})
    return dict(num_class=num_class, angle_bin_num=angle_bin_num, ground_aware=ground_aware, centerness=centerness,
                corner=corner, weights=w, beta=beta, centerness_min=centerness_min, centerness_max=centerness_max)


def code_size(cfg):
    return 6 + 2 * cfg['angle_bin_num'] + (2 if cfg['ground_aware'] else 1)


def smooth_l1(d, beta):
    n = np.abs(d)
    return n if beta < 1e-5 else np.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def smooth_l1_grad(d, beta):
    return np.sign(d) if beta < 1e-5 else np.where(np.abs(d) < beta, d / beta, np.sign(d))


def bce_with_logits(x, t):
    return np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def centerness_label(points, box_labels, pos):
    """generate_centerness_label: the cube root of the product of the min / max face-distance ratios, in the frame turned about
    z by the LAST column of the box labels (for nine-column labels that is rx, not rz: the reference's behaviour, kept)"""
    p, b = points.astype(np.float64), box_labels.astype(np.float64)
    d = p - b[:, :3]
    a = b[:, -1]
    c, s = np.cos(a), np.sin(a)
    loc = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], -1)
    half = b[:, 3:6] / 2
    lo, hi = np.minimum(half - loc, half + loc), np.maximum(half - loc, half + loc)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(pos[:, None], lo / np.where(pos[:, None], hi, 1.0), 0.0)
    return np.where(pos, np.maximum(ratio.prod(-1), 1e-6) ** (1 / 3.0), 0.0)


def corners(centre, size, yaw):
    loc = size[:, None, :] * TEMPLATE[None]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    return np.stack([loc[..., 0] * c - loc[..., 1] * s + centre[:, None, 0], loc[..., 0] * s + loc[..., 1] * c + centre[:, None, 1],
                     loc[..., 2] + centre[:, None, 2]], -1)


def decode7(reg_preds, points, nb):
    """the first seven box columns of PointBinResidual6DCoder.decode: centre, sizes, yaw, and the bin the yaw came from"""
    k = reg_preds[:, 6:6 + nb].argmax(-1)
    res = np.take_along_axis(reg_preds[:, 6 + nb:6 + 2 * nb], k[:, None], -1)[:, 0]
    return reg_preds[:, :3] + points, np.exp(reg_preds[:, 3:6]), (k + res) * (2 * np.pi / nb), k


def corner_term(reg_preds, points, box_labels, nb):
    """-> (loss (n,), d/d centre (n, 3), d/d log-size (n, 3), d/d residual of the decoded bin (n,), the bin)"""
    centre, size, yaw, k = decode7(reg_preds, points, nb)
    pc = corners(centre, size, yaw)
    g = box_labels.astype(np.float64)
    e0 = pc - corners(g[:, :3], g[:, 3:6], g[:, 6])
    e1 = pc - corners(g[:, :3], g[:, 3:6], g[:, 6] + np.pi)
    l0, l1 = smooth_l1(e0, 1.0).sum(-1), smooth_l1(e1, 1.0).sum(-1)
    first = l0 <= l1                                                     # (n, 8): the branch each corner takes
    loss = np.where(first, l0, l1).mean(-1)
    s = smooth_l1_grad(np.where(first[..., None], e0, e1), 1.0) / 8      # d loss / d corner (n, 8, 3)
    c, sn = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    loc = size[:, None, :] * TEMPLATE[None]
    d_loc = np.stack([s[..., 0] * c + s[..., 1] * sn, -s[..., 0] * sn + s[..., 1] * c, s[..., 2]], -1)
    d_yaw = (s[..., 0] * (-loc[..., 0] * sn - loc[..., 1] * c) + s[..., 1] * (loc[..., 0] * c - loc[..., 1] * sn)).sum(-1)
    return loss, s.sum(1), (d_loc * loc).sum(1), d_yaw * (2 * np.pi / nb), k, np.minimum(np.abs(l0 - l1), 1e30)


def evaluate(inputs, cfg, upstream=1.0, grad=True):
    """-> dict: total, vote_loss_reg, point_loss_cls, point_loss_box (normalised as get_loss does), the counts n_vote_pos,
    n_pos, n_pitch_pos, n_valid, the per-point vectors loss_vote, loss_cls, loss_box (total = sum loss_vote / max(n_vote_pos, 1)
    + sum loss_cls / max(n_valid, 1) + sum loss_box / max(n_pos, 1)), centerness, and with grad=True d_vote, d_cls, d_reg
    = upstream * d total / d (vote_preds, cls_preds, reg_preds)"""
    f = {k: np.asarray(inputs[k]) for k in INPUT_KEYS}
    vp, cp, rp = (f[k].astype(np.float64) for k in ('vote_preds', 'cls_preds', 'reg_preds'))
    vl, rl = f['vote_reg_labels'].astype(np.float64), f['reg_labels'].astype(np.float64)
    w, beta, nb, nc = cfg['weights'], cfg['beta'], cfg['angle_bin_num'], cfg['num_class']
    n = len(vp)
    assert cp.shape == (n, nc) and rp.shape == (n, code_size(cfg)) and rl.shape == rp.shape
    vote_pos = f['vote_cls_labels'] > 0
    cls_lab = f['cls_labels'].astype(np.int64)
    pos, valid = cls_lab > 0, cls_lab >= 0
    fg = pos.astype(np.float64)
    n_vote, n_pos, n_valid = float(vote_pos.sum()), float(pos.sum()), float(valid.sum())
    inv_vote, inv_cls, inv_box = 1 / max(n_vote, 1.0), 1 / max(n_valid, 1.0), 1 / max(n_pos, 1.0)

    # vote
    dv = vp - vl
    vote_rows = smooth_l1(dv, beta).sum(-1) * vote_pos
    vote_loss = w['vote_reg_weight'] * vote_rows.sum() * inv_vote

    # classification
    # the centerness label carries no gradient; 'centerness_points' (optional) holds it still while vote_preds is perturbed
    cen = centerness_label(np.asarray(inputs.get('centerness_points', f['vote_preds'])), f['box_labels'], pos)
    target = np.zeros((n, nc))
    rows = np.nonzero(pos)[0]
    target[rows, cls_lab[rows] - 1] = 1.0
    if cfg['centerness']:
        target *= (cfg['centerness_min'] + (cfg['centerness_max'] - cfg['centerness_min']) * cen)[:, None]
    loss_cls = bce_with_logits(cp, target).mean(-1) * valid * w['point_cls_weight']
    cls_loss = loss_cls.sum() * inv_cls

    # box
    off = smooth_l1(rp[:, :6] - rl[:, :6], beta).sum(-1) * fg * w['point_offset_reg_weight']
    lab_bin = rl[:, 6:6 + nb].argmax(-1)
    logits = rp[:, 6:6 + nb]
    mx = logits.max(-1)
    lse = mx + np.log(np.exp(logits - mx[:, None]).sum(-1))
    ang_cls = (lse - np.take_along_axis(logits, lab_bin[:, None], -1)[:, 0]) * fg * w['point_angle_cls_weight']
    d_res = (np.take_along_axis(rp[:, 6 + nb:6 + 2 * nb], lab_bin[:, None], -1)
             - np.take_along_axis(rl[:, 6 + nb:6 + 2 * nb], lab_bin[:, None], -1))[:, 0]
    ang_reg = smooth_l1(d_res, beta) * fg * w['point_angle_reg_weight']
    pc = 6 + 2 * nb
    if cfg['ground_aware']:
        x, t = rp[:, pc], rl[:, pc]
        p = sigmoid(x)
        alpha_w = t * FOCAL_ALPHA + (1 - t) * (1 - FOCAL_ALPHA)
        pt = t * (1 - p) + (1 - t) * p
        bce = bce_with_logits(x, t)
        pitch_cls = alpha_w * pt ** FOCAL_GAMMA * bce * fg * w['point_pitch_cls_weight']
        pitch_w = (t > 0).astype(np.float64)
        d_pitch = rp[:, pc + 1] - rl[:, pc + 1]
    else:
        pitch_cls = np.zeros(n)
        pitch_w = fg
        d_pitch = rp[:, pc] - rl[:, pc]
    n_pitch = float(pitch_w.sum())
    scale = max(n_pos, 1.0) / max(n_pitch, 1.0)
    pitch_reg = smooth_l1(d_pitch, beta) * pitch_w * scale * w['point_pitch_reg_weight']
    loss_box = off + ang_cls + ang_reg + pitch_cls + pitch_reg
    gap = np.full((n, 8), np.inf)
    if cfg['corner']:
        with np.errstate(over='ignore', invalid='ignore'):
            c_loss, c_ctr, c_size, c_res, c_bin, c_gap = corner_term(rp, vp, f['box_labels'], nb)
        loss_box = loss_box + np.where(pos, c_loss * w['point_corner_weight'], 0.0)     # a select: never 0 * inf
        gap = np.where(pos[:, None], c_gap, np.inf)
    box_loss = loss_box.sum() * inv_box

    out = dict(total=vote_loss + cls_loss + box_loss, vote_loss_reg=vote_loss, point_loss_cls=cls_loss, point_loss_box=box_loss,
               n_vote_pos=n_vote, n_pos=n_pos, n_pitch_pos=n_pitch, n_valid=n_valid, loss_vote=w['vote_reg_weight'] * vote_rows, loss_cls=loss_cls, loss_box=loss_box,
               centerness=cen, corner_gap=gap)
    if not grad:
        return out

    g = float(upstream)
    d_vote = g * w['vote_reg_weight'] * inv_vote * smooth_l1_grad(dv, beta) * vote_pos[:, None]
    d_cls = g * w['point_cls_weight'] * inv_cls * (sigmoid(cp) - target) / nc * valid[:, None]
    d_reg = np.zeros_like(rp)
    gb = g * inv_box
    d_reg[:, :6] = gb * w['point_offset_reg_weight'] * fg[:, None] * smooth_l1_grad(rp[:, :6] - rl[:, :6], beta)
    soft = np.exp(logits - lse[:, None])
    soft[np.arange(n), lab_bin] -= 1.0
    d_reg[:, 6:6 + nb] = gb * w['point_angle_cls_weight'] * fg[:, None] * soft
    d_reg[np.arange(n), 6 + nb + lab_bin] = gb * w['point_angle_reg_weight'] * fg * smooth_l1_grad(d_res, beta)
    if cfg['ground_aware']:
        d_focal = alpha_w * (FOCAL_GAMMA * pt ** (FOCAL_GAMMA - 1) * (1 - 2 * t) * p * (1 - p) * bce + pt ** FOCAL_GAMMA * (p - t))
        d_reg[:, pc] = gb * w['point_pitch_cls_weight'] * fg * d_focal
        d_reg[:, pc + 1] = gb * w['point_pitch_reg_weight'] * pitch_w * scale * smooth_l1_grad(d_pitch, beta)
    else:
        d_reg[:, pc] = gb * w['point_pitch_reg_weight'] * pitch_w * scale * smooth_l1_grad(d_pitch, beta)
    if cfg['corner']:
        gc = np.where(pos, gb * w['point_corner_weight'], 0.0)
        sel = lambda a: np.where(pos.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)      # noqa: E731
        d_reg[:, :3] += gc[:, None] * sel(c_ctr)
        d_reg[:, 3:6] += gc[:, None] * sel(c_size)
        d_reg[np.arange(n), 6 + nb + c_bin] += gc * sel(c_res)
        d_vote = d_vote + gc[:, None] * sel(c_ctr)
    out.update(d_vote=d_vote, d_cls=d_cls, d_reg=d_reg)
    return out


def err(value, truth):
    """max |value - truth| / max |truth| (0 when both are all zero)"""
    value, truth = np.asarray(value, np.float64), np.asarray(truth, np.float64)
    scale = np.abs(truth).max() if truth.size else 0.0
    diff = np.abs(value - truth).max() if truth.size else 0.0
    return 0.0 if diff == 0.0 else diff / scale if scale > 0 else np.inf


# ---- the inputs of tests/golden/head_loss_ref.npz -------------------------------------------------------------------
def fixture_cases(fx):
    return json.loads(str(fx['cases']))


def fixture_config(case, angle_bin_num=12):
    return config(num_class=case['num_class'], angle_bin_num=angle_bin_num, ground_aware=case['ground_aware'],
                  centerness=case['centerness'], corner=case['corner'], centerness_min=case['centerness_min'],
                  centerness_max=case['centerness_max'])


def fixture_inputs(targets, fx, case):
    """the arrays of one case: labels from tests/golden/targets_ref.npz (the rows fx['rows']), predictions from the fixture.
    Without ground_aware the code loses its pitch-class column and the pitch label is the box's ry."""
    rows = fx['rows']
    n = len(rows)
    tag = 'mask%d_c' % case['radius_index']
    reg, box = targets[tag + '1_reg'][rows].astype(np.float32), targets[tag + '1_box'][rows].astype(np.float32)
    cls = targets[tag + '%d_cls' % case['num_class']][rows].astype(np.int64)
    vcls, vreg = targets['simple0_cls'][rows].astype(np.int64), targets['simple0_reg'][rows].astype(np.float32)
    preds = fx['reg_preds'].astype(np.float32)
    if not case['ground_aware']:
        reg = np.concatenate([reg[:, :-2], box[:, 7:8]], -1)
        preds = np.concatenate([preds[:, :-2], fx['pitch_preds_plain'][:, None].astype(np.float32)], -1)
    if case['background']:
        reg, box, cls, vcls, vreg = (np.zeros_like(a) for a in (reg, box, cls, vcls, vreg))
    return dict(vote_preds=targets['points'].reshape(-1, 3)[rows].astype(np.float32), vote_reg_labels=vreg, vote_cls_labels=vcls,
                cls_preds=np.ascontiguousarray(fx['cls_preds'][:, :case['num_class']].astype(np.float32)), cls_labels=cls,
                reg_preds=np.ascontiguousarray(preds), reg_labels=np.ascontiguousarray(reg), box_labels=box), n
