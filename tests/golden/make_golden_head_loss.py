"""Regenerates tests/golden/head_loss_ref.npz: what the reference's training loss computes, in fp32, on the points and labels
of tests/golden/targets_ref.npz.

The reference's OWN build_losses, get_loss, get_cls_layer_loss, get_box_layer_loss and generate_centerness_label of its
PointHeadBox6DVote run on CPU torch under the stubs of make_golden.py, with loss.backward() for the gradients: the head is
built without layers, forward_ret_dict is filled by hand (labels from targets_ref.npz, point_box_preds from the reference's own
decode_torch).  Nothing of the reference's text is restated here.  The reference runs in fp32 only (its rotate_points_along_z
casts to float), so the float64 truth is the CPU model tests/models/head_loss.py and this file records the reference's fp32
result plus, for every quantity, err = max|ref - model| / max|model|.  The engine's bound is 4 x that, floored at 16 * 2^-24.

Inputs: every ROW_STEP-th row of targets_ref.npz, labels at radius 1.0 and 2.0; predictions = labels + noise (sigma 0.15), bin
logits 3 * one-hot + 1.5 * noise, random class and pitch logits; the cases of CASES (num_class 1 and 3, centerness on / off /
with a range, corner on / off, ground_aware on / off, one all-background batch).  No row is exempt: rows are resampled until
the top-two bin logits of every row differ by >= MARGIN and the two corner losses of every corner of every foreground row
differ by >= MARGIN, and that is asserted, as is the coverage (foreground >= 10 % of the rows, ignored >= 0.5 %, pitch-positive
and pitch-negative each >= 5 % of the foreground, each smooth-L1 branch >= 10 % of the foreground elements).

    python tests/golden/make_golden_head_loss.py            (authoring container only: needs the reference checkout)
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.models import head_loss as model  # noqa: E402

F32 = np.float32
ROW_STEP = 8
MARGIN = 1e-3
SIGMA = 0.15
CODER = dict(angle_bin_num=12, use_mean_size=False, minus=False, threshold=10, factor=45)


def case(name, radius_index, num_class, centerness, corner, ground_aware, cmin=0.0, cmax=1.0, background=False, grads=False):
    return dict(name=name, radius_index=radius_index, num_class=num_class, centerness=centerness, corner=corner,
                ground_aware=ground_aware, centerness_min=cmin, centerness_max=cmax, background=background, grads=grads)


CASES = [case('r2_c1_full', 1, 1, True, True, True, grads=True),
         case('r1_c3_full', 0, 3, True, True, True, grads=True),
         case('r2_c3_plain', 1, 3, False, False, True),
         case('r1_c1_corner_flat', 0, 1, False, True, False),
         case('r2_c1_centerness_flat', 1, 1, True, False, False),
         case('r1_c3_flat', 0, 3, False, False, False),
         case('r2_c3_range', 1, 3, True, True, True, cmin=0.2, cmax=0.9),
         case('background', 1, 1, True, True, True, background=True)]


def reference():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    easydict = mg.install_reference_stubs()
    sys.path.insert(0, mg.REF)
    from pcdet.models.dense_heads.point_head_box6d_vote import PointHeadBox6DVote as RefHead
    from pcdet.utils import box_coder_utils as ref_coders
    assert ref_coders.__file__.startswith(mg.REF)
    return sys.modules['easydict'].EasyDict, RefHead, ref_coders


def ref_head(EasyDict, RefHead, ref_coders, c):
    """the reference head without its layers: only what its loss methods read"""
    head = RefHead.__new__(RefHead)
    torch.nn.Module.__init__(head)
    head.num_class = c['num_class']
    head.box_coder = ref_coders.PointBinResidual6DCoder(ground_aware=c['ground_aware'], **CODER)
    loss_cfg = dict(LOSS_CLS='WeightedBinaryCrossEntropyLoss' + ('WithCenterness' if c['centerness'] else ''),
                    LOSS_REG='WeightedSmoothL1Loss', LOSS_WEIGHTS=dict(model.DEFAULT_WEIGHTS),
                    CORNER_LOSS_REGULARIZATION=c['corner'],
                    LOSS_CLS_CONFIG=dict(centerness_min=c['centerness_min'], centerness_max=c['centerness_max']))
    head.model_cfg = EasyDict(LOSS_CONFIG=loss_cfg)
    head.build_losses(head.model_cfg.LOSS_CONFIG)
    return head


def run_reference(head, inputs):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inputs.items()}
    for k in ('vote_preds', 'cls_preds', 'reg_preds'):
        t[k].requires_grad_(True)
    head.forward_ret_dict = {
        'point_vote_coords': t['vote_preds'], 'vote_cls_labels': t['vote_cls_labels'], 'vote_reg_labels': t['vote_reg_labels'],
        'point_cls_preds': t['cls_preds'], 'point_reg_preds': t['reg_preds'], 'point_cls_labels': t['cls_labels'],
        'point_reg_labels': t['reg_labels'], 'point_box_labels': t['box_labels'],
        'point_box_preds': head.box_coder.decode_torch(t['reg_preds'], t['vote_preds'])}
    loss, tb = head.get_loss()
    loss.backward()
    with torch.no_grad():
        loss_cls = head.get_cls_layer_loss()[0]
        loss_box = head.get_box_layer_loss()[0]
        cen = head.generate_centerness_label(t['vote_preds'], t['box_labels'], t['cls_labels'] > 0)
    out = dict(total=loss.item(), vote_loss_reg=tb['vote_loss_reg'], point_loss_cls=tb['point_loss_cls'],
               point_loss_box=tb['point_loss_box'], n_pos=tb['point_pos_num'], loss_cls=loss_cls.numpy(), loss_box=loss_box.numpy(),
               centerness=cen.numpy(), d_vote=t['vote_preds'].grad.numpy(), d_cls=t['cls_preds'].grad.numpy(),
               d_reg=t['reg_preds'].grad.numpy())
    assert abs(tb['point_loss_vote'] - tb['vote_loss_reg']) == 0
    return out


def draw(rng, reg, box):
    """predictions around the labels of the rows `reg` / `box` (radius 2.0: the largest foreground set)"""
    n, nb = len(reg), CODER['angle_bin_num']
    preds = (reg + SIGMA * rng.standard_normal(reg.shape)).astype(F32)
    preds[:, 6:6 + nb] = (3.0 * reg[:, 6:6 + nb] + 1.5 * rng.standard_normal((n, nb))).astype(F32)
    preds[:, 6 + 2 * nb] = (2.0 * rng.standard_normal(n)).astype(F32)
    plain = (box[:, 7] + SIGMA * rng.standard_normal(n)).astype(F32)
    cls = (2.0 * rng.standard_normal((n, 3))).astype(F32)
    return preds, plain, cls


def main():
    EasyDict, RefHead, ref_coders = reference()
    targets = dict(np.load(os.path.join(HERE, 'targets_ref.npz')))
    total = targets['points'].shape[0] * targets['points'].shape[1]
    rows = np.arange(0, total, ROW_STEP)
    n, nb = len(rows), CODER['angle_bin_num']
    rng = np.random.default_rng(20261017)
    reg, box = targets['mask1_c1_reg'][rows], targets['mask1_c1_box'][rows]
    preds, plain, cls = draw(rng, reg, box)
    fx = {'rows': rows, 'reg_preds': preds, 'pitch_preds_plain': plain, 'cls_preds': cls,
          'cases': np.array(json.dumps(CASES))}
    probe = next(c for c in CASES if c['radius_index'] == 1 and c['corner'] and not c['background'])

    def margins():
        top = np.sort(fx['reg_preds'][:, 6:6 + nb].astype(np.float64), -1)
        inputs, _ = model.fixture_inputs(targets, fx, probe)
        gap = model.evaluate(inputs, model.fixture_config(probe), grad=False)['corner_gap'].min(-1)
        return (top[:, -1] - top[:, -2] < MARGIN) | (gap < MARGIN)
    for _ in range(100):                                     # resample the rows that sit near a discontinuity
        bad = margins()
        if not bad.any():
            break
        p2, q2, _ = draw(rng, reg, box)
        fx['reg_preds'][bad], fx['pitch_preds_plain'][bad] = p2[bad], q2[bad]
        print("resampled %d rows" % bad.sum())
    assert not margins().any()

    errs = {}
    for c in CASES:
        inputs, _ = model.fixture_inputs(targets, fx, c)
        cfg = model.fixture_config(c)
        want = model.evaluate(inputs, cfg)
        got = run_reference(ref_head(EasyDict, RefHead, ref_coders, c), inputs)
        pos = inputs['cls_labels'] > 0
        assert got['n_pos'] == want['n_pos'] == pos.sum()
        if not c['background']:                              # coverage
            assert pos.mean() >= 0.10 and (inputs['cls_labels'] < 0).mean() >= 0.005, (pos.mean(), (inputs['cls_labels'] < 0).mean())
            pitch = box_pitch = inputs['reg_labels'][pos, 6 + 2 * nb] > 0 if c['ground_aware'] else None
            if pitch is not None:
                assert 0.05 <= box_pitch.mean() <= 0.95, pitch.mean()
            small = np.abs(inputs['reg_preds'][pos, :6].astype(np.float64) - inputs['reg_labels'][pos, :6]) < cfg['beta']
            assert 0.10 <= small.mean() <= 0.90, small.mean()
            if c['corner']:
                assert want['corner_gap'][pos].min() >= MARGIN
        else:
            assert pos.sum() == 0 and got['point_loss_box'] == 0 and not got['d_reg'].any() and not got['d_vote'].any()
        assert np.isfinite(got['total']) and all(np.isfinite(got[k]).all() for k in ('d_vote', 'd_cls', 'd_reg'))
        # zero patterns the tests rely on
        assert not got['loss_box'][~pos].any() and not got['d_reg'][~pos].any() and not got['d_cls'][inputs['cls_labels'] < 0].any()
        assert not want['loss_box'][~pos].any() and not want['d_reg'][~pos].any()
        for k in ('total', 'vote_loss_reg', 'point_loss_cls', 'point_loss_box', 'loss_cls', 'loss_box', 'centerness', 'd_vote',
                  'd_cls', 'd_reg'):
            e = model.err(got[k], want[k])
            errs[c['name'] + '/' + k] = e
            fx['%s_err_%s' % (c['name'], k)] = np.float64(e)
            if k.startswith('d_') and not c['grads']:
                continue
            fx['%s_%s' % (c['name'], k)] = np.asarray(got[k], F32)
        fx[c['name'] + '_n_pos'] = np.int64(got['n_pos'])
        print("%-22s loss %.6f (vote %.6f cls %.6f box %.6f) foreground %d ignored %d" % (
            c['name'], got['total'], got['vote_loss_reg'], got['point_loss_cls'], got['point_loss_box'], pos.sum(),
            (inputs['cls_labels'] < 0).sum()))
    print("err of the reference's fp32 result against the float64 model (max|ref - model| / max|model|):")
    for k in ('total', 'vote_loss_reg', 'point_loss_cls', 'point_loss_box', 'loss_cls', 'loss_box', 'centerness', 'd_vote', 'd_cls',
              'd_reg'):
        vals = [errs[c['name'] + '/' + k] for c in CASES]
        print("  %-15s max %.3g   (%s)" % (k, max(vals), ' '.join('%.2g' % v for v in vals)))
    path = os.path.join(HERE, 'head_loss_ref.npz')
    np.savez_compressed(path, **fx)
    print("head_loss_ref.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
