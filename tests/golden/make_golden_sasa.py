"""Regenerates tests/golden/sasa_ref.npz: what the reference's PointSASALoss computes, in fp32, on a few hundred points per
layer drawn around a handful of sloped boxes.

The reference's OWN PointSASALoss runs on CPU torch under the stubs of make_golden.py:
  * loss_forward with loss.backward(), for BCE and Focal;
  * assign_target — its own enlarge_box3d, per-scene loop and ignore logic — with the one thing that cannot run here, the
    compiled points_in_boxes_gpu behind roiaware_pool3d_utils, answered by the float64 model (tests/models/sasa.py).
Nothing of the reference's text is restated here.  The float64 truth is the model; this file records the reference's fp32
result and, for every quantity, err = max|ref - model| / max|model|.  The engine's bound is 4 x that, floored at 16 * 2^-24.

Inputs: three point sets of two scenes and three layers each.  `main`: six sloped boxes and one all-zero padding row per scene,
35 % of the points drawn inside a box, 15 % in the shell between a box and the box enlarged by 0.2, 50 % anywhere.  `shell`:
two boxes far apart, the middle layer entirely in the shell (all ignored: the normaliser clamps at 1).  `background`: the points
of `main`, the boxes moved away.  No row is exempt from the label comparison: points are resampled until face_distance >= 1e-3
for EVERY point (ten times the project's stated rounding band of 1e-4), and that is asserted, as is the coverage (foreground
>= 10 %, ignored >= 2 %, background >= 10 % of each layer of `main`).

    python tests/golden/make_golden_sasa.py            (authoring container only: needs the reference checkout)
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.models import sasa as model  # noqa: E402

F32 = np.float32
FACE = 1e-3
EXTRA = [0.2, 0.2, 0.2]
WEIGHTS = [0.01, 0.1, 1.0]


def case(name, func, ignore, extra, points='main', layer_weights=None, no_scores=()):
    return dict(name=name, func=func, set_ignore_flag=ignore, extra_width=extra, points=points,
                layer_weights=layer_weights or WEIGHTS, no_scores=list(no_scores))


CASES = [case('bce_ignore', 'BCE', True, EXTRA),
         case('focal_ignore', 'Focal', True, EXTRA, no_scores=[1]),
         case('bce_extra', 'BCE', False, EXTRA, layer_weights=[0.01, 0.0, 1.0]),
         case('focal_plain', 'Focal', False, None),
         case('bce_plain', 'BCE', False, None, no_scores=[0]),
         case('background', 'BCE', True, EXTRA, points='background'),
         case('all_ignored', 'BCE', True, EXTRA, points='shell')]


def reference():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.install_reference_stubs()
    sys.path.insert(0, mg.REF)
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_cuda
    from pcdet.utils import loss_utils as ref_loss
    assert ref_loss.__file__.startswith(mg.REF)

    def points_in_boxes_gpu(boxes, points, out):             # the compiled op's signature; the reference's wrapper calls it
        for k in range(boxes.shape[0]):
            out[k] = torch.from_numpy(model.points_in_boxes7_scene(points[k].numpy(), boxes[k].numpy()))
    roiaware_pool3d_cuda.points_in_boxes_gpu = points_in_boxes_gpu
    return ref_loss.PointSASALoss


def sloped_boxes(rng, centres):
    m = len(centres)
    box = np.zeros((m, 10), F32)
    box[:, :3] = centres
    box[:, 3], box[:, 4], box[:, 5] = rng.uniform(3.5, 4.5, m), rng.uniform(1.5, 2.0, m), rng.uniform(1.4, 1.8, m)
    box[:, 6], box[:, 7], box[:, 8] = rng.uniform(-np.pi, np.pi, m), rng.uniform(-0.15, 0.15, m), rng.uniform(-0.15, 0.15, m)
    box[:, 9] = 1
    return box


def draw(rng, boxes, kind):
    """one point: 0 inside a box, 1 in the shell between a box and the enlarged box, 2 anywhere"""
    if kind == 2:
        return np.array([rng.uniform(0, 48), rng.uniform(-16, 16), rng.uniform(-3, 3)])
    real = boxes[boxes[:, 3] > 0]
    b = real[rng.integers(len(real))].astype(np.float64)
    if kind == 0:
        loc = rng.uniform(-0.49, 0.49, 3) * b[3:6]
    else:
        loc = rng.uniform(-0.5, 0.5, 3) * (b[3:6] + 0.2)
        axis = rng.integers(3)
        loc[axis] = rng.choice([-1, 1]) * (b[3 + axis] / 2 + rng.uniform(0.005, 0.095))
    c, s = np.cos(b[6]), np.sin(b[6])
    return np.array([b[0] + loc[0] * c - loc[1] * s, b[1] + loc[0] * s + loc[1] * c, b[2] + loc[2]])


def point_set(rng, gt_boxes, sizes, kinds_of):
    """-> coords per layer (b, m_i, 3) fp32, every point >= FACE from every decision face (of the fp32 values stored)"""
    coords = []
    for li, m in enumerate(sizes):
        layer = np.zeros((len(gt_boxes), m, 3), F32)
        for k, boxes in enumerate(gt_boxes):
            kinds = kinds_of(li, m, rng)
            for j in range(m):
                for _ in range(1000):
                    p = draw(rng, boxes, kinds[j]).astype(F32)
                    if model.face_distance(p[None].astype(np.float64), boxes, EXTRA)[0] >= FACE:
                        break
                else:
                    raise AssertionError("no point found")
                layer[k, j] = p
        coords.append(layer)
    return coords


def mixed(li, m, rng):
    return rng.choice(3, m, p=[0.35, 0.15, 0.5])


def run_reference(RefLoss, c, coords, scores, gt_boxes):
    loss_mod = RefLoss(func=c['func'], layer_weights=c['layer_weights'], extra_width=c['extra_width'],
                       set_ignore_flag=c['set_ignore_flag'])
    b = gt_boxes.shape[0]
    l_points = []
    for xyz in coords:
        bs = np.repeat(np.arange(b, dtype=F32), xyz.shape[1])[:, None]
        l_points.append(torch.from_numpy(np.concatenate([bs, xyz.reshape(-1, 3)], 1)))
    l_scores = [None if s is None else torch.from_numpy(s.copy()).requires_grad_(True) for s in scores]
    l_labels = loss_mod(l_points, l_scores, torch.from_numpy(gt_boxes))
    l_loss = loss_mod.loss_forward(l_scores, l_labels)
    live = [v for v in l_loss if v is not None]
    total = sum(live) if live else torch.zeros(())
    if live:
        total.backward()
    return dict(labels=[None if v is None else v.numpy() for v in l_labels],
                losses=[None if v is None else float(v.detach()) for v in l_loss], total=float(total.detach()),
                d_scores=[None if (s is None or v is None) else s.grad.numpy() for s, v in zip(l_scores, l_loss)])


def main():
    RefLoss = reference()
    rng = np.random.default_rng(20261019)
    fx = {'cases': np.array(json.dumps(CASES))}
    sets = {}
    centres = lambda: np.stack([rng.uniform(8, 40, 6), rng.uniform(-12, 12, 6), rng.uniform(-1.0, 0.5, 6)], 1)   # noqa: E731
    main_boxes = np.stack([np.concatenate([sloped_boxes(rng, centres()), np.zeros((1, 10), F32)]) for _ in range(2)])
    main_coords = point_set(rng, main_boxes, [192, 96, 48], mixed)
    sets['main'] = (main_coords, main_boxes)
    away = main_boxes.copy()
    away[:, :6, 0] += 200
    sets['background'] = (main_coords, away)
    shell_boxes = np.stack([sloped_boxes(rng, np.array([[10.0, -4, 0], [30.0, 5, -0.5]])) for _ in range(2)])
    sets['shell'] = (point_set(rng, shell_boxes, [64, 48, 32], lambda li, m, r: np.ones(m, int) if li == 1 else mixed(li, m, r)),
                     shell_boxes)
    for name, (coords, boxes) in sets.items():
        fx[name + '_gt_boxes'] = boxes
        for i, xyz in enumerate(coords):
            fx['%s_coords_%d' % (name, i)] = xyz
            fx['%s_scores_%d' % (name, i)] = (2.0 * rng.standard_normal((xyz.shape[0] * xyz.shape[1], 1))).astype(F32)
            for k in range(len(boxes)):                      # every point, no row exempt
                assert model.face_distance(xyz[k], boxes[k], EXTRA).min() >= FACE

    errs = {}
    for c in CASES:
        coords, scores, gt_boxes = model.fixture_inputs(fx, c)
        got = run_reference(RefLoss, c, coords, scores, gt_boxes)
        labels = [None if (s is None or w == 0) else model.assign(xyz, gt_boxes, c['extra_width'], c['set_ignore_flag'])
                  for xyz, s, w in zip(coords, scores, c['layer_weights'])]
        want = model.loss(scores, labels, c['layer_weights'], c['func'])
        for i, lab in enumerate(labels):
            assert (lab is None) == (got['labels'][i] is None) == (want['losses'][i] is None), (c['name'], i)
            if lab is None:
                continue
            np.testing.assert_array_equal(got['labels'][i], lab)
            frac = [np.mean(lab == v) for v in (1, -1, 0)]
            if c['points'] == 'main':                        # coverage
                assert frac[0] >= 0.10 and frac[2] >= 0.10 and (frac[1] >= 0.02 or not c['set_ignore_flag']), (c['name'], i, frac)
                assert c['set_ignore_flag'] or frac[1] == 0
            if c['points'] == 'background':
                assert frac[2] == 1.0
            if c['points'] == 'shell' and i == 1:
                assert frac[1] == 1.0 and got['losses'][i] == 0 and not got['d_scores'][i].any()
            assert not got['d_scores'][i][lab < 0].any() and not want['d_scores'][i].reshape(-1)[lab < 0].any()
            fx['%s_labels_%d' % (c['name'], i)] = lab.astype(np.int64)
            for key, ref_v, model_v in (('loss_%d' % i, got['losses'][i], want['losses'][i]),
                                        ('d_scores_%d' % i, got['d_scores'][i], want['d_scores'][i])):
                errs[c['name'] + '/' + key] = e = model.err(ref_v, model_v)
                fx['%s_err_%s' % (c['name'], key)] = np.float64(e)
                fx['%s_%s' % (c['name'], key)] = np.asarray(ref_v, F32)
        errs[c['name'] + '/total'] = e = model.err(got['total'], want['total'])
        fx[c['name'] + '_err_total'], fx[c['name'] + '_total'] = np.float64(e), F32(got['total'])
        assert np.isfinite(got['total'])
        print("%-14s total %.6f  layers %s  labels (fg, ignored, bg) %s" % (
            c['name'], got['total'], ['-' if v is None else '%.6f' % v for v in got['losses']],
            ['-' if lab is None else tuple(int((lab == v).sum()) for v in (1, -1, 0)) for lab in labels]))
    print("err of the reference's fp32 result against the float64 model (max|ref - model| / max|model|): max %.3g" % max(errs.values()))
    for k, v in sorted(errs.items()):
        print("  %-28s %.3g" % (k, v))
    path = os.path.join(HERE, 'sasa_ref.npz')
    np.savez_compressed(path, **fx)
    print("sasa_ref.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
