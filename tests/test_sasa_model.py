"""The CPU model of the SASA loss (tests/models/sasa.py, float64) against what the reference's PointSASALoss computed in fp32
(tests/golden/sasa_ref.npz, written by tests/golden/make_golden_sasa.py), and its analytic gradient against central differences
of its own forward.

Bounds, as for the head loss (tests/test_head_loss_model.py).  For a float tensor T, err(T) = max|T - T_model| / max|T_model|.
The generator recorded err of the reference's fp32 result for every quantity of every case; the bound of a quantity is 4 x the
recorded value (two independent fp32 roundings of chains of equal length, different libm), floored at 16 * 2^-24.  The same
function bounds the engine in tests/test_sasa_gpu.py.  Labels and counts are exact: every fixture point keeps >= 1e-3 from
every decision face."""
import os

import numpy as np
import pytest

from tests.models import sasa as model

HERE = os.path.dirname(os.path.abspath(__file__))
EXTRA = [0.2, 0.2, 0.2]


def load():
    return dict(np.load(os.path.join(HERE, 'golden', 'sasa_ref.npz')))


@pytest.fixture(scope="module")
def fx():
    return load()


def case_names():
    return [c['name'] for c in model.fixture_cases(load())]


def case_of(fx, name):
    return next(c for c in model.fixture_cases(fx) if c['name'] == name)


def bound(fx, case_name, key):
    """4 x the reference's own recorded fp32 error of this quantity in this case, floored at 16 * 2^-24"""
    return max(4.0 * float(fx['%s_err_%s' % (case_name, key)]), model.FLOOR)


def bound_any_case(fx, key):
    """for inputs outside the fixture: the largest bound any fixture case gives a quantity of this kind (loss, d_scores, total)"""
    return max([model.FLOOR] + [4.0 * float(v) for k, v in fx.items() if '_err_' + key in k])


def model_labels(fx, case):
    coords, scores, gt_boxes = model.fixture_inputs(fx, case)
    return [None if (s is None or w == 0) else model.assign(xyz, gt_boxes, case['extra_width'], case['set_ignore_flag'])
            for xyz, s, w in zip(coords, scores, case['layer_weights'])]


def test_the_fixture_covers_what_it_promises(fx):
    cases = model.fixture_cases(fx)
    assert {c['func'] for c in cases} == {'BCE', 'Focal'} and {c['set_ignore_flag'] for c in cases} == {True, False}
    assert any(c['extra_width'] is None for c in cases) and any(c['extra_width'] == EXTRA and not c['set_ignore_flag'] for c in cases)
    assert {c['points'] for c in cases} == {'main', 'background', 'shell'}
    assert any(c['no_scores'] for c in cases) and any(0 in c['layer_weights'] for c in cases)     # both ways of skipping a layer
    assert os.path.getsize(os.path.join(HERE, 'golden', 'sasa_ref.npz')) < (1 << 20)
    for name in ('main', 'background', 'shell'):
        boxes = fx[name + '_gt_boxes']
        assert boxes.shape[2] == 10 and np.abs(boxes[:, :, 7:9]).max() > 0.05           # sloped: pitch and roll are set
        for i in range(3):
            xyz = fx['%s_coords_%d' % (name, i)]
            assert xyz.shape[0] == boxes.shape[0] and xyz.shape[0] * xyz.shape[1] >= 64
            for k in range(len(boxes)):                      # no row is exempt
                assert model.face_distance(xyz[k], boxes[k], EXTRA).min() >= 1e-3
    assert not fx['main_gt_boxes'][:, -1].any()              # a padding row
    for key, value in fx.items():                            # a recorded error beyond 64 roundings would mean a wrong model
        if '_err_' in key:
            assert float(value) <= 64 * 2.0 ** -24, key


@pytest.mark.parametrize("name", case_names())
def test_model_against_the_reference_fixture(fx, name):
    case = case_of(fx, name)
    coords, scores, gt_boxes = model.fixture_inputs(fx, case)
    labels = model_labels(fx, case)
    out = model.loss(scores, labels, case['layer_weights'], case['func'])
    for i, lab in enumerate(labels):
        skipped = i in case['no_scores'] or case['layer_weights'][i] == 0
        assert (lab is None) == skipped == (out['losses'][i] is None) == ('%s_labels_%d' % (name, i) not in fx)
        if skipped:
            assert not out['sums'][4 * i:4 * i + 4].any()
            continue
        np.testing.assert_array_equal(lab, fx['%s_labels_%d' % (name, i)])                # labels: exact
        frac = [np.mean(lab == v) for v in (1, -1, 0)]
        if case['points'] == 'main':
            assert frac[0] >= 0.10 and frac[2] >= 0.10 and (frac[1] >= 0.02 if case['set_ignore_flag'] else frac[1] == 0)
        elif case['points'] == 'background':
            assert frac[2] == 1.0
        elif i == 1:                                                                   # the all-ignored layer: the normaliser clamps
            assert frac[1] == 1.0 and out['losses'][i] == 0 and out['sums'][4 * i + 1] == 0
        assert tuple(out['sums'][4 * i + 1:4 * i + 4]) == ((lab >= 0).sum(), (lab > 0).sum(), (lab < 0).sum())
        assert not out['d_scores'][i].reshape(-1)[lab < 0].any() and not fx['%s_d_scores_%d' % (name, i)].reshape(-1)[lab < 0].any()
        for key, value in (('loss_%d' % i, out['losses'][i]), ('d_scores_%d' % i, out['d_scores'][i])):
            e = model.err(fx['%s_%s' % (name, key)], value)
            print("%s %s: err %.3g (bound %.3g)" % (name, key, e, bound(fx, name, key)))
            assert e <= bound(fx, name, key), (key, e)
    assert model.err(fx[name + '_total'], out['total']) <= bound(fx, name, 'total')


def test_first_box_wins_and_the_margin(fx):
    boxes = np.zeros((3, 7))
    boxes[:, 3:6] = [4, 2, 2]
    boxes[1, 0] = 1.0                                        # overlaps box 0
    boxes[2, 0] = 50.0
    pts = np.array([[0.5, 0, 0], [2.5, 0, 0], [50, 0.5, 0.9], [50, 0, 1.0 + 1e-9], [50, 1.0 + 5e-6, 0], [50, 1.0 + 2e-5, 0], [9, 9, 9]])
    np.testing.assert_array_equal(model.points_in_boxes7_scene(pts, boxes), [0, 1, 2, -1, 2, -1, -1])
    # a zero-sized box holds the points within the margin of its centre line; NaN is outside
    zero = np.zeros((1, 7))
    np.testing.assert_array_equal(model.points_in_boxes7_scene(np.array([[0, 0, 0], [5e-6, 0, 0], [0, 0, 1e-9], [np.nan, 0, 0]]), zero),
                                  [0, 0, -1, -1])
    # a padding row enlarged by extra_width is a small box at the origin
    np.testing.assert_array_equal(model.assign(np.array([[[0.05, 0.05, 0.05], [0.2, 0, 0]]]), np.zeros((1, 1, 10)), EXTRA, True), [-1, 0])


@pytest.mark.parametrize("name", ['bce_ignore', 'focal_ignore', 'focal_plain'])
def test_analytic_gradient_against_central_differences(fx, name):
    case = case_of(fx, name)
    _, scores, _ = model.fixture_inputs(fx, case)
    scores = [None if s is None else s.astype(np.float64) for s in scores]
    labels = model_labels(fx, case)
    base = model.loss(scores, labels, case['layer_weights'], case['func'])
    h = 1e-6
    for i, s in enumerate(scores):
        if s is None or labels[i] is None:
            continue
        # every point adds its own term to the layer's sum (the counts are constants): one pair of evaluations serves all rows
        terms = lambda x: case['layer_weights'][i] * np.where(labels[i] >= 0, model.point_loss(      # noqa: E731
            x.reshape(-1), (labels[i] > 0).astype(np.float64), case['func'])[0], 0.0) / max((labels[i] >= 0).sum(), 1)
        numeric = (terms(s + h) - terms(s - h)) / (2 * h)
        scale = np.abs(base['d_scores'][i]).max()
        worst = np.abs(numeric - base['d_scores'][i].reshape(-1)).max() / scale
        print("%s layer %d: central differences off by %.3g of the tensor's max" % (name, i, worst))
        assert scale > 0 and worst <= 1e-7, (i, worst)
    twice = model.loss(scores, labels, case['layer_weights'], case['func'], upstream=0.5)
    for a, b in zip(twice['d_scores'], base['d_scores']):
        if b is not None:
            np.testing.assert_allclose(a, 0.5 * b, rtol=1e-15, atol=0)
