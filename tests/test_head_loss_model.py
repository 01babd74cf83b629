"""The CPU model of the head's training loss (tests/models/head_loss.py, float64) against what the reference computed in fp32
(tests/golden/head_loss_ref.npz, written by tests/golden/make_golden_head_loss.py), and its analytic gradient against central
differences of its own forward.

Bounds.  For a float tensor T, err(T) = max|T - T_model| / max|T_model|.  The generator recorded err of the reference's fp32
result for every quantity of every case; the bound of a quantity is 4 x the recorded value (two independent fp32 roundings of
chains of equal length, different libm), floored at 16 * 2^-24 (16 roundings: the longest per-element chain).  The same
function bounds the engine in tests/test_head_loss_gpu.py."""
import os

import numpy as np
import pytest

from tests.models import head_loss as model

HERE = os.path.dirname(os.path.abspath(__file__))
FLOATS = ('total', 'vote_loss_reg', 'point_loss_cls', 'point_loss_box', 'loss_cls', 'loss_box', 'centerness', 'd_vote', 'd_cls',
          'd_reg')


def load():
    return (dict(np.load(os.path.join(HERE, 'golden', 'targets_ref.npz'))),
            dict(np.load(os.path.join(HERE, 'golden', 'head_loss_ref.npz'))))


@pytest.fixture(scope="module")
def data():
    return load()


def case_names():
    return [c['name'] for c in model.fixture_cases(load()[1])]


def bound(fx, case_name, key):
    """4 x the reference's own recorded fp32 error of this quantity in this case, floored at 16 * 2^-24"""
    return max(4.0 * float(fx['%s_err_%s' % (case_name, key)]), model.FLOOR)


def bound_any_case(fx, key):
    """for inputs outside the fixture: the largest bound any fixture case gives this quantity"""
    return max(bound(fx, c['name'], key) for c in model.fixture_cases(fx))


def test_the_fixture_covers_what_it_promises(data):
    targets, fx = data
    cases = model.fixture_cases(fx)
    assert {c['num_class'] for c in cases} == {1, 3} and {c['radius_index'] for c in cases} == {0, 1}
    for key in ('centerness', 'corner', 'ground_aware'):
        assert {c[key] for c in cases} == {True, False}, key
    assert sum(c['background'] for c in cases) == 1 and sum(c['grads'] for c in cases) == 2
    assert any(c['centerness_min'] > 0 and c['centerness_max'] < 1 for c in cases)
    assert os.path.getsize(os.path.join(HERE, 'golden', 'head_loss_ref.npz')) < (1 << 20)
    for c in cases:
        for key in FLOATS:                                   # a recorded error beyond 64 roundings would mean a wrong model
            assert float(fx['%s_err_%s' % (c['name'], key)]) <= 64 * 2.0 ** -24, (c['name'], key)


@pytest.mark.parametrize("name", case_names())
def test_model_against_the_reference_fixture(data, name):
    targets, fx = data
    case = next(c for c in model.fixture_cases(fx) if c['name'] == name)
    inputs, n = model.fixture_inputs(targets, fx, case)
    cfg = model.fixture_config(case)
    out = model.evaluate(inputs, cfg)
    labels = inputs['cls_labels']
    pos = labels > 0
    # counts and zero patterns: exact
    assert out['n_pos'] == int(fx[name + '_n_pos']) == pos.sum()
    assert out['n_valid'] == (labels >= 0).sum() and out['n_vote_pos'] == (inputs['vote_cls_labels'] > 0).sum()
    assert not out['loss_box'][~pos].any() and not out['d_reg'][~pos].any() and not out['d_cls'][labels < 0].any()
    assert not out['centerness'][~pos].any() and not out['loss_cls'][labels < 0].any()
    assert not fx[name + '_loss_box'][~pos].any() and not fx[name + '_centerness'][~pos].any()
    if case['background']:
        assert out['n_pos'] == 0 and out['point_loss_box'] == 0 and out['vote_loss_reg'] == 0
        assert not out['d_reg'].any() and not out['d_vote'].any() and np.isfinite(out['total']) and out['point_loss_cls'] > 0
    else:
        assert pos.mean() >= 0.10 and (labels < 0).mean() >= 0.005
        assert ((out['centerness'][pos] > 0) & (out['centerness'][pos] <= 1)).all()
        if case['corner']:
            assert out['corner_gap'][pos].min() >= 1e-3                   # no corner sits on the min's discontinuity
        top = np.sort(inputs['reg_preds'][:, 6:6 + cfg['angle_bin_num']].astype(np.float64), -1)
        assert (top[:, -1] - top[:, -2]).min() >= 1e-3                    # nor any row on the argmax's
    # every float quantity: within the fp32 bound
    for key in FLOATS:
        if key.startswith('d_') and not case['grads']:
            assert name + '_' + key not in fx
            continue
        e = model.err(fx[name + '_' + key], out[key])
        print("%s %s: err %.3g (recorded %.3g, bound %.3g)" % (name, key, e, float(fx['%s_err_%s' % (name, key)]), bound(fx, name, key)))
        assert e <= bound(fx, name, key), (key, e)
    if case['grads']:
        for key in ('d_vote', 'd_cls', 'd_reg'):
            np.testing.assert_array_equal(fx[name + '_' + key] == 0, out[key] == 0, err_msg=key)


def row_terms(out):
    """what each row adds to the total (the counts are constants)"""
    return (out['loss_vote'] / max(out['n_vote_pos'], 1.0) + out['loss_cls'] / max(out['n_valid'], 1.0)
            + out['loss_box'] / max(out['n_pos'], 1.0))


@pytest.mark.parametrize("name", [n for n in case_names() if n != 'background'])
def test_analytic_gradient_against_central_differences(data, name):
    """200 random coordinates per tensor, each in a row of its own, so that one pair of evaluations serves them all and the
    difference is taken of the ROW's term of the total (1e-3 of the total: its rounding stays far below the tolerance).
    The centerness label carries no gradient and is held at the unperturbed vote coordinates."""
    targets, fx = data
    case = next(c for c in model.fixture_cases(fx) if c['name'] == name)
    inputs, n = model.fixture_inputs(targets, fx, case)
    inputs = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in inputs.items()}
    inputs['centerness_points'] = inputs['vote_preds'].copy()
    cfg = model.fixture_config(case)
    base = model.evaluate(inputs, cfg, upstream=1.0)
    rng = np.random.default_rng(7)
    h = 1e-7
    for key, grad in (('vote_preds', 'd_vote'), ('cls_preds', 'd_cls'), ('reg_preds', 'd_reg')):
        width = inputs[key].shape[1]
        fg = np.nonzero(inputs['cls_labels'] > 0)[0]
        rows = np.concatenate([rng.choice(fg, 150, replace=False), rng.choice(np.setdiff1d(np.arange(n), fg), 50, replace=False)])
        cols = rng.integers(0, width, len(rows))
        step = np.zeros_like(inputs[key])
        step[rows, cols] = h
        hi = model.evaluate(dict(inputs, **{key: inputs[key] + step}), cfg, grad=False)
        lo = model.evaluate(dict(inputs, **{key: inputs[key] - step}), cfg, grad=False)
        numeric = (row_terms(hi) - row_terms(lo))[rows] / (2 * h)
        analytic = base[grad][rows, cols]
        scale = np.abs(base[grad]).max()
        assert scale > 0 and np.abs(analytic).max() > 0.1 * scale
        worst = np.abs(numeric - analytic).max() / scale
        print("%s %s: central differences off by %.3g of the tensor's max" % (name, grad, worst))
        assert worst <= 1e-6, (key, worst)
    # the upstream gradient scales everything
    twice = model.evaluate(inputs, cfg, upstream=2.0)
    for grad in ('d_vote', 'd_cls', 'd_reg'):
        np.testing.assert_allclose(twice[grad], 2.0 * base[grad], rtol=1e-15, atol=0)
