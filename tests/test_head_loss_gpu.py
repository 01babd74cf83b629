"""The head's training loss on the GPU (de6d_amd/csrc/ext/head_loss.hip and the layers above it) against the float64 CPU model
(tests/models/head_loss.py): forward scalars, per-point vectors, centerness and the three gradients on every fixture case and
on a large random case; exact counts; bit-identical repeats; a captured graph; the head and the detector on the tiny model.
The bounds are those of tests/test_head_loss_model.py: 4 x the reference's own recorded fp32 error, floored at 16 * 2^-24."""
import os

import numpy as np
import pytest
import torch

from tests.models import head_loss as model
from tests.test_head_loss_model import bound, bound_any_case, case_names, load

pytestmark = pytest.mark.gpu

F32 = np.float32
SCALARS = (('total', 0), ('vote_loss_reg', 1), ('point_loss_cls', 2), ('point_loss_box', 3))
COUNTS = (('n_vote_pos', 4), ('n_pos', 5), ('n_pitch_pos', 6), ('n_valid', 7))
ORDER = ('vote_preds', 'vote_reg_labels', 'vote_cls_labels', 'cls_preds', 'cls_labels', 'reg_preds', 'reg_labels', 'box_labels')


@pytest.fixture(scope="module")
def data():
    return load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spec_of(cfg):
    from de6d_amd.ops import head_loss
    return head_loss.LossSpec(cfg['num_class'], cfg['angle_bin_num'], ground_aware=cfg['ground_aware'], centerness=cfg['centerness'],
                              corner=cfg['corner'], weights=cfg['weights'], beta=cfg['beta'], centerness_min=cfg['centerness_min'],
                              centerness_max=cfg['centerness_max'])


def run_gpu(inputs, cfg, upstream=1.0):
    """forward with the per-point vectors and backward -> dict of NumPy arrays under the model's keys, plus the raw sums"""
    from de6d_amd.ops import head_loss
    spec = spec_of(cfg)
    t = [dev(inputs[k]) for k in ORDER]
    sums, (loss_cls, loss_box, cen) = head_loss.forward(spec, *t, per_point=True)
    plain = head_loss.forward(spec, *t)
    g = torch.tensor(upstream, dtype=torch.float32, device='cuda')
    d_vote, d_cls, d_reg = head_loss.backward(spec, sums, g, *t)
    torch.cuda.synchronize()
    assert torch.equal(plain, sums)                                       # the per-point outputs change nothing
    s = sums.cpu().numpy()
    out = {k: float(s[i]) for k, i in SCALARS + COUNTS}
    out.update(loss_cls=loss_cls.cpu().numpy(), loss_box=loss_box.cpu().numpy(), centerness=cen.cpu().numpy(),
               d_vote=d_vote.cpu().numpy(), d_cls=d_cls.cpu().numpy(), d_reg=d_reg.cpu().numpy(), sums=s)
    return out


def compare(got, want, inputs, limit, tag):
    labels = inputs['cls_labels']
    pos = labels > 0
    for k, _ in COUNTS:                                                   # counts: exact
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in ('loss_cls', 'loss_box', 'centerness', 'd_vote', 'd_cls', 'd_reg'):
        assert got[k].dtype == F32 and got[k].shape == want[k].shape and np.isfinite(got[k]).all(), (tag, k)
    assert not got['loss_box'][~pos].any() and not got['d_reg'][~pos].any() and not got['centerness'][~pos].any(), tag
    assert not got['d_cls'][labels < 0].any() and not got['loss_cls'][labels < 0].any(), tag
    assert not got['d_vote'][(inputs['vote_cls_labels'] <= 0) & ~pos].any(), tag
    for k in ('total', 'vote_loss_reg', 'point_loss_cls', 'point_loss_box', 'loss_cls', 'loss_box', 'centerness', 'd_vote', 'd_cls',
              'd_reg'):
        e = model.err(got[k], want[k])
        print("%s %s: err %.3g (bound %.3g)" % (tag, k, e, limit(k)))
        assert e <= limit(k), (tag, k, e, limit(k))


@pytest.mark.parametrize("name", case_names())
def test_every_fixture_case_against_the_model(data, name):
    targets, fx = data
    case = next(c for c in model.fixture_cases(fx) if c['name'] == name)
    inputs, n = model.fixture_inputs(targets, fx, case)
    cfg = model.fixture_config(case)
    want = model.evaluate(inputs, cfg, upstream=1.0)
    got = run_gpu(inputs, cfg)
    compare(got, want, inputs, lambda k: bound(fx, name, k), name)
    assert got['n_pos'] == int(fx[name + '_n_pos'])
    if case['background']:                                                # no foreground: finite values, no box or vote gradient
        assert got['point_loss_box'] == 0 and got['vote_loss_reg'] == 0 and got['total'] > 0
        assert not got['d_reg'].any() and not got['d_vote'].any() and got['d_cls'].any()
    # an upstream gradient other than 1 is read from the device and scales every gradient
    half = run_gpu(inputs, cfg, upstream=0.5)
    for k in ('d_vote', 'd_cls', 'd_reg'):
        np.testing.assert_array_equal(half[k], (0.5 * got[k].astype(np.float64)).astype(F32), err_msg=k)


def random_case(seed, n, num_class, nb=12, ground_aware=True):
    """labels like those of the assignment (zero rows for background and ignored points) and predictions around them; rows near
    a discontinuity (top-two bin logits or the two corner losses closer than 1e-3) are redrawn until none is left"""
    rng = np.random.default_rng(seed)
    code = 6 + 2 * nb + (2 if ground_aware else 1)
    cfg = model.config(num_class=num_class, angle_bin_num=nb, ground_aware=ground_aware, centerness=True, corner=True,
                       centerness_min=0.1, centerness_max=0.95,
                       weights=dict(vote_reg_weight=0.7, point_cls_weight=1.3, point_offset_reg_weight=0.9, point_angle_cls_weight=0.2,
                                    point_angle_reg_weight=1.1, point_pitch_cls_weight=0.3, point_pitch_reg_weight=0.8,
                                    point_corner_weight=0.6))
    labels = rng.choice([-1, 0, 0, 1, 2, 3], n).astype(np.int64)
    labels[labels > num_class] = 1
    pos = labels > 0
    box = np.zeros((n, 9), F32)
    box[:, :3] = rng.uniform(-30, 30, (n, 3))
    box[:, 3:6] = rng.uniform(0.5, 5, (n, 3))
    box[:, 6] = rng.uniform(-np.pi, np.pi, n)
    box[:, 7] = rng.uniform(-0.5, 0.5, n)
    box[:, 8] = rng.uniform(-0.3, 0.3, n)
    points = (box[:, :3] + rng.uniform(-0.4, 0.4, (n, 3)) * box[:, 3:6]).astype(F32)
    per = 2 * np.pi / nb
    shifted = np.mod(np.mod(box[:, 6].astype(np.float64), 2 * np.pi) + per / 2, 2 * np.pi)
    k = np.minimum(np.floor(shifted / per).astype(np.int64), nb - 1)
    reg = np.zeros((n, code), F32)
    reg[:, :3] = box[:, :3] - points
    reg[:, 3:6] = np.log(box[:, 3:6])
    reg[np.arange(n), 6 + k] = 1.0
    reg[np.arange(n), 6 + nb + k] = (shifted - (k * per + per / 2)) / per
    thr, fac = np.deg2rad(10), np.deg2rad(45)
    if ground_aware:
        steep = box[:, 7] < -thr
        reg[:, 6 + 2 * nb] = steep
        reg[:, 6 + 2 * nb + 1] = np.where(steep, (-thr - box[:, 7]) / fac, 0.0)
    else:
        reg[:, 6 + 2 * nb] = box[:, 7]
    reg[~pos], box[~pos] = 0, 0
    vcls = (rng.random(n) < 0.4).astype(np.int64)
    vreg = np.where(vcls[:, None] > 0, points + rng.normal(0, 0.3, (n, 3)), 0).astype(F32)

    def draw():
        preds = (reg + 0.15 * rng.standard_normal(reg.shape)).astype(F32)
        preds[:, 6:6 + nb] = (3.0 * reg[:, 6:6 + nb] + 1.5 * rng.standard_normal((n, nb))).astype(F32)
        if ground_aware:
            preds[:, 6 + 2 * nb] = (2.0 * rng.standard_normal(n)).astype(F32)
        return preds
    inputs = dict(vote_preds=points, vote_reg_labels=vreg, vote_cls_labels=vcls,
                  cls_preds=(2.0 * rng.standard_normal((n, num_class))).astype(F32), cls_labels=labels, reg_preds=draw(),
                  reg_labels=reg, box_labels=box)
    for _ in range(50):
        top = np.sort(inputs['reg_preds'][:, 6:6 + nb].astype(np.float64), -1)
        gap = model.evaluate(inputs, cfg, grad=False)['corner_gap'].min(-1)
        bad = gap < 1e-3
        if nb > 1:
            bad |= top[:, -1] - top[:, -2] < 1e-3
        if not bad.any():
            break
        inputs['reg_preds'][bad] = draw()[bad]
    assert not bad.any()
    return inputs, cfg


@pytest.mark.parametrize("n,num_class,nb,ground_aware", [(20480, 3, 12, True), (2048, 1, 12, True), (1000, 16, 32, False),
                                                         (129, 2, 1, True), (1, 1, 5, False)])
def test_random_cases_against_the_model(data, n, num_class, nb, ground_aware):
    _, fx = data
    inputs, cfg = random_case(100 + n, n, num_class, nb, ground_aware)
    want = model.evaluate(inputs, cfg, upstream=1.0)
    got = run_gpu(inputs, cfg)
    compare(got, want, inputs, lambda k: bound_any_case(fx, k), 'random n=%d' % n)
    if n >= 1000:
        assert want['n_pos'] > 0.3 * n and want['n_valid'] < n and 0 < want['n_pitch_pos'] <= want['n_pos']


def test_two_runs_give_the_same_bits_and_needs_input_grad_is_honoured(data):
    from de6d_amd.ops import head_loss
    inputs, cfg = random_case(5, 20480, 3)
    first, second = run_gpu(inputs, cfg), run_gpu(inputs, cfg)
    for k in ('sums', 'loss_cls', 'loss_box', 'centerness', 'd_vote', 'd_cls', 'd_reg'):
        assert first[k].tobytes() == second[k].tobytes(), k
    spec = spec_of(cfg)
    t = [dev(inputs[k]) for k in ORDER]
    sums = head_loss.forward(spec, *t)
    g = torch.ones((), dtype=torch.float32, device='cuda')
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        grads = head_loss.backward(spec, sums, g, *t, need=need)
        for wanted, got, k in zip(need, grads, ('d_vote', 'd_cls', 'd_reg')):
            assert (got is not None) == wanted
            if wanted:
                assert got.cpu().numpy().tobytes() == first[k].tobytes(), (need, k)
    # through autograd: only the tensors that require a gradient get one, and the loss is a 0-d view of sums
    leaves = [t[0].clone().requires_grad_(True), t[3].clone(), t[5].clone().requires_grad_(True)]
    loss, sums2 = head_loss.HeadLoss.apply(spec, leaves[0], leaves[1], leaves[2], t[1], t[2], t[4], t[6], t[7])
    assert loss.dim() == 0 and loss.requires_grad and not sums2.requires_grad and torch.equal(sums2, sums)
    (2.0 * loss).backward()                                                # a power of two: every gradient scales exactly
    assert leaves[1].grad is None
    for leaf, k in ((leaves[0], 'd_vote'), (leaves[2], 'd_reg')):
        np.testing.assert_array_equal(leaf.grad.cpu().numpy(), (2.0 * first[k].astype(np.float64)).astype(F32), err_msg=k)
    # n = 0: nothing launched, zeros
    empty = [x[:0].contiguous() for x in t]
    assert not head_loss.forward(spec, *empty).any()


def test_centerness_and_corner_entries_against_the_model(data):
    from de6d_amd.ops import head_loss
    _, fx = data
    inputs, cfg = random_case(9, 4096, 3)
    pos = inputs['cls_labels'] > 0
    cen = head_loss.centerness_labels(dev(inputs['vote_preds']), dev(inputs['box_labels']), dev(pos)).cpu().numpy()
    want = model.centerness_label(inputs['vote_preds'], inputs['box_labels'], pos)
    assert not cen[~pos].any() and model.err(cen, want) <= bound_any_case(fx, 'centerness')
    centre, size, yaw, _ = model.decode7(inputs['reg_preds'].astype(np.float64), inputs['vote_preds'].astype(np.float64), 12)
    pred = np.concatenate([centre, size, yaw[:, None]], -1).astype(F32)[pos]
    gt = np.ascontiguousarray(inputs['box_labels'][pos, :7])
    got = head_loss.corner_loss(dev(pred), dev(gt)).cpu().numpy()
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    e0 = model.corners(p64[:, :3], p64[:, 3:6], p64[:, 6]) - model.corners(g64[:, :3], g64[:, 3:6], g64[:, 6])
    e1 = model.corners(p64[:, :3], p64[:, 3:6], p64[:, 6]) - model.corners(g64[:, :3], g64[:, 3:6], g64[:, 6] + np.pi)
    want = np.minimum(model.smooth_l1(e0, 1.0).sum(-1), model.smooth_l1(e1, 1.0).sum(-1)).mean(-1)
    assert model.err(got, want) <= bound_any_case(fx, 'loss_box')


# ---- the head and the detector ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_loss.yaml')
    return cfg, build_model(cfg, seed=11, device='cuda')


def prepared(net, seed, b=3, n=2048, m=16):
    from tests.test_targets_gpu import boxes_around, forward
    bd, _ = forward(net, seed, b, n)
    vote = bd['point_vote_coords'].cpu().numpy()
    bd['gt_boxes'] = dev(boxes_around(seed + 10, vote[:, 1:4].reshape(b, -1, 3), b, 10, m))
    return bd


def model_of_head(head):
    """the model evaluated on the tensors prepare_loss stored"""
    ret = head.forward_ret_dict
    inputs = dict(vote_preds=ret['point_vote_coords'], vote_reg_labels=ret['vote_reg_labels'], vote_cls_labels=ret['vote_cls_labels'],
                  cls_preds=ret['point_cls_preds'], cls_labels=ret['point_cls_labels'], reg_preds=ret['point_reg_preds'],
                  reg_labels=ret['point_reg_labels'], box_labels=ret['point_box_labels'])
    inputs = {k: v.detach().cpu().numpy() for k, v in inputs.items()}
    loss_cfg = head.model_cfg.LOSS_CONFIG
    cfg = model.config(num_class=head.num_class, angle_bin_num=head.box_coder.angle_bin_num, ground_aware=head.box_coder.ground_aware,
                       centerness='WithCenterness' in loss_cfg.LOSS_CLS, corner=bool(loss_cfg.get('CORNER_LOSS_REGULARIZATION', False)),
                       weights=dict(loss_cfg.LOSS_WEIGHTS), centerness_min=loss_cfg.LOSS_CLS_CONFIG['centerness_min'],
                       centerness_max=loss_cfg.LOSS_CLS_CONFIG['centerness_max'])
    return inputs, model.evaluate(inputs, cfg)


def test_head_and_detector_on_the_tiny_loss_config(data, tiny):
    _, fx = data
    cfg, net = tiny
    head = net.point_head
    loss_cfg = cfg.MODEL.POINT_HEAD.LOSS_CONFIG
    assert loss_cfg.CORNER_LOSS_REGULARIZATION is True and dict(loss_cfg.LOSS_CLS_CONFIG) == {'centerness_min': 0.0, 'centerness_max': 1.0}
    bd = prepared(net, 31)
    ret = head.prepare_loss(bd, requires_grad=True)
    assert ret is head.forward_ret_dict and ret['point_vote_coords'].shape[1] == 3
    loss, tb = head.get_loss()
    inputs, want = model_of_head(head)
    assert want['n_pos'] > 10 and want['n_vote_pos'] > 0
    limit = lambda k: bound_any_case(fx, k)                                # noqa: E731
    assert sorted(tb) == ['point_loss_box', 'point_loss_cls', 'point_loss_vote', 'point_pos_num', 'vote_loss_reg']
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in tb.values()) and loss.dim() == 0 and loss.is_cuda
    assert float(tb['point_pos_num']) == want['n_pos']
    for key, name in (('point_loss_vote', 'vote_loss_reg'), ('vote_loss_reg', 'vote_loss_reg'), ('point_loss_cls', 'point_loss_cls'),
                      ('point_loss_box', 'point_loss_box')):
        assert model.err(float(tb[key]), want[name]) <= limit(name), key
    assert model.err(float(loss), want['total']) <= limit('total')
    loss.backward()
    for key, name in (('point_vote_coords', 'd_vote'), ('point_cls_preds', 'd_cls'), ('point_reg_preds', 'd_reg')):
        assert model.err(ret[key].grad.cpu().numpy(), want[name]) <= limit(name), key
    # the layer methods, under the reference's names and return shapes
    vote_loss, tb0 = head.get_vote_layer_loss()
    assert model.err(float(vote_loss), want['vote_loss_reg']) <= limit('vote_loss_reg') and 'vote_loss_reg' in tb0
    loss_cls, cls_w, tb1 = head.get_cls_layer_loss()
    assert model.err(loss_cls.cpu().numpy(), want['loss_cls']) <= limit('loss_cls') and float(tb1['point_pos_num']) == want['n_pos']
    np.testing.assert_array_equal(cls_w.cpu().numpy(), (inputs['cls_labels'] >= 0).astype(F32))
    loss_box, box_w, _ = head.get_box_layer_loss()
    assert model.err(loss_box.cpu().numpy(), want['loss_box']) <= limit('loss_box')
    np.testing.assert_array_equal(box_w.cpu().numpy(), (inputs['cls_labels'] > 0).astype(F32))
    pos = ret['point_cls_labels'] > 0
    cen = head.generate_centerness_label(ret['point_vote_coords'].detach(), ret['point_box_labels'], pos)
    assert model.err(cen.cpu().numpy(), want['centerness']) <= limit('centerness')
    corner = head.get_corner_loss_lidar(ret['point_box_preds'][:, :7].contiguous(), ret['point_box_labels'][:, :7].contiguous())
    assert corner.shape == pos.shape and torch.isfinite(corner).all()
    # the detector: the same numbers from a fresh batch_dict
    bd2 = prepared(net, 31)
    loss2, tb2, disp = net.get_training_loss(bd2)
    assert disp == {} and torch.equal(loss2, loss.detach()) and sorted(tb2) == sorted(tb)
    for k in tb:
        assert torch.equal(tb2[k], tb[k]), k
    # training-mode forward keeps raising
    net.train()
    try:
        with pytest.raises(NotImplementedError):
            net({'batch_size': 1})
    finally:
        net.eval()


def test_a_captured_graph_replays_to_the_bits_of_the_eager_run(tiny):
    _, net = tiny
    head = net.point_head
    keys = ('point_candidate_coords', 'point_vote_coords', 'gt_boxes')
    preds = ('point_cls_preds', 'point_reg_preds')

    def step(bd):
        ret = head.prepare_loss(bd, requires_grad=True)
        loss, tb = head.get_loss()
        grads = torch.autograd.grad(loss, [ret['point_vote_coords'], ret['point_cls_preds'], ret['point_reg_preds']])
        return (loss.detach(), tb['point_loss_box'], tb['point_pos_num']) + grads

    runs = []
    for j in range(3):
        bd = prepared(net, 40 + j)
        run = {k: bd[k].clone() for k in keys}
        run.update({k: head.forward_ret_dict[k].detach().clone() for k in preds})
        runs.append(run)
    static = {k: v.clone() for k, v in runs[0].items()}

    def bind():
        for k in preds:
            head.forward_ret_dict[k] = static[k]
    eager = []
    for r in runs:
        for k in static:
            static[k].copy_(r[k])
        bind()
        eager.append([x.clone() for x in step(static)])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        bind()
        step(static)                                                       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    bind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static)
    for r, want in list(zip(runs, eager))[::-1] + list(zip(runs, eager)):
        for k in static:
            static[k].copy_(r[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(out, want):
            assert torch.equal(got, w)
        assert float(want[2]) > 5 and want[5].any()


def test_out_of_scope_keys_raise(tiny):
    import copy
    cfg, net = tiny
    head = net.point_head
    good = copy.deepcopy(head.model_cfg.LOSS_CONFIG)
    assert head.build_losses(good) is not None

    def changed(**kw):
        c = copy.deepcopy(good)
        for k, v in kw.items():
            c[k] = v
        return c
    weights = dict(good.LOSS_WEIGHTS)
    for bad, word in ((changed(LOSS_SASA_CONFIG={'use': True}), 'LOSS_SASA_CONFIG'),
                      (changed(AXIS_ALIGNED_IOU_LOSS_REGULARIZATION=True), 'AXIS_ALIGNED_IOU_LOSS_REGULARIZATION'),
                      (changed(LOSS_CLS='FocalLoss'), 'LOSS_CLS'), (changed(LOSS_CLS='WeightedCrossEntropy'), 'LOSS_CLS'),
                      (changed(LOSS_REG='WeightedL1Loss'), 'LOSS_REG'),
                      (changed(LOSS_WEIGHTS=dict(weights, code_weights=[1.0] * 32)), 'code_weights')):
        with pytest.raises(NotImplementedError, match=word):
            head.build_losses(bad)
    coder = head.box_coder
    try:
        coder.pred_velo = True
        with pytest.raises(NotImplementedError, match='pred_velo'):
            head.build_losses(good)
        del coder.pred_velo
        coder.use_mean_size = True
        with pytest.raises(NotImplementedError, match='use_mean_size'):
            head.build_losses(good)
        coder.use_mean_size = False
        head.box_coder = object()
        with pytest.raises(NotImplementedError, match='BOX_CODER'):
            head.build_losses(good)
    finally:
        head.box_coder = coder
        coder.use_mean_size = False
        if hasattr(coder, 'pred_velo'):
            del coder.pred_velo
    with pytest.raises(KeyError):
        head.build_losses(changed(LOSS_WEIGHTS={k: v for k, v in weights.items() if k != 'point_corner_weight'}))
    head.build_losses(good)
    head.train()
    try:
        with pytest.raises(NotImplementedError):
            head({'batch_size': 1})
    finally:
        head.eval()
