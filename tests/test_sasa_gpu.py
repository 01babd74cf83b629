"""The SASA loss on the GPU (de6d_amd/csrc/ext/sasa_loss.hip and the layers above it): labels exact against the reference's
recorded labels and the float64 model (tests/models/sasa.py) — every test point keeps >= 1e-3 from every decision face —
losses and gradients within the bound of tests/test_sasa_model.py, bit-identical repeats, capturable into a graph, and the tiny
model's confidence layers trained through it.  Every comparison prints its figure (pytest -s) before it asserts."""
import copy

import numpy as np
import pytest
import torch

from tests.models import sasa as model
from tests.test_sasa_model import EXTRA, bound, bound_any_case, case_names, case_of, load

pytestmark = pytest.mark.gpu

F32 = np.float32
WEIGHTS = [0.01, 0.1, 1.0]


@pytest.fixture(scope="module")
def fx():
    return load()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def spec_of(case):
    from de6d_amd.ops import sasa_loss
    return sasa_loss.SasaSpec(case['func'], case['layer_weights'], case['extra_width'], case['set_ignore_flag'])


def run_gpu(case, coords, scores, gt_boxes, upstream=1.0, reuse_labels=True):
    """labels, sums and d_scores of the three entry points on host arrays"""
    from de6d_amd.ops import sasa_loss
    spec = spec_of(case)
    c, s, g = [dev(x) for x in coords], [dev(x) for x in scores], dev(gt_boxes)
    sums, labels = sasa_loss.forward(spec, c, s, g, labels=True)
    grad = torch.tensor([upstream], dtype=torch.float32, device='cuda')
    d = sasa_loss.backward(spec, sums, grad, c, s, g, labels=labels if reuse_labels else None)
    torch.cuda.synchronize()
    return [host(t) for t in labels], host(sums).astype(np.float64), [host(t) for t in d]


def model_of(case, coords, scores, gt_boxes, upstream=1.0):
    labels = [None if (s is None or w == 0) else model.assign(xyz, gt_boxes, case['extra_width'], case['set_ignore_flag'])
              for xyz, s, w in zip(coords, scores, case['layer_weights'])]
    return labels, model.loss(scores, labels, case['layer_weights'], case['func'], upstream=upstream)


def compare(got, want, limit, tag):
    """labels and counts exact, zeros where the label is -1, floats within limit(key)"""
    labels, sums, d = got
    wlabels, w = want
    n = len(wlabels)
    for i in range(n):
        assert (labels[i] is None) == (wlabels[i] is None) == (d[i] is None), (tag, i)
        if wlabels[i] is None:
            assert not sums[4 * i:4 * i + 4].any(), (tag, i)
            continue
        assert labels[i].dtype == np.int64
        np.testing.assert_array_equal(labels[i], wlabels[i], err_msg='%s labels %d' % (tag, i))
        np.testing.assert_array_equal(sums[4 * i + 1:4 * i + 4], w['sums'][4 * i + 1:4 * i + 4], err_msg='%s counts %d' % (tag, i))
        assert not d[i].reshape(-1)[wlabels[i] < 0].any(), (tag, i)
        assert d[i].shape == w['d_scores'][i].shape and np.isfinite(d[i]).all()
        for key, g, t in (('loss_%d' % i, sums[4 * i], w['losses'][i]), ('d_scores_%d' % i, d[i], w['d_scores'][i])):
            e = model.err(g, t)
            print("sasa %s %s: err %.3g (limit %.3g)" % (tag, key, e, limit(key)))
            assert e <= limit(key), (tag, key, e)
    e = model.err(sums[4 * n], w['total'])
    print("sasa %s total: err %.3g (limit %.3g)" % (tag, e, limit('total')))
    assert e <= limit('total'), (tag, e)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_every_fixture_case_labels_exact_loss_and_gradient_within_the_bound(fx, name):
    case = case_of(fx, name)
    coords, scores, gt_boxes = model.fixture_inputs(fx, case)
    got = run_gpu(case, coords, scores, gt_boxes)
    for i, lab in enumerate(got[0]):                         # the reference's own labels, every row
        assert (lab is None) == ('%s_labels_%d' % (name, i) not in fx)
        if lab is not None:
            np.testing.assert_array_equal(lab, fx['%s_labels_%d' % (name, i)])
    compare(got, model_of(case, coords, scores, gt_boxes), lambda key: bound(fx, name, key), name)
    # an upstream gradient of 0.5 halves every gradient; labels computed again in the backward give the same bits
    half = run_gpu(case, coords, scores, gt_boxes, upstream=0.5, reuse_labels=False)
    for a, b in zip(half[2], got[2]):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, F32(0.5) * b)
    np.testing.assert_array_equal(half[1], got[1])


# ---- points_in_boxes7 -----------------------------------------------------------------------------------------------------
def yaw_boxes(rng, m, spread):
    box = np.zeros((m, 10), F32)
    box[:, 0], box[:, 1], box[:, 2] = rng.uniform(0, spread, m), rng.uniform(-spread / 2, spread / 2, m), rng.uniform(-1, 1, m)
    box[:, 3], box[:, 4], box[:, 5] = rng.uniform(2, 5, m), rng.uniform(1, 3, m), rng.uniform(1, 2, m)
    box[:, 6], box[:, 7], box[:, 8], box[:, 9] = rng.uniform(-4, 7, m), rng.uniform(-0.2, 0.2, m), rng.uniform(-0.2, 0.2, m), 1
    return box


def safe_points(rng, boxes, n, spread):
    """(n, 3) fp32 points, about half of them near a box, every one >= 1e-3 from every decision face of the scene"""
    def draw(k):
        pts = np.stack([rng.uniform(-2, spread + 2, k), rng.uniform(-spread / 2 - 2, spread / 2 + 2, k), rng.uniform(-2.5, 2.5, k)], 1)
        if len(boxes):
            b = boxes[rng.integers(len(boxes), size=k)].astype(np.float64)
            loc = rng.uniform(-0.6, 0.6, (k, 3)) * (b[:, 3:6] + 0.2)
            c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
            near = np.stack([b[:, 0] + loc[:, 0] * c - loc[:, 1] * s, b[:, 1] + loc[:, 0] * s + loc[:, 1] * c, b[:, 2] + loc[:, 2]], 1)
            pts = np.where((rng.random(k) < 0.5)[:, None], near, pts)
        return pts.astype(F32)
    pts = draw(n)
    for _ in range(100):
        bad = model.face_distance(pts, boxes, EXTRA) < 1e-3
        if not bad.any():
            return pts
        pts[bad] = draw(int(bad.sum()))
    raise AssertionError("no safe points")


def scene_set(seed, b, sizes, m, spread=None, padding=0):
    """b scenes of m boxes (and `padding` all-zero rows after them), points per scene and layer as in `sizes`"""
    rng = np.random.default_rng(seed)
    spread = spread or 8.0 + 3.0 * m ** 0.5
    gt = np.stack([yaw_boxes(rng, m, spread) for _ in range(b)]) if m else np.zeros((b, 0, 10), F32)
    if m > 2:                                                # overlapping boxes: first and last hit differ
        gt[:, m // 2:, :3] = gt[:, :m - m // 2, :3] + rng.uniform(-0.5, 0.5, (b, m - m // 2, 3)).astype(F32)
    gt = np.concatenate([gt, np.zeros((b, padding, 10), F32)], 1)
    coords = [np.stack([safe_points(rng, gt[k], n, spread) for k in range(b)]) for n in sizes]
    scores = [(2.0 * rng.standard_normal((b * n, 1))).astype(F32) for n in sizes]
    return coords, scores, gt


@pytest.mark.parametrize("m", [1, 5, 130])
def test_points_in_boxes7_first_box_in_all_three_layouts(m):
    from de6d_amd.ops import box_targets, sasa_loss
    from de6d_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    b, n = 3, 300
    (pts,), _, gt = scene_set(50 + m, b, [n], m)
    for extra in (None, EXTRA):
        want = model.points_in_boxes7(pts.reshape(-1, 3), gt, n_per_scene=n, extra_width=extra)
        dense = sasa_loss.points_in_boxes7(dev(pts), dev(gt), extra_width=extra)
        assert dense.dtype == torch.int32 and dense.shape == (b * n,)
        np.testing.assert_array_equal(host(dense), want)
        # stacked rows [pad, x, y, z, scene, pad], shuffled: any scene in any order
        rows = np.full((b * n, 6), 9.5, F32)
        rows[:, 1:4], rows[:, 4] = pts.reshape(-1, 3), np.repeat(np.arange(b, dtype=F32), n)
        perm = np.random.default_rng(m).permutation(b * n)
        stacked = sasa_loss.points_in_boxes7(dev(rows[perm]), dev(gt), extra_width=extra, xyz_col=1, bs_col=4)
        np.testing.assert_array_equal(host(stacked), want[perm])
        wide = np.concatenate([np.zeros((b * n, 1), F32), pts.reshape(-1, 3)], 1)
        flat = sasa_loss.points_in_boxes7(dev(wide), dev(gt), extra_width=extra, xyz_col=1, bs_col=-1, n_per_scene=n)
        np.testing.assert_array_equal(host(flat), want)
    assert (want >= 0).mean() > 0.15
    if m > 2:                                                # the first box, where points_in_boxes9 takes the last
        flat_gt = gt.copy()
        flat_gt[:, :, 7:9] = 0
        last = host(box_targets.points_in_boxes9(dev(pts), dev(flat_gt)))
        plain = model.points_in_boxes7(pts.reshape(-1, 3), gt, n_per_scene=n)
        assert ((last > plain) & (plain >= 0)).any()
    # the reference's name: (B, N, 3), (B, M, 7) -> (B, N) int32
    got = roiaware_pool3d_utils.points_in_boxes_gpu(dev(pts), dev(gt[:, :, :7].copy()))
    assert got.shape == (b, n) and got.dtype == torch.int32
    np.testing.assert_array_equal(host(got).reshape(-1), model.points_in_boxes7(pts.reshape(-1, 3), gt, n_per_scene=n))
    with pytest.raises(NotImplementedError):
        roiaware_pool3d_utils.points_in_boxes_cpu(pts[0], gt[0, :, :7])
    with pytest.raises(NotImplementedError):
        roiaware_pool3d_utils.RoIAwarePool3d(7)


# ---- shapes at which the kernels can go wrong -----------------------------------------------------------------------------
SIZES = [300, 77, 1]          # per scene, B = 3: partial slabs, a slab boundary inside a scene, a one-row segment


def case(func='BCE', ignore=True, extra=EXTRA, weights=WEIGHTS):
    return dict(func=func, set_ignore_flag=ignore, extra_width=extra, layer_weights=list(weights))


@pytest.mark.parametrize("m", [0, 1, 5, 130])
@pytest.mark.parametrize("func,ignore", [('BCE', True), ('Focal', False)])
def test_partial_slabs_scene_boundaries_and_box_chunks(fx, m, func, ignore):
    coords, scores, gt = scene_set(900 + m, 3, SIZES, m)
    c = case(func, ignore)
    got = run_gpu(c, coords, scores, gt)
    want = model_of(c, coords, scores, gt)
    compare(got, want, lambda key: bound_any_case(fx, key.rstrip('_0123456789')), 'm%d_%s' % (m, func))
    if m >= 5:
        assert all((lab == 1).any() and (lab == 0).any() for lab in want[0][:2])
        assert not ignore or (want[0][0] == -1).any()
    if m == 0:
        assert all(not lab.any() for lab in got[0])


def test_skipped_segments_padding_rows_and_nan_coordinates(fx):
    from de6d_amd.ops import sasa_loss
    limit = lambda key: bound_any_case(fx, key.rstrip('_0123456789'))                                        # noqa: E731
    coords, scores, gt = scene_set(77, 3, SIZES, 5)
    # a skipped middle segment (no scores) and a weight of 0: no labels, zero sums, the others unchanged
    full = run_gpu(case(), coords, scores, gt)
    for c, s in ((case(), [scores[0], None, scores[2]]), (case(weights=[0.01, 0.0, 1.0]), scores)):
        got = run_gpu(c, coords, s, gt)
        compare(got, model_of(c, coords, s, gt), limit, 'skipped')
        assert got[0][1] is None and got[2][1] is None
        np.testing.assert_array_equal(got[1][[0, 1, 2, 3, 8, 9, 10, 11]], full[1][[0, 1, 2, 3, 8, 9, 10, 11]])
        np.testing.assert_array_equal(got[2][0], full[2][0])
    # every layer skipped: nothing launched, zero sums
    spec = spec_of(case(weights=[0.0, 0.0, 0.0]))
    sums, labels = sasa_loss.forward(spec, [dev(x) for x in coords], [dev(x) for x in scores], dev(gt), labels=True)
    assert labels == [None] * 3 and not host(sums).any() and sums.shape == (13,)
    # an all-zero padding row enlarged by extra_width is a small box at the origin
    at_origin, _, pad = scene_set(78, 3, SIZES, 5, padding=2)
    at_origin[0][1, 5] = [0.05, -0.05, 0.05]
    at_origin[2][2, 0] = [0.02, -0.04, -0.03]
    for ignore, want_label in ((True, -1), (False, 1)):
        got = run_gpu(case(ignore=ignore), at_origin, scores, pad)
        compare(got, model_of(case(ignore=ignore), at_origin, scores, pad), limit, 'padding')
        assert got[0][0][300 + 5] == want_label and got[0][2][2] == want_label
    assert run_gpu(case(ignore=False, extra=None), at_origin, scores, pad)[0][0][300 + 5] == 0
    # NaN coordinates: outside every box, nothing becomes non-finite
    nan = [x.copy() for x in coords]
    inside = np.nonzero(full[0][0] == 1)[0][:3]
    for k, row in enumerate(inside):
        nan[0].reshape(-1, 3)[row, k] = np.nan
    nan[1][0, 3] = np.nan
    got = run_gpu(case(), nan, scores, gt, reuse_labels=False)
    assert not got[0][0][inside].any() and got[0][1][3] == 0
    assert np.isfinite(got[1]).all() and all(np.isfinite(d).all() for d in got[2])
    keep = np.ones(len(full[0][0]), bool)
    keep[inside] = False
    np.testing.assert_array_equal(got[0][0][keep], full[0][0][keep])


def test_two_runs_give_the_same_bits(fx):
    coords, scores, gt = scene_set(5, 3, [1000, 300, 77], 40)
    a, b = run_gpu(case('Focal'), coords, scores, gt), run_gpu(case('Focal'), coords, scores, gt)
    np.testing.assert_array_equal(a[1], b[1])
    for x, y in zip(a[0] + a[2], b[0] + b[2]):
        np.testing.assert_array_equal(x, y)
    assert a[1][1] > 256 and a[1][2] > 0 and a[1][3] > 0


def test_a_captured_graph_replays_to_the_bits_of_the_eager_run():
    from de6d_amd.ops import sasa_loss
    spec = spec_of(case())
    runs = [scene_set(60 + j, 3, SIZES, 5, spread=14.0) for j in range(3)]
    static = dict(coords=[dev(x) for x in runs[0][0]], scores=[dev(x).requires_grad_(True) for x in runs[0][1]], gt=dev(runs[0][2]))

    def load_run(r):
        with torch.no_grad():
            for dst, src in zip(static['coords'] + static['scores'] + [static['gt']], r[0] + r[1] + [r[2]]):
                dst.copy_(dev(src))

    def step():
        loss, sums = sasa_loss.SasaLoss.apply(spec, static['gt'], static['coords'], None, *static['scores'])
        return (loss.detach(), sums) + torch.autograd.grad(loss, static['scores'])
    spec.extra(torch.device('cuda', torch.cuda.current_device()))            # the one upload, before the capture
    eager = []
    for r in runs:
        load_run(r)
        eager.append([x.clone() for x in step()])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                             # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for r, want in list(zip(runs, eager))[::-1] + list(zip(runs, eager)):
        load_run(r)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(out, want):
            assert torch.equal(got, w)
        assert float(want[1][2]) > 0 and want[2].any()


def test_the_reference_names_on_a_fixture_case(fx):
    from de6d_amd.pcdet.utils import loss_utils
    name = 'bce_ignore'
    c = case_of(fx, name)
    coords, scores, gt_boxes = model.fixture_inputs(fx, c)
    with pytest.raises(NotImplementedError):
        loss_utils.PointSASALoss(func='CrossEntropy', layer_weights=WEIGHTS)
    with pytest.raises(AssertionError):
        loss_utils.PointSASALoss(func='BCE', layer_weights=WEIGHTS, set_ignore_flag=True)
    mod = loss_utils.PointSASALoss(func=c['func'], layer_weights=c['layer_weights'], extra_width=c['extra_width'], set_ignore_flag=True)
    b = gt_boxes.shape[0]
    l_points = [dev(np.concatenate([np.repeat(np.arange(b, dtype=F32), x.shape[1])[:, None], x.reshape(-1, 3)], 1)) for x in coords]
    l_scores = [dev(s).requires_grad_(True) for s in scores]
    single = mod.assign_target(l_points[1], dev(gt_boxes))
    assert single.dtype == torch.int64 and single.shape == (l_points[1].shape[0],)
    np.testing.assert_array_equal(host(single), fx[name + '_labels_1'])
    l_labels = mod(l_points, l_scores, dev(gt_boxes))
    l_loss = mod.loss_forward(l_scores, l_labels)
    assert len(l_loss) == 3 and all(v.dim() == 0 and v.is_cuda for v in l_loss)
    (l_loss[0] + 0.5 * l_loss[2]).backward()                 # each layer's loss carries its own upstream gradient
    _, want = model_of(c, coords, scores, gt_boxes)
    for i, factor in ((0, 1.0), (2, 0.5)):
        np.testing.assert_array_equal(host(l_labels[i]), fx['%s_labels_%d' % (name, i)])
        assert model.err(float(l_loss[i].detach()), want['losses'][i]) <= bound(fx, name, 'loss_%d' % i)
        assert model.err(host(l_scores[i].grad), factor * want['d_scores'][i]) <= bound(fx, name, 'd_scores_%d' % i)
    assert not host(l_scores[1].grad).any()
    skipping = loss_utils.PointSASALoss(func='BCE', layer_weights=[0.01, 0.0, 1.0])
    labels = skipping(l_points, [l_scores[0].detach(), l_scores[1].detach(), None], dev(gt_boxes))
    assert labels[1] is None and labels[2] is None and labels[0] is not None
    assert [v is None for v in skipping.loss_forward([s.detach() for s in l_scores], labels)] == [False, True, True]


# ---- the tiny model -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_sasa.yaml')
    return cfg, build_model(cfg, seed=11, device='cuda'), build_model(load_config('synthetic_models/det6d_tiny_loss.yaml'), seed=11,
                                                                     device='cuda')


def prepared(net, seed, b=3, n=2048, m=16):
    """an eval forward plus gt_boxes around the vote points and around points of the first two SA levels"""
    from tests.test_targets_gpu import boxes_around, forward
    bd, _ = forward(net, seed, b, n)
    vote = host(bd['point_vote_coords'])[:, 1:4].reshape(b, -1, 3)
    level = host(bd['point_coords_list'][1])[:, 1:4].reshape(b, -1, 3)
    bd['gt_boxes'] = dev(boxes_around(seed + 10, np.concatenate([vote, level[:, ::4]], 1), b, 10, m))
    return bd


def clear_grads(net):
    for p in net.parameters():
        p.grad = None


def confidence_parameters(net):
    return [('SA_modules.%d.confidence_mlp.%s' % (i, k), p) for i, sa in enumerate(net.backbone_3d.SA_modules)
            if sa.confidence_mlp is not None for k, p in sa.confidence_mlp.named_parameters()]


def test_head_and_detector_on_the_tiny_sasa_config(tiny):
    from de6d_amd.ops import sasa_loss
    cfg, net, plain = tiny
    head = net.point_head
    sasa_cfg = cfg.MODEL.POINT_HEAD.LOSS_CONFIG.LOSS_SASA_CONFIG
    assert dict(sasa_cfg) == {'func': 'BCE', 'layer_weights': WEIGHTS, 'extra_width': EXTRA, 'set_ignore_flag': True}
    bd = prepared(net, 31)
    outputs = {k: bd[k].clone() for k in ('batch_box_preds', 'batch_cls_preds', 'point_vote_coords')}
    loss, tb, disp = net.get_training_loss(bd, requires_grad=True)
    assert head.enable_sasa and disp == {} and loss.dim() == 0 and loss.is_cuda
    # the head loss of the config without LOSS_SASA_CONFIG (the same seed: the same weights) plus the ops-level SASA loss
    bd_plain = prepared(plain, 31)
    loss_plain, tb_plain, _ = plain.get_training_loss(bd_plain)
    assert not plain.point_head.enable_sasa and plain.point_head.get_sasa_layer_loss() == (None, None)
    spec = sasa_loss.SasaSpec(**dict(sasa_cfg))
    coords, scores = list(bd['point_coords_list']), bd['point_scores_list']
    assert [s is None for s in scores] == [False, False, True]
    sums, labels = sasa_loss.forward(spec, coords, scores, bd['gt_boxes'], labels=True)
    assert torch.equal(loss.detach(), loss_plain + sums[-1])
    assert sorted(tb) == sorted(list(tb_plain) + ['point_loss_sasa', 'point_loss_sasa_layer_0', 'point_loss_sasa_layer_1'])
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in tb.values())
    assert torch.equal(tb['point_loss_sasa'], sums[-1]) and torch.equal(tb['point_loss_sasa_layer_0'], sums[0])
    assert torch.equal(tb['point_loss_sasa_layer_1'], sums[4]) and all(torch.equal(tb[k], tb_plain[k]) for k in tb_plain)
    counts = host(sums)
    assert counts[2] > 0 and counts[6] > 0 and counts[3] + counts[7] > 0 and float(sums[-1]) > 0       # foreground and ignored points
    ret = head.forward_ret_dict
    assert all(torch.equal(a, b) for a, b in zip(ret['point_sasa_labels'][:2], labels[:2])) and ret['point_sasa_labels'][2] is None
    # requires_grad=True: the scores are leaves and receive the ops-level gradient
    loss.backward()
    want = sasa_loss.backward(spec, sums, torch.ones(1, device='cuda'), coords, scores, bd['gt_boxes'])
    for i in (0, 1):
        assert ret['point_sasa_preds'][i].is_leaf and torch.equal(ret['point_sasa_preds'][i].grad, want[i])
        assert ret['point_sasa_preds'][i].grad.abs().max() > 0
    assert all(p.grad is None for p in net.parameters())
    loss2, tb2 = head.get_sasa_layer_loss()
    assert torch.equal(loss2.detach(), sums[-1]) and sorted(tb2) == ['point_loss_sasa', 'point_loss_sasa_layer_0', 'point_loss_sasa_layer_1']
    # the eval outputs of a forward are bit-identical before and after
    bd_again = prepared(net, 31)
    assert all(torch.equal(bd_again[k], v) for k, v in outputs.items())
    # configuration errors
    good = copy.deepcopy(head.model_cfg.LOSS_CONFIG)

    def changed(**kw):
        c = copy.deepcopy(good)
        c['LOSS_SASA_CONFIG'] = dict(dict(good.LOSS_SASA_CONFIG), **kw)
        return c
    try:
        with pytest.raises(NotImplementedError, match='LOSS_SASA_CONFIG.*use'):
            head.build_losses(changed(use=True))
        with pytest.raises(NotImplementedError):
            head.build_losses(changed(func='CrossEntropy'))
        with pytest.raises(ValueError, match='layer_weights'):
            head.build_losses(changed(layer_weights=[0.1] * 4))
        with pytest.raises(KeyError, match='layer_weights'):
            head.build_losses(changed(layer_weights=None))
        with pytest.raises(AssertionError):
            head.build_losses(changed(extra_width=None))
    finally:
        head.build_losses(good)
    assert head.enable_sasa


def replay(seq, rows, d_scores, dtype):
    """the confidence nn.Sequential as a deep copy on the CPU in `dtype`, eval mode, fed the level's feature columns"""
    mod = copy.deepcopy(seq).cpu().to(dtype).eval()
    out = mod(rows.to(dtype).t().unsqueeze(0)).squeeze(0).t()
    out.backward(d_scores.to(dtype))
    return {k: p.grad.double().numpy() for k, p in mod.named_parameters()}


def test_tiny_model_confidence_layer_gradients(tiny):
    _, net, _ = tiny
    head = net.point_head
    named = confidence_parameters(net)
    ids = {id(p) for _, p in named}
    assert len(named) >= 8
    bd = prepared(net, 33, b=2)
    forward_scores = [None if s is None else s.clone() for s in bd['point_scores_list']]
    clear_grads(net)
    ret = head.prepare_loss(bd, requires_grad=True, sasa=True, sa_modules=net.backbone_3d.SA_modules)
    preds = ret['point_sasa_preds']
    # score parity: the SA layers run again at the forward's centres, then the confidence chain layer by layer (det6d_linear),
    # against the forward's fused aggregation + confidence route
    for i in (0, 1):
        diff = float((preds[i].detach() - forward_scores[i]).abs().max())
        print("sasa level %d: re-evaluated scores differ from the forward's by %.3g (max |score| %.3g)" % (
            i, diff, float(forward_scores[i].abs().max())))
        assert preds[i].shape == forward_scores[i].shape and torch.equal(preds[i].detach(), forward_scores[i])
        preds[i].retain_grad()
    assert preds[2] is None
    loss, _ = head.get_loss()
    loss.backward()
    torch.cuda.synchronize()
    for name, p in net.named_parameters():
        if id(p) in ids:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
        else:
            assert p.grad is None, name                      # nothing else of the backbone, nothing of the head
    err = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))                          # noqa: E731
    assert len(ret['point_sasa_rows']) == 3 and ret['point_sasa_rows'][2] is None
    for i, (sa, rows) in enumerate(zip(net.backbone_3d.SA_modules, ret['point_sasa_rows'][:2])):
        c = sa._folded['out_channels']
        feats = rows.detach().cpu().reshape(-1, rows.shape[-1])[:, 3:3 + c]
        d = preds[i].grad.cpu()
        t64, t32 = replay(sa.confidence_mlp, feats, d, torch.float64), replay(sa.confidence_mlp, feats, d, torch.float32)
        for k, p in sa.confidence_mlp.named_parameters():
            ref, eng = err(t32[k], t64[k]), err(p.grad.cpu().double().numpy(), t64[k])
            limit = max(4.0 * ref, 16.0 * 2.0 ** -24)
            print('sasa tiny level %d %-12s engine %.3e  fp32 replay %.3e  limit %.3e' % (i, k, eng, ref, limit))
            assert eng <= limit, (i, k, eng, ref)
    # sasa and head together fill both parameter sets; the loss is the same bits
    clear_grads(net)
    bd2 = prepared(net, 33, b=2)
    loss2 = net.get_training_loss(bd2, requires_grad=True, head=True, sasa=True)[0]
    assert torch.equal(loss2.detach(), loss.detach())
    loss2.backward()
    for name, p in net.named_parameters():
        wanted = id(p) in ids or name.startswith('point_head.')
        assert (p.grad is not None) == wanted, name
    clear_grads(net)
    # training mode and a config without the SASA loss raise
    net.train()
    try:
        with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
            head.prepare_loss(bd2, requires_grad=True, sasa=True, sa_modules=net.backbone_3d.SA_modules)
    finally:
        net.eval()
    with pytest.raises(RuntimeError, match='sa_modules'):
        head.prepare_loss(bd2, requires_grad=True, sasa=True)
    with pytest.raises(RuntimeError, match='LOSS_SASA_CONFIG'):
        tiny[2].point_head.prepare_loss(prepared(tiny[2], 33, b=2), sasa=True)
