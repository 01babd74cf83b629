"""Target assignment on the GPU (de6d_amd/csrc/ext/box_targets.hip and the layers above it): bit-exact against the CPU model
(tests/models/box_targets.py) everywhere, equal to the reference's recorded results (tests/golden/targets_ref.npz) outside the
stored exemption masks, capturable into a graph, and without effect on the inference outputs."""
import os

import numpy as np
import pytest
import torch

from tests.models import box_targets as model
from tests.test_targets_model import CAP, check_encoded, points_in, random_boxes, stacked
from tests.util import make_batch

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(HERE, 'golden', 'targets_ref.npz')))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scenes(seed, b, n, m, overlap=True, classes=True):
    """b scenes: m boxes each (10 columns, the last the class), n points drawn around the boxes (about a third inside)"""
    rng = np.random.default_rng(seed)
    boxes = np.stack([random_boxes(rng, m, spread=5.0 + 2.0 * m ** 0.5) for _ in range(b)])
    if overlap and m > 1:
        boxes[:, m // 2:, :3] = boxes[:, :m - m // 2, :3] + rng.uniform(-1, 1, (b, m - m // 2, 3)).astype(F32)
    pts = np.empty((b, n, 3), F32)
    for s in range(b):
        pts[s] = points_in(rng, boxes[s], -(-n // m), 0.75).reshape(-1, 3)[rng.permutation(m * -(-n // m))[:n]]
    cls = rng.integers(1, 4, (b, m, 1)).astype(F32)
    return pts, np.concatenate([boxes, cls], -1) if classes else boxes


def run_both(points, boxes, **kw):
    """det6d_ext_assign_targets9 on the GPU and the model on the same arrays -> asserts equality, returns the model's result"""
    from de6d_amd.ops import box_targets
    layout = dict(xyz_col=kw.pop('xyz_col'), bs_col=kw.pop('bs_col'))
    n_per_scene = kw.pop('n_per_scene', 1)
    dense_rows = dict(n_per_scene=n_per_scene) if points.ndim == 2 and layout['bs_col'] < 0 else {}
    got = box_targets.assign_targets9(dev(points), dev(boxes), **layout, **dense_rows, **kw)
    want = model.assign_targets9(points.reshape(-1, points.shape[-1]), boxes, n_per_scene=n_per_scene, **layout, **kw)
    for g, w, name in zip(got, want, ('box_idx', 'cls_labels', 'box_labels')):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want


SHAPES = [(1, 256, 1), (1, 1000, 7), (8, 256, 32), (8, 1000, 128), (8, 16384, 32), (80, 256, 7), (80, 1000, 32),
          (1, 16384, 1024), (8, 1000, 1024), (80, 16384, 7), (1, 16384, 128), (8, 256, 1)]


@pytest.mark.parametrize("b,n,m", SHAPES)
def test_bit_exact_against_the_model_dense_and_stacked(b, n, m):
    pts, boxes = scenes(1000 + b + n + m, b, n, m)
    kw = dict(class_col=9, num_class=3, central_radius=1.5, n_cols=9, extra_width=[0.2, 0.1, 0.3])
    idx, cls, _ = run_both(pts, boxes, xyz_col=0, bs_col=-1, n_per_scene=n, **kw)
    assert (idx >= 0).mean() > 0.2 and (cls == -1).any() and (cls > 0).any()
    if m > 1:
        assert len(np.unique(idx)) > min(m, 64) // 2
    # the same points as stacked rows [pad, pad, x, y, z, scene, pad]: ld wider than the payload, columns elsewhere
    rows = np.full((b * n, 7), 9.5, F32)
    rows[:, 2:5] = pts.reshape(-1, 3)
    rows[:, 5] = np.repeat(np.arange(b, dtype=F32), n)
    idx2, _, _ = run_both(rows, boxes, xyz_col=2, bs_col=5, **kw)
    np.testing.assert_array_equal(idx2, idx)
    # vote targets: no ball, no class, three columns, no extra width, dense rows of width 5
    wide = np.concatenate([np.zeros((b, n, 1), F32), pts, np.ones((b, n, 1), F32)], -1)
    run_both(wide, boxes, xyz_col=1, bs_col=-1, n_per_scene=n, n_cols=3)


def test_ragged_scenes_shuffled_rows_and_scene_indices_out_of_range():
    b, m = 8, 32
    pts, boxes = scenes(77, b, 1000, m)
    rng = np.random.default_rng(78)
    counts = [0, 1, 255, 256, 257, 1000, 63, 700]                        # scene 0 has no points at all
    rows = np.concatenate([np.concatenate([np.full((c, 1), s, F32), pts[s, :c]], -1) for s, c in enumerate(counts)])
    kw = dict(xyz_col=1, bs_col=0, class_col=9, num_class=3, central_radius=2.0, n_cols=9)
    ordered = run_both(rows, boxes, **kw)
    perm = rng.permutation(len(rows))                                   # every workgroup sees many scenes
    shuffled = run_both(rows[perm], boxes, **kw)
    for a, s in zip(ordered, shuffled):
        np.testing.assert_array_equal(a[perm], s)
    bad = rows[perm].copy()
    bad[::5, 0] = np.resize(np.array([-1, 8, 9, 4096, 1e9, -1e9, np.nan, np.inf, -np.inf, -0.5, 2.5], F32), len(bad[::5]))
    idx, cls, lab = run_both(bad, boxes, **kw)
    outside = ~((bad[:, 0] >= 0) & (bad[:, 0] < b))
    assert outside.sum() > 100 and (idx[outside] == -1).all() and (cls[outside] == 0).all() and (lab[outside] == 0).all()
    # dense layout whose row count is not a multiple of the scene length: the tail belongs to scenes >= b
    flat = pts.reshape(-1, 3)[:7 * 1000 + 300]
    run_both(flat, boxes[:7], xyz_col=0, bs_col=-1, n_per_scene=1000, n_cols=3)
    run_both(pts.reshape(-1, 3), boxes[:5], xyz_col=0, bs_col=-1, n_per_scene=1000, n_cols=3)


def test_points_on_faces_edges_and_corners_as_the_model_sees_them():
    rng = np.random.default_rng(5)
    m = 32
    boxes = random_boxes(rng, m, spread=40.0)
    rot = model.rotations(boxes[:, 6:9]).astype(np.float64)
    signs = np.array([[sx, sy, sz] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)], np.float64)   # 27 spots
    local = signs[None] * (boxes[:, None, 3:6].astype(np.float64) / 2)
    base = (np.einsum('mij,mkj->mki', rot, local) + boxes[:, None, :3].astype(np.float64)).astype(F32).reshape(-1, 3)
    pts = [base]
    for step in (1, 2, 8):                                              # and their fp32 neighbours, a few ulps either way
        for towards in (np.inf, -np.inf):
            p = base.copy()
            for _ in range(step):
                p = np.nextafter(p, F32(towards))
            pts.append(p)
    pts = np.concatenate(pts)
    idx, _, _ = run_both(pts[None], boxes[None], xyz_col=0, bs_col=-1, n_per_scene=len(pts), n_cols=9, central_radius=1.0)
    surface = idx.reshape(7, m, 27)[:, :, np.abs(signs).sum(1) > 0]
    assert (surface >= 0).any() and (surface < 0).any()                 # the set straddles the boundary: both answers occur
    assert (idx.reshape(7, m, 27)[:, :, 13] >= 0).all()                 # the centres


def test_overlapping_padding_and_degenerate_boxes():
    rng = np.random.default_rng(6)
    boxes = random_boxes(rng, 8, spread=3.0)
    boxes = np.concatenate([boxes, boxes[:4], np.zeros((4, 9), F32)])    # boxes 8..11 repeat 0..3; 12..15 are padding
    boxes[5, 3] = 0.0
    boxes[6, 4] = -2.0
    boxes[7, 5] = np.nan
    pts = np.concatenate([points_in(rng, boxes[:8], 64, 0.45).reshape(-1, 3), np.zeros((4, 3), F32),
                          np.array([[0.05, -0.05, 0.09], [np.nan, 0, 0], [0, np.inf, 0]], F32)])
    idx, _, _ = run_both(pts[None], boxes[None], xyz_col=0, bs_col=-1, n_per_scene=len(pts), n_cols=9)
    assert (idx[:256].reshape(4, 64) >= np.arange(8, 12)[:, None]).all()          # the highest index wins
    assert not np.isin(idx, [5, 6, 7, 12, 13, 14, 15]).any()
    idx, _, _ = run_both(pts[None], boxes[None], xyz_col=0, bs_col=-1, n_per_scene=len(pts), n_cols=9, extra_width=[0.2, 0.2, 0.2])
    assert (idx[-7:-2] == 15).all() and (idx[-2:] == -1).all()                    # an enlarged padding row is a cube at the origin
    zeros = np.zeros((1, 6, 10), F32)                                             # a scene with no boxes
    idx, cls, lab = run_both(pts[None], zeros, xyz_col=0, bs_col=-1, n_per_scene=len(pts), n_cols=9, class_col=9, num_class=3)
    assert (idx == -1).all() and (cls == 0).all() and (lab == 0).all()
    run_both(pts[None], zeros[:, :0], xyz_col=0, bs_col=-1, n_per_scene=len(pts), n_cols=3)      # m = 0: the fill values


def test_wrappers_and_the_mirror_of_box_utils(ref):
    from de6d_amd import _lib
    from de6d_amd.ops import box_targets
    from de6d_amd.pcdet.utils import box_utils
    pts, boxes = ref['points'], ref['gt_boxes']
    for s in (0, 3):
        flags = box_utils.points_in_boxes3d(dev(np.concatenate([pts[s], np.ones((len(pts[s]), 1), F32)], -1)), dev(boxes[s, :, :9]))
        assert flags.dtype == torch.int64 and flags.is_cuda and flags.shape == (len(pts[s]),)
        np.testing.assert_array_equal(flags.cpu().numpy(), model.points_in_boxes9_scene(pts[s], boxes[s])[0])
        keep = ~ref['band0'][s]
        np.testing.assert_array_equal(flags.cpu().numpy()[keep], ref['flags'][s][keep])
    idx = box_targets.points_in_boxes9(dev(stacked(pts)), dev(boxes), extra_width=ref['extra_width'].tolist())
    np.testing.assert_array_equal(idx.cpu().numpy(), model.points_in_boxes9(stacked(pts), boxes, xyz_col=1, bs_col=0,
                                                                           extra_width=ref['extra_width']))
    large = box_utils.enlarge_box3d(dev(boxes[0]), [0.2, 0.1, 0.3])
    np.testing.assert_array_equal(large.cpu().numpy()[:, 3:6], boxes[0][:, 3:6] + np.array([0.2, 0.1, 0.3], F32))
    with pytest.raises(_lib.Det6dError):
        box_targets.points_in_boxes9(torch.from_numpy(stacked(pts)), dev(boxes))              # host tensor
    with pytest.raises(_lib.Det6dError):
        box_targets.points_in_boxes9(dev(stacked(pts)).double(), dev(boxes))
    with pytest.raises(_lib.Det6dError):
        box_targets.points_in_boxes9(dev(pts), dev(boxes[:2]))                                # scene counts differ


@pytest.fixture(scope="module")
def tiny():
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_targets.yaml')
    return cfg, build_model(cfg, seed=11, device='cuda')


def test_head_methods_on_the_fixture_scenes(ref, tiny):
    head = tiny[1].point_head
    b, n, _ = ref['points'].shape
    rows, boxes = stacked(ref['points']), ref['gt_boxes']
    for ei, extra in enumerate((None, ref['extra_width'].tolist())):
        mask = ref['band%d' % ei]
        assert (mask.reshape(b, n).mean(1) <= CAP).all()
        ret = head.assign_targets_simple(dev(rows), dev(boxes), extra_width=extra, set_ignore_flag=False)
        cls, reg = ret['point_cls_labels'].cpu().numpy(), ret['point_reg_labels'].cpu().numpy()
        _, mcls, mreg = model.assign_targets9(rows, boxes, xyz_col=1, bs_col=0, extra_width=extra, n_cols=3)
        np.testing.assert_array_equal(cls, mcls)
        np.testing.assert_array_equal(reg, mreg)
        keep = ~mask.reshape(-1)
        np.testing.assert_array_equal(cls[keep], ref['simple%d_cls' % ei][keep])
        np.testing.assert_array_equal(reg[keep], ref['simple%d_reg' % ei][keep])
    ret = head.assign_stack_targets_simple(dev(rows), dev(boxes), set_ignore_flag=False)
    np.testing.assert_array_equal(ret['point_cls_labels'].cpu().numpy(), model.assign_targets9(rows, boxes, xyz_col=1, bs_col=0)[1])
    for ri, radius in enumerate(ref['radii'].tolist()):
        mask = ref['mask%d_exempt' % ri]
        assert (mask.reshape(b, n).mean(1) <= CAP).all()
        keep = ~mask.reshape(-1)
        for num_class in (1, 3):
            head.num_class = num_class
            try:
                ret = head.assign_stack_targets_mask(dev(rows), dev(boxes), set_ignore_flag=False, use_ball_constraint=True,
                                                     central_radius=radius)
            finally:
                head.num_class = 1
            cls = ret['point_cls_labels'].cpu().numpy()
            _, mcls, mbox = model.assign_targets9(rows, boxes, xyz_col=1, bs_col=0, class_col=9, num_class=num_class,
                                                  central_radius=radius, n_cols=9)
            assert cls.dtype == np.int64
            np.testing.assert_array_equal(cls, mcls)
            np.testing.assert_array_equal(cls[keep], ref['mask%d_c%d_cls' % (ri, num_class)][keep])
        box, reg = ret['point_box_labels'].cpu().numpy(), ret['point_reg_labels'].cpu().numpy()
        np.testing.assert_array_equal(box, mbox)
        assert reg.shape == (b * n, head.box_coder.code_size) and (reg[mcls <= 0] == 0).all() and (box[mcls <= 0] == 0).all()
        np.testing.assert_array_equal(box[keep], ref['mask%d_c1_box' % ri][keep])
        check_encoded(reg[keep], ref['mask%d_c1_reg' % ri][keep], head.box_coder)


def boxes_around(seed, centres, b, m_real, m):
    """(b, m, 10) ground truth: m_real boxes per scene centred near points of `centres` (b, p, 3), then zero rows"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((b, m, 10), F32)
    for s in range(b):
        bx = random_boxes(rng, m_real, spread=0.5)
        bx[:, :3] += centres[s, rng.choice(centres.shape[1], m_real, replace=False)]
        bx[:, 3:6] *= 2
        gt[s, :m_real] = np.concatenate([bx, np.ones((m_real, 1), F32)], -1)
    return gt


def forward(net, seed, b, n):
    pts = make_batch(seed, b, n)
    flat = np.concatenate([np.repeat(np.arange(b, dtype=F32), n)[:, None], pts.reshape(b * n, -1)], 1).astype(F32)
    bd = {'batch_size': b, 'points': dev(flat)}
    with torch.no_grad():
        pred, _ = net(bd)
    return bd, pred


def model_training_targets(head, cand, vote, gt, radius, extra):
    _, vcls, vreg = model.assign_targets9(cand, gt, xyz_col=1, bs_col=0, extra_width=extra, n_cols=3)
    idx, pcls, pbox = model.assign_targets9(vote, gt, xyz_col=1, bs_col=0, class_col=9, num_class=head.num_class,
                                            central_radius=radius, n_cols=9)
    return vcls, vreg, idx, pcls, pbox


def test_assign_training_targets_of_the_tiny_model(tiny):
    cfg, net = tiny
    head = net.point_head
    b, n = 3, 2048
    bd, _ = forward(net, 31, b, n)
    cand, vote = bd['point_candidate_coords'].cpu().numpy(), bd['point_vote_coords'].cpu().numpy()
    p = len(vote) // b
    gt = boxes_around(32, vote[:, 1:4].reshape(b, p, 3), b, 12, 16)
    bd['gt_boxes'] = dev(gt)
    assert cfg.MODEL.POINT_HEAD.TARGET_CONFIG.GT_CENTRAL_RADIUS == 10.0
    for radius, extra in ((10.0, None), (1.0, [0.2, 0.2, 0.2])):
        head.model_cfg.TARGET_CONFIG.GT_CENTRAL_RADIUS = radius
        if extra is not None:
            head.model_cfg.TARGET_CONFIG.VOTE_EXTRA_WIDTH = extra
        try:
            ret = head.assign_training_targets(bd)
        finally:
            head.model_cfg.TARGET_CONFIG.GT_CENTRAL_RADIUS = 10.0
            head.model_cfg.TARGET_CONFIG.pop('VOTE_EXTRA_WIDTH', None)
        assert sorted(ret) == ['point_box_labels', 'point_cls_labels', 'point_reg_labels', 'vote_cls_labels', 'vote_reg_labels']
        vcls, vreg, idx, pcls, pbox = model_training_targets(head, cand, vote, gt, radius, extra)
        assert (vcls > 0).sum() > 10 and (pcls > 0).sum() > 10
        np.testing.assert_array_equal(ret['vote_cls_labels'].cpu().numpy(), vcls)
        np.testing.assert_array_equal(ret['vote_reg_labels'].cpu().numpy(), vreg)
        np.testing.assert_array_equal(ret['point_cls_labels'].cpu().numpy(), pcls)
        np.testing.assert_array_equal(ret['point_box_labels'].cpu().numpy(), pbox)
        assert ret['vote_cls_labels'].dtype == torch.int64 and ret['vote_reg_labels'].shape == (b * p, 3)
        assert ret['point_reg_labels'].shape == (b * p, head.box_coder.code_size) and ret['point_box_labels'].shape == (b * p, 9)
        # the encoded targets: the coder's own expressions on the CPU, from the model's labels
        fg = (idx >= 0) & (pcls != -1)
        code = head.box_coder.encode_torch(torch.from_numpy(pbox.copy()), torch.from_numpy(vote[:, 1:4].copy())).numpy()
        want = np.where(fg[:, None], code[:, :head.box_coder.code_size], F32(0))
        got = ret['point_reg_labels'].cpu().numpy()
        np.testing.assert_array_equal(got[:, :3], want[:, :3])
        np.testing.assert_array_equal(got != 0, want != 0)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


def test_what_is_out_of_scope_raises(tiny):
    from de6d_amd.runtime import load_config, build_model
    head = tiny[1].point_head
    pts, gt = dev(np.zeros((4, 4), F32)), dev(np.zeros((1, 2, 10), F32))
    with pytest.raises(NotImplementedError):
        head.assign_targets_simple(pts, gt)                                     # set_ignore_flag defaults to True
    with pytest.raises(NotImplementedError):
        head.assign_stack_targets_simple(pts, gt, extend_gt_boxes=gt, set_ignore_flag=True)
    with pytest.raises(NotImplementedError):
        head.assign_stack_targets_mask(pts, gt, set_ignore_flag=True, use_ball_constraint=False)
    with pytest.raises(AssertionError):
        head.assign_stack_targets_mask(pts, gt, set_ignore_flag=False, use_ball_constraint=False)
    head.model_cfg.TARGET_CONFIG.ASSIGN_METHOD = 'iou'
    try:
        with pytest.raises(NotImplementedError, match='iou'):
            head.assign_targets({'point_vote_coords': pts, 'gt_boxes': gt})
    finally:
        head.model_cfg.TARGET_CONFIG.ASSIGN_METHOD = 'mask'
    plain = build_model(load_config('synthetic_models/det6d_tiny.yaml'), seed=11, device='cuda').point_head
    with pytest.raises(KeyError, match='ASSIGN_METHOD'):
        plain.assign_targets({'point_vote_coords': pts, 'gt_boxes': gt})
    head.train()
    try:
        with pytest.raises(NotImplementedError):
            head({'batch_size': 1})
    finally:
        head.eval()


def test_a_captured_graph_replayed_on_new_inputs_equals_eager(tiny):
    _, net = tiny
    head = net.point_head
    b, n, m = 3, 2048, 16
    runs = []
    for j in range(3):
        bd, _ = forward(net, 40 + j, b, n)
        vote = bd['point_vote_coords'].cpu().numpy()
        bd['gt_boxes'] = dev(boxes_around(50 + j, vote[:, 1:4].reshape(b, -1, 3), b, 10 + j, m))
        runs.append({k: bd[k].clone() for k in ('point_candidate_coords', 'point_vote_coords', 'gt_boxes')})
    head.model_cfg.TARGET_CONFIG.VOTE_EXTRA_WIDTH = [0.2, 0.2, 0.2]
    try:
        eager = [{k: v.clone() for k, v in head.assign_training_targets(r).items()} for r in runs]
        static = {k: v.clone() for k, v in runs[0].items()}
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            head.assign_training_targets(static)                                # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = head.assign_training_targets(static)
    finally:
        head.model_cfg.TARGET_CONFIG.pop('VOTE_EXTRA_WIDTH', None)
    for r, want in list(zip(runs, eager))[::-1] + list(zip(runs, eager)):
        for k in static:
            static[k].copy_(r[k])
        graph.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), k
        assert (want['point_cls_labels'] > 0).sum() > 5 and (want['vote_cls_labels'] > 0).sum() > 0


@pytest.mark.parametrize("cfg_name,b,n", [('synthetic_models/det6d_tiny_targets.yaml', 2, 2048),
                                          ('kitti_models/det6d_car_targets.yaml', 1, 16384)])
def test_eval_outputs_are_unchanged_by_the_new_methods(cfg_name, b, n):
    from de6d_amd.runtime import load_config, build_model
    plain = build_model(load_config(cfg_name.replace('_targets', '')), seed=5, device='cuda')
    net = build_model(load_config(cfg_name), seed=5, device='cuda')
    bd0, pred0 = forward(plain, 61, b, n)
    bd1, pred1 = forward(net, 61, b, n)
    before = {k: bd1[k].clone() for k in ('point_candidate_coords', 'point_vote_coords', 'batch_box_preds', 'batch_cls_preds')}
    vote = bd1['point_vote_coords'].cpu().numpy()
    bd1['gt_boxes'] = dev(boxes_around(62, vote[:, 1:4].reshape(b, -1, 3), b, 8, 12))
    ret = net.point_head.assign_training_targets(bd1)
    assert (ret['point_cls_labels'] != 0).any()
    bd2, pred2 = forward(net, 61, b, n)
    for k, v in before.items():
        assert torch.equal(bd1[k], v) and torch.equal(bd2[k], v) and torch.equal(bd0[k], v), k
    for p0, p1, p2 in zip(pred0, pred1, pred2):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(p0[k], p1[k]) and torch.equal(p1[k], p2[k]), k
