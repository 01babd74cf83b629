"""Regenerates tests/golden/targets_ref.npz: what the reference's point-in-box test and target assignment compute.

The reference's OWN box_utils.points_in_boxes3d (a scipy Delaunay hull test per box on float64 corners) and the OWN
assign_targets_simple / assign_targets of its PointHeadBox6DVote run on CPU torch under the stubs of make_golden.py, on one
generated batch; inputs and outputs are stored.  Nothing of the reference's text is restated here.

The engine decides membership from fp32 local coordinates, the reference from a float64 hull walk: they may differ only for a
point within rounding distance of a face.  The generator therefore stores, per configuration, a mask of EXEMPT points:
  * band: for some box that takes part, the point is within BAND = 1e-4 m of one of its face planes while within 1e-3 m of the
    box along the other two axes (float64, rotation from scipy);
  * ball: the point lies in a box and | |p - c| - central_radius | < 1e-4 m (the reference compares an fp32 norm with the
    radius, the engine a float64 sum of squares with its square).
At most CAP = 0.1 % of the points of any scene may be exempt (asserted), and the coverage that keeps the cap honest is
asserted too: >= 20 % of every scene's points inside a box, >= 100 points inside more than one box, a scene with zero-padded
box rows, pitch up to +-0.5 rad and roll up to +-0.3 rad, >= 5 % of in-box points outside the ball of radius 1.0, yaw away
from every bin edge and pitch away from the ground threshold by 1e-4 rad (the one-hot parts of the encoded targets are exact).

    python tests/golden/make_golden_targets.py            (authoring container only: needs the reference checkout)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

F32 = np.float32
B, N, M = 4, 4096, 32
PADDED_SCENE, PADDED_REAL = 3, 20            # scene 3: 20 boxes and 12 all-zero rows
RADII = (1.0, 2.0, 10.0)
EXTRAS = (None, (0.2, 0.2, 0.2))
BAND, NEAR, CAP = 1e-4, 1e-3, 1e-3
CODER = dict(angle_bin_num=12, use_mean_size=False, ground_aware=True, minus=False, threshold=10, factor=45)


def reference():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    easydict = mg.install_reference_stubs()
    sys.path.insert(0, mg.REF)
    from pcdet.models.dense_heads.point_head_box6d_vote import PointHeadBox6DVote as RefHead
    from pcdet.utils import box_coder_utils as ref_coders
    from pcdet.utils import box_utils as ref_box_utils
    assert ref_box_utils.__file__.startswith(mg.REF)
    return easydict, RefHead, ref_coders, ref_box_utils


def ref_head(easydict, RefHead, ref_coders, num_class, radius):
    """the reference head without its layers: only what its assignment methods read"""
    head = RefHead.__new__(RefHead)
    torch.nn.Module.__init__(head)
    head.num_class = num_class
    head.box_coder = ref_coders.PointBinResidual6DCoder(**CODER)
    head.model_cfg = easydict(TARGET_CONFIG=dict(ASSIGN_METHOD='mask', GT_CENTRAL_RADIUS=radius))
    return head


def scene(rng, real, overlap):
    from scipy.spatial.transform import Rotation
    ctr = np.stack([rng.uniform(2, 68, real), rng.uniform(-38, 38, real), rng.uniform(-3, 1, real)], -1)
    if overlap:
        ctr[real // 2:] = ctr[:real - real // 2] + rng.uniform(-1, 1, (real - real // 2, 3))
    dims = np.stack([rng.uniform(0.5, 5, real), rng.uniform(0.4, 2.2, real), rng.uniform(0.8, 2, real)], -1)
    per_bin = 2 * np.pi / CODER['angle_bin_num']
    thr = np.deg2rad(CODER['threshold'])
    while True:                                   # yaw off the bin edges, pitch off the ground threshold
        ang = np.stack([rng.uniform(-np.pi, np.pi, real), rng.uniform(-0.5, 0.5, real), rng.uniform(-0.3, 0.3, real)], -1)
        ang32 = ang.astype(F32).astype(np.float64)
        edge = np.abs((np.mod(ang32[:, 0], 2 * np.pi) / per_bin - 0.5) - np.round(np.mod(ang32[:, 0], 2 * np.pi) / per_bin - 0.5))
        if (edge * per_bin >= 1e-4).all() and (np.abs(np.abs(ang32[:, 1]) - thr) >= 1e-4).all():
            break
    cls = rng.integers(1, 4, real).astype(np.float64)
    boxes = np.zeros((M, 10), F32)
    boxes[:real] = np.concatenate([ctr, dims, ang, cls[:, None]], -1).astype(F32)
    k = rng.integers(0, real, N)
    loc = rng.uniform(-0.75, 0.75, (N, 3)) * dims[k]
    rot = Rotation.from_euler('zyx', ang[k]).as_matrix()
    pts = (np.einsum('nij,nj->ni', rot, loc) + ctr[k]).astype(F32)
    return pts, boxes


def membership64(pts, boxes, extra):
    """float64 geometry of one scene -> (count of boxes containing each point, band mask)"""
    from scipy.spatial.transform import Rotation
    p = pts.astype(np.float64)
    count = np.zeros(len(p), np.int64)
    band = np.zeros(len(p), bool)
    e = np.zeros(3) if extra is None else np.asarray(extra, np.float64)
    for bx in boxes.astype(np.float64):
        w = (bx[3:6].astype(F32) + e.astype(F32)).astype(np.float64)       # the enlarged sizes are fp32 values in both
        if not (w > 0).all():
            continue
        rot = Rotation.from_euler('zyx', bx[6:9]).as_matrix()
        margin = w / 2 - np.abs((p - bx[:3]) @ rot)
        count += (margin >= 0).all(1)
        close = margin > -NEAR
        for k in range(3):
            others = [j for j in range(3) if j != k]
            band |= (np.abs(margin[:, k]) < BAND) & close[:, others].all(1)
    return count, band


def main():
    easydict, RefHead, ref_coders, ref_box_utils = reference()
    rng = np.random.default_rng(20261016)
    pts, boxes = zip(*[scene(rng, PADDED_REAL if s == PADDED_SCENE else M, s % 2 == 1) for s in range(B)])
    pts, boxes = np.stack(pts), np.stack(boxes)
    assert (boxes[PADDED_SCENE, PADDED_REAL:] == 0).all()
    assert np.abs(boxes[..., 7]).max() > 0.45 and np.abs(boxes[..., 8]).max() > 0.25
    stacked = np.concatenate([np.repeat(np.arange(B, dtype=F32), N)[:, None], pts.reshape(-1, 3)], -1)
    out = {'points': pts, 'gt_boxes': boxes, 'radii': np.array(RADII, F32), 'extra_width': np.array(EXTRAS[1], F32),
           'coder_angle_bin_num': np.array(CODER['angle_bin_num']), 'coder_threshold': np.array(CODER['threshold']),
           'coder_factor': np.array(CODER['factor'])}
    t_pts, t_boxes = torch.from_numpy(stacked), torch.from_numpy(boxes)

    # the hull test itself, scene by scene, and the coverage / band masks
    flags = np.stack([ref_box_utils.points_in_boxes3d(pts[s], boxes[s, :, :9]) for s in range(B)]).astype(np.int32)
    out['flags'] = flags
    multi = 0
    for ei, extra in enumerate(EXTRAS):
        band = np.zeros((B, N), bool)
        for s in range(B):
            count, band[s] = membership64(pts[s], boxes[s], extra)
            if extra is None:
                assert (count > 0).mean() >= 0.20, "scene %d: only %.1f %% of the points inside a box" % (s, 100 * (count > 0).mean())
                multi += int((count > 1).sum())
                assert (((count > 0) != (flags[s] >= 0)) & ~band[s]).sum() == 0
        out['band%d' % ei] = band
        print("extra_width %s: points in the band per scene %s" % (extra, band.sum(1)))
    assert multi >= 100, multi
    print("points inside more than one box:", multi, "; inside a box: %.1f %%" % (100 * (flags >= 0).mean()))

    # vote targets: assign_targets_simple for both widths
    head = ref_head(easydict, RefHead, ref_coders, 1, 2.0)
    for ei, extra in enumerate(EXTRAS):
        ret = head.assign_targets_simple(points=t_pts, gt_boxes=t_boxes.clone(),
                                         extra_width=None if extra is None else list(extra), set_ignore_flag=False)
        out['simple%d_cls' % ei] = ret['point_cls_labels'].numpy().astype(np.int64)
        out['simple%d_reg' % ei] = ret['point_reg_labels'].numpy().astype(F32)
        exempt = out['band%d' % ei]
        assert (exempt.mean(1) <= CAP).all(), exempt.sum(1)
    assert ((out['simple0_cls'].reshape(B, N) > 0) == (flags >= 0)).all()

    # head targets: assign_targets (mask + ball) for every radius, class-agnostic and with three classes
    centre = boxes[np.arange(B)[:, None], np.maximum(flags, 0), :3].astype(np.float64)
    dist = np.linalg.norm(pts.astype(np.float64) - centre, axis=-1)
    for ri, radius in enumerate(RADII):
        ball = (flags >= 0) & (np.abs(dist - radius) < BAND)
        exempt = out['band0'] | ball
        assert (exempt.mean(1) <= CAP).all(), exempt.sum(1)
        out['mask%d_exempt' % ri] = exempt
        for num_class in (1, 3):
            head = ref_head(easydict, RefHead, ref_coders, num_class, radius)
            ret = head.assign_targets({'point_vote_coords': t_pts, 'gt_boxes': t_boxes.clone()})
            cls = ret['point_cls_labels'].numpy().astype(np.int64)
            tag = 'mask%d_c%d' % (ri, num_class)
            out[tag + '_cls'] = cls
            if num_class == 1:
                out[tag + '_reg'] = ret['point_reg_labels'].numpy().astype(F32)
                out[tag + '_box'] = ret['point_box_labels'].numpy().astype(F32)
                assert out[tag + '_reg'].shape == (B * N, head.box_coder.code_size) and out[tag + '_box'].shape == (B * N, 9)
        cls = out['mask%d_c1_cls' % ri]
        print("radius %g: foreground %d, ignored %d, exempt per scene %s" % (radius, (cls > 0).sum(), (cls < 0).sum(), exempt.sum(1)))
        if radius == 1.0:
            assert (cls < 0).sum() >= 0.05 * (cls != 0).sum()
    np.savez_compressed(os.path.join(HERE, 'targets_ref.npz'), **out)
    print("targets_ref.npz: %d bytes" % os.path.getsize(os.path.join(HERE, 'targets_ref.npz')))


if __name__ == '__main__':
    main()
