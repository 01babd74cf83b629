#!/usr/bin/env python
"""Generates the golden fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the authoring container (needs /root/reference and oracle/_ref); the fixtures it
writes are data (inputs + expected outputs) and are what travels to the GPU box.

  nms_ref.npz      (boxes, thr) -> IoU matrices from the reference's OWN iou3d_cpu.cpp (oracle/_ref)
                   + keep lists from the greedy scan of iou3d_nms.cpp:116-132 applied to them
  ref_iou.npz      the same iou3d_cpu.cpp on the inputs of test_oracle_ref.py (IoU matrices) and test_nms_filter.py
                   (IoU > 0 bit masks of every box family, with a digest of its inputs)
  box_coder.npz    (code, points) -> boxes9 from the reference's PointBinResidual6DCoder.decode_torch
                   (core/pcdet/utils/box_coder_utils.py imported standalone)
  producer.npz     raw frames -> ids chosen by the reference's OWN DataProcessor
                   (mask_points_and_boxes_outside_range + sample_points, data_processor.py:78-90,145-178,
                   np.random seeded) in each of its four branches; the parts of the result that do not
                   depend on the generator (in-range set, kept far points, multiplicities) pin the
                   selection rule of det6d_prepare_points
  annos.npz        detections -> KITTI annotation dicts and label-file lines from the reference's OWN
                   KittiDataset / SlopedKittiDataSet.generate_prediction_dicts (+ box_utils, Calibration)
  slope.npz        SlopeAug: (boxes, points, seed) -> sloped boxes / points from the reference's OWN
                   augmentor_utils.random_global_make_slope (plain and smooth) and box_utils.boxes3d_to_corners_3d
  kitti_eval.npz   KITTI / SlopedKITTI evaluator: synthetic label + detection annotations -> per-metric overlaps,
                   precision / recall tables, mAP numbers and the printed report of the reference's OWN
                   eval.py (both copies) executed as plain Python (numba.jit stubbed to the identity; the
                   numba.cuda launch of rotate_iou_gpu_eval replaced by a loop over the reference's own
                   devRotateIoUEval device function)
  extension_api.json  names + positional arities of the reference's two pybind modules (parsed from its *_api.cpp and headers)
  det6d_full.npz, det6d_full_sloped.npz, det6d_full_3class.npz, det6d_full_65536.npz   the same whole-model golden at the
                   FULL widths of BASELINE configs[1] (two scenes), [2], [3] and [4] (one 65536-point scene)
                   (gen_model_full, gen_model_full_other, gen_model_full_65536)
  det6d_tiny.npz   whole-model golden: the reference's Python model code (PointNet2FSMSG,
                   PointHeadBox6DVote, Detector3DTemplate.post_processing; torch-CPU Conv/BN/ReLU)
                   built from tests' tiny config with seeded weights, run on seeded scenes.  Its
                   five extension modules are not buildable here (CUDA), so — as SURVEY.md 8c / A.5
                   describe — they are replaced by the CPU oracle's ops; missing third-party
                   imports irrelevant to the path (easydict, numba, spconv, SharedArray, skimage)
                   are stubbed.  The fixture pins every piece of glue arithmetic and data flow
                   around the ops; the index ops themselves stay unpinned at the reference level.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/core"

from oracle import ops as oops  # noqa: E402
from oracle import ref as oref  # noqa: E402
from tests.util import make_batch, random_boxes  # noqa: E402


# ----------------------------------------------------------------------------- NMS fixtures
def gen_nms():
    out = {}
    cases = [(1, 30.0), (2, 3.0), (63, 12.0), (64, 12.0), (65, 12.0), (256, 25.0), (512, 40.0)]
    for k, spread in cases:
        boxes = random_boxes(100 + k, k, spread=spread)
        if k >= 8:
            boxes[3] = boxes[1]                    # identical boxes
            boxes[5, 3:5] = 0.0                    # zero-area box
            boxes[6] = boxes[2]; boxes[6, 0] += boxes[2, 3]  # touching, same heading
            boxes[7, 6] = 0.0; boxes[7 - 1, 6] = np.pi / 2   # axis aligned / right angle
        iou = oref.boxes_iou_bev_cpu(boxes, boxes)
        out["boxes_%d" % k] = boxes
        out["iou_%d" % k] = iou
        for thr in (0.01, 0.1, 0.7):
            out["keep_%d_%s" % (k, str(thr).replace('.', 'p'))] = oops.nms_from_iou(iou, thr)
    # Round-4 review: 7 sizes x 3 thresholds is a thin pin for a mask kernel.  24 more sets of random size K in [1, 1024]
    # (block-boundary sizes included) in which a third of the boxes are NEAR-THRESHOLD partners of earlier boxes: the same
    # footprint shifted along its heading by d = l (1 - t) / (1 + t) (IoU == t for equal boxes), t one of the three test
    # thresholds, pushed off the threshold by a relative 1e-4 .. 1e-2 either way, some with a small extra yaw.  Only boxes
    # and keep lists are stored (an IoU matrix of K = 1024 is 4 MB); `rmargin_*` records how close to the threshold the
    # reference's own IoUs come (the parity tests' IoU tolerance is 2e-5).
    rng = np.random.default_rng(20261003)
    sizes = [1, 2, 3, 64, 65, 127, 128, 129, 1023, 1024] + [int(v) for v in rng.integers(1, 1025, 14)]
    out["random_sizes"] = np.array(sizes, np.int64)
    for c, k in enumerate(sizes):
        boxes = random_boxes(7000 + c, k, spread=float(rng.uniform(6.0, 60.0)))
        for j in range(1, k):
            if rng.uniform() < 0.34:
                i = int(rng.integers(0, j))
                t = (0.01, 0.1, 0.7)[int(rng.integers(0, 3))]
                eps = float(10.0 ** rng.uniform(-4.0, -2.0)) * (1.0 if rng.uniform() < 0.5 else -1.0)
                length = float(boxes[i, 3])
                d = length * (1.0 - t * (1.0 + eps)) / (1.0 + t * (1.0 + eps))
                boxes[j] = boxes[i]
                boxes[j, 0] += np.float32(d * np.cos(boxes[i, 6]))
                boxes[j, 1] += np.float32(d * np.sin(boxes[i, 6]))
                if rng.uniform() < 0.25:
                    boxes[j, 6] += np.float32(rng.uniform(-0.02, 0.02))
        iou = oref.boxes_iou_bev_cpu(boxes, boxes)
        out["rboxes_%d" % c] = boxes
        off = iou[~np.eye(k, dtype=bool)] if k > 1 else np.zeros(1, np.float32)
        for thr in (0.01, 0.1, 0.7):
            tag = str(thr).replace('.', 'p')
            out["rkeep_%d_%s" % (c, tag)] = oops.nms_from_iou(iou, thr)
            out["rmargin_%d_%s" % (c, tag)] = np.float32(np.abs(off - np.float32(thr)).min())
    np.savez_compressed(os.path.join(HERE, "nms_ref.npz"), **out)
    print("nms_ref.npz", len(out), "arrays")


def gen_ref_iou():
    """ref_iou.npz: the reference's iou3d_cpu.cpp (oracle/_ref) on the inputs of tests/test_oracle_ref.py (IoU matrices) and
    of tests/test_nms_filter.py (per family: which pairs have IoU > 0, as a packed bit mask, and a digest of the inputs)"""
    from tests import test_oracle_ref as t_ref
    from tests import test_nms_filter as t_filter
    out = {}
    for seed, k, spread in t_ref.CASES:
        boxes = random_boxes(seed, k, spread=spread)
        out["boxes_%d" % seed], out["iou_%d" % seed] = boxes, oref.boxes_iou_bev_cpu(boxes, boxes)
    boxes = t_ref.degenerate_boxes()
    out["boxes_degenerate"], out["iou_degenerate"] = boxes, oref.boxes_iou_bev_cpu(boxes, boxes)
    rng = np.random.default_rng(t_filter.SEED)
    for rep in range(t_filter.REPS):
        for f, (name, a, b) in enumerate(t_filter.families(rng)):
            with np.errstate(invalid='ignore'):
                positive = oref.boxes_iou_bev_cpu(a, b) > 0        # NaN > 0 is False, as in the mask kernel's `iou > thresh`
            out["filter_positive_%d_%d" % (rep, f)] = np.packbits(positive.ravel())
            out["filter_digest_%d_%d" % (rep, f)] = np.array(t_filter.inputs_digest(a, b))
    np.savez_compressed(os.path.join(HERE, "ref_iou.npz"), **out)
    print("ref_iou.npz", len(out), "arrays")


# ----------------------------------------------------------------------------- box coder
def gen_box_coder():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_box_coder_utils", os.path.join(REF, "pcdet/utils/box_coder_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(7)
    out = {}
    for name, kw in (("ga", dict(ground_aware=True, minus=False)), ("ga_minus", dict(ground_aware=True, minus=True)),
                     ("plain", dict(ground_aware=False))):
        coder = mod.PointBinResidual6DCoder(use_mean_size=False, angle_bin_num=12, threshold=10, factor=45, **kw)
        code = (rng.normal(size=(400, coder.code_size)) * 1.5).astype(np.float32)
        code[:10, 6:18] = 0.0  # all-equal yaw logits -> argmax 0
        pts = (rng.normal(size=(400, 3)) * 20).astype(np.float32)
        boxes = coder.decode_torch(torch.from_numpy(code), torch.from_numpy(pts)).numpy()
        out["code_" + name], out["pts_" + name], out["boxes_" + name] = code, pts, boxes
    np.savez_compressed(os.path.join(HERE, "box_coder.npz"), **out)
    print("box_coder.npz")


# ----------------------------------------------------------------------------- whole model
def install_reference_stubs():
    class EasyDict(dict):
        def __init__(self, d=None, **kw):
            super().__init__()
            for k, v in dict(d or {}, **kw).items():
                self[k] = v

        def __setitem__(self, k, v):
            if isinstance(v, dict) and not isinstance(v, EasyDict):
                v = EasyDict(v)
            elif isinstance(v, (list, tuple)):
                v = type(v)(EasyDict(x) if isinstance(x, dict) and not isinstance(x, EasyDict) else x for x in v)
            super().__setitem__(k, v)

        __setattr__ = __setitem__

        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("SharedArray")
    mod("easydict", EasyDict=EasyDict)
    ident = lambda *a, **k: (a[0] if a and callable(a[0]) and not k else (lambda f: f))  # noqa: E731
    cuda = mod("numba.cuda", jit=ident, local=types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype)))
    mod("numba", jit=ident, cuda=cuda, njit=ident, prange=range, float32=np.float32, int32=np.int32)
    mod("skimage"); mod("skimage.io"); mod("skimage.transform")

    class _Any(types.ModuleType):
        def __getattr__(self, k):
            return type(k, (), {})
    sys.modules["spconv"] = _Any("spconv")
    sys.modules["spconv.pytorch"] = _Any("spconv.pytorch")
    sys.modules["spconv"].__dict__["pytorch"] = sys.modules["spconv.pytorch"]
    mod("pcdet.version", __version__="ref")

    # ---- the five extension modules: CPU oracle ops behind the reference's pybind signatures ----
    def T(a):
        return a.detach().cpu().numpy()

    def fps(b, n, m, xyz, temp, idx):
        idx.copy_(torch.from_numpy(oops.fps(T(xyz), m))); return 1

    def fpsw(b, n, m, xyz, w, temp, idx):
        idx.copy_(torch.from_numpy(oops.fps_weights(T(xyz), T(w), m))); return 1

    def gather(b, c, n, npoints, points, idx, out):
        out.copy_(torch.from_numpy(oops.gather_points(T(points), T(idx)))); return 1

    def bq(b, n, m, radius, ns, new_xyz, xyz, idx):
        idx.copy_(torch.from_numpy(oops.ball_query(radius, ns, T(xyz), T(new_xyz)))); return 1

    def bqc(b, n, m, radius, ns, new_xyz, xyz, cnt, idx):
        c, i = oops.ball_query_cnt(radius, ns, T(xyz), T(new_xyz))
        cnt.copy_(torch.from_numpy(c)); idx.copy_(torch.from_numpy(i)); return 1

    def bqd(b, n, m, rin, rout, ns, new_xyz, xyz, cnt, idx):
        c, i = oops.ball_query_dilated(rin, rout, ns, T(xyz), T(new_xyz))
        cnt.copy_(torch.from_numpy(c)); idx.copy_(torch.from_numpy(i)); return 1

    def group(b, c, n, npoints, ns, points, idx, out):
        out.copy_(torch.from_numpy(oops.group_points(T(points), T(idx)))); return 1

    def three_nn(b, n, m, unknown, known, d2, idx):
        d, i = oops.three_nn(T(unknown), T(known))
        d2.copy_(torch.from_numpy(d)); idx.copy_(torch.from_numpy(i))

    def three_interp(b, c, m, n, points, idx, w, out):
        out.copy_(torch.from_numpy(oops.three_interpolate(T(points), T(idx), T(w))))

    mod("pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda",
        farthest_point_sampling_wrapper=fps, furthest_point_sampling_weights_wrapper=fpsw,
        gather_points_wrapper=gather, ball_query_wrapper=bq, ball_query_cnt_wrapper=bqc,
        ball_query_dilated_wrapper=bqd, group_points_wrapper=group, three_nn_wrapper=three_nn,
        three_interpolate_wrapper=three_interp)
    mod("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda")

    def nms_gpu(boxes, keep, thr):
        k = oops.nms(T(boxes), thr)
        keep[:len(k)] = torch.from_numpy(k); return len(k)

    def overlap(a, b, out):
        out.copy_(torch.from_numpy(oops.boxes_overlap_bev(T(a), T(b)))); return 1

    def ioubev(a, b, out):
        out.copy_(torch.from_numpy(oops.boxes_iou_bev(T(a), T(b)))); return 1

    mod("pcdet.ops.iou3d_nms.iou3d_nms_cuda", nms_gpu=nms_gpu, boxes_overlap_bev_gpu=overlap,
        boxes_iou_bev_gpu=ioubev, boxes_iou_bev_cpu=ioubev)
    mod("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda")
    mod("pcdet.ops.roipoint_pool3d.roipoint_pool3d_cuda")

    torch.cuda.IntTensor = torch.IntTensor
    torch.cuda.FloatTensor = torch.FloatTensor
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.synchronize = lambda *a, **k: None
    return EasyDict


def gen_model():
    import yaml
    EasyDict = install_reference_stubs()
    sys.path.insert(0, REF)
    import pcdet.models as ref_models  # the REFERENCE's package (REF is first on sys.path)
    assert ref_models.__file__.startswith(REF)

    cfg = yaml.safe_load(open(os.path.join(ROOT, "de6d_amd/cfgs/synthetic_models/det6d_tiny.yaml")))
    # weights come from OUR builder (same parameter names/shapes; checked below) so that the test
    # can rebuild them from the seed instead of shipping a checkpoint
    from de6d_amd.runtime import load_config, build_model
    ours = build_model(load_config('synthetic_models/det6d_tiny.yaml'), seed=2024)
    sd = ours.state_dict()

    class DS(object):
        class_names = cfg['CLASS_NAMES']
        point_feature_encoder = EasyDict(num_point_features=4)
        grid_size = None
        voxel_size = None
        point_cloud_range = np.array(cfg['DATA_CONFIG']['POINT_CLOUD_RANGE'], np.float32)
        depth_downsample_factor = None

    ref = ref_models.build_network(EasyDict(cfg['MODEL']), num_class=1, dataset=DS())
    ref_sd = ref.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), "state-dict key order differs from the reference"
    for k in sd:
        assert ref_sd[k].shape == sd[k].shape, k
    ref.load_state_dict(sd)
    ref.eval()

    b, n, seed = 2, 2048, 300
    batch = make_batch(seed, b, n, tilt=True)
    pts = np.concatenate([np.repeat(np.arange(b, dtype=np.float32), n)[:, None], batch.reshape(b * n, 4)], 1).astype(np.float32)
    bd = {'batch_size': b, 'points': torch.from_numpy(pts)}
    with torch.no_grad():
        pred, _ = ref(bd)
    out = dict(seed=np.int64(2024), scene_seed=np.int64(seed), b=np.int64(b), n=np.int64(n),
               n_state=np.int64(len(sd)), n_params=np.int64(sum(p.numel() for p in ref.parameters())))
    for i, t in enumerate(bd['point_coords_list']):
        out['point_coords_list_%d' % i] = t.numpy()
    for i, t in enumerate(bd['point_scores_list']):
        if t is not None:
            out['point_scores_list_%d' % i] = t.numpy()
    for key in ('point_features', 'point_coords', 'point_candidate_coords', 'point_vote_coords', 'batch_index',
                'batch_cls_preds', 'batch_box_preds', 'point_reg_preds', 'point_cls_scores', 'vote_offsets'):
        out[key] = bd[key].numpy()
    for i, p in enumerate(pred):
        out['pred_boxes_%d' % i] = p['pred_boxes'].numpy()
        out['pred_scores_%d' % i] = p['pred_scores'].numpy()
        out['pred_labels_%d' % i] = p['pred_labels'].numpy()
    np.savez_compressed(os.path.join(HERE, "det6d_tiny.npz"), **out)
    print("det6d_tiny.npz: %d detections" % sum(len(p['pred_scores']) for p in pred))

    # full-size construction facts: parameter count and key list of the reference
    full = yaml.safe_load(open(os.path.join(ROOT, "de6d_amd/cfgs/kitti_models/det6d_car.yaml")))
    ref_full = ref_models.build_network(EasyDict(full['MODEL']), num_class=1, dataset=DS())
    keys = list(ref_full.state_dict().keys())
    shapes = [list(v.shape) for v in ref_full.state_dict().values()]
    import json
    json.dump({"keys": keys, "shapes": shapes, "n_params": int(sum(p.numel() for p in ref_full.parameters()))},
              open(os.path.join(HERE, "det6d_car_state_dict.json"), "w"))
    print("det6d_car_state_dict.json", len(keys), "entries")


# ----------------------------------------------------------------------------- whole model, FULL width
FULL_CASES = (  # name, scene generator, scene seed, tilt
    ('uniform', 'make_batch', 4100, False),
    ('beam', 'beam_batch', 4200, True),
)


def gen_model_full(cfg_rel='kitti_models/det6d_car.yaml', out_name='det6d_full.npz', cases=None, weight_seed=31, n_points=16384):
    """det6d_car.yaml (the benchmarked widths: K up to 1536, twelve stacked layers between the input and the boxes) through
    the REFERENCE's own Python model (pointnet2_backbone.py:199-263, point_head_box6d_vote.py:794-903,
    detector3d_template.py:178-284; torch-CPU Conv/BN/ReLU), one 16384-point scene per case, the oracle's ops behind the
    extension-module names as in gen_model().  Stores what pins the north star at this width: the sampled point sets of
    all three levels, the confidence scores that drive S-FPS, the candidate / vote points, box codes, decoded boxes, class
    logits and the kept detections.  Inputs and weights are regenerated from seeds by the tests (nothing of the reference
    travels)."""
    import yaml
    EasyDict = install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pcdet.models as ref_models
    assert ref_models.__file__.startswith(REF)
    from tests import util as tutil
    from de6d_amd.runtime import load_config, build_model
    cfg = yaml.safe_load(open(os.path.join(ROOT, "de6d_amd/cfgs", cfg_rel)))
    cases = FULL_CASES if cases is None else cases
    ours = build_model(load_config(cfg_rel), seed=weight_seed)
    sd = ours.state_dict()

    class DS(object):
        class_names = cfg['CLASS_NAMES']
        point_feature_encoder = EasyDict(num_point_features=4)
        grid_size = None
        voxel_size = None
        point_cloud_range = np.array(cfg['DATA_CONFIG']['POINT_CLOUD_RANGE'], np.float32)
        depth_downsample_factor = None

    ref = ref_models.build_network(EasyDict(cfg['MODEL']), num_class=len(cfg['CLASS_NAMES']), dataset=DS())
    assert list(ref.state_dict().keys()) == list(sd.keys())
    ref.load_state_dict(sd)
    ref.eval()
    out = dict(weight_seed=np.int64(weight_seed), n=np.int64(n_points), cases=np.array([c[0] for c in cases]), cfg=np.array(cfg_rel))
    for name, gen, seed, tilt in cases:
        b, n = 1, n_points
        batch = getattr(tutil, gen)(seed, b, n, tilt=tilt)
        pts = np.concatenate([np.repeat(np.arange(b, dtype=np.float32), n)[:, None], batch.reshape(b * n, 4)], 1).astype(np.float32)
        bd = {'batch_size': b, 'points': torch.from_numpy(pts)}
        with torch.no_grad():
            pred, _ = ref(bd)
        out[name + '_scene_seed'] = np.int64(seed)
        out[name + '_tilt'] = np.int64(tilt)
        out[name + '_generator'] = np.array(gen)
        for i, t in enumerate(bd['point_coords_list']):
            out['%s_point_coords_list_%d' % (name, i)] = t.numpy()[:, 1:]
        for i, t in enumerate(bd['point_scores_list']):
            if t is not None:
                out['%s_point_scores_list_%d' % (name, i)] = t.numpy()
        for key in ('point_candidate_coords', 'point_vote_coords', 'batch_cls_preds', 'batch_box_preds', 'point_reg_preds',
                    'vote_offsets'):
            out[name + '_' + key] = bd[key].numpy()
        # 512-wide features: keep a strided sample (the whole tensor is 0.5 MB per case)
        fstride = 8 if n_points <= 16384 else 32          # (key name kept from the first fixture; the stride travels beside it)
        out['features_stride'] = np.int64(fstride)
        out[name + '_point_features_s8'] = bd['point_features'].numpy()[:, ::fstride]
        p = pred[0]
        out[name + '_pred_boxes'] = p['pred_boxes'].numpy()
        out[name + '_pred_scores'] = p['pred_scores'].numpy()
        out[name + '_pred_labels'] = p['pred_labels'].numpy()
        print("%s %s: %d detections, labels %s" % (out_name, name, len(p['pred_scores']), np.unique(p['pred_labels'].numpy())))
    np.savez_compressed(os.path.join(HERE, out_name), **out)
    print(out_name, os.path.getsize(os.path.join(HERE, out_name)), "bytes")


def gen_model_full_other():
    """the same pin for the other two model configurations of BASELINE.json at their full widths: configs[2] SlopedKITTI Car
    (ground-aware pitch branch of the box coder and the head, on a tilted ray-cast scene) and configs[3] KITTI 3-class (three
    class logits per candidate, per-class anchors) — det6d_full_sloped.npz / det6d_full_3class.npz"""
    gen_model_full('slopedkitti_models/det6d_car.yaml', 'det6d_full_sloped.npz', (('beam', 'beam_batch', 4300, True),), weight_seed=37)
    gen_model_full('kitti_models/det6d_3class.yaml', 'det6d_full_3class.npz', (('beam', 'beam_batch', 4400, False),), weight_seed=41)


def gen_model_full_65536():
    """BASELINE configs[4]: one 65536-point scene through the reference's Python model (16384 / 2048+2048 / 1024+1024 sampled
    points: the sizes the cooperative sampler and the large-cloud ball query serve) — det6d_full_65536.npz"""
    gen_model_full('synthetic_models/det6d_65536.yaml', 'det6d_full_65536.npz', (('uniform', 'make_batch', 4500, False),), weight_seed=43,
                   n_points=65536)


# ----------------------------------------------------------------------------- feature propagation, boxes_iou3d_gpu
from tests.golden.fp_config import FP_BACKBONE  # noqa: E402


def gen_fp():
    """fp.npz: (a) the reference's PointNet2FSMSG WITH feature propagation (pointnet2_backbone.py:178-191,249-255 ->
    PointnetFPModule.forward, pointnet2_modules.py:144-174: three_nn, inverse-distance weights, three_interpolate,
    cat with the skip features, shared Conv2d/BN/ReLU) on a seeded 2 x 2048 scene, torch-CPU math, oracle ops behind the
    extension names; (b) the reference's boxes_iou3d_gpu (iou3d_nms_utils.py:48-81) on seeded boxes."""
    EasyDict = install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pcdet.models.backbones_3d.pointnet2_backbone import PointNet2FSMSG as RefBackbone
    from pcdet.ops.iou3d_nms import iou3d_nms_utils as ref_iou
    import pcdet
    assert pcdet.__file__.startswith(REF)
    from de6d_amd.pcdet.models.backbones_3d.pointnet2_backbone import PointNet2FSMSG as OurBackbone
    from de6d_amd.pcdet.config import EasyDict as OurEasyDict
    from de6d_amd.runtime import randomize_bn_stats
    torch.manual_seed(77)
    ours = OurBackbone(OurEasyDict(FP_BACKBONE), input_channels=4)
    with torch.no_grad():
        randomize_bn_stats(ours)
    sd = ours.state_dict()
    ref = RefBackbone(EasyDict(FP_BACKBONE), input_channels=4)
    assert list(ref.state_dict().keys()) == list(sd.keys())
    ref.load_state_dict(sd)
    ref.eval()
    b, n, seed = 2, 2048, 910
    batch = make_batch(seed, b, n)
    pts = np.concatenate([np.repeat(np.arange(b, dtype=np.float32), n)[:, None], batch.reshape(b * n, 4)], 1).astype(np.float32)
    bd = {'batch_size': b, 'points': torch.from_numpy(pts)}
    with torch.no_grad():
        bd = ref(bd)
    out = dict(weight_seed=np.int64(77), scene_seed=np.int64(seed), b=np.int64(b), n=np.int64(n),
               point_features=bd['point_features'].numpy(), point_coords=bd['point_coords'].numpy(),
               num_point_features=np.int64(ref.num_point_features))
    for i, t in enumerate(bd['point_coords_list']):
        out['point_coords_list_%d' % i] = t.numpy()
    # stand-alone module: 3 known points or fewer than 3 distinct ones, no skip features
    from pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import PointnetFPModule as RefFP
    from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import PointnetFPModule as OurFP
    torch.manual_seed(78)
    ofp = OurFP(mlp=[12, 20, 8])
    with torch.no_grad():
        randomize_bn_stats(ofp)
    rfp = RefFP(mlp=[12, 20, 8])
    rfp.load_state_dict(ofp.state_dict())
    rfp.eval()
    rng = np.random.default_rng(5)
    unknown = rng.uniform(-3, 3, (2, 300, 3)).astype(np.float32)
    known = rng.uniform(-3, 3, (2, 40, 3)).astype(np.float32)
    known[1, 5] = known[1, 4]                      # duplicate known points: equal distances
    unknown[0, 7] = known[0, 3]                    # an unknown point ON a known one: dist 0, weight ~ 1
    kf = rng.normal(size=(2, 12, 40)).astype(np.float32)
    with torch.no_grad():
        y = rfp(torch.from_numpy(unknown), torch.from_numpy(known), None, torch.from_numpy(kf))
    out.update(fp_unknown=unknown, fp_known=known, fp_known_feats=kf, fp_out=y.numpy(), fp_seed=np.int64(78))
    boxes_a = random_boxes(31, 40, spread=12.0)
    boxes_b = random_boxes(32, 50, spread=12.0)
    boxes_b[:5] = boxes_a[:5]
    boxes_b[5, 2] += 10.0                          # no height overlap
    out.update(iou3d_a=boxes_a, iou3d_b=boxes_b,
               iou3d=ref_iou.boxes_iou3d_gpu(torch.from_numpy(boxes_a), torch.from_numpy(boxes_b)).numpy(),
               iou_bev=ref_iou.boxes_iou_bev(torch.from_numpy(boxes_a), torch.from_numpy(boxes_b)).numpy())
    np.savez_compressed(os.path.join(HERE, "fp.npz"), **out)
    print("fp.npz", os.path.getsize(os.path.join(HERE, "fp.npz")), "bytes; features", out['point_features'].shape)


# ----------------------------------------------------------------------------- input producer
def producer_frame(seed, n, x_hi=80.0):
    """(n, 4) frame [x, y, z, id]: the last column is a unique id so rows can be traced"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, x_hi, n), rng.uniform(-50, 50, n), rng.uniform(-3, 1, n),
                     np.arange(n)], 1).astype(np.float32)


PRODUCER_CASES = {  # name: (frame seed, raw points, x upper bound, NUM_POINTS)
    'keep_far': (1, 3000, 55.0, 1500),     # N < n_in and N > n_far: all far + random near
    'any_subset': (2, 3000, 80.0, 600),    # N <= n_far: random subset of everything
    'pad_once': (3, 1500, 80.0, 1400),     # n_in <= N <= 2 n_in: duplicates drawn without replacement
    'pad_many': (4, 400, 80.0, 1024),      # N > 2 n_in: duplicates drawn with replacement
}


def gen_producer():
    EasyDict = install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pcdet.datasets.processor.data_processor import DataProcessor
    pc_range = np.array([0, -40, -3, 70.4, 40, 1], np.float32)
    out = {'point_cloud_range': pc_range}
    for name, (seed, n, x_hi, num_points) in PRODUCER_CASES.items():
        cfgs = [EasyDict(NAME='mask_points_and_boxes_outside_range', REMOVE_OUTSIDE_BOXES=True),
                EasyDict(NAME='sample_points', NUM_POINTS=EasyDict(train=num_points, test=num_points)),
                EasyDict(NAME='shuffle_points', SHUFFLE_ENABLED=EasyDict(train=True, test=False))]
        dp = DataProcessor(cfgs, point_cloud_range=pc_range, training=False, num_point_features=4)
        frame = producer_frame(seed, n, x_hi)
        np.random.seed(1000 + seed)
        res = dp.forward({'points': frame.copy()})['points']
        assert res.shape == (num_points, 4)
        ids = res[:, 3].astype(np.int64)
        assert np.array_equal(res, frame[ids])
        masked = dp.mask_points_and_boxes_outside_range({'points': frame.copy()}, config=cfgs[0])['points']
        in_ids = masked[:, 3].astype(np.int64)
        depth = np.linalg.norm(masked[:, 0:3], axis=1)
        n_in, n_far = len(in_ids), int((depth >= 40.0).sum())
        branch = ('keep_far' if num_points > n_far else 'any_subset') if num_points < n_in else \
                 ('pad_many' if num_points - n_in > n_in else 'pad_once')
        assert branch == name, (name, branch, n_in, n_far)
        out[name + '_frame'] = frame
        out[name + '_num_points'] = np.int64(num_points)
        out[name + '_in_ids'] = in_ids
        out[name + '_far_ids'] = in_ids[depth >= 40.0]
        out[name + '_chosen_ids'] = ids
    np.savez_compressed(os.path.join(HERE, "producer.npz"), **out)
    print("producer.npz", {k: PRODUCER_CASES[k][3] for k in PRODUCER_CASES})


# ----------------------------------------------------------------------------- output consumer
def kitti_calib(seed):
    """a KITTI-like calibration (values of the order of sequence 0000xx), slightly perturbed per seed"""
    rng = np.random.default_rng(seed)
    P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]], np.float32)
    R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
                   [0.007402527, 0.004351614, 0.9999631]], np.float32)
    V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                    [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float32)
    P2[:, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
    V2C[:, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
    return {'P2': P2, 'R0': R0, 'Tr_velo2cam': V2C, 'P3': P2.copy()}


def annos_inputs():
    frames = []
    for i, k in enumerate((37, 0, 5)):
        rng = np.random.default_rng(500 + i)
        boxes = random_boxes(600 + i, max(k, 1), spread=30.0)[:k]
        boxes[:, 0] = np.abs(boxes[:, 0]) + 4.0           # in front of the camera
        pitch = np.where(rng.uniform(size=k) < 0.5, 0.0, -rng.uniform(0.17, 0.4, k))
        b9 = np.concatenate([boxes, pitch[:, None], np.zeros((k, 1))], 1).astype(np.float32)
        frames.append(dict(boxes=b9, scores=rng.uniform(0.1, 1.0, k).astype(np.float32),
                           labels=rng.integers(1, 4, k).astype(np.int64), calib=kitti_calib(i),
                           image_shape=np.array([375 - i, 1242 - 2 * i], np.int32), frame_id='%06d' % (7 + i)))
    return frames


def gen_annos():
    import tempfile
    from pathlib import Path
    install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pcdet.datasets.kitti.kitti_dataset import KittiDataset
    from pcdet.datasets.slopedkitti.kitti_dataset import SlopedKittiDataset
    from pcdet.utils.calibration_kitti import Calibration
    names = ['Car', 'Pedestrian', 'Cyclist']
    frames = annos_inputs()
    out = {'n_frames': np.int64(len(frames))}
    for tag, cls, ncol in (('kitti', KittiDataset, 7), ('sloped', SlopedKittiDataset, 9)):
        batch = {'frame_id': [f['frame_id'] for f in frames], 'calib': [Calibration(f['calib']) for f in frames],
                 'image_shape': torch.from_numpy(np.stack([f['image_shape'] for f in frames]))}
        preds = [{'pred_boxes': torch.from_numpy(f['boxes'][:, :ncol].copy()), 'pred_scores': torch.from_numpy(f['scores']),
                  'pred_labels': torch.from_numpy(f['labels'])} for f in frames]
        with tempfile.TemporaryDirectory() as tmp:
            annos = cls.generate_prediction_dicts(batch, preds, names, output_path=Path(tmp))
            for i, (f, a) in enumerate(zip(frames, annos)):
                for key in ('alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'boxes_lidar', 'pitch', 'roll'):
                    if key in a:
                        out['%s_%d_%s' % (tag, i, key)] = np.asarray(a[key])
                out['%s_%d_name' % (tag, i)] = np.asarray(a['name']).astype('U16')
                out['%s_%d_txt' % (tag, i)] = np.array(open(os.path.join(tmp, f['frame_id'] + '.txt')).read())
    for i, f in enumerate(frames):
        for key in ('boxes', 'scores', 'labels', 'image_shape'):
            out['in_%d_%s' % (i, key)] = f[key]
        for key in ('P2', 'R0', 'Tr_velo2cam'):
            out['in_%d_%s' % (i, key)] = f['calib'][key]
        out['in_%d_frame_id' % i] = np.array(f['frame_id'])
    np.savez_compressed(os.path.join(HERE, "annos.npz"), **out)
    print("annos.npz", len(out), "arrays")


# ----------------------------------------------------------------------------- SlopeAug
def gen_slope():
    install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pcdet.datasets.augmentor import augmentor_utils as ref_aug
    from pcdet.utils import box_utils as ref_box
    from tests.util import make_scene
    out = {}
    params = (20.0, 10.0, *np.deg2rad([20.0, 8.0]))
    out['params'] = np.array(params)
    for case, (seed, smooth) in enumerate(((1, False), (2, False), (3, True), (4, True))):
        points = make_scene(700 + case, 2048)
        boxes = random_boxes(800 + case, 24, spread=35.0).astype(np.float32)
        boxes[:, 0] = np.abs(boxes[:, 0]) + 2.0
        np.random.seed(seed)
        gt, pts, pivot, angle = ref_aug.random_global_make_slope(boxes.copy(), points.copy(), params=params, smooth=smooth)
        out['in_%d_points' % case], out['in_%d_boxes' % case] = points, boxes
        out['in_%d_seed' % case], out['in_%d_smooth' % case] = np.int64(seed), np.bool_(smooth)
        out['out_%d_points' % case], out['out_%d_boxes' % case] = pts, gt
        out['out_%d_pivot' % case], out['out_%d_angle' % case] = np.asarray(pivot), np.asarray(angle)
        out['out_%d_corners' % case] = ref_box.boxes3d_to_corners_3d(gt.copy())
    np.savez_compressed(os.path.join(HERE, "slope.npz"), **out)
    print("slope.npz", len(out), "arrays; moved points per case:",
          [int((out['out_%d_points' % c] != out['in_%d_points' % c]).any(1).sum()) for c in range(4)])


# ----------------------------------------------------------------------------- evaluator
def eval_annos(n_frames=12, seed=4242):
    """synthetic split: ground-truth annos (float64, as kitti_common loads them) and detection annos
    (float32, as generate_prediction_dicts writes them) in camera coordinates"""
    rng = np.random.default_rng(seed)
    names = np.array(['Car', 'Pedestrian', 'Cyclist', 'Van', 'DontCare', 'Person_sitting'])
    size = {'Car': (3.9, 1.5, 1.6), 'Van': (4.8, 2.0, 1.9), 'Pedestrian': (0.8, 1.75, 0.6), 'Cyclist': (1.8, 1.7, 0.6),
            'Person_sitting': (0.8, 1.2, 0.6), 'DontCare': (-1, -1, -1)}
    gts, dts = [], []
    for f in range(n_frames):
        k = int(rng.integers(0 if f == 3 else 3, 9))
        nm = names[rng.choice(len(names), k, p=[0.45, 0.15, 0.12, 0.1, 0.1, 0.08])]
        loc = np.stack([rng.uniform(-12, 12, k), rng.uniform(1.4, 1.9, k), rng.uniform(6, 45, k)], 1)
        dims = np.array([size[n] for n in nm]).reshape(k, 3) * rng.uniform(0.9, 1.1, (k, 1))
        ry = rng.uniform(-np.pi, np.pi, k)
        h_img = 720.0 * dims[:, 1] / loc[:, 2]
        u = 620 + 720 * loc[:, 0] / loc[:, 2]
        v = 180 + 720 * (loc[:, 1] - dims[:, 1] / 2) / loc[:, 2]
        w_img = h_img * rng.uniform(0.8, 2.0, k)
        bbox = np.stack([u - w_img / 2, v - h_img / 2, u + w_img / 2, v + h_img / 2], 1)
        gt = dict(name=nm, truncated=rng.choice([0.0, 0.1, 0.25, 0.6], k), occluded=rng.integers(0, 4, k),
                  alpha=-np.arctan2(loc[:, 0], loc[:, 2]) + ry, bbox=bbox, dimensions=dims, location=loc, rotation_y=ry,
                  pitch=np.where(rng.uniform(size=k) < 0.5, 0.0, -rng.uniform(0.17, 0.4, k)), roll=np.zeros(k),
                  score=np.zeros(k))
        dc = nm == 'DontCare'
        gt['dimensions'][dc] = -1; gt['location'][dc] = -1000; gt['rotation_y'][dc] = -10; gt['alpha'][dc] = -10
        gts.append(gt)
        # detections: noisy copies of most real objects + a few false alarms
        keep = (~dc) & (rng.uniform(size=k) < 0.85)
        m, fa = int(keep.sum()), int(rng.integers(0, 4))
        jit = lambda a, s: a + rng.normal(0, s, a.shape)   # noqa: E731
        d_loc = np.concatenate([jit(loc[keep], 0.12), np.stack([rng.uniform(-12, 12, fa), rng.uniform(1.4, 1.9, fa), rng.uniform(6, 45, fa)], 1)])
        d_dims = np.concatenate([dims[keep] * rng.uniform(0.93, 1.07, (m, 3)), np.tile(size['Car'], (fa, 1))])
        d_ry = np.concatenate([jit(ry[keep], 0.08), rng.uniform(-np.pi, np.pi, fa)])
        d_bbox = np.concatenate([jit(bbox[keep], 2.0), np.stack([rng.uniform(0, 900, fa), rng.uniform(100, 200, fa)], 1).repeat(2, 1)
                                 + np.array([0, 0, 60, 45.0])])
        d_name = np.concatenate([np.where(nm[keep] == 'Van', 'Car', np.where(nm[keep] == 'Person_sitting', 'Pedestrian', nm[keep])),
                                 rng.choice(['Car', 'Pedestrian', 'Cyclist'], fa)])
        if fa and dc.any():                                   # a false alarm sitting on a DontCare region
            d_bbox[m] = bbox[dc][0] + np.array([1.0, 1.0, -1.0, -1.0]); d_name[m] = 'Car'
        n_dt = m + fa
        dt = dict(name=d_name, truncated=np.zeros(n_dt), occluded=np.zeros(n_dt),
                  alpha=(-np.arctan2(d_loc[:, 0], d_loc[:, 2]) + d_ry).astype(np.float32), bbox=d_bbox.astype(np.float32),
                  dimensions=d_dims.astype(np.float32), location=d_loc.astype(np.float32), rotation_y=d_ry.astype(np.float32),
                  pitch=np.concatenate([jit(gt['pitch'][keep], 0.03), np.zeros(fa)]).astype(np.float32),
                  roll=np.zeros(n_dt, np.float32),
                  score=np.concatenate([rng.uniform(0.35, 1.0, m), rng.uniform(0.05, 0.6, fa)]).astype(np.float32))
        dts.append(dt)
    return gts, dts


def gen_eval():
    import copy
    import importlib
    install_reference_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    out = {}
    gts, dts = eval_annos()
    for tag, pkg in (('kitti', 'pcdet.datasets.kitti.kitti_object_eval_python'),
                     ('sloped', 'pcdet.datasets.slopedkitti.kitti_object_eval_python')):
        ev = importlib.import_module(pkg + '.eval')
        riou = importlib.import_module(pkg + '.rotate_iou')

        def rotate_iou_loop(boxes, query_boxes, criterion=-1, device_id=0, _r=riou):
            # host half of rotate_iou_gpu_eval (rotate_iou.py:302-330) with the kernel launch replaced by a
            # loop over the reference's own device function, same (query, box) argument order as :297-299
            b32, q32 = boxes.astype(np.float32), query_boxes.astype(np.float32)
            iou = np.zeros((b32.shape[0], q32.shape[0]), np.float32)
            for n in range(b32.shape[0]):
                for k in range(q32.shape[0]):
                    iou[n, k] = _r.devRotateIoUEval(q32[k], b32[n], criterion)
            return iou.astype(boxes.dtype)

        ev.rotate_iou_gpu_eval = rotate_iou_loop
        detail = {}
        g, d = copy.deepcopy(gts), copy.deepcopy(dts)
        fn = ev.get_official_eval_result if tag == 'kitti' else ev.get_slopedkitti_eval_result
        text, ret = fn(g, d, ['Car', 'Pedestrian', 'Cyclist'], PR_detail_dict=detail)
        out[tag + '_report'] = np.array(text)
        out[tag + '_ret_keys'] = np.array(sorted(ret))
        out[tag + '_ret_vals'] = np.array([ret[k] for k in sorted(ret)])
        for key, val in detail.items():
            out['%s_precision_%s' % (tag, key)] = val
        for metric in range(3 if tag == 'kitti' else 4):
            ov = ev.calculate_iou_partly(copy.deepcopy(dts), copy.deepcopy(gts), metric, 100)[0]
            for f, block in enumerate(ov):
                out['%s_overlap_m%d_f%d' % (tag, metric, f)] = np.asarray(block)
        print(tag, 'report:\n' + text[:600])
    for f, (g, d) in enumerate(zip(gts, dts)):
        for key, val in g.items():
            out['gt_%d_%s' % (f, key)] = np.asarray(val) if key != 'name' else np.asarray(val).astype('U16')
        for key, val in d.items():
            out['dt_%d_%s' % (f, key)] = np.asarray(val) if key != 'name' else np.asarray(val).astype('U16')
    out['n_frames'] = np.int64(len(gts))
    np.savez_compressed(os.path.join(HERE, "kitti_eval.npz"), **out)
    print("kitti_eval.npz", len(out), "arrays")


# ----------------------------------------------------------------------------- extension API
def gen_extension_api():
    """extension_api.json: what the reference's two pybind modules export — python name -> positional arity — parsed from
    pointnet2_api.cpp:11-30 / iou3d_nms_api.cpp:11-17 (the m.def lines) and the C++ prototypes they bind
    (sampling_gpu.h:9-39, ball_query_gpu.h:9-25, group_points_gpu.h, interpolate_gpu.h, gridify.h, iou3d_nms.h:9-12,
    iou3d_cpu.h).  tests/test_boundary.py holds de6d_amd's drop-in modules to exactly these names and arities."""
    import json
    import re

    def strip_comments(text):
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        return re.sub(r'//[^\n]*', '', text)

    def prototypes(paths):
        protos = {}
        for path in paths:
            text = strip_comments(open(path).read())
            for ret, name, args in re.findall(r'\b(int|void)\s+(\w+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S):
                args = args.strip()
                # split on top-level commas (std::vector<float> has none inside, but stay general)
                depth, parts, cur = 0, [], ''
                for ch in args:
                    depth += ch == '<'
                    depth -= ch == '>'
                    if ch == ',' and depth == 0:
                        parts.append(cur); cur = ''
                    else:
                        cur += ch
                if cur.strip():
                    parts.append(cur)
                protos[name] = dict(returns=ret, arity=len(parts), args=[' '.join(a.split()) for a in parts])
        return protos

    def module(api_cpp, headers):
        protos = prototypes(headers)
        out = {}
        for pyname, cname in re.findall(r'm\.def\(\s*"(\w+)"\s*,\s*&(\w+)', strip_comments(open(api_cpp).read())):
            out[pyname] = dict(binds=cname, **protos[cname])
        return out

    pn = os.path.join(REF, 'pcdet/ops/pointnet2/pointnet2_batch/src')
    iou = os.path.join(REF, 'pcdet/ops/iou3d_nms/src')
    api = {
        'pointnet2_batch_cuda': module(os.path.join(pn, 'pointnet2_api.cpp'),
                                       [os.path.join(pn, h) for h in ('sampling_gpu.h', 'ball_query_gpu.h', 'group_points_gpu.h',
                                                                      'interpolate_gpu.h', 'gridify.h')]),
        'iou3d_nms_cuda': module(os.path.join(iou, 'iou3d_nms_api.cpp'), [os.path.join(iou, h) for h in ('iou3d_nms.h', 'iou3d_cpu.h')]),
        'import_sites': {
            'pointnet2_batch_cuda': 'pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda',   # pointnet2_utils.py:7
            'iou3d_nms_cuda': 'pcdet.ops.iou3d_nms.iou3d_nms_cuda',                              # iou3d_nms_utils.py:9
        },
    }
    with open(os.path.join(HERE, 'extension_api.json'), 'w') as f:
        json.dump(api, f, indent=1, sort_keys=True)
    print('extension_api.json', {k: len(v) for k, v in api.items()})


if __name__ == "__main__":
    if sys.argv[1:] == ['extension_api']:          # needs neither the oracle nor oracle/_ref
        gen_extension_api()
        sys.exit(0)
    oops.build()
    assert oref.available(), "build oracle/_ref first: make -C oracle _ref"
    gens = dict(nms=gen_nms, ref_iou=gen_ref_iou, box_coder=gen_box_coder, model=gen_model, producer=gen_producer, annos=gen_annos,
                slope=gen_slope, eval=gen_eval, model_full=gen_model_full, model_full_other=gen_model_full_other, model_full_65536=gen_model_full_65536, fp=gen_fp,
                extension_api=gen_extension_api)
    for name in (sys.argv[1:] or list(gens)):      # `python make_golden.py model_full` regenerates one fixture
        gens[name]()
