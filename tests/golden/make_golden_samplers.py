"""Regenerates tests/golden/samplers_ref.npz: what the reference's c-fps and df-fps branches compute, on CPU torch.

The reference's own PointnetSAModuleFSMSG.forward (core/pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py) runs with
the stubs of make_golden.py (its extension modules replaced, Tensor.cuda() the identity).  Two of its callees are intercepted:
gather_operation receives the picks of a c-fps layer, furthest_point_sample_weights receives the weights of a df-fps layer;
each records its argument and ends the forward pass there.  Nothing of the reference's text is restated here.

  * c-fps: scores.sigmoid() ** gamma then .topk(m).  torch's weights differ from d6_sigmoid_powf in the last bits, so a scene
    qualifies only if every gap between consecutive weights among the top m + 1 exceeds twice the largest model-vs-torch
    difference of that scene.  This is ASSERTED for every scene; none is dropped or truncated.
  * df-fps: the weights of the torch.unique expression for (i) single-scene batches with points outside the range on every
    side, (ii) one batch of 4 scenes whose keys all lie in [0, 1400) (asserted), where per-batch and per-scene counts agree.

    python tests/golden/make_golden_samplers.py            (authoring container only: needs the reference checkout)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.models import pillar_density, score_topk  # noqa: E402

F32 = np.float32
#: (n, m, gamma) x seeds
TOPK_SHAPES = [(4096, 512, 1.0), (1024, 256, 0.5), (512, 256, 2.0)]
TOPK_SEEDS = [102, 103, 106]


class Recorded(Exception):
    pass


def reference_layer():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.install_reference_stubs()
    sys.path.insert(0, mg.REF)
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as ref_modules
    assert ref_modules.__file__.startswith(mg.REF)
    return ref_modules


def run_sampler(ref_modules, method, npoint, gamma, xyz, scores, hook):
    """the reference layer with ONE sampler over the whole cloud, up to the call of `hook` (an attribute of its
    pointnet2_utils), whose arguments are returned"""
    layer = ref_modules.PointnetSAModuleFSMSG(npoint_list=[npoint], sample_range_list=[[0, xyz.shape[1]]],
                                              sample_method_list=[method], radii=[1.0], nsamples=[4], mlps=[[0, 8]],
                                              weight_gamma=gamma)
    seen = {}

    def record(*args):
        seen['args'] = args
        raise Recorded()
    utils = ref_modules.pointnet2_utils
    saved = getattr(utils, hook)
    setattr(utils, hook, record)
    try:
        layer(torch.from_numpy(xyz), None, scores=None if scores is None else torch.from_numpy(scores))
    except Recorded:
        pass
    finally:
        setattr(utils, hook, saved)
    return seen['args']


def gen_topk(ref_modules, out):
    si = 0
    for n, m, gamma in TOPK_SHAPES:
        for seed in TOPK_SEEDS:
            scores = np.random.default_rng(seed).standard_normal(n).astype(F32)
            xyz = np.zeros((1, n, 3), F32)
            _, idx = run_sampler(ref_modules, 'c-fps', m, gamma, xyz, scores[None], 'gather_operation')
            picks = idx[0].numpy().astype(np.int32)
            w_torch = (torch.from_numpy(scores).sigmoid() ** gamma).numpy()
            w_model = score_topk.weights(scores, gamma)
            diff = float(np.abs(w_torch.astype(np.float64) - w_model).max())
            top = np.sort(w_model.astype(np.float64))[::-1][:m + 1]
            gap = float((top[:-1] - top[1:]).min())
            assert gap > 2 * diff, "scene (n=%d, m=%d, gamma=%g, seed=%d) does not qualify: gap %.3g, difference %.3g" % (
                n, m, gamma, seed, gap, diff)
            np.testing.assert_array_equal(picks, score_topk.topk_scores(scores, m, gamma))
            print("c-fps %d: n=%d m=%d gamma=%g seed=%d smallest gap %.3g, model-vs-torch %.3g" % (si, n, m, gamma, seed, gap, diff))
            out['topk_picks%d' % si] = picks
            out['topk_meta%d' % si] = np.array([n, m, seed], np.int32)
            out['topk_gamma%d' % si] = np.array(gamma, F32)
            si += 1
    out['topk_nscenes'] = np.array(si)


def cloud(rng, b, n, xr, yr):
    return np.stack([rng.uniform(*xr, (b, n)), rng.uniform(*yr, (b, n)), rng.uniform(-3, 1, (b, n))], -1).astype(F32)


def gen_pillars(ref_modules, out):
    rng = np.random.default_rng(300)
    # (i) single scenes with points outside the range on every side: x < 0, cx >= 35, negative cy, y past the far edge
    batches = [cloud(rng, 1, 2048, (-12, 84), (-52, 52)), cloud(rng, 1, 1000, (-3, 72), (-41, 41))]
    # dense clusters: counts far above 1
    batches[1][0, :400, :2] = rng.normal([20, 3], 1.5, (400, 2)).astype(F32)
    # (ii) a batch of 4 scenes inside the range: keys in [0, 1400), where counting per batch equals counting per scene
    inside = cloud(rng, 4, 1024, (0.01, 69.9), (-39.6, 39.6))
    k = np.stack([pillar_density.keys(s) for s in inside])
    assert k.min() >= 0 and k.max() < pillar_density.SCALE_XY
    batches.append(inside)
    for bi, xyz in enumerate(batches):
        if xyz.shape[0] == 1:
            k = pillar_density.keys(xyz[0])
            assert k.min() < 0 and k.max() >= pillar_density.SCALE_XY and xyz[0, :, 0].min() < 0
        _, w, m = run_sampler(ref_modules, 'df-fps', 64, 1.0, xyz, None, 'furthest_point_sample_weights')
        w = w.numpy()
        assert w.dtype == np.float32 and w.shape == xyz.shape[:2]
        np.testing.assert_array_equal(w, pillar_density.pillar_weights(xyz))
        print("df-fps %d: %s, counts up to %d" % (bi, xyz.shape, int(round(1 / w.min()))))
        out['pillar_xyz%d' % bi] = xyz
        out['pillar_weights%d' % bi] = w
    out['pillar_nbatches'] = np.array(len(batches))


def main():
    ref_modules = reference_layer()
    out = {}
    gen_topk(ref_modules, out)
    gen_pillars(ref_modules, out)
    np.savez_compressed(os.path.join(HERE, 'samplers_ref.npz'), **out)


if __name__ == '__main__':
    main()
