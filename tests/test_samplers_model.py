"""CPU checks of the c-fps and df-fps models (tests/models/score_topk.py, pillar_density.py): they reproduce what the
reference's branches computed on CPU torch (tests/golden/samplers_ref.npz), the tie rule of the top-k on constructed inputs,
per-scene pillar counting, and the new configs build and route their samplers to the extension library."""
import os

import numpy as np
import pytest
import torch

from tests.models import pillar_density, score_topk

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'samplers_ref.npz')


def golden_scores(n, seed):
    """the scores of a golden c-fps scene (tests/golden/make_golden_samplers.py)"""
    return np.random.default_rng(seed).standard_normal(n).astype(F32)


def tie_cases():
    """(name, weights-or-scores, is_scores, gamma, m, expected picks) of the constructed tie inputs; shared with the GPU test"""
    nan = np.nan
    cases = []
    n, m = 300, 77
    cases.append(('all equal', np.full(n, 0.25, F32), 1.0, m, np.arange(m)))
    s = np.zeros(n, F32)
    s[10:20], s[100:130] = 3.0, 1.0          # 10 highest, then a run of 30 equal straddling the m-th place (m = 25)
    cases.append(('run straddles m', s, 1.0, 25, np.r_[np.arange(10, 20), np.arange(100, 115)]))
    s = np.linspace(-2, 2, n).astype(F32)
    s[[7, 150, 299]] = nan
    cases.append(('nan first', s, 1.0, 6, np.array([7, 150, 299, 298, 297, 296])))
    cases.append(('gamma 0', np.linspace(-3, 3, n).astype(F32), 0.0, m, np.arange(m)))         # every weight is 1
    s = np.full(n, -100.0, F32)
    s[50:60], s[200:205] = 100.0, 0.0        # sigmoid saturates to 1 / 0 on both sides
    cases.append(('saturated', s, 1.0, 20, np.r_[np.arange(50, 60), np.arange(200, 205), np.arange(0, 5)]))
    s = np.random.default_rng(5).integers(-3, 4, n).astype(F32)
    w = score_topk.weights(s, 2.0)
    cases.append(('m = n', s, 2.0, n, np.array(sorted(range(n), key=lambda k: (-float(w[k]), k)))))
    return cases


@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_topk_tie_rule(oracle_ops, case):
    _, scores, gamma, m, want = case
    got = score_topk.topk_scores(scores, m, gamma)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)


def test_topk_rule_on_plain_weights():
    w = np.array([1, np.nan, 3, 3, 2, 3], F32)
    np.testing.assert_array_equal(score_topk.topk_weights(w, 4), [1, 2, 3, 5])
    # ... one of the orders torch.topk may produce: the same values in the same order, the same index set
    vals, idx = torch.from_numpy(w).topk(4)
    np.testing.assert_array_equal(vals.numpy(), w[score_topk.topk_weights(w, 4)])
    assert sorted(idx.tolist()) == [1, 2, 3, 5]
    np.testing.assert_array_equal(score_topk.topk_weights(np.array([0.0, -0.0, 0.0], F32), 3), [0, 1, 2])
    np.testing.assert_array_equal(score_topk.topk_weights(np.array([np.inf, np.nan, -np.inf, np.inf], F32), 4), [1, 0, 3, 2])


def test_topk_model_gives_torchs_picks_on_the_golden_scenes(oracle_ops):
    g = np.load(GOLDEN)
    assert int(g['topk_nscenes']) == 9
    for si in range(int(g['topk_nscenes'])):
        n, m, seed = (int(v) for v in g['topk_meta%d' % si])
        gamma = float(g['topk_gamma%d' % si])
        scores = golden_scores(n, seed)
        np.testing.assert_array_equal(score_topk.topk_scores(scores, m, gamma), g['topk_picks%d' % si], err_msg='scene %d' % si)
        # the scene qualifies: torch's weights cannot reorder the top m + 1
        w = score_topk.weights(scores, gamma)
        diff = np.abs((torch.from_numpy(scores).sigmoid() ** gamma).numpy().astype(np.float64) - w).max()
        top = np.sort(w.astype(np.float64))[::-1][:m + 1]
        assert (top[:-1] - top[1:]).min() > 2 * diff


def test_topk_weights_are_the_s_fps_weights(oracle_ops):
    s = golden_scores(777, 1)
    for gamma in (1.0, 0.5, 2.0):
        assert score_topk.weights(s, gamma).tobytes() == oracle_ops.sigmoid_pow(s, gamma).tobytes()


def test_pillar_model_gives_the_references_weights(oracle_ops):
    g = np.load(GOLDEN)
    assert int(g['pillar_nbatches']) == 3
    outside = 0
    for bi in range(int(g['pillar_nbatches'])):
        xyz, want = g['pillar_xyz%d' % bi], g['pillar_weights%d' % bi]
        got = pillar_density.pillar_weights(xyz)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), 'batch %d' % bi
        k = np.stack([pillar_density.keys(s) for s in xyz])
        if xyz.shape[0] > 1:
            assert k.min() >= 0 and k.max() < pillar_density.SCALE_XY
        else:
            outside += int(k.min() < 0 and k.max() >= pillar_density.SCALE_XY and xyz[..., 0].min() < 0)
    assert outside == 2


def test_pillars_are_counted_per_scene():
    g = np.load(GOLDEN)
    scene = g['pillar_xyz0'][0]            # keys on both sides of [0, 1400): a batch-wide count would mix the two copies
    single = pillar_density.pillar_weights(scene)
    twice = pillar_density.pillar_weights(np.stack([scene, scene]))
    np.testing.assert_array_equal(twice[0], single)
    np.testing.assert_array_equal(twice[1], single)


def test_out_of_range_points_collide_inside_their_scene():
    # key = cx * 40 + cy: (cx, cy) = (0, 45) and (1, 5) share key 45; (0, -1) and (-1, 39) share key -1
    def at(cx, cy):
        return [2.0 * cx + 1.0, -39.68 + 2.0 * cy + 1.0, 0.0]
    xyz = np.array([at(0, 45), at(1, 5), at(1, 5), at(0, -1), at(-1, 39), at(3, 3)], F32)
    np.testing.assert_array_equal(pillar_density.keys(xyz), [45, 45, 45, -1, -1, 123])
    np.testing.assert_array_equal(pillar_density.counts(xyz), [3, 3, 3, 2, 2, 1])
    w = pillar_density.pillar_weights(xyz)
    assert w.tobytes() == (F32(1) / np.array([3, 3, 3, 2, 2, 1], F32)).tobytes()


def test_pillar_edges_follow_fp32():
    # the y origin is the fp32 value of -39.68 and the subtraction is rounded once, in fp32
    y0 = F32(-39.68)
    ys = np.array([y0, np.nextafter(y0, F32(-100)), y0 + F32(2.0), np.nextafter(y0 + F32(2.0), F32(-100))], F32)
    xyz = np.stack([np.full(4, 1.0, F32), ys, np.zeros(4, F32)], 1)
    np.testing.assert_array_equal(pillar_density.keys(xyz), [0, -1, 1, 0])
    xs = np.array([0.0, -0.0, -1e-30, 2.0, np.nextafter(F32(2), F32(0))], F32)
    xyz = np.stack([xs, np.full(5, y0, F32), np.zeros(5, F32)], 1)
    np.testing.assert_array_equal(pillar_density.keys(xyz), [0, 0, -40, 40, 0])


@pytest.mark.parametrize("name,method", [('synthetic_models/det6d_tiny_cfps.yaml', 'c-fps'),
                                         ('synthetic_models/det6d_tiny_dffps.yaml', 'df-fps'),
                                         ('kitti_models/det6d_car_cfps.yaml', 'c-fps'),
                                         ('kitti_models/det6d_car_dffps.yaml', 'df-fps')])
def test_configs_build_and_route_the_sampler_to_the_extension_library(name, method):
    from de6d_amd import _lib
    from de6d_amd.runtime import load_config, build_model, hoist_plan
    base = load_config(name.replace('_cfps', '').replace('_dffps', ''))
    cfg = load_config(name)
    model = build_model(cfg, seed=1)
    sa = model.backbone_3d.SA_modules
    assert [m.sample_method_list for m in sa][:3] == [['d-fps'], [method, 'd-fps'], [method, 'd-fps']]
    assert list(model.state_dict()) == list(build_model(base, seed=1).state_dict())
    # only the d-fps launches are hoisted, as in the base config
    n = base.MODEL.BACKBONE_3D.SA_CONFIG.SAMPLE_RANGE_LIST[0][0][1]
    assert hoist_plan(sa, n) == hoist_plan(build_model(base, seed=1).backbone_3d.SA_modules, n)
    # the layer hands the method to the library (which has no CPU path) instead of refusing it
    layer = sa[1]
    (lo, hi), npoint = layer.sample_range_list[0], layer.npoint_list[0]
    xyz, scores = torch.zeros((1, hi, 3)), torch.zeros((1, hi))
    idx = torch.zeros((1, sum(layer.npoint_list)), dtype=torch.int32)
    with pytest.raises(_lib.Det6dError, match="device tensors"):
        layer._sample_one(xyz, scores, lo, hi, method, npoint, idx, 0)
