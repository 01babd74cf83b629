"""c-fps and df-fps on the GPU (de6d_amd/csrc/ext/sort_samplers.hip), bit-exact everywhere: the top-k against the CPU model
(tests/models/score_topk.py), the constructed tie / NaN inputs and torch's picks (tests/golden/samplers_ref.npz); the pillar
weights against the model (tests/models/pillar_density.py) and the reference's weights; df-fps picks against the oracle's
weighted FPS; whole c-fps / df-fps models against oracle/model.py with the models' picks; captured passes equal to eager."""
import os

import numpy as np
import pytest
import torch

from tests.models import pillar_density, score_topk
from tests.test_samplers_model import golden_scores, tie_cases
from tests.util import make_batch

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'samplers_ref.npz')


def topk(scores, m, gamma=1.0, **kw):
    from de6d_amd.ops import sort_samplers as op
    return op.topk_scores(torch.from_numpy(np.ascontiguousarray(scores, F32)).cuda(), m, gamma, **kw).cpu().numpy()


def weights_of(xyz, **kw):
    from de6d_amd.ops import sort_samplers as op
    return op.pillar_weights(torch.from_numpy(np.ascontiguousarray(xyz, F32)).cuda(), **kw).cpu().numpy()


def clouds(seed, b, n, spread=1.0):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(35 - 47 * spread, 35 + 47 * spread, (b, n)), rng.uniform(-52 * spread, 52 * spread, (b, n)),
                    rng.uniform(-3, 1, (b, n))], -1).astype(F32)
    xyz[:, : n // 4, :2] = rng.normal([20, 3], 2.0, (b, n // 4, 2)).astype(F32)          # a dense cluster: long runs
    return xyz


# ---- c-fps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("b", [1, 8, 80])
@pytest.mark.parametrize("n,m", [(512, 256), (4096, 512), (16384, 2048), (16384, 16384), (1000, 77)])
def test_topk_bit_exact_against_the_model(oracle_ops, n, m, b, gamma):
    scores = np.random.default_rng(n + m + b).standard_normal((b, n)).astype(F32)
    scores[:, ::7] = np.round(scores[:, ::7])                 # exact ties among the weights
    got = topk(scores, m, gamma)
    assert got.dtype == np.int32 and got.shape == (b, m)
    for s in range(b):
        np.testing.assert_array_equal(got[s], score_topk.topk_scores(scores[s], m, gamma), err_msg='scene %d' % s)


@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_topk_tie_rule(oracle_ops, case):
    _, scores, gamma, m, want = case
    np.testing.assert_array_equal(topk(scores[None], m, gamma)[0], want)
    np.testing.assert_array_equal(want, score_topk.topk_scores(scores, m, gamma))


def test_topk_slice_offset_and_bias_into_a_wider_index_buffer(oracle_ops):
    scores = np.random.default_rng(2).standard_normal((3, 1536)).astype(F32)
    scores[:, 600:900] = 0.5
    idx = torch.full((3, 700), -7, dtype=torch.int32, device='cuda')
    topk(scores, 256, 0.5, lo=512, hi=1536, idx_out=idx, idx_offset=300, idx_bias=1000)
    got = idx.cpu().numpy()
    assert (got[:, :300] == -7).all() and (got[:, 556:] == -7).all()
    for s in range(3):
        np.testing.assert_array_equal(got[s, 300:556], score_topk.topk_scores(scores[s, 512:], 256, 0.5) + 512 + 1000)
    got = topk(scores, 100, 1.0, lo=37, hi=1000)
    for s in range(3):
        np.testing.assert_array_equal(got[s], score_topk.topk_scores(scores[s, 37:1000], 100) + 37)


def test_topk_gives_torchs_picks_on_the_golden_scenes(oracle_ops):
    g = np.load(GOLDEN)
    for si in range(int(g['topk_nscenes'])):
        n, m, seed = (int(v) for v in g['topk_meta%d' % si])
        got = topk(golden_scores(n, seed)[None], m, float(g['topk_gamma%d' % si]))[0]
        np.testing.assert_array_equal(got, g['topk_picks%d' % si], err_msg='scene %d' % si)


# ---- df-fps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", [(1, 512), (8, 4096), (80, 1000), (2, 16384), (3, 40)])
def test_pillar_weights_bit_exact_against_the_model(b, n):
    xyz = clouds(b + n, b, n)
    got = weights_of(xyz)
    assert got.dtype == np.float32 and got.shape == (b, n)
    assert got.tobytes() == pillar_density.pillar_weights(xyz).tobytes()


def test_pillar_weights_of_one_pillar_and_of_a_slice():
    xyz = clouds(9, 2, 16384, spread=0.0)
    xyz[..., 0], xyz[..., 1] = 11.0, 1.0                                # every point in one pillar: one run of 16384
    assert (weights_of(xyz) == F32(1) / F32(16384)).all()
    xyz = clouds(10, 3, 1536)
    got = weights_of(xyz, lo=512, hi=1536)
    assert got.tobytes() == pillar_density.pillar_weights(np.ascontiguousarray(xyz[:, 512:])).tobytes()
    got = weights_of(xyz, lo=100, hi=700)
    assert got.tobytes() == pillar_density.pillar_weights(np.ascontiguousarray(xyz[:, 100:700])).tobytes()


def test_pillar_weights_are_the_references_on_the_golden_batches():
    g = np.load(GOLDEN)
    for bi in range(int(g['pillar_nbatches'])):
        assert weights_of(g['pillar_xyz%d' % bi]).tobytes() == g['pillar_weights%d' % bi].tobytes(), 'batch %d' % bi
    scene = g['pillar_xyz0'][0]                        # per scene: two copies in one batch give the single-scene weights twice
    twice = weights_of(np.stack([scene, scene]))
    assert twice[0].tobytes() == twice[1].tobytes() == g['pillar_weights0'][0].tobytes()


@pytest.mark.parametrize("b,n,m", [(2, 4096, 512), (3, 512, 256), (1, 16384, 1024)])
def test_df_fps_picks_against_the_oracle(oracle_ops, b, n, m):
    from de6d_amd.ops import sort_samplers as op
    xyz = clouds(b + n + m, b, n, spread=0.8)
    got = op.pillar_density_fps(torch.from_numpy(xyz).cuda(), m).cpu().numpy()
    np.testing.assert_array_equal(got, pillar_density.df_fps(xyz, m))
    idx = torch.full((b, m + 9), -7, dtype=torch.int32, device='cuda')
    lo, hi, k = n // 4, n, m // 2
    op.pillar_density_fps(torch.from_numpy(xyz).cuda(), k, lo, hi, idx, 5)
    got = idx.cpu().numpy()
    assert (got[:, :5] == -7).all() and (got[:, 5 + k:] == -7).all()
    np.testing.assert_array_equal(got[:, 5:5 + k], pillar_density.df_fps(xyz[:, lo:hi], k) + lo)


# ---- whole models --------------------------------------------------------------------------------------------------------
def flat_points(batch):
    b, n, _ = batch.shape
    bidx = np.repeat(np.arange(b, dtype=np.float32), n)[:, None]
    return np.concatenate([bidx, batch.reshape(b * n, 4)], 1).astype(np.float32)


@pytest.fixture
def oracle_with_samplers(monkeypatch):
    """oracle/model.py's sa_layer with the c-fps / df-fps picks of the CPU models; everything after the picks is the oracle's"""
    from oracle import model as omodel
    from oracle import ops
    orig = omodel.sa_layer

    def sa_layer(sd, prefix, spec, xyz, feats, scores=None, new_xyz=None):
        if new_xyz is not None or not {'c-fps', 'df-fps'} & set(spec['sample_method_list']):
            return orig(sd, prefix, spec, xyz, feats, scores, new_xyz)
        b, n, _ = xyz.shape
        idx_list = []
        for (lo, hi), method, npoint in zip(spec['sample_range_list'], spec['sample_method_list'], spec['npoint_list']):
            hi = n if hi == -1 else hi
            sl = np.ascontiguousarray(xyz[:, lo:hi])
            if method == 'd-fps':
                idx = ops.fps(sl, npoint)
            elif method == 'c-fps':
                idx = np.stack([score_topk.topk_scores(scores[s, lo:hi], npoint, spec['gamma']) for s in range(b)])
            elif method == 'df-fps':
                idx = pillar_density.df_fps(sl, npoint)
            else:
                raise NotImplementedError(method)
            idx_list.append(idx + lo)
        sample_idx = np.concatenate(idx_list, axis=-1).astype(np.int32)
        nx = ops.gather_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), sample_idx).transpose(0, 2, 1)
        out = orig(sd, prefix, spec, xyz, feats, scores, np.ascontiguousarray(nx))
        out[3]['sample_idx'] = sample_idx
        return out
    monkeypatch.setattr(omodel, 'sa_layer', sa_layer)
    return omodel


@pytest.mark.parametrize("cfg_name,b,n,seed", [('synthetic_models/det6d_tiny_cfps.yaml', 3, 2048, 21),
                                               ('synthetic_models/det6d_tiny_dffps.yaml', 3, 2048, 22),
                                               ('kitti_models/det6d_car_cfps.yaml', 2, 16384, 23),
                                               ('kitti_models/det6d_car_dffps.yaml', 2, 16384, 24)])
def test_model_bit_exact_against_the_oracle(oracle_ops, oracle_with_samplers, cfg_name, b, n, seed):
    from de6d_amd.runtime import load_config, build_model
    from tests.test_model_gpu import check
    cfg = load_config(cfg_name)
    model = build_model(cfg, seed=seed, device='cuda')
    pts = flat_points(make_batch(seed, b, n))
    bd = {'batch_size': b, 'points': torch.from_numpy(pts).cuda()}
    with torch.no_grad():
        pred, _ = model(bd)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    ref = oracle_with_samplers.forward(cfg.MODEL, sd, pts, b)
    check(bd, pred, ref, b)


@pytest.mark.parametrize("cfg_name", ['synthetic_models/det6d_tiny_cfps.yaml', 'synthetic_models/det6d_tiny_dffps.yaml'])
def test_layer_forward_matches_the_models(oracle_ops, cfg_name):
    """the channel-major forward() of a c-fps / df-fps layer takes the same picks as the rows path"""
    from de6d_amd.runtime import load_config, build_model
    model = build_model(load_config(cfg_name), seed=3, device='cuda')
    sa = model.backbone_3d.SA_modules[1]
    b, n, c = 2, 1024, sa.in_channels
    rng = np.random.default_rng(7)
    xyz = clouds(7, b, n, spread=0.7)
    feats = np.maximum(rng.standard_normal((b, n, c)), 0).astype(F32)
    scores = rng.standard_normal((b, n)).astype(F32)
    with torch.no_grad():
        new_xyz, _, _ = sa(torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda().transpose(1, 2).contiguous(),
                           scores=torch.from_numpy(scores).cuda())
    (lo, hi), npoint, method = sa.sample_range_list[0], sa.npoint_list[0], sa.sample_method_list[0]
    hi = n if hi == -1 else hi
    if method == 'c-fps':
        want = np.stack([score_topk.topk_scores(scores[s, lo:hi], npoint, sa.weight_gamma) for s in range(b)]) + lo
    else:
        want = pillar_density.df_fps(xyz[:, lo:hi], npoint) + lo
    np.testing.assert_array_equal(new_xyz[:, :npoint].cpu().numpy(), np.take_along_axis(xyz, want[..., None].astype(np.int64), 1))


@pytest.mark.parametrize("cfg_name", ['kitti_models/det6d_car_cfps.yaml', 'kitti_models/det6d_car_dffps.yaml'])
def test_captured_and_grouped_passes_equal_eager(oracle_ops, cfg_name):
    from de6d_amd.runtime import load_config, build_model, GraphedDet6D, Det6DGroup
    model = build_model(load_config(cfg_name), seed=9, device='cuda')
    b, n, k = 2, 16384, 3
    batches = [torch.from_numpy(flat_points(make_batch(700 + j, b, n))).cuda() for j in range(k)]
    with torch.no_grad():
        eager = [model({'batch_size': b, 'points': pts})[0] for pts in batches]
    assert sum(len(p['pred_scores']) for want in eager for p in want) > 0
    runner = GraphedDet6D(model, b, n)
    for pts, want in zip(batches, eager):
        for g, e in zip(runner.launch(pts).finalize(), want):
            assert torch.equal(g['pred_boxes'], e['pred_boxes']) and torch.equal(g['pred_scores'], e['pred_scores'])
    group = Det6DGroup(model, b, n, k, torch.cuda.Stream(priority=-1))
    for r, pts in zip(group.runners, batches):
        r.points.copy_(pts)
    torch.cuda.synchronize()
    for r, want in zip(group.launch(count=k), eager):
        for g, e in zip(r.finalize(), want):
            assert torch.equal(g['pred_boxes'], e['pred_boxes']) and torch.equal(g['pred_scores'], e['pred_scores'])
