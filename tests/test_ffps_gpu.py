"""F-FPS on the GPU (de6d_amd/csrc/ext/fps_features.hip): the sampler and the matrix sampler bit-exact against the CPU model
(tests/models/ffps.py) and the reference's picks (tests/golden/ffps_ref.npz); whole f-fps models bit-exact against
oracle/model.py with the model's f-fps picks; captured passes equal to the eager run."""
import os

import numpy as np
import pytest
import torch

from tests.models import ffps
from tests.util import make_batch

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ffps_ref.npz')


def scenes(seed, b, n, c):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(0, 70.4, (b, n)), rng.uniform(-40, 40, (b, n)), rng.uniform(-3, 1, (b, n))], -1).astype(F32)
    return xyz, np.maximum(rng.standard_normal((b, n, c)), 0).astype(F32)


def run(xyz, feats, m, gamma=1.0, **kw):
    from de6d_amd.ops import ffps as op
    rows = torch.from_numpy(ffps.rows_of(xyz, feats)).cuda()
    out = op.fps_features(rows, feats.shape[-1], m, gamma, **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("n,c,m", [(2048, 16, 512), (4096, 64, 512), (512, 128, 256), (16384, 64, 2048), (1000, 32, 200),
                                   (40, 8, 40), (256, 16, 256)])
def test_sampler_bit_exact_against_the_model(oracle_ops, n, c, m):
    xyz, feats = scenes(n + c, 2, n, c)
    got = run(xyz, feats, m)
    for s in range(2):
        np.testing.assert_array_equal(got[s], ffps.fps_features(xyz[s], feats[s], m), err_msg='scene %d' % s)


def test_duplicates_gamma_and_zero_channels(oracle_ops):
    xyz, feats = scenes(1, 1, 1024, 32)
    xyz[0, 1::2], feats[0, 1::2] = xyz[0, 0::2], feats[0, 0::2]
    for gamma in (0.0, 1.0, 2.5):
        np.testing.assert_array_equal(run(xyz, feats, 300, gamma)[0], ffps.fps_features(xyz[0], feats[0], 300, gamma))
    feats[:] = 0.25
    np.testing.assert_array_equal(run(xyz, feats, 300)[0], ffps.fps_features(xyz[0], feats[0], 300))
    empty = np.zeros((1, 1024, 0), F32)
    np.testing.assert_array_equal(run(xyz, empty, 100)[0], ffps.fps_features(xyz[0], None, 100))


def test_slice_offset_and_bias_into_a_wider_index_buffer(oracle_ops):
    xyz, feats = scenes(2, 3, 1536, 24)
    idx = torch.full((3, 700), -7, dtype=torch.int32, device='cuda')
    run(xyz, feats, 256, lo=512, hi=1536, idx_out=idx, idx_offset=300, idx_bias=1000)
    got = idx.cpu().numpy()
    assert (got[:, :300] == -7).all() and (got[:, 556:] == -7).all()
    for s in range(3):
        want = ffps.fps_features(xyz[s, 512:], feats[s, 512:], 256) + 512 + 1000
        np.testing.assert_array_equal(got[s, 300:556], want)


@pytest.mark.parametrize("b", [1, 80])
def test_batch_sizes(oracle_ops, b):
    xyz, feats = scenes(b, b, 512, 32)
    got = run(xyz, feats, 64)
    for s in range(b):
        np.testing.assert_array_equal(got[s], ffps.fps_features(xyz[s], feats[s], 64), err_msg='scene %d' % s)


def test_matrix_sampler_against_the_model_and_the_reference(oracle_ops):
    from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    g = np.load(GOLDEN)
    mat = g['matrix0']
    n, _, m = (int(v) for v in g['meta0'])
    got = pu.furthest_point_sample_matrix(torch.from_numpy(mat)[None].cuda().contiguous(), m).cpu().numpy()[0]
    np.testing.assert_array_equal(got, g['picks0'])
    rng = np.random.default_rng(4)
    mats = rng.integers(0, 5, (2, 1500, 1500)).astype(F32)      # exact ties everywhere
    got = pu.furthest_point_sample_matrix(torch.from_numpy(mats).cuda(), 300).cpu().numpy()
    for s in range(2):
        np.testing.assert_array_equal(got[s], ffps.fps_matrix(mats[s], 300))


def test_sampler_on_the_golden_scenes(oracle_ops):
    g = np.load(GOLDEN)
    for si in range(int(g['nscenes'])):
        n, c, m = (int(v) for v in g['meta%d' % si])
        got = run(g['xyz%d' % si][None], g['feats%d' % si][None], m, float(g['gamma%d' % si]))[0]
        np.testing.assert_array_equal(got, g['picks%d' % si], err_msg='scene %d' % si)


def flat_points(batch):
    b, n, _ = batch.shape
    bidx = np.repeat(np.arange(b, dtype=np.float32), n)[:, None]
    return np.concatenate([bidx, batch.reshape(b * n, 4)], 1).astype(np.float32)


@pytest.fixture
def oracle_with_ffps(monkeypatch):
    """oracle/model.py's sa_layer with the f-fps picks of the CPU model; everything after the picks is the oracle's own"""
    from oracle import model as omodel
    from oracle import ops
    orig = omodel.sa_layer

    def sa_layer(sd, prefix, spec, xyz, feats, scores=None, new_xyz=None):
        if new_xyz is not None or 'f-fps' not in spec['sample_method_list']:
            return orig(sd, prefix, spec, xyz, feats, scores, new_xyz)
        b, n, _ = xyz.shape
        idx_list = []
        for (lo, hi), method, npoint in zip(spec['sample_range_list'], spec['sample_method_list'], spec['npoint_list']):
            hi = n if hi == -1 else hi
            sl = np.ascontiguousarray(xyz[:, lo:hi])
            if method == 'd-fps':
                idx = ops.fps(sl, npoint)
            elif method == 'f-fps':
                f = feats[:, :, lo:hi].transpose(0, 2, 1)
                idx = np.stack([ffps.fps_features(sl[s], f[s], npoint, spec['gamma']) for s in range(b)])
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


@pytest.mark.parametrize("cfg_name,b,n,seed", [('synthetic_models/det6d_tiny_ffps.yaml', 3, 2048, 21),
                                               ('kitti_models/det6d_car_ffps.yaml', 2, 16384, 22)])
def test_ffps_model_bit_exact_against_the_oracle(oracle_ops, oracle_with_ffps, cfg_name, b, n, seed):
    from de6d_amd.runtime import load_config, build_model
    from tests.test_model_gpu import check
    cfg = load_config(cfg_name)
    model = build_model(cfg, seed=seed, device='cuda')
    pts = flat_points(make_batch(seed, b, n))
    bd = {'batch_size': b, 'points': torch.from_numpy(pts).cuda()}
    with torch.no_grad():
        pred, _ = model(bd)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    ref = oracle_with_ffps.forward(cfg.MODEL, sd, pts, b)
    check(bd, pred, ref, b)


def test_ffps_model_layer_forward_matches_forward_rows(oracle_ops):
    """the channel-major forward() of an f-fps layer samples on the same rows as forward_rows()"""
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_ffps.yaml')
    model = build_model(cfg, seed=3, device='cuda')
    sa = model.backbone_3d.SA_modules[1]
    b, n, c = 2, 1024, sa.in_channels
    xyz, feats = scenes(7, b, n, c)
    x, f = torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda()
    scores = torch.zeros((b, n), device='cuda')
    with torch.no_grad():
        new_xyz, _, _ = sa(x, f.transpose(1, 2).contiguous(), scores=scores)
    (lo, hi), npoint = sa.sample_range_list[0], sa.npoint_list[0]
    hi = n if hi == -1 else hi
    want = np.stack([ffps.fps_features(xyz[s, lo:hi], feats[s, lo:hi], npoint, sa.weight_gamma) for s in range(b)]) + lo
    np.testing.assert_array_equal(new_xyz[:, :npoint].cpu().numpy(), np.take_along_axis(xyz, want[..., None].astype(np.int64), 1))


def test_captured_and_grouped_passes_equal_eager(oracle_ops):
    from de6d_amd.runtime import load_config, build_model, GraphedDet6D, Det6DGroup
    cfg = load_config('synthetic_models/det6d_tiny_ffps.yaml')
    model = build_model(cfg, seed=9, device='cuda')
    b, n, k = 2, 2048, 3
    batches = [torch.from_numpy(flat_points(make_batch(700 + j, b, n))).cuda() for j in range(k)]
    with torch.no_grad():
        eager = [model({'batch_size': b, 'points': pts})[0] for pts in batches]
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
