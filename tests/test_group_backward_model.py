"""The float64 model of the grouped-MLP backward (tests/models/group_backward.py) against torch CPU float64 autograd of the
reference's formulation (pointnet2_modules.py:305-312, point_head_box6d_vote.py:815-821): Conv2d / BatchNorm2d (eval) / ReLU on
cat([xyz[idx] - new_xyz, feat[idx]]), the cnt mask, F.max_pool2d, and the vote clamp as torch.max / torch.min.  No GPU.
Held to 1e-12 relative: both sides are float64, they differ by the order of a few sums."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.models import group_backward as model
from tests.models import mlp_backward as mlp

B, N, M, NS, CF = 2, 24, 5, 8, 4                 # 3 + CF = 7 input channels
WIDTHS = (7, 6, 5)
RANGE = (3.0, 3.0, 2.0)
TOL = 1e-12


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def make_seq(gen):
    mods, pre = [], WIDTHS[0]
    for width in WIDTHS[1:]:
        bn = nn.BatchNorm2d(width)
        bn.weight.data = torch.rand(width, generator=gen, dtype=torch.float64) + 0.5
        bn.bias.data = torch.randn(width, generator=gen, dtype=torch.float64) * 0.3
        bn.running_mean = torch.randn(width, generator=gen, dtype=torch.float64) * 0.2
        bn.running_var = torch.rand(width, generator=gen, dtype=torch.float64) + 0.5
        mods += [nn.Conv2d(pre, width, kernel_size=1, bias=False), bn, nn.ReLU()]
        pre = width
    seq = nn.Sequential(*mods).double().eval()
    for m in seq:
        if isinstance(m, nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=gen, dtype=torch.float64) * 0.6
    return seq


def test_group_and_clamp_against_torch_autograd():
    rng = np.random.default_rng(5)
    gen = torch.Generator().manual_seed(5)
    cnt, idx = model.padded_query(rng, B, N, M, NS, counts=(0, NS, 1, 3))
    assert (cnt == 0).any() and (cnt == NS).any()
    xyz = rng.normal(size=(B, N, 3))
    feat = rng.normal(size=(B, N, CF))
    cand = rng.normal(size=(B * M, 3))
    off = rng.normal(size=(B * M, 3)) * 2.5       # some inside, some outside the range, none on a bound
    assert (np.abs(off) > np.asarray(RANGE)).any() and (np.abs(off) < np.asarray(RANGE)).any()
    g_pooled = rng.normal(size=(B * M, WIDTHS[-1]))
    g_vote = rng.normal(size=(B * M, 3))
    seq = make_seq(gen)

    # ---- the reference's formulation under autograd
    t_off = torch.from_numpy(off).requires_grad_(True)
    r = torch.tensor(RANGE, dtype=torch.float64)
    clamped = torch.max(torch.min(t_off, r), -r)
    new_xyz = (torch.from_numpy(cand) + clamped).view(B, M, 3)
    new_xyz.retain_grad()
    t_idx = torch.from_numpy(idx.astype(np.int64))
    bi = torch.arange(B)[:, None, None]
    grouped_xyz = torch.from_numpy(xyz)[bi, t_idx] - new_xyz[:, :, None, :]              # (B, M, ns, 3)
    grouped = torch.cat([grouped_xyz, torch.from_numpy(feat)[bi, t_idx]], dim=-1).permute(0, 3, 1, 2)   # (B, C, M, ns)
    y = seq(grouped)
    y = y * (torch.from_numpy(cnt) > 0)[:, None, :, None]
    pooled = F.max_pool2d(y, kernel_size=[1, NS]).squeeze(-1).permute(0, 2, 1).reshape(B * M, -1)
    loss = (pooled * torch.from_numpy(g_pooled)).sum() + (new_xyz.view(-1, 3) * torch.from_numpy(g_vote)).sum()
    loss.backward()

    # ---- the model
    pts = np.concatenate([xyz, feat], axis=2)
    layers, params = mlp.fold_sequential64(seq)
    ctr = model.vote_points(off, cand, RANGE).reshape(B, M, 3)
    assert rel(ctr, new_xyz.detach().numpy()) <= TOL
    x0, acts, pooled64 = model.group_forward(pts, idx, cnt, ctr, layers)
    assert rel(pooled64, pooled.detach().numpy()) <= TOL
    d_ctr, grads = model.group_backward(x0, layers, acts, cnt, NS, g_pooled)
    d_vote = d_ctr + g_vote
    assert np.abs(new_xyz.grad.numpy()).max() > 0
    assert rel(d_vote, new_xyz.grad.numpy().reshape(-1, 3)) <= TOL
    d_off = model.vote_backward(off, RANGE, d_vote)
    assert rel(d_off, t_off.grad.numpy()) <= TOL
    assert (d_off == 0).any() and (d_off != 0).any()
    # an empty ball sends nothing to its centre
    empty = cnt.reshape(-1) == 0
    assert not d_ctr[empty].any()
    # every parameter gradient, through the derivative of the fold
    blocks = mlp.blocks_of(seq)
    for (conv, bn, _), (dw, ds), p in zip(blocks, grads, params):
        g = mlp.param_grads(dw, ds, **p)
        assert rel(g['conv_weight'].reshape(conv.weight.shape), conv.weight.grad.numpy()) <= TOL
        assert rel(g['bn_weight'], bn.weight.grad.numpy()) <= TOL
        assert rel(g['bn_bias'], bn.bias.grad.numpy()) <= TOL


def test_the_lowest_slot_wins_a_tie():
    ns, c = 4, 3
    y = np.zeros((2 * ns, c))
    y[:, 0] = [1.0, 5.0, 5.0, 2.0, 0.5, 0.25, 0.5, 0.5]           # two distinct slots hold the positive maximum: 1 and 2; 0, 2, 3
    y[:, 1] = [0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0, 3.0]            # a channel whose maximum is 0 passes nothing
    y[:, 2] = [2.0, 2.0, 2.0, 2.0, 7.0, 1.0, 1.0, 1.0]            # all equal: slot 0
    g = np.array([[10.0, 20.0, 30.0], [40.0, 50.0, 60.0]])
    dz = model.pool_backward(y, np.array([4, 2]), g, ns, c)
    want = np.zeros((2 * ns, c))
    want[1, 0], want[0, 2] = 10.0, 30.0
    want[4, 0], want[5, 1], want[4, 2] = 40.0, 50.0, 60.0
    np.testing.assert_array_equal(dz, want)
    # an empty ball passes nothing, whatever its rows hold
    dz = model.pool_backward(y, np.array([0, 2]), g, ns, c)
    want[:ns] = 0.0
    np.testing.assert_array_equal(dz, want)
    # a slice of a wider d(pooled)
    wide = np.concatenate([np.full((2, 2), -1.0), g], axis=1)
    np.testing.assert_array_equal(model.pool_backward(y, np.array([0, 2]), wide, ns, c, gcol0=2), want)


def test_the_clamp_mask_inside_outside_bound_and_nan():
    off = np.array([[0.0, 2.9, -1.9], [3.5, -3.5, 2.5], [np.nan, 3.0, -2.0], [-3.0, np.nan, 2.0]])
    dv = np.arange(1.0, 13.0).reshape(4, 3)
    want = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.0, 8.0, 9.0], [10.0, 0.0, 12.0]])        # on a bound: the whole gradient
    np.testing.assert_array_equal(model.vote_backward(off, RANGE, dv), want)
    cand = np.ones((4, 3))
    vote = model.vote_points(off, cand, RANGE)
    np.testing.assert_array_equal(vote[1], [4.0, -2.0, 3.0])
    np.testing.assert_array_equal(vote[2], [-2.0, 4.0, -1.0])       # a NaN offset ends on -R, as the kernel's selects do


def test_gather_layout_and_centre_sum():
    rng = np.random.default_rng(1)
    cnt, idx = model.padded_query(rng, 2, 9, 3, 4, counts=(0, 4))
    pts = rng.integers(-4, 5, size=(2, 9, 8)).astype(np.float32)
    ctr = rng.integers(-4, 5, size=(2, 3, 3)).astype(np.float32)
    out = model.group_gather(pts, idx, ctr, k=6, ldout=8)
    assert out.shape == (24, 8) and not out[:, 6:].any()
    r = (1 * 3 + 2) * 4 + 1
    np.testing.assert_array_equal(out[r, :3], pts[1, idx[1, 2, 1], :3] - ctr[1, 2])
    np.testing.assert_array_equal(out[r, 3:6], pts[1, idx[1, 2, 1], 3:6])
    dx = rng.integers(-3, 4, size=(24, 5)).astype(np.float64)
    np.testing.assert_array_equal(model.centre_grad(dx, 4)[2], -dx[8:12, :3].sum(0))
