"""The grouped-MLP backward on the GPU (de6d_amd/csrc/ext/group_backward.hip and the layers above it) against the float64 model
(tests/models/group_backward.py): the four kernels alone (exact: they do no arithmetic beyond one subtract and one ordered
sum), bit-identical repeats of a whole grouped chain, the tiny model's whole-head gradients against a float64 CPU replay, the
step from a captured graph, and the data-parallel all-reduce.

Bounds.  group_gather, pool_backward and vote_backward EQUAL the model on the same fp32 inputs.  centre_grad: exact on small
integers; on random floats |got - truth64| <= (ns + 2) * 2^-24 * sum_s |dx| per element, the bound of an fp32 sum of ns terms.
The tiny model: DESIGN.md §5 "Truth and bounds": err = max|T - T64| / max|T64| per tensor, held to 4 x the error of the same
replay in fp32 on the CPU, floored at 16 * 2^-24.  Every test prints its largest ratio to its bound (pytest -s) before it
asserts."""
import copy

import numpy as np
import pytest
import torch

from tests.models import group_backward as model

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
SENTINEL = 7777.0
B, N = 2, 40
SHAPES = ((4, 1), (7, 3), (67, 96), (36, 100))                           # (k gathered input width, c pooled width)
RANGE = (3.0, 3.0, 2.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def round4(v):
    return (v + 3) // 4 * 4


def query(rng, m, ns):
    """empty, single-hit, partial and full balls first, the rest random"""
    return model.padded_query(rng, B, N, m, ns, counts=(0, 1, max(ns // 2, 1), ns, ns))


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (1, 6, 16, 32))
@pytest.mark.parametrize("m", (1, 5, 33))
def test_gather_and_pool_backward_equal_the_model(m, ns):
    from de6d_amd.ops import group_backward as op
    rng = np.random.default_rng(m * 100 + ns)
    cnt, idx = query(rng, m, ns)
    rows, groups = B * m * ns, B * m
    ctr = np.full((B, m, 4), SENTINEL, F32)
    ctr[..., :3] = rng.normal(size=(B, m, 3)).astype(F32)
    for k, c in SHAPES:
        # gather: 16-byte route (rows of a multiple of four floats) and the scalar route (an odd row length)
        for ldp in (round4(k) + 4, k + 2 + (k & 1)):
            pts = np.full((B, N, ldp), SENTINEL, F32)
            pts[..., :k] = rng.normal(size=(B, N, k)).astype(F32)
            ldout = round4(k) + 4
            out = torch.full((rows + 1, ldout), SENTINEL, dtype=torch.float32, device='cuda')
            op.group_gather(dev(pts), dev(idx), dev(ctr), k=k, out=out[:rows])
            got = out.cpu().numpy()
            want = model.group_gather(pts, idx, ctr, k=k, ldout=ldout)
            np.testing.assert_array_equal(got[:rows].astype(np.float64), want, err_msg='gather k=%d ldp=%d' % (k, ldp))
            assert (got[rows] == SENTINEL).all() and not got[:rows, k:].any()
        # pool_backward: Y as a function of the hit (padding slots repeat a hit's bits), a ReLU output with exact zeros; the
        # first group is the empty ball, the last one carries the designed cases whatever the draw
        table = np.maximum(rng.normal(size=(B, N, c)), 0.0).astype(F32)
        r0, lo = (groups - 1) * ns, (ns - 1) // 2
        for ldy, lddz, ldg, gcol0 in ((round4(c) + 4, round4(c) + 4, round4(c) + 8, 4), (c + 3, c + 1, c + 5, 3)):
            y = np.full((rows, ldy), SENTINEL, F32)
            y[:, :c] = table[np.arange(B)[:, None, None], idx].reshape(rows, c)
            if ns >= 2:
                y[r0:r0 + ns, 0] = 0.25
                y[r0 + lo, 0] = y[r0 + ns - 1, 0] = 9.0                      # two distinct slots hold the positive maximum
            if c > 1:
                y[r0:r0 + ns, c - 1] = -np.arange(ns, dtype=F32)              # an all-non-positive channel (maximum 0 at slot 0)
            cnt_case = cnt.copy()
            cnt_case.reshape(-1)[-1] = ns                                     # the designed group is a full ball
            assert cnt_case.reshape(-1)[0] == 0
            g = np.full((groups, ldg), SENTINEL, F32)
            g[:, gcol0:gcol0 + c] = rng.normal(size=(groups, c)).astype(F32) + 3.0
            dz = torch.full((rows, lddz), SENTINEL, dtype=torch.float32, device='cuda')
            op.pool_backward(dev(y), dev(cnt_case), dev(g), ns, c, gcol0=gcol0, dz=dz)
            got = dz.cpu().numpy()
            want = model.pool_backward(y, cnt_case, g, ns, c, gcol0=gcol0)
            np.testing.assert_array_equal(got[:, :c].astype(np.float64), want, err_msg='pool c=%d ldy=%d' % (c, ldy))
            assert (got[:, c:] == SENTINEL).all()
            assert not got[:ns, :c].any()                                     # the empty ball passes nothing
            if ns >= 2:
                assert got[r0 + lo, 0] == g[-1, gcol0] and got[r0 + ns - 1, 0] == 0   # the lowest slot won
            if c > 1:
                assert not got[r0:r0 + ns, c - 1].any()
    print('group_backward kernels m=%d ns=%d: gather and pool_backward equal the model' % (m, ns))


@pytest.mark.parametrize("ns", (1, 6, 16, 32))
@pytest.mark.parametrize("m", (1, 5, 33))
def test_centre_grad_and_vote_backward(m, ns):
    from de6d_amd.ops import group_backward as op
    rng = np.random.default_rng(m * 7 + ns)
    rows, groups = B * m * ns, B * m
    worst = 0.0
    for integers in (True, False):
        dx = np.full((rows, 5), SENTINEL, F32)
        dx[:, :3] = rng.integers(-3, 4, size=(rows, 3)).astype(F32) if integers else rng.normal(size=(rows, 3)).astype(F32)
        out = torch.full((groups, 4), SENTINEL, dtype=torch.float32, device='cuda')
        op.centre_grad(dev(dx), ns, out=out)
        got = out.cpu().numpy()
        assert (got[:, 3] == SENTINEL).all()
        want = model.centre_grad(dx, ns)
        if integers:
            np.testing.assert_array_equal(got[:, :3].astype(np.float64), want)
        else:
            lim = (ns + 2) * U * np.abs(dx[:, :3].astype(np.float64)).reshape(groups, ns, 3).sum(1)
            err = np.abs(got[:, :3].astype(np.float64) - want)
            worst = float((err / np.maximum(lim, 1e-300)).max())
            print('group_backward centre_grad m=%d ns=%d: largest ratio to the bound %.4f' % (m, ns, worst))
            assert np.isfinite(got[:, :3]).all() and (err <= lim).all(), worst
    # the clamp: the designed case, then random offsets around the bounds, in padded buffers
    off = np.array([[0.0, 2.9, -1.9], [3.5, -3.5, 2.5], [np.nan, 3.0, -2.0], [-3.0, np.nan, 2.0]], F32)
    more = (rng.normal(size=(rows, 3)) * 2.5).astype(F32)
    off = np.concatenate([off, more])
    offb = np.full((off.shape[0], 4), SENTINEL, F32)
    offb[:, :3] = off
    dv = np.full((off.shape[0], 5), SENTINEL, F32)
    dv[:, :3] = rng.normal(size=(off.shape[0], 3)).astype(F32)
    out = torch.full((off.shape[0], 4), SENTINEL, dtype=torch.float32, device='cuda')
    op.vote_backward(dev(offb), RANGE, dev(dv), out=out)
    got = out.cpu().numpy()
    assert (got[:, 3] == SENTINEL).all()
    np.testing.assert_array_equal(got[:, :3].astype(np.float64), model.vote_backward(off, RANGE, dv))
    np.testing.assert_array_equal(got[:4, :3] != 0, [[True] * 3, [False] * 3, [False, True, True], [True, False, True]])


# ---- 1b. beyond the launch cap -------------------------------------------------------------------------------------------
# group_backward.hip launches at most 2048 workgroups of 256 lanes and walks the rest by grid-stride loops.  Every kernel once
# with more lanes than that, by a ragged rest, the lanes per row / group placed so that the wrap falls inside one.
CAP = 2048 * 256


def beyond_cap(lanes, inner):
    return CAP < lanes < 2 * CAP and lanes % CAP != 0 and CAP % inner != 0


def test_gather_beyond_the_launch_cap():
    from de6d_amd.ops import group_backward as op
    m, ns, k = 1100, 16, 67
    rng = np.random.default_rng(m + ns)
    cnt, idx = model.padded_query(rng, B, N, m, ns, counts=(0, 1, ns // 2, ns, ns))
    rows = B * m * ns
    ctr = np.full((B, m, 4), SENTINEL, F32)
    ctr[..., :3] = rng.normal(size=(B, m, 3)).astype(F32)
    ldout = round4(k) + 4
    assert beyond_cap(rows * (ldout // 4), ldout // 4)                    # 633 600 float4 lanes
    assert rows * ldout > 2 * CAP and (rows * ldout) % CAP and CAP % ldout   # 2 534 400 scalar lanes: a fifth, ragged trip
    for ldp in (round4(k) + 4, k + 2 + (k & 1)):
        pts = np.full((B, N, ldp), SENTINEL, F32)
        pts[..., :k] = rng.normal(size=(B, N, k)).astype(F32)
        out = torch.full((rows + 1, ldout), SENTINEL, dtype=torch.float32, device='cuda')
        op.group_gather(dev(pts), dev(idx), dev(ctr), k=k, out=out[:rows])
        got = out.cpu().numpy()
        want = model.group_gather(pts, idx, ctr, k=k, ldout=ldout)
        np.testing.assert_array_equal(got[:rows].astype(np.float64), want, err_msg='gather ldp=%d' % ldp)
        assert (got[rows] == SENTINEL).all() and not got[:rows, k:].any()


@pytest.mark.parametrize("c,vec", ((1020, True), (251, False)))
def test_pool_backward_beyond_the_launch_cap(c, vec):
    """four channels per lane (255 lanes per group) and one (251): the empty first ball, the designed tie and the non-positive
    channel of test_gather_and_pool_backward_equal_the_model in the last group"""
    from de6d_amd.ops import group_backward as op
    m, ns = 1100, 4
    rng = np.random.default_rng(c)
    cnt, idx = model.padded_query(rng, B, N, m, ns, counts=(0, 1, ns // 2, ns, ns))
    rows, groups = B * m * ns, B * m
    ldy, lddz, ldg, gcol0 = (round4(c) + 4, round4(c) + 4, round4(c) + 8, 4) if vec else (c + 3, c + 1, c + 5, 3)
    assert vec == (c % 4 == 0 and ldy % 4 == 0 and lddz % 4 == 0)
    per_group = c // 4 if vec else c
    assert beyond_cap(groups * per_group, per_group)
    table = np.maximum(rng.normal(size=(B, N, c)), 0.0).astype(F32)
    r0, lo = (groups - 1) * ns, (ns - 1) // 2
    y = np.full((rows, ldy), SENTINEL, F32)
    y[:, :c] = table[np.arange(B)[:, None, None], idx].reshape(rows, c)
    y[r0:r0 + ns, 0] = 0.25
    y[r0 + lo, 0] = y[r0 + ns - 1, 0] = 9.0                              # two distinct slots hold the positive maximum
    y[r0:r0 + ns, c - 1] = -np.arange(ns, dtype=F32)                      # an all-non-positive channel (maximum 0 at slot 0)
    cnt.reshape(-1)[-1] = ns                                              # the designed group is a full ball
    assert cnt.reshape(-1)[0] == 0
    g = np.full((groups, ldg), SENTINEL, F32)
    g[:, gcol0:gcol0 + c] = rng.normal(size=(groups, c)).astype(F32) + 3.0
    dz = torch.full((rows, lddz), SENTINEL, dtype=torch.float32, device='cuda')
    op.pool_backward(dev(y), dev(cnt), dev(g), ns, c, gcol0=gcol0, dz=dz)
    got = dz.cpu().numpy()
    want = model.pool_backward(y, cnt, g, ns, c, gcol0=gcol0)
    np.testing.assert_array_equal(got[:, :c].astype(np.float64), want)
    assert (got[:, c:] == SENTINEL).all()
    assert not got[:ns, :c].any()                                         # the empty ball passes nothing
    assert got[r0 + lo, 0] == g[-1, gcol0] and got[r0 + ns - 1, 0] == 0   # the lowest slot won
    assert not got[r0:r0 + ns, c - 1].any()


def test_centre_grad_and_vote_backward_beyond_the_launch_cap():
    from de6d_amd.ops import group_backward as op
    groups, ns = 175001, 3
    rng = np.random.default_rng(groups)
    rows = groups * ns
    assert beyond_cap(groups * 3, 3)
    for integers in (True, False):
        dx = np.full((rows, 5), SENTINEL, F32)
        dx[:, :3] = rng.integers(-3, 4, size=(rows, 3)).astype(F32) if integers else rng.normal(size=(rows, 3)).astype(F32)
        out = torch.full((groups, 4), SENTINEL, dtype=torch.float32, device='cuda')
        op.centre_grad(dev(dx), ns, out=out)
        got = out.cpu().numpy()
        assert (got[:, 3] == SENTINEL).all()
        want = model.centre_grad(dx, ns)
        if integers:
            np.testing.assert_array_equal(got[:, :3].astype(np.float64), want)
        else:
            lim = (ns + 2) * U * np.abs(dx[:, :3].astype(np.float64)).reshape(groups, ns, 3).sum(1)
            err = np.abs(got[:, :3].astype(np.float64) - want)
            worst = float((err / np.maximum(lim, 1e-300)).max())
            print('group_backward centre_grad groups=%d ns=%d: largest ratio to the bound %.4f' % (groups, ns, worst))
            assert np.isfinite(got[:, :3]).all() and (err <= lim).all(), worst
    n = groups                                                            # vote_backward: as many rows
    off = np.array([[0.0, 2.9, -1.9], [3.5, -3.5, 2.5], [np.nan, 3.0, -2.0], [-3.0, np.nan, 2.0]], F32)
    off = np.concatenate([off, (rng.normal(size=(n - 4, 3)) * 2.5).astype(F32)])
    offb = np.full((n, 4), SENTINEL, F32)
    offb[:, :3] = off
    dv = np.full((n, 5), SENTINEL, F32)
    dv[:, :3] = rng.normal(size=(n, 3)).astype(F32)
    out = torch.full((n, 4), SENTINEL, dtype=torch.float32, device='cuda')
    op.vote_backward(dev(offb), RANGE, dev(dv), out=out)
    got = out.cpu().numpy()
    assert (got[:, 3] == SENTINEL).all()
    np.testing.assert_array_equal(got[:, :3].astype(np.float64), model.vote_backward(off, RANGE, dv))
    np.testing.assert_array_equal(got[:4, :3] != 0, [[True] * 3, [False] * 3, [False, True, True], [True, False, True]])


# ---- 2. determinism -----------------------------------------------------------------------------------------------------
def folded(rng, krows, k, cout):
    w = np.zeros((krows, round4(cout)), F32)
    w[:k, :cout] = rng.normal(size=(k, cout)).astype(F32) / np.sqrt(k)
    return [dev(w).requires_grad_(True), dev((rng.normal(size=cout) * 0.3).astype(F32)).requires_grad_(True), cout, 1]


def test_repeats_and_a_busy_chip_give_the_same_bits():
    from de6d_amd.ops import fused, group_backward as op
    rng = np.random.default_rng(3)
    b, n, m, cf = 2, 256, 33, 13
    ld = round4(3 + cf)
    rows = np.zeros((b, n, ld), F32)
    rows[..., :3] = rng.uniform(-4, 4, size=(b, n, 3)).astype(F32)
    rows[..., 3:3 + cf] = rng.normal(size=(b, n, cf)).astype(F32)
    rows_d = dev(rows)
    xyz = dev(rows[..., :3])
    ctr = dev(rng.uniform(-4, 4, size=(b, m, 3)).astype(F32))
    ca, ia, cb, ib = fused.ball_query_pair(xyz, ctr, (0.0, 2.0, 6), (0.0, 3.5, 16))
    found = [(ca, ia), (cb, ib)]
    groups = [[folded(rng, ld, 3 + cf, 24), folded(rng, 24, 24, 20)], [folded(rng, ld, 3 + cf, 32), folded(rng, 32, 32, 36), folded(rng, 36, 36, 12)]]
    g_out = dev(rng.normal(size=(b * m, 32)).astype(F32))
    params = [t for g in groups for l in g for t in l[:2]]

    def step():
        c = ctr.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        pooled = op.grouped_chain(rows_d, c, found, [[tuple(l) for l in g] for g in groups], 32)
        pooled.backward(g_out)
        return [pooled.detach().clone(), c.grad.clone()] + [p.grad.clone() for p in params]

    first, again = step(), step()
    big_a = torch.randn((16384, 512), device='cuda')
    big_w = torch.randn((512, 512), device='cuda')
    big_y = torch.empty((16384, 512), device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):
            fused.linear(big_a, big_w, None, 1, big_y)
    busy = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert first[0].shape == (b * m, 32) and first[0].abs().max() > 0 and first[1].abs().max() > 0
    assert all(t.abs().max() > 0 and torch.isfinite(t).all() for t in first[2:])
    for a, bb, e in zip(first, again, busy):
        assert torch.equal(a, bb) and torch.equal(a, e)


# ---- 3. the tiny model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_loss.yaml')
    return cfg, build_model(cfg, seed=11, device='cuda')


STACKS = ('vote_layers', 'SA_module.mlps', 'shared_fc_layer', 'cls_layers', 'reg_layers')


def stack(head, name):
    mod = head
    for part in name.split('.'):
        mod = getattr(mod, part)
    return mod


def head_parameters(head):
    return [(s + '.' + k, p) for s in STACKS for k, p in stack(head, s).named_parameters()]


def clear_grads(net):
    for p in net.parameters():
        p.grad = None


def replay(head, inp, dtype):
    """the whole head as deep copies on the CPU in `dtype`, eval mode: the candidates' rows come in, the engine's idx / cnt are
    constants, pooling is a gather at the engine's winner slots; backward from d_cls, d_reg and the loss's own d_vote"""
    mods = {s: copy.deepcopy(stack(head, s)).cpu().to(dtype).eval() for s in STACKS}
    t = lambda a: a.to(dtype)                                                                            # noqa: E731
    cand, rows, cin = t(inp['cand_rows']), t(inp['rows']), inp['cin']
    b, p, _ = cand.shape
    off = mods['vote_layers'](cand[:, :, 3:3 + cin].reshape(b * p, cin).t().unsqueeze(0)).squeeze(0).t()
    r = torch.tensor(inp['range'], dtype=dtype)
    vote = cand[:, :, :3].reshape(b * p, 3) + torch.max(torch.min(off, r), -r)
    bi = torch.arange(b)[:, None, None]
    pooled = []
    for seq, (cnt, idx), win in zip(mods['SA_module.mlps'], inp['found'], inp['winners']):
        ns = idx.shape[2]
        g = rows[bi, idx.long()]                                                                         # (b, p, ns, ld)
        x0 = torch.cat([g[..., :3] - vote.view(b, p, 1, 3), g[..., 3:3 + cin]], dim=-1)
        y = seq(x0.reshape(1, b * p, ns, 3 + cin).permute(0, 3, 1, 2)).squeeze(0).permute(1, 2, 0)        # (b * p, ns, c)
        top = y.gather(1, win.long().unsqueeze(1)).squeeze(1)
        pooled.append(top * (cnt.reshape(-1, 1) > 0).to(dtype))
    pooled = torch.cat(pooled, dim=1)
    mid = mods['shared_fc_layer'](pooled.t().unsqueeze(0))
    cls, reg = mods['cls_layers'](mid).squeeze(0).t(), mods['reg_layers'](mid).squeeze(0).t()
    torch.autograd.backward([cls, reg, vote], [t(inp['d_cls']), t(inp['d_reg']), t(inp['d_vote'])])
    grads = {s + '.' + k: q.grad.double().numpy() for s in STACKS for k, q in mods[s].named_parameters()}
    outs = dict(vote=vote.detach().double().numpy(), pooled=pooled.detach().double().numpy(),
                cls=cls.detach().double().numpy(), reg=reg.detach().double().numpy())
    return grads, outs


def test_tiny_model_whole_head_gradients(tiny):
    from de6d_amd import parallel
    from de6d_amd.ops import fused, group_backward as op
    from tests.test_head_loss_gpu import prepared
    _, net = tiny
    head = net.point_head
    bd = prepared(net, 31, b=2)
    fr = head.forward_ret_dict
    eval_cls, eval_reg = fr['point_cls_preds'].clone(), fr['point_reg_preds'].clone()
    eval_pooled, eval_vote = fr['point_pooled_features'].clone(), bd['point_vote_coords'][:, 1:4].clone()
    clear_grads(net)
    ret = head.prepare_loss(bd, requires_grad=True, head=True)
    # the re-evaluated tensors are the bits the eval forward left
    assert torch.equal(ret['point_vote_coords'], eval_vote) and torch.equal(ret['point_pooled_features'], eval_pooled)
    assert torch.equal(ret['point_cls_preds'], eval_cls) and torch.equal(ret['point_reg_preds'], eval_reg)
    assert not ret['point_vote_coords'].is_leaf and not ret['point_pooled_features'].is_leaf
    for key in ('point_vote_coords', 'point_cls_preds', 'point_reg_preds'):
        ret[key].retain_grad()
    loss, _ = head.get_loss()
    loss.backward()
    torch.cuda.synchronize()
    named = head_parameters(head)
    ids = {id(p) for _, p in named}
    assert len(named) >= 20 and {n.split('.')[0] for n, _ in named} >= {'vote_layers', 'SA_module'}
    for name, p in named:
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
    for name, p in net.named_parameters():
        if id(p) not in ids:
            assert p.grad is None, name                                   # the backbone

    # what the replay takes from the engine: inputs, the constants of the ball queries, the winner slots, the upstream gradients
    sa = head.SA_module
    b, p, _ = ret['cand_rows'].shape
    vote3 = ret['point_vote_coords'].detach().view(b, p, 3).contiguous()
    shells = [(0.0, radius, ns) for radius, ns in zip(sa.radii, sa.nsamples)]
    ca, ia, cb, ib = fused.ball_query_pair(ret['xyz'], vote3, shells[0], shells[1])
    found, winners = [(ca, ia), (cb, ib)], []
    for (cnt, idx), layers in zip(found, sa._prepare(vote3.device)['groups']):
        _, acts = op.group_forward(ret['rows'], idx, cnt, vote3, layers)
        c, ns = layers[-1][2], idx.shape[2]
        winners.append(torch.from_numpy(acts[-1][:, :c].cpu().numpy().reshape(b * p, ns, c).argmax(axis=1)))   # the lowest slot
    assert int((ca > 0).sum()) > 0 and int((cb > 0).sum()) > 0
    inp = dict(cand_rows=ret['cand_rows'].cpu(), rows=ret['rows'].cpu(), cin=head.input_channels,
               range=tuple(head.vote_cfg.MAX_TRANSLATION_RANGE), found=[(c_.cpu(), i_.cpu()) for c_, i_ in found], winners=winners,
               d_cls=ret['point_cls_preds'].grad.cpu(), d_reg=ret['point_reg_preds'].grad.cpu(),
               d_vote=ret['point_vote_coords'].grad.cpu())
    (t64, o64), (t32, _) = replay(head, inp, torch.float64), replay(head, inp, torch.float32)
    # the replay is the engine's forward: sanity on its outputs (the forward kernels have their own tests)
    for key, eng in (('vote', eval_vote), ('pooled', eval_pooled[..., :o64['pooled'].shape[1]].reshape(b * p, -1)),
                     ('cls', eval_cls), ('reg', eval_reg)):
        assert np.abs(eng.cpu().numpy() - o64[key]).max() <= 1e-4 * max(1.0, np.abs(o64[key]).max()), key
    got = {name: q.grad.cpu().double().numpy() for name, q in named}
    err = lambda a, bb: float(np.abs(a - bb).max() / max(np.abs(bb).max(), 1e-300))                        # noqa: E731
    worst = 0.0
    for name in sorted(t64):
        assert np.abs(t64[name]).max() > 0, name
        ref, eng = err(t32[name], t64[name]), err(got[name], t64[name])
        limit = max(4.0 * ref, 16.0 * U)
        worst = max(worst, eng / limit)
        print('group_backward tiny %-32s engine %.3e  fp32 replay %.3e  limit %.3e' % (name, eng, ref, limit))
        assert eng <= limit, (name, eng, ref)
    print('group_backward tiny: largest ratio to the bound %.4f' % worst)

    # the detector: the same loss bits with the whole head's graph, the towers' graph and none
    losses = []
    for kw in (dict(head=True), dict(towers=True), dict()):
        bdi = prepared(net, 31, b=2)
        losses.append(net.get_training_loss(bdi, requires_grad=True, **kw)[0].detach().clone())
    assert all(torch.equal(x, loss.detach()) for x in losses)
    # 5. a data-parallel step's all-reduce, without a process group: nothing to do, the gradients stay
    before = [q.grad.clone() for _, q in named]
    assert parallel.allreduce_gradients([q for _, q in named]) == 0
    assert all(torch.equal(x, q.grad) for x, (_, q) in zip(before, named))
    # the errors: a missing reference names its key; training mode is refused
    kept = head.forward_ret_dict.pop('cand_rows')
    with pytest.raises(RuntimeError, match="cand_rows"):
        head.prepare_loss(bd, requires_grad=True, head=True)
    head.forward_ret_dict['cand_rows'] = kept
    net.train()
    try:
        with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
            head.prepare_loss(bd, requires_grad=True, head=True)
    finally:
        net.eval()
    clear_grads(net)


# ---- 4. graph capture ---------------------------------------------------------------------------------------------------
def test_a_captured_graph_replays_the_eager_gradients(tiny):
    """prepare_loss(head=True) + get_loss + backward on one stream, captured: no side streams, so no parallel branches"""
    from tests.test_head_loss_gpu import prepared
    _, net = tiny
    head = net.point_head
    bd = prepared(net, 33, b=2)
    named = head_parameters(head)

    def step():
        clear_grads(net)
        head.prepare_loss(bd, requires_grad=True, head=True)
        loss, _ = head.get_loss()
        loss.backward()
        return loss.detach()

    loss_eager = step().clone()
    eager = [p.grad.clone() for _, p in named]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_static = step()
    static = [p.grad for _, p in named]
    for _ in range(2):
        for g in static:
            g.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_static, loss_eager)
        for (name, _), g, e in zip(named, static, eager):
            assert torch.equal(g, e), name
    clear_grads(net)
