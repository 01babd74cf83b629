"""The MLP backward on the GPU (de6d_amd/csrc/ext/mlp_backward.hip and the layers above it) against the float64 model
(tests/models/mlp_backward.py): exact on small integers (every order of summation is exact there), within the forward error
bound of an fp32 inner product on random floats, bit-identical repeats, a two-tower chain through FoldedChain, and the tiny
model's parameter gradients against a float64 CPU replay of its three stacks, eager and from a captured graph.

Bounds.  Random floats: |got - truth64| <= (L + 2) * 2^-24 * sum_i |a_i| |b_i| per element (L the reduction length): the
standard bound of an fp32 inner product in any order, no measured constant.  The tiny model: DESIGN.md §5 "Truth and
bounds": err = max|T - T64| / max|T64| per tensor, held to 4 x the error of the same replay in fp32 on the CPU, floored at
16 * 2^-24.  Every test prints the largest ratio to its bound (pytest -s) before it asserts."""
import copy

import numpy as np
import pytest
import torch

from tests.models import mlp_backward as model

pytestmark = pytest.mark.gpu

F32 = np.float32
S = model.SLAB
ROWS = (1, 31, 33, S, S + 1, 2 * S + 7)
SHAPES = ((4, 1), (36, 3), (32, 32), (224, 96), (96, 27), (100, 33))
HEAD_SHAPES = ((2048, 1536, 512), (2048, 512, 128), (2048, 128, 32), (2048, 128, 1))
SENTINEL = 7777.0
XCOL0, WROW0, DXCOL0 = 3, 5, 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def round4(v):
    return (v + 3) // 4 * 4


def make_case(rows, k, n, seed, integers):
    """operands inside wider buffers whose padding holds SENTINEL: x at columns [XCOL0, XCOL0 + k), w at rows [WROW0, WROW0 + k)"""
    rng = np.random.default_rng(seed)
    draw = (lambda shape: rng.integers(-3, 4, size=shape).astype(F32)) if integers else (lambda shape: rng.normal(size=shape).astype(F32))
    ldx, ldw, lddz = round4(XCOL0 + k) + 4, round4(n) + 4, n + 3
    x = np.full((rows, ldx), SENTINEL, F32)
    w = np.full((WROW0 + k + 1, ldw), SENTINEL, F32)
    dz = np.full((rows, lddz), SENTINEL, F32)
    x[:, XCOL0:XCOL0 + k] = draw((rows, k))
    if not integers:
        x[:, XCOL0:XCOL0 + k][rng.random((rows, k)) < 0.2] = 0.0
    x[0, XCOL0], x[-1, XCOL0 + k - 1] = 0.0, -2.0                         # a zero and a negative under the mask, whatever the draw
    w[WROW0:WROW0 + k, :n] = draw((k, n))
    dz[:, :n] = draw((rows, n))
    before = draw((rows, k))
    return x, w, dz, before


def run_case(x, w, dz, before, k, n, flags, need=(True, True, True)):
    """one call into sentinel-padded output buffers -> (dx, dw, dshift) as NumPy blocks, None where not asked for"""
    from de6d_amd.ops import mlp_backward as op
    rows = x.shape[0]
    dxb = np.full((rows, DXCOL0 + k + 5), SENTINEL, F32)
    dxb[:, DXCOL0:DXCOL0 + k] = before if flags & 2 else np.nan
    dwb = np.full((k, n + 1), SENTINEL, F32)
    dwb[:, :n] = np.nan
    dsb = np.full((n + 2,), SENTINEL, F32)
    dsb[:n] = np.nan
    tx, tw, ts = dev(dxb), dev(dwb), dev(dsb)
    out = op.linear_backward(dev(x), dev(w), dev(dz), xcol0=XCOL0, wrow0=WROW0, k=k, n=n, relu_input=bool(flags & 1), dx=tx,
                             accumulate_dx=bool(flags & 2), need=need, dxcol0=DXCOL0, dw=tw, dshift=ts)
    torch.cuda.synchronize()
    assert [o is not None for o in out] == list(need)
    gx, gw, gs = tx.cpu().numpy(), tw.cpu().numpy(), ts.cpu().numpy()
    # the padding survives, and what was not asked for is not touched
    assert (gx[:, :DXCOL0] == SENTINEL).all() and (gx[:, DXCOL0 + k:] == SENTINEL).all()
    assert (gw[:, n:] == SENTINEL).all() and (gs[n:] == SENTINEL).all()
    if not need[0]:
        np.testing.assert_array_equal(gx, dxb)
    if not need[1]:
        np.testing.assert_array_equal(gw, dwb)
    if not need[2]:
        np.testing.assert_array_equal(gs, dsb)
    return (gx[:, DXCOL0:DXCOL0 + k] if need[0] else None, gw[:, :n] if need[1] else None, gs[:n] if need[2] else None)


def truth(x, w, dz, before, k, n, flags):
    return model.linear_backward(x, w, dz, XCOL0, WROW0, k, n, relu_input=bool(flags & 1), dx_before=before if flags & 2 else None)


@pytest.mark.parametrize("k,n", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_small_integers_are_exact(rows, k, n):
    x, w, dz, before = make_case(rows, k, n, seed=rows * 131 + k, integers=True)
    mags = model.magnitudes(x, w, dz, XCOL0, WROW0, k, n, dx_before=before)
    assert all(m.max() < 2 ** 24 for m in mags)                           # every partial sum is an exact fp32 integer
    for flags in (3, 0):                                                  # mask + add onto a non-zero buffer; and neither
        want = truth(x, w, dz, before, k, n, flags)
        got = run_case(x, w, dz, before, k, n, flags)
        for g, t, name in zip(got, want, ('dx', 'dw', 'dshift')):
            np.testing.assert_array_equal(g.astype(np.float64), t, err_msg='%s flags=%d' % (name, flags))
    want = truth(x, w, dz, before, k, n, 1)
    for skip in range(3):                                                 # each output NULL in turn
        need = tuple(i != skip for i in range(3))
        got = run_case(x, w, dz, before, k, n, 1, need)
        for i, name in enumerate(('dx', 'dw', 'dshift')):
            if need[i]:
                np.testing.assert_array_equal(got[i].astype(np.float64), want[i], err_msg='%s without output %d' % (name, skip))


def check_bound(got, want, mags, lengths, tag):
    """per element |got - truth| <= (L + 2) 2^-24 sum |a||b|; -> the largest ratio to the bound per quantity"""
    ratios = []
    for g, t, m, length, name in zip(got, want, mags, lengths, ('dx', 'dw', 'dshift')):
        lim = model.bound(length, m)
        err = np.abs(g.astype(np.float64) - t)
        ratio = float((err / np.maximum(lim, 1e-300)).max())
        ratios.append(ratio)
        assert np.isfinite(g).all() and (err <= lim).all(), (tag, name, ratio)
    print('mlp_backward bound ratio %s: dx %.4f dw %.4f dshift %.4f' % ((tag,) + tuple(ratios)))
    return ratios


@pytest.mark.parametrize("k,n", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_random_floats_within_the_inner_product_bound(rows, k, n):
    x, w, dz, before = make_case(rows, k, n, seed=rows * 17 + n, integers=False)
    want = truth(x, w, dz, before, k, n, 3)
    mags = model.magnitudes(x, w, dz, XCOL0, WROW0, k, n, dx_before=before)
    got = run_case(x, w, dz, before, k, n, 3)
    check_bound(got, want, mags, (n + 1, rows, rows), (rows, k, n))      # dx: n products and the add


@pytest.fixture(scope="module")
def head_cases():
    """the head's real layer shapes at 2048 rows: operands on the device, the float64 truth computed once"""
    cases = {}
    for rows, k, n in HEAD_SHAPES:
        rng = np.random.default_rng(k + n)
        x = np.maximum(rng.normal(size=(rows, k)), 0.0).astype(F32)       # a ReLU output, as the hidden layers see it
        w = np.zeros((k, round4(n)), F32)
        w[:, :n] = rng.normal(size=(k, n)).astype(F32) / np.sqrt(k)
        dz = rng.normal(size=(rows, n)).astype(F32)
        cases[(rows, k, n)] = dict(x=x, w=w, dz=dz, want=model.linear_backward(x, w, dz, k=k, n=n, relu_input=True),
                                   mags=model.magnitudes(x, w, dz, k=k, n=n))
    return cases


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_the_heads_layer_shapes_within_the_bound(head_cases, shape):
    from de6d_amd.ops import mlp_backward as op
    rows, k, n = shape
    c = head_cases[shape]
    got = op.linear_backward(dev(c['x']), dev(c['w']), dev(c['dz']), k=k, n=n, relu_input=True)
    got = [g.cpu().numpy() for g in got]
    assert got[0].shape == (rows, k) and got[1].shape == (k, n) and got[2].shape == (n,)
    check_bound(got, c['want'], c['mags'], (n, rows, rows), shape)


def test_repeats_and_a_busy_chip_give_the_same_bits(head_cases):
    from de6d_amd.ops import fused, mlp_backward as op
    shape = (2048, 512, 128)
    c = head_cases[shape]
    x, w, dz = dev(c['x']), dev(c['w']), dev(c['dz'])
    first = op.linear_backward(x, w, dz, k=512, n=128, relu_input=True)
    again = op.linear_backward(x, w, dz, k=512, n=128, relu_input=True)
    # a forward GEMM keeps the chip busy on another stream while the backward runs
    big_a = torch.randn((16384, 512), device='cuda')
    big_w = torch.randn((512, 512), device='cuda')
    big_y = torch.empty((16384, 512), device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):
            fused.linear(big_a, big_w, None, 1, big_y)
    busy = op.linear_backward(x, w, dz, k=512, n=128, relu_input=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b, e in zip(first, again, busy):
        assert torch.equal(a, b) and torch.equal(a, e)


# ---- a two-tower chain through FoldedChain ------------------------------------------------------------------------------
def folded(rng, k, cout, act):
    w = np.zeros((round4(k), round4(cout)), F32)
    w[:k, :cout] = rng.normal(size=(k, cout)).astype(F32) / np.sqrt(k)
    return [dev(w).requires_grad_(True), dev((rng.normal(size=cout) * 0.3).astype(F32)).requires_grad_(True), cout, act]


def test_two_tower_chain_through_folded_chain():
    """224 -> 96 -> {32 -> 3, 32 -> 27} on 130 rows.  Every layer call is held to the per-element bound against the float64
    model evaluated on THAT call's inputs (the fp32 activations and the fp32 dz the call before it left); FoldedChain's own
    results are the bits of the same calls made by hand."""
    from de6d_amd.ops import mlp_backward as op
    rng = np.random.default_rng(42)
    rows = 130
    trunk = [folded(rng, 224, 96, 1)]
    towers = [[folded(rng, 96, 32, 1), folded(rng, 32, 3, 0)], [folded(rng, 96, 32, 1), folded(rng, 32, 27, 0)]]
    x = dev(rng.normal(size=(rows, 224)).astype(F32)).requires_grad_(True)
    g_out = [dev(rng.normal(size=(rows, 3)).astype(F32)), dev(rng.normal(size=(rows, 27)).astype(F32))]
    outs = op.folded_chain(x, [tuple(l) for l in trunk], [[tuple(l) for l in t] for t in towers])
    assert [tuple(o.shape) for o in outs] == [(rows, 3), (rows, 27)]
    torch.autograd.backward(list(outs), g_out)
    torch.cuda.synchronize()

    # the forward, in float64 from the fp32 parameters: sanity only (the forward kernels have their own tests)
    to64 = lambda chain: [(l[0].detach().cpu().numpy().astype(np.float64)[:, :l[2]], l[1].detach().cpu().numpy().astype(np.float64), l[3])  # noqa: E731
                          for l in chain]
    mid64 = model.chain_forward(x.detach().cpu().numpy(), to64(trunk))[-1]
    for t, o in zip(towers, outs):
        l64 = to64(t)
        l64[0] = (l64[0][0][:96], l64[0][1], l64[0][2])
        l64[1] = (l64[1][0][:32], l64[1][1], l64[1][2])
        want = model.chain_forward(mid64, l64)[-1]
        assert np.abs(o.detach().cpu().numpy() - want).max() <= 1e-4 * max(1.0, np.abs(want).max())

    # the same calls by hand, keeping every intermediate
    with torch.no_grad():
        det = lambda chain: [(l[0].detach(), l[1].detach(), l[2], l[3]) for l in chain]                   # noqa: E731
        acts = op.chain_forward(x.detach(), det(trunk), hidden_last=True)
        mid = acts[-1]
        calls, d_mid = [], None
        for t, g in zip(towers, g_out):
            ta = op.chain_forward(mid, det(t))
            h = ta[0]
            d_h, dw1, ds1 = op.linear_backward(h, t[1][0].detach(), g, k=32, n=t[1][2], relu_input=True)
            calls.append((h, t[1], g, None, True, (d_h, dw1, ds1), 32, t[1][2]))
            before = None if d_mid is None else d_mid.clone()
            d_mid, dw0, ds0 = op.linear_backward(mid, t[0][0].detach(), d_h, k=96, n=32, relu_input=True, dx=d_mid,
                                                 accumulate_dx=d_mid is not None)
            calls.append((mid, t[0], d_h, before, True, (d_mid.clone(), dw0, ds0), 96, 32))
        d_x, dwt, dst = op.linear_backward(x.detach(), trunk[0][0].detach(), d_mid, k=224, n=96)
        calls.append((x.detach(), trunk[0], d_mid, None, False, (d_x, dwt, dst), 224, 96))
        torch.cuda.synchronize()
    for inp, layer, dz, before, masked, got, k, n in calls:
        a = [t.cpu().numpy() for t in (inp, layer[0].detach(), dz)]
        b = None if before is None else before.cpu().numpy()
        want = model.linear_backward(*a, k=k, n=n, relu_input=masked, dx_before=b)
        mags = model.magnitudes(*a, k=k, n=n, dx_before=b)
        check_bound([t.cpu().numpy() for t in got], want, mags, (n + 1, rows, rows), ('chain', k, n))
        # FoldedChain: the same bits, the block inside a gradient of the folded tensor's shape, zeros in the padding
        gw = layer[0].grad
        assert gw.shape == layer[0].shape and torch.equal(gw[:k, :n], got[1]) and torch.equal(layer[1].grad, got[2])
        assert not gw[k:].any() and not gw[:, n:].any()
    assert torch.equal(x.grad, calls[-1][5][0])


# ---- the tiny model -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from de6d_amd.runtime import load_config, build_model
    cfg = load_config('synthetic_models/det6d_tiny_loss.yaml')
    return cfg, build_model(cfg, seed=11, device='cuda')


STACKS = ('shared_fc_layer', 'cls_layers', 'reg_layers')


def tower_parameters(head):
    return [(s + '.' + k, p) for s in STACKS for k, p in getattr(head, s).named_parameters()]


def clear_grads(net):
    for p in net.parameters():
        p.grad = None


def replay(head, pooled, d_cls, d_reg, dtype):
    """the three stacks as deep copies on the CPU in `dtype`, eval mode, fed the pooled features; backward from d_cls, d_reg"""
    mods = [copy.deepcopy(getattr(head, s)).cpu().to(dtype).eval() for s in STACKS]
    x = pooled.to(dtype).clone().requires_grad_(True)
    mid = mods[0](x.t().unsqueeze(0))
    cls, reg = mods[1](mid).squeeze(0).t(), mods[2](mid).squeeze(0).t()
    torch.autograd.backward([cls, reg], [d_cls.to(dtype), d_reg.to(dtype)])
    grads = {s + '.' + k: p.grad.double().numpy() for s, m in zip(STACKS, mods) for k, p in m.named_parameters()}
    grads['pooled'] = x.grad.double().numpy()
    return grads


def test_tiny_model_parameter_gradients(tiny):
    from de6d_amd import parallel
    from tests.test_head_loss_gpu import prepared
    _, net = tiny
    head = net.point_head
    bd = prepared(net, 31, b=2)
    eval_cls, eval_reg = head.forward_ret_dict['point_cls_preds'].clone(), head.forward_ret_dict['point_reg_preds'].clone()
    pooled_ref = head.forward_ret_dict['point_pooled_features']
    clear_grads(net)
    ret = head.prepare_loss(bd, requires_grad=True, towers=True)
    # the re-evaluated predictions are the bits the eval forward left; the pooled features are the same memory
    assert torch.equal(ret['point_cls_preds'], eval_cls) and torch.equal(ret['point_reg_preds'], eval_reg)
    assert ret['point_pooled_features'].data_ptr() == pooled_ref.data_ptr() and ret['point_pooled_features'].is_leaf
    assert ret['point_vote_coords'].is_leaf and ret['point_vote_coords'].requires_grad
    ret['point_cls_preds'].retain_grad(), ret['point_reg_preds'].retain_grad()
    loss, _ = head.get_loss()
    loss.backward()
    torch.cuda.synchronize()
    named = tower_parameters(head)
    ids = {id(p) for _, p in named}
    assert len(named) >= 10
    for name, p in named:
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
    for name, p in net.named_parameters():
        if id(p) not in ids:
            assert p.grad is None, name                                   # vote_layers, the head's SA layer, the backbone
    assert ret['point_vote_coords'].grad is not None and ret['point_pooled_features'].grad is not None

    # float64 and fp32 CPU replays from the d_cls / d_reg head_loss.backward produced on the GPU
    k0 = sum(seq[-3].out_channels for seq in head.SA_module.mlps)
    pooled = ret['point_pooled_features'].detach().cpu().reshape(-1, ret['point_pooled_features'].shape[-1])[:, :k0]
    d_cls, d_reg = ret['point_cls_preds'].grad.cpu(), ret['point_reg_preds'].grad.cpu()
    t64, t32 = replay(head, pooled, d_cls, d_reg, torch.float64), replay(head, pooled, d_cls, d_reg, torch.float32)
    got = {name: p.grad.cpu().double().numpy() for name, p in named}
    got['pooled'] = ret['point_pooled_features'].grad.cpu().double().numpy().reshape(pooled.shape[0], -1)[:, :k0]
    err = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))                          # noqa: E731
    for name in sorted(t64):
        assert np.abs(t64[name]).max() > 0, name
        ref, eng = err(t32[name], t64[name]), err(got[name], t64[name])
        limit = max(4.0 * ref, 16.0 * 2.0 ** -24)
        print('mlp_backward tiny %-28s engine %.3e  fp32 replay %.3e  limit %.3e' % (name, eng, ref, limit))
        assert eng <= limit, (name, eng, ref)

    # the detector: the same loss bits with and without the towers' graph
    bd2 = prepared(net, 31, b=2)
    loss_t = net.get_training_loss(bd2, requires_grad=True, towers=True)[0]
    bd3 = prepared(net, 31, b=2)
    loss_p = net.get_training_loss(bd3, requires_grad=True, towers=False)[0]
    assert torch.equal(loss_t.detach(), loss_p.detach()) and torch.equal(loss_t.detach(), loss.detach())
    # a data-parallel step's all-reduce, without a process group: nothing to do, the gradients stay
    before = [p.grad.clone() for _, p in named]
    assert parallel.allreduce_gradients([p for _, p in named]) == 0
    assert all(torch.equal(b, p.grad) for b, (_, p) in zip(before, named))
    # training mode: the existing error
    net.train()
    try:
        with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
            head.prepare_loss(bd3, requires_grad=True, towers=True)
    finally:
        net.eval()
    clear_grads(net)


def test_a_captured_graph_replays_the_eager_gradients(tiny):
    """prepare_loss(towers=True) + get_loss + backward on one stream, captured: no side streams, so no parallel branches"""
    from tests.test_head_loss_gpu import prepared
    _, net = tiny
    head = net.point_head
    bd = prepared(net, 33, b=2)
    named = tower_parameters(head)

    def step():
        clear_grads(net)
        head.prepare_loss(bd, requires_grad=True, towers=True)
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
