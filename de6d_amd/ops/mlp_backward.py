"""Tensor layer of the MLP backward of libdet6d_hip_ext.so (include/det6d_ext.h: det6d_ext_linear_backward): the gradients of
folded Conv1d / BatchNorm / ReLU stacks as det6d_linear evaluates them.

  linear_backward   one layer: (dx, dw, dshift) from the layer's input, its folded weights and dL/d(pre-activation output)
  chain_backward    a folded chain [(W, shift, cout, act)] (fold_sequential / run_chain's format) walked from its last layer
  FoldedChain       torch.autograd.Function: a trunk and the towers that read its output; forward = the forward kernels
                    (fused.linear, layer by layer, keeping the activations), backward = chain_backward
  folded_params     ties the cached folded (W, shift) of a stack to the module's own parameters (conv.weight, bn.weight,
                    bn.bias, the last conv.bias): the VALUES are the cached tensors the eval forward uses, the gradient of a
                    folded pair reaches the parameters by the derivative of fold_layer

Asynchronous on the current stream; nothing here reads a result on the host, so a step can be captured into a graph.
BatchNorm is frozen (eval mode): running mean and variance are constants."""
import torch

from .. import _lib as L
from . import fused

RELU_INPUT, ACCUMULATE_DX = 1, 2
#: rows per slab of the dw / dshift reduction (DET6D_EXT_LINEAR_BACKWARD_SLAB): part of the arithmetic contract
SLAB = 256


def _rows2d(t, what):
    if t.dim() != 2 or t.dtype != torch.float32:
        raise L.Det6dError("linear_backward: %s must be a 2-d float32 tensor, got %s %s" % (what, tuple(t.shape), t.dtype))
    return t


def linear_backward(x, w, dz, *, xcol0=0, wrow0=0, k=None, n=None, relu_input=False, dx=None, accumulate_dx=False,
                    need=(True, True, True), dxcol0=0, dw=None, dshift=None):
    """x (rows, ldx): the layer's input in columns [xcol0, xcol0 + k); w (.., ldw): the folded weights in rows
    [wrow0, wrow0 + k), columns [0, n); dz (rows, >= n) = dL/d(pre-activation output).  -> (dx, dw, dshift), None where need[i]
    is false.  relu_input: x is a ReLU output and dx is masked by x > 0 (it is then the previous layer's dz).  dx / dw / dshift
    may be handed in (dx at columns [dxcol0, dxcol0 + k) of a wider buffer; dw (k, >= n)); accumulate_dx adds into dx.
    What is not handed in is allocated dense; the workspace comes from torch's allocator."""
    L.require_cuda(x, w, dz, dx, dw, dshift)
    _rows2d(x, 'x'), _rows2d(w, 'w'), _rows2d(dz, 'dz')
    rows = x.shape[0]
    k = w.shape[0] - wrow0 if k is None else k
    n = dz.shape[1] if n is None else n
    if dz.shape[0] != rows:
        raise L.Det6dError("linear_backward: x has %d rows, dz %d" % (rows, dz.shape[0]))
    if wrow0 < 0 or wrow0 + k > w.shape[0] or k < 1:
        raise L.Det6dError("linear_backward: weight rows [%d, %d) of %d" % (wrow0, wrow0 + k, w.shape[0]))
    need_dx, need_dw, need_ds = need
    if accumulate_dx and (dx is None or not need_dx):
        raise L.Det6dError("linear_backward: accumulate_dx needs the dx buffer to add into")
    dev = x.device
    if need_dx and dx is None:
        dx, dxcol0 = torch.empty((rows, k), dtype=torch.float32, device=dev), 0
    if need_dw and dw is None:
        dw = torch.empty((k, n), dtype=torch.float32, device=dev)
    if need_ds and dshift is None:
        dshift = torch.empty((n,), dtype=torch.float32, device=dev)
    dx = dx if need_dx else None
    dw = dw if need_dw else None
    dshift = dshift if need_ds else None
    for t, rws, what in ((dx, rows, 'dx'), (dw, k, 'dw')):
        if t is not None and (_rows2d(t, what).shape[0] != rws):
            raise L.Det6dError("linear_backward: %s has %d rows, %d expected" % (what, t.shape[0], rws))
    if dshift is not None and (dshift.dtype != torch.float32 or dshift.numel() < n):
        raise L.Det6dError("linear_backward: dshift must hold %d float32" % n)
    ws_bytes = int(L.ext_lib().det6d_ext_linear_backward_workspace_bytes(rows, k, n))
    if ws_bytes < 0:
        raise L.Det6dError("linear_backward: rows = %d, k = %d, n = %d is out of range" % (rows, k, n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes and (need_dw or need_ds) else None
    flags = (RELU_INPUT if relu_input else 0) | (ACCUMULATE_DX if accumulate_dx else 0)
    L.call_ext("det6d_ext_linear_backward", rows, k, n, L.ptr(x), x.shape[1], xcol0, L.ptr(w), w.shape[1], wrow0, L.ptr(dz),
               dz.shape[1], flags, L.ptr(dx), dx.shape[1] if dx is not None else 0, dxcol0, L.ptr(dw),
               dw.shape[1] if dw is not None else 0, L.ptr(dshift), L.ptr(ws), ws_bytes if ws is not None else 0, L.stream_ptr())
    return dx, dw, dshift


def chain_forward(x, layers, out=None, hidden_last=False):
    """fused.run_chain, keeping every layer's output: -> [activation of layer 0, ..., of the last layer].  Hidden activations
    are (rows, padded width) with zeroed padding columns (the next layer's K), the last one is `out` or a dense (rows, cout) —
    unless hidden_last says that it feeds further layers too (a trunk under towers)."""
    if out is None and not hidden_last:
        out = torch.empty((x.numel() // x.shape[-1], layers[-1][2]), dtype=torch.float32, device=x.device)
    return fused.run_chain(x, layers, out=None if hidden_last else out, keep=True)


def chain_backward(x, layers, activations, dz_last, *, k0=None, wrow0=0, relu_input=False, dx=None, accumulate_dx=False,
                   need_dx=True, need_params=True):
    """Walks a folded chain [(W, shift, cout, act)] from its last layer to its first.  x (rows, ldx): the chain's input;
    activations[i]: the output of layer i a forward kept (the last one is not read); dz_last: dL/d(the last layer's
    PRE-activation output) — for a last layer without activation, the gradient of the chain's output.
    k0 / wrow0: the first layer consumes columns [0, k0) of x through weight rows [wrow0, wrow0 + k0) (default: every row of
    W from wrow0).  relu_input: x itself is a ReLU output (the chain is a tower on a trunk): the returned dx is masked, i.e. it
    is the dz of the trunk's last layer; dx / accumulate_dx: the second tower adds into the first one's buffer.
    -> (dx or None, [(dW, dshift)] per layer or None).  dW has the shape of the folded W: rows and columns of the padding
    carry no gradient and stay zero."""
    grads = [None] * len(layers)
    dz = dz_last
    for li in range(len(layers) - 1, -1, -1):
        w, _, cout, _ = layers[li]
        first = li == 0
        inp = x if first else activations[li - 1]
        k = (w.shape[0] - wrow0 if k0 is None else k0) if first else layers[li - 1][2]
        r0 = wrow0 if first else 0
        masked = relu_input if first else layers[li - 1][3] == 1
        dw = ds = None
        if need_params:
            full = torch.zeros_like(w)
            dw, ds = full[r0:r0 + k], torch.empty((cout,), dtype=torch.float32, device=w.device)
            grads[li] = (full, ds)
        want_dx = need_dx or not first
        if not (want_dx or need_params):
            return None, None
        dz, _, _ = linear_backward(inp, w, dz, wrow0=r0, k=k, n=cout, relu_input=masked, dx=dx if first else None,
                                   accumulate_dx=accumulate_dx and first, need=(want_dx, need_params, need_params), dw=dw,
                                   dshift=ds)
    return (dz if need_dx else None), (grads if need_params else None)


class FoldedChain(torch.autograd.Function):
    """outs = FoldedChain.apply(x, spec, *tensors): a trunk of folded layers and the towers that read its output (no towers:
    the trunk alone).  spec = (k0, [(cout, act)] of the trunk, [[(cout, act)] of a tower, ...]); tensors = W, shift of every
    layer, trunk first.  Use folded_chain().  The forward is fused.linear layer by layer (the kernels and the folded tensors of
    the eval forward: the same bits); the backward is one det6d_ext_linear_backward per layer.  Every returned output must be
    that of a layer without activation (the head's logits and box codes); with towers the trunk's own output is not returned."""

    @staticmethod
    def forward(ctx, x, spec, *tensors):
        k0, trunk_spec, tower_specs = spec
        x = x.detach()
        x2 = x.reshape(-1, x.shape[-1])
        it = iter(tensors)
        take = lambda s: [(next(it).detach(), next(it).detach(), c, a) for c, a in s]                    # noqa: E731
        trunk, towers = take(trunk_spec), [take(s) for s in tower_specs]
        for chain in (towers or [trunk]):
            if not chain or chain[-1][3] != 0:
                raise NotImplementedError("FoldedChain returns the outputs of layers without activation only")
        acts = chain_forward(x2, trunk, hidden_last=bool(towers)) if trunk else []
        mid = acts[-1] if trunk else x2
        tower_acts = [chain_forward(mid, t) for t in towers]
        ctx.k0, ctx.trunk, ctx.towers = k0, trunk, towers
        outs = tuple(a[-1] for a in tower_acts) if towers else (acts[-1],)
        # (the outputs themselves are not kept: the backward never reads a last layer's activation)
        ctx.x, ctx.acts, ctx.tower_acts = x2, acts if towers else acts[:-1], [a[:-1] for a in tower_acts]
        return outs

    @staticmethod
    def backward(ctx, *grad_outs):
        trunk, towers = ctx.trunk, ctx.towers
        need_x = ctx.needs_input_grad[0]
        need_p = any(ctx.needs_input_grad[2:])
        gouts = [None if g is None else g.detach().to(torch.float32).contiguous() for g in grad_outs]
        flat = []
        if not towers:
            g = gouts[0] if gouts[0] is not None else ctx.x.new_zeros((ctx.x.shape[0], trunk[-1][2]))
            dx, grads = chain_backward(ctx.x, trunk, ctx.acts, g, k0=ctx.k0, need_dx=need_x, need_params=need_p)
            flat = grads or []
        else:
            mid = ctx.acts[-1] if trunk else ctx.x
            mid_relu = bool(trunk) and trunk[-1][3] == 1
            need_mid = bool(trunk) or need_x
            dmid, tower_grads = None, []
            for t, acts, g in zip(towers, ctx.tower_acts, gouts):
                g = g if g is not None else ctx.x.new_zeros((ctx.x.shape[0], t[-1][2]))
                d, grads = chain_backward(mid, t, acts, g, k0=None if trunk else ctx.k0, relu_input=mid_relu, dx=dmid,
                                          accumulate_dx=dmid is not None, need_dx=need_mid, need_params=need_p)
                dmid = d if dmid is None else dmid
                tower_grads += grads or [None] * len(t)
            if trunk:
                dx, grads = chain_backward(ctx.x, trunk, ctx.acts, dmid, k0=ctx.k0, need_dx=need_x, need_params=need_p)
                flat = (grads or [None] * len(trunk)) + tower_grads
            else:
                dx, flat = dmid, tower_grads
        out = []
        for pair in flat:
            out += list(pair) if pair is not None else [None, None]
        if dx is not None:
            ldx = ctx.x.shape[1]
            if dx.shape[1] != ldx:                                  # the padding columns of x carry no gradient
                full = torch.zeros_like(ctx.x)
                full[:, :dx.shape[1]] = dx
                dx = full
        return (dx, None) + tuple(out)


def folded_chain(x, trunk, towers=(), k0=None):
    """x (rows, ldx); trunk and every tower a list [(W, shift, cout, act)] on the device -> the tuple of the towers' outputs
    (the trunk's output when there are no towers).  Gradients reach x and every W and shift that requires one."""
    spec = (k0, [(c, a) for _, _, c, a in trunk], [[(c, a) for _, _, c, a in t] for t in towers])
    tensors = [t for chain in [trunk] + list(towers) for w, s, _, _ in chain for t in (w, s)]
    return FoldedChain.apply(x, spec, *tensors)


class FoldedParams(torch.autograd.Function):
    """W, shift = FoldedParams.apply(W_cached, shift_cached, meta, conv.weight, conv.bias, bn.weight, bn.bias): the values are
    the cached folded tensors (what fold_layer made of these parameters); the backward is the derivative of fold_layer with
    running mean and variance constant.  meta = (k_offset, running_mean, running_var, eps) or (k_offset, None, None, 0)."""

    @staticmethod
    def forward(ctx, w_fold, shift_fold, meta, conv_w, conv_b, gamma, beta):
        ctx.meta = meta
        ctx.save_for_backward(conv_w, conv_b, gamma)
        return w_fold.view_as(w_fold), shift_fold.view_as(shift_fold)

    @staticmethod
    def backward(ctx, d_w, d_shift):
        k_offset, mean, var, eps = ctx.meta
        conv_w, conv_b, gamma = ctx.saved_tensors
        cout, cin = conv_w.shape[0], conv_w[0].numel()
        w2 = conv_w.reshape(cout, cin)
        block_t = d_w[k_offset:k_offset + cin, :cout].t() if d_w is not None else torch.zeros_like(w2)
        d_shift = d_shift[:cout] if d_shift is not None else torch.zeros((cout,), dtype=w2.dtype, device=w2.device)
        if mean is None:
            return None, None, None, block_t.reshape(conv_w.shape), (d_shift if conv_b is not None else None), None, None
        inv = 1.0 / torch.sqrt(var + eps)
        s = gamma * inv
        d_gamma = (block_t * w2).sum(1) - mean * d_shift
        if conv_b is not None:
            d_gamma = d_gamma + conv_b * d_shift
        return (None, None, None, (block_t * s[:, None]).reshape(conv_w.shape), (d_shift * s if conv_b is not None else None),
                d_gamma * inv, d_shift)


def folded_params(seq, layers, k_offset=0):
    """seq: an nn.Sequential of Conv(/BN/ReLU) blocks in eval mode, its parameters on the device; layers: its cached folded
    chain [(W, shift, cout, act)] (fold_sequential + to_device) -> the same chain whose W and shift carry a graph to the
    module's parameters."""
    mods, out, i = list(seq), [], 0
    for w_fold, shift_fold, cout, act in layers:
        conv = mods[i]
        bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) else None
        i += 1 + (bn is not None) + act
        if bn is not None and bn.training:
            raise RuntimeError("the HIP head folds BatchNorm: call .eval() first")
        if conv.weight.device != w_fold.device:
            raise L.Det6dError("folded_params: the module's parameters must live on the device of the folded tensors")
        meta = (k_offset, bn.running_mean, bn.running_var, bn.eps) if bn is not None else (k_offset, None, None, 0.0)
        w, shift = FoldedParams.apply(w_fold, shift_fold, meta, conv.weight, conv.bias, bn.weight if bn is not None else None,
                                      bn.bias if bn is not None else None)
        out.append((w, shift, cout, act))
        k_offset = 0
    return out
