"""float64 model of the MLP backward (include/det6d_ext.h: det6d_ext_linear_backward; de6d_amd/ops/mlp_backward.py): one
layer, a folded chain, and the map from the gradient of a folded (W, shift) pair to the module's own parameters.
Everything is NumPy float64: the truth the kernels are held against.  `magnitudes` gives, per output element, the sum of
the absolute products of its inner product: the scale of the forward error bound of an fp32 sum in ANY order,
|got - truth| <= (L + 2) * 2^-24 * sum_i |a_i| |b_i| for a reduction of length L."""
import numpy as np

F64 = np.float64
#: rows per slab of the dw / dshift reduction (DET6D_EXT_LINEAR_BACKWARD_SLAB)
SLAB = 256
U = 2.0 ** -24


def _operands(x, w, dz, xcol0, wrow0, k, n):
    k = w.shape[0] - wrow0 if k is None else k
    n = dz.shape[1] if n is None else n
    return (np.asarray(x, F64)[:, xcol0:xcol0 + k], np.asarray(w, F64)[wrow0:wrow0 + k, :n], np.asarray(dz, F64)[:, :n])


def linear_backward(x, w, dz, xcol0=0, wrow0=0, k=None, n=None, relu_input=False, dx_before=None):
    """-> (dx (rows, k), dw (k, n), dshift (n)); dx_before: the buffer ACCUMULATE_DX adds into"""
    X, W, DZ = _operands(x, w, dz, xcol0, wrow0, k, n)
    dx = DZ @ W.T
    if relu_input:
        dx = np.where(X > 0, dx, 0.0)                       # a NaN compares false
    if dx_before is not None:
        dx = np.asarray(dx_before, F64) + dx
    return dx, X.T @ DZ, DZ.sum(0)


def magnitudes(x, w, dz, xcol0=0, wrow0=0, k=None, n=None, dx_before=None):
    """sum_i |a_i| |b_i| of every element of (dx, dw, dshift); the add of ACCUMULATE_DX is one more term"""
    X, W, DZ = _operands(x, w, dz, xcol0, wrow0, k, n)
    mx = np.abs(DZ) @ np.abs(W).T
    if dx_before is not None:
        mx = mx + np.abs(np.asarray(dx_before, F64))
    return mx, np.abs(X).T @ np.abs(DZ), np.abs(DZ).sum(0)


def bound(length, magnitude):
    return (length + 2) * U * magnitude


def chain_forward(x, layers):
    """layers [(W (k, n), shift (n), act)] in float64 -> the output of every layer"""
    acts, h = [], np.asarray(x, F64)
    for w, shift, act in layers:
        h = h @ w + shift
        if act:
            h = np.maximum(h, 0.0)
        acts.append(h)
    return acts


def chain_backward(x, layers, acts, dz_last, relu_input=False):
    """-> (dx, [(dW, dshift)]): the chain walked from its last layer, every hidden dz = the next call's masked dx"""
    grads, dz = [None] * len(layers), np.asarray(dz_last, F64)
    for li in range(len(layers) - 1, -1, -1):
        inp = np.asarray(x, F64) if li == 0 else acts[li - 1]
        masked = relu_input if li == 0 else bool(layers[li - 1][2])
        dz, dw, ds = linear_backward(inp, layers[li][0], dz, relu_input=masked)
        grads[li] = (dw, ds)
    return dz, grads


def fold(conv_w, conv_b=None, gamma=None, beta=None, mean=None, var=None, eps=0.0):
    """fold_layer in float64: conv_w (cout, cin) -> W (cin, cout), shift (cout)"""
    w = np.asarray(conv_w, F64).reshape(conv_w.shape[0], -1)
    if gamma is None:
        return w.T.copy(), (np.zeros(w.shape[0]) if conv_b is None else np.asarray(conv_b, F64))
    s = np.asarray(gamma, F64) / np.sqrt(np.asarray(var, F64) + eps)
    shift = np.asarray(beta, F64) - np.asarray(mean, F64) * s
    if conv_b is not None:
        shift = shift + np.asarray(conv_b, F64) * s
    return (w * s[:, None]).T.copy(), shift


def param_grads(d_w, d_shift, conv_w, conv_b=None, gamma=None, mean=None, var=None, eps=0.0):
    """the gradient of a folded block (d_w (cin, cout), d_shift (cout)) at the module's parameters, running statistics constant
    -> dict(conv_weight, conv_bias, bn_weight, bn_bias), None where the layer has no such parameter"""
    w = np.asarray(conv_w, F64).reshape(conv_w.shape[0], -1)
    bt, ds = np.asarray(d_w, F64).T, np.asarray(d_shift, F64)
    if gamma is None:
        return dict(conv_weight=bt.copy(), conv_bias=None if conv_b is None else ds, bn_weight=None, bn_bias=None)
    inv = 1.0 / np.sqrt(np.asarray(var, F64) + eps)
    s = np.asarray(gamma, F64) * inv
    d_gamma = (bt * w).sum(1) - np.asarray(mean, F64) * ds
    if conv_b is not None:
        d_gamma = d_gamma + np.asarray(conv_b, F64) * ds
    return dict(conv_weight=bt * s[:, None], conv_bias=None if conv_b is None else ds * s, bn_weight=d_gamma * inv, bn_bias=ds)


def blocks_of(seq):
    """an nn.Sequential of Conv(/BN/ReLU) blocks -> [(conv, bn or None, act)]"""
    import torch.nn as nn
    mods, out, i = list(seq), [], 0
    while i < len(mods):
        conv = mods[i]
        bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], (nn.BatchNorm1d, nn.BatchNorm2d)) else None
        j = i + (2 if bn is not None else 1)
        act = 1 if j < len(mods) and isinstance(mods[j], nn.ReLU) else 0
        out.append((conv, bn, act))
        i = j + act
    return out


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(F64)


def fold_sequential64(seq):
    """the float64 chain [(W, shift, act)] of a Sequential in eval mode, and per layer the arguments of param_grads"""
    layers, params = [], []
    for conv, bn, act in blocks_of(seq):
        p = dict(conv_w=_np(conv.weight), conv_b=_np(conv.bias))
        if bn is not None:
            p.update(gamma=_np(bn.weight), mean=_np(bn.running_mean), var=_np(bn.running_var), eps=bn.eps)
        w, shift = fold(beta=_np(bn.bias) if bn is not None else None, **p)
        layers.append((w, shift, act))
        params.append(p)
    return layers, params


def sequential_grads(seq, x, d_out, relu_input=False):
    """dL/dx and the gradients of every parameter of `seq` (named as in its state dict), given d_out = dL/d(output)"""
    layers, params = fold_sequential64(seq)
    acts = chain_forward(x, layers)
    dx, grads = chain_backward(x, layers, acts, d_out, relu_input=relu_input)
    named, i = {}, 0
    for (conv, bn, act), (dw, ds), p in zip(blocks_of(seq), grads, params):
        g = param_grads(dw, ds, **p)
        named['%d.weight' % i] = g['conv_weight'].reshape(conv.weight.shape)
        if conv.bias is not None:
            named['%d.bias' % i] = g['conv_bias']
        if bn is not None:
            named['%d.weight' % (i + 1)], named['%d.bias' % (i + 1)] = g['bn_weight'], g['bn_bias']
        i += 1 + (bn is not None) + act
    return acts[-1], dx, named
