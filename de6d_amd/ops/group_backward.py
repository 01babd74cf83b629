"""Tensor layer of the grouped-MLP backward of libdet6d_hip_ext.so (include/det6d_ext.h: det6d_ext_group_gather,
det6d_ext_group_pool_backward, det6d_ext_group_centre_grad, det6d_ext_vote_backward): the gradient of a set-abstraction
layer's radius groups with respect to their CENTRES and their parameters, and of the vote offsets' clamp.

  group_gather      X0 = [pts[idx] - centre | features[idx] | zeros] as a (B * M * ns, ld) matrix
  pool_backward     d(pooled) routed to the winning slot of every (centre, channel): the dz of the group's last layer
  centre_grad       minus the sum over a centre's slots of the first layer's three coordinate columns of dx
  vote_backward     the clamp mask of vote = candidate + clamp(off, -R, R)
  group_forward     the dense, layer-by-layer evaluation of one group, every layer written out
  GroupedChain      torch.autograd.Function over all groups of a layer (grouped_chain()): forward = group_forward + the masked
                    max-pool into one pooled tensor; backward = pool_backward, mlp_backward's layer calls, centre_grad
  VotePoints        torch.autograd.Function: fused.vote_points / vote_backward

Ball membership (idx, cnt) carries no gradient; the points' own coordinates and features are constants (nothing consumes their
gradient until a backbone backward exists); BatchNorm is frozen.  Asynchronous on the current stream; nothing here reads a
result on the host, so a step can be captured into a graph."""
import torch

from .. import _lib as L
from . import fused, mlp_backward

MAX_SLOTS = 128


def _f32(t, dims, what, who):
    if t.dim() != dims or t.dtype != torch.float32:
        raise L.Det6dError("%s: %s must be a %d-d float32 tensor, got %s %s" % (who, what, dims, tuple(t.shape), t.dtype))
    return t


def _i32(t, shape, what, who):
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape):
        raise L.Det6dError("%s: %s must be an int32 tensor of shape %s, got %s %s" % (who, what, tuple(shape), tuple(t.shape), t.dtype))
    return t


def group_gather(pts, idx, ctr, k=None, out=None):
    """pts (B, n, ldp) point rows [xyz | features | pad]; idx (B, M, ns) int32; ctr (B, M, >= 3) -> out (B * M * ns, ldout):
    columns [0, 3) = pts[idx] - ctr, [3, k) copied, [k, ldout) zero.  k defaults to ldp; out to a dense (rows, round4(k))."""
    who = "group_gather"
    L.require_cuda(pts, idx, ctr, out)
    _f32(pts, 3, 'pts', who), _f32(ctr, 3, 'ctr', who)
    b, n, ldp = pts.shape
    if idx.dim() != 3 or idx.shape[0] != b:
        raise L.Det6dError("%s: idx must be (B, M, ns) with B = %d, got %s" % (who, b, tuple(idx.shape)))
    _, m, ns = idx.shape
    _i32(idx, (b, m, ns), 'idx', who)
    if ctr.shape[0] != b or ctr.shape[1] != m or ctr.shape[2] < 3:
        raise L.Det6dError("%s: ctr must be (%d, %d, >= 3), got %s" % (who, b, m, tuple(ctr.shape)))
    k = ldp if k is None else k
    rows = b * m * ns
    if out is None:
        out = torch.empty((rows, fused.round4(k)), dtype=torch.float32, device=pts.device)
    if _f32(out, 2, 'out', who).shape[0] != rows:
        raise L.Det6dError("%s: out has %d rows, %d expected" % (who, out.shape[0], rows))
    L.call_ext("det6d_ext_group_gather", b, n, m, ns, L.ptr(pts), ldp, k, L.ptr(idx), L.ptr(ctr), ctr.shape[2], L.ptr(out),
               out.shape[1], L.stream_ptr())
    return out


def pool_backward(y, cnt, g, ns, c, gcol0=0, dz=None):
    """y (groups * ns, ldy): the last layer's ReLU output; cnt (groups,) int32 (any shape with that many elements); g (groups,
    ldg): d(pooled), the group's slice at columns [gcol0, gcol0 + c) -> dz (groups * ns, >= c): g at the lowest slot holding a
    positive maximum of a non-empty ball, zeros elsewhere.  dz defaults to a dense (rows, c)."""
    who = "pool_backward"
    L.require_cuda(y, cnt, g, dz)
    _f32(y, 2, 'y', who), _f32(g, 2, 'g', who)
    groups = g.shape[0]
    if ns < 1 or y.shape[0] != groups * ns:
        raise L.Det6dError("%s: y has %d rows, %d groups of %d expected" % (who, y.shape[0], groups, ns))
    _i32(cnt.reshape(-1), (groups,), 'cnt', who)
    if dz is None:
        dz = torch.empty((groups * ns, c), dtype=torch.float32, device=y.device)
    if _f32(dz, 2, 'dz', who).shape[0] != groups * ns:
        raise L.Det6dError("%s: dz has %d rows, %d expected" % (who, dz.shape[0], groups * ns))
    L.call_ext("det6d_ext_group_pool_backward", groups, ns, c, L.ptr(y), y.shape[1], L.ptr(cnt), L.ptr(g), g.shape[1], gcol0,
               L.ptr(dz), dz.shape[1], L.stream_ptr())
    return dz


def centre_grad(dx, ns, out=None):
    """dx (groups * ns, >= 3) -> out (groups, >= 3): columns [0, 3) = minus the slot sums, ascending"""
    who = "centre_grad"
    L.require_cuda(dx, out)
    _f32(dx, 2, 'dx', who)
    if ns < 1 or dx.shape[0] % ns:
        raise L.Det6dError("%s: dx has %d rows, no multiple of ns = %d" % (who, dx.shape[0], ns))
    groups = dx.shape[0] // ns
    if out is None:
        out = torch.empty((groups, 3), dtype=torch.float32, device=dx.device)
    if _f32(out, 2, 'out', who).shape[0] != groups:
        raise L.Det6dError("%s: out has %d rows, %d expected" % (who, out.shape[0], groups))
    L.call_ext("det6d_ext_group_centre_grad", groups, ns, L.ptr(dx), dx.shape[1], L.ptr(out), out.shape[1], L.stream_ptr())
    return out


def vote_backward(off, rng, dvote, out=None):
    """off (rows, >= 3): the UNCLAMPED offsets; rng = (Rx, Ry, Rz); dvote (rows, >= 3) -> out (rows, >= 3): columns [0, 3) =
    dvote where -R <= off <= R, else 0 (NaN: 0)"""
    who = "vote_backward"
    L.require_cuda(off, dvote, out)
    _f32(off, 2, 'off', who), _f32(dvote, 2, 'dvote', who)
    rows = off.shape[0]
    if dvote.shape[0] != rows:
        raise L.Det6dError("%s: off has %d rows, dvote %d" % (who, rows, dvote.shape[0]))
    if out is None:
        out = torch.empty((rows, 3), dtype=torch.float32, device=off.device)
    if _f32(out, 2, 'out', who).shape[0] != rows:
        raise L.Det6dError("%s: out has %d rows, %d expected" % (who, out.shape[0], rows))
    L.call_ext("det6d_ext_vote_backward", rows, L.ptr(off), off.shape[1], float(rng[0]), float(rng[1]), float(rng[2]),
               L.ptr(dvote), dvote.shape[1], L.ptr(out), out.shape[1], L.stream_ptr())
    return out


def group_forward(xyz_rows, idx, cnt, ctr, layers):
    """One radius group, dense and layer by layer.  xyz_rows (B, n, ld) point rows; idx (B, M, ns), cnt (B, M) the ball query's
    padded lists; ctr (B, M, 3); layers the folded chain [(W, shift, cout, act)] whose first W has ld rows
    -> (X0 (B * M * ns, ld), [activation of layer 0, ..., of the last layer]).
    X0 is what the backward needs as an operand (group_gather).  The first layer itself is det6d_linear's gathered mode on the
    point rows: it adds the three coordinate products LAST in the chain, as every grouped route of the eval forward does, so the
    activations are the bits those routes compute; a plain GEMM over X0 would add them first.  Hidden activations are
    (rows, padded width) with zeroed padding; the last one too.  Pooling (fused.group_maxpool) is the caller's step."""
    b, m, ns = idx.shape
    _i32(cnt.reshape(-1), (b * m,), 'cnt', "group_forward")
    w0 = layers[0][0]
    if w0.shape[0] != xyz_rows.shape[-1]:
        raise L.Det6dError("group_forward: the first layer has %d weight rows, the point rows %d floats" % (w0.shape[0], xyz_rows.shape[-1]))
    x0 = group_gather(xyz_rows, idx, ctr, out=torch.empty((b * m * ns, w0.shape[0]), dtype=torch.float32, device=xyz_rows.device))
    first = fused.layer(xyz_rows, layers[0], idx=idx, ctr=ctr)
    return x0, [first] + fused.run_chain(first, layers[1:], keep=True)


class GroupedChain(torch.autograd.Function):
    """pooled = GroupedChain.apply(ctr, rows_pts, spec, *tensors); use grouped_chain().  spec = (found, [[(cout, act)] per
    group], pooled_width); tensors = W, shift of every layer, group by group.  Gradients reach ctr and every W and shift that
    requires one, not rows_pts."""

    @staticmethod
    def forward(ctx, ctr, rows_pts, spec, *tensors):
        found, group_specs, pooled_width = spec
        ctr, rows_pts = ctr.detach().contiguous(), rows_pts.detach()
        b, m = ctr.shape[0], ctr.shape[1]
        it = iter(tensors)
        groups = [[(next(it).detach(), next(it).detach(), c, a) for c, a in s] for s in group_specs]
        pooled = fused.pooled_buffer(b * m, pooled_width, ctr.device)
        saved, col = [], 0
        for (cnt, idx), layers in zip(found, groups):
            if layers[-1][3] != 1:
                raise NotImplementedError("GroupedChain pools ReLU outputs: the last layer of a group must have its ReLU")
            ns = idx.shape[2]
            if ns > MAX_SLOTS:
                raise NotImplementedError("GroupedChain: nsample = %d (at most %d)" % (ns, MAX_SLOTS))
            x0, acts = group_forward(rows_pts, idx, cnt, ctr, layers)
            fused.group_maxpool(acts[-1], ns, layers[-1][2], cnt, pooled, col)
            saved.append((x0, acts, cnt, ns, col))
            col += layers[-1][2]
        if col != pooled_width:
            raise L.Det6dError("grouped_chain: the groups pool %d channels, pooled_width = %d" % (col, pooled_width))
        ctx.groups, ctx.saved, ctx.ctr_shape = groups, saved, tuple(ctr.shape)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        need_ctr = ctx.needs_input_grad[0]
        flags = ctx.needs_input_grad[3:]
        need_p = any(flags)
        d_pooled = d_pooled.detach().to(torch.float32).contiguous()
        d_ctr, out = None, []
        for layers, (x0, acts, cnt, ns, col) in zip(ctx.groups, ctx.saved):
            if not (need_ctr or need_p):
                out += [None, None] * len(layers)
                continue
            dz = pool_backward(acts[-1], cnt, d_pooled, ns, layers[-1][2], gcol0=col)
            grads = []
            if len(layers) > 1:                                  # layers 1 ..: their input is layer 0's ReLU output
                dz, grads = mlp_backward.chain_backward(acts[0], layers[1:], acts[1:], dz, k0=layers[0][2], relu_input=True,
                                                        need_params=need_p)
                grads = grads or [None] * (len(layers) - 1)
            w0, _, c0, _ = layers[0]
            first = None
            if need_p:                                           # the first layer's dw over every column of X0, no dx
                full, ds = torch.zeros_like(w0), torch.empty((c0,), dtype=torch.float32, device=w0.device)
                mlp_backward.linear_backward(x0, w0, dz, k=w0.shape[0], n=c0, need=(False, True, True), dw=full, dshift=ds)
                first = (full, ds)
            if need_ctr:                                         # ... and only the three coordinate columns of its dx
                dx0, _, _ = mlp_backward.linear_backward(x0, w0, dz, k=3, wrow0=0, n=c0, need=(True, False, False))
                g = centre_grad(dx0, ns)
                d_ctr = g if d_ctr is None else d_ctr + g        # the groups' parts are added in group order
            for pair in [first] + list(grads):
                out += list(pair) if pair is not None else [None, None]
        out = [g if f else None for g, f in zip(out, flags)]
        if d_ctr is not None:
            d_ctr = d_ctr.view(ctx.ctr_shape)
        return (d_ctr, None, None) + tuple(out)


def grouped_chain(rows_pts, ctr, found, groups, pooled_width):
    """rows_pts (B, n, ld) point rows; ctr (B, M, 3) the centres; found [(cnt (B, M), idx (B, M, ns))] per group (the ball
    queries around ctr, dense padded lists); groups [[(W, shift, cout, act)]] per group, on the device (folded_params gives them
    a graph to the module's parameters) -> pooled (B * M, round4(pooled_width)), padding columns zero."""
    spec = (list(found), [[(c, a) for _, _, c, a in g] for g in groups], pooled_width)
    tensors = [t for g in groups for w, s, _, _ in g for t in (w, s)]
    return GroupedChain.apply(ctr, rows_pts, spec, *tensors)


class VotePoints(torch.autograd.Function):
    """vote (B, P, 3) = VotePoints.apply(off (B * P, >= 3), cand_rows (B, P, ld), (Rx, Ry, Rz)): fused.vote_points; the backward
    is the clamp mask on the unclamped offsets (at off == +-R the whole gradient passes)."""

    @staticmethod
    def forward(ctx, off, cand_rows, rng):
        off = off.detach().contiguous()
        b, p = cand_rows.shape[0], cand_rows.shape[1]
        vote = torch.empty((b, p, 3), dtype=torch.float32, device=off.device)
        fused.vote_points(off, cand_rows.detach(), rng, vote)
        ctx.off, ctx.rng = off, tuple(float(v) for v in rng)
        return vote

    @staticmethod
    def backward(ctx, d_vote):
        off = ctx.off
        d_vote = d_vote.detach().to(torch.float32).contiguous().view(-1, 3)
        out = torch.empty_like(off) if off.shape[1] == 3 else torch.zeros_like(off)
        vote_backward(off, ctx.rng, d_vote, out=out)
        return out, None, None
