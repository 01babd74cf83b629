"""Tensor wrappers of the sort-based samplers of libdet6d_hip_ext.so (include/det6d_ext.h): c-fps (the top-k of
sigmoid(score) ** gamma) and the pillar-density weights of df-fps.  Asynchronous on the current stream; nothing here reads a
result on the host, so all of it can be captured into a graph."""
import torch

from .. import _lib as L
from . import pointnet2_batch_hip as pn2


def topk_scores(scores, m, gamma=1.0, lo=0, hi=None, idx_out=None, idx_offset=0, idx_bias=0):
    """c-fps of the slice [lo, hi) of scores (B, N): the m highest sigmoid(score) ** gamma in descending order, NaN first,
    equal weights by ascending index.  Picks + lo + idx_bias go to idx_out[:, idx_offset:idx_offset + m] (a new (B, m) int32
    tensor when idx_out is None)."""
    L.require_cuda(scores, idx_out)
    b, n_total = scores.shape
    hi = n_total if hi is None or hi == -1 else hi
    if idx_out is None:
        idx_out = torch.empty((b, m), dtype=torch.int32, device=scores.device)
    L.call_ext("det6d_ext_topk_scores", b, n_total, lo, hi, m, L.ptr(scores), float(gamma), L.ptr(idx_out), idx_out.shape[1],
               idx_offset, idx_bias, L.stream_ptr())
    return idx_out


def pillar_weights(xyz, lo=0, hi=None):
    """(B, hi - lo) weights 1 / (points of the same scene and slice in the same 2 m x 2 m pillar) of xyz (B, N, 3): the
    weights of the reference's df-fps sampler, counted per scene"""
    L.require_cuda(xyz)
    b, n_total, _ = xyz.shape
    hi = n_total if hi is None or hi == -1 else hi
    weights = torch.empty((b, max(hi - lo, 0)), dtype=torch.float32, device=xyz.device)
    L.call_ext("det6d_ext_pillar_weights", b, n_total, lo, hi, L.ptr(xyz), L.ptr(weights), L.stream_ptr())
    return weights


def pillar_density_fps(xyz, m, lo=0, hi=None, idx_out=None, idx_offset=0):
    """df-fps of the slice [lo, hi) of xyz (B, N, 3): furthest_point_sample_weights(slice, pillar_weights, m) + lo into
    idx_out[:, idx_offset:idx_offset + m] (a new (B, m) int32 tensor when idx_out is None)"""
    b, n_total, _ = xyz.shape
    hi = n_total if hi is None or hi == -1 else hi
    n = hi - lo
    weights = pillar_weights(xyz, lo, hi)
    sl = xyz if (lo == 0 and hi == n_total) else xyz[:, lo:hi].contiguous()
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device=xyz.device)
    idx = torch.empty((b, m), dtype=torch.int32, device=xyz.device)
    pn2.furthest_point_sampling_weights_wrapper(b, n, m, sl, weights, temp, idx)
    if idx_out is None:
        return idx + lo if lo else idx
    idx_out[:, idx_offset:idx_offset + m] = idx + lo
    return idx_out
