"""Tensor wrappers of the F-FPS entry points of libdet6d_hip_ext.so (include/det6d_ext.h): feature-space farthest point
sampling without the distance matrix, and the reference's matrix sampler.  Asynchronous on the current stream."""
import torch

from .. import _lib as L


def workspace(b, n, device='cuda'):
    """scratch of one det6d_ext_fps_features launch over b scenes of n points (per-point norms + per-scene counters)"""
    nbytes = int(L.ext_lib().det6d_ext_fps_features_workspace_bytes(b, n))
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)


def skip_stats(ws, b, n):
    """(point-rounds whose feature row was read, wave-rounds that read any) per scene, from the workspace of the last launch
    on it (synchronises)"""
    off = int(L.ext_lib().det6d_ext_fps_features_workspace_bytes(b, n)) - b * 128
    words = ws[off:off + b * 128].view(torch.int32).view(b, 16, 2).cpu().to(torch.int64)
    return words[:, :, 0].sum(1), words[:, :, 1].sum(1)


def fps_features(rows, c, m, gamma=1.0, lo=0, hi=None, idx_out=None, idx_offset=0, idx_bias=0, ws=None):
    """F-FPS of the slice [lo, hi) of rows (B, N, ld) [x, y, z, f_0 .. f_{c-1}, pad] on cdist(xyz) + cdist(f) * gamma.
    Picks + lo + idx_bias go to idx_out[:, idx_offset:idx_offset + m] (a new (B, m) int32 tensor when idx_out is None)."""
    L.require_cuda(rows, idx_out)
    b, n_total, ld = rows.shape
    hi = n_total if hi is None or hi == -1 else hi
    if idx_out is None:
        idx_out = torch.empty((b, m), dtype=torch.int32, device=rows.device)
    if ws is None:
        ws = workspace(b, hi - lo, rows.device)
    L.call_ext("det6d_ext_fps_features", b, n_total, lo, hi, m, L.ptr(rows), ld, c, float(gamma), L.ptr(ws),
               ws.numel(), L.ptr(idx_out), idx_out.shape[1], idx_offset, idx_bias, L.stream_ptr())
    return idx_out


def fps_matrix(matrix, m, temp=None):
    """furthest_point_sample_matrix: FPS on a (B, N, N) distance matrix -> (B, m) int32; temp (B, N) starts at 1e10 unless
    given (it holds the final min-distances afterwards)"""
    L.require_cuda(matrix, temp)
    b, n, n2 = matrix.shape
    assert n == n2, "a (B, N, N) matrix"
    if temp is None:
        temp = torch.full((b, n), 1e10, dtype=torch.float32, device=matrix.device)
    idx = torch.empty((b, m), dtype=torch.int32, device=matrix.device)
    L.call_ext("det6d_ext_fps_matrix", b, n, m, L.ptr(matrix), L.ptr(temp), L.ptr(idx), L.stream_ptr())
    return idx
