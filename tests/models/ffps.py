"""Executable CPU model of F-FPS (de6d_amd/csrc/ext/fps_features.hip, include/det6d_ext.h) — TEST INFRASTRUCTURE ONLY.

The reference's f-fps (pointnet2_modules.py:382-387) is furthest_point_sampling_matrix_kernel (sampling_gpu.cu:268-373) on
cdist(xyz, xyz) + cdist(f, f) * gamma (pointnet2_utils.py:37-44).  torch.cdist (above 25 rows) is the matrix-multiply form
[-2x, |x|^2, 1] . [y, 1, |y|^2], clamp_min(0), sqrt; its GEMM summation order is not specified, so the engine fixes its own:
  * |v|^2: sequential sum of rounded squares in channel order (numpy float32, below);
  * G(i, j): ONE ascending fmaf chain from 0 over (-2 v_i) . v_j, then + |v_i|^2, then + |v_j|^2 — exactly what
    oracle.ops.linear computes for the row [-2 v_i, |v_i|^2, 1] against the columns [v_j; 1; |v_j|^2] (numpy has no fmaf,
    and emulating one in float64 rounds twice);
  * d = sqrt(clamp(G_xyz)) + fl(sqrt(clamp(G_feat)) * gamma), clamp(g) = g <= 0 ? 0 : g (NaN stays NaN);
  * selection: the reference's rule restated lane by lane — first pick 0, temp from 1e10, d2 = fminf(d, temp) (a NaN distance
    is ignored), every thread tid of S = opt_n_threads(n) keeps a strict > maximum over k = tid + i S (start -1, index 0),
    then the halving tree keeps v2 > v1 ? i2 : i1.
"""
import math

import numpy as np

from oracle import ops

F32 = np.float32


def opt_n_threads(n):
    """cuda_utils.h:10-14"""
    return max(min(1 << int(math.log(n) / math.log(2.0)), 1024), 1)


def norms(v):
    """(n, C) -> (n,): sequential sum of rounded squares, channel order"""
    v = np.asarray(v, F32)
    s = np.zeros(v.shape[0], F32)
    for c in range(v.shape[1]):
        s = (s + (v[:, c] * v[:, c]).astype(F32)).astype(F32)
    return s


class Gram:
    """rows G(i, :) of one point set: i in the x role (the last pick), every point in the y role"""

    def __init__(self, v):
        v = np.ascontiguousarray(v, F32)
        self.v, self.n2 = v, norms(v)
        n, c = v.shape
        self.w = np.ascontiguousarray(np.concatenate([v.T, np.ones((1, n), F32), self.n2[None, :]], 0))   # (c + 2, n)

    def row(self, i):
        a = np.concatenate([F32(-2) * self.v[i], [self.n2[i], F32(1)]]).astype(F32)[None, :]
        return ops.linear(a, self.w)[0]


def clamp0(g):
    return np.where(g <= 0, F32(0), g).astype(F32)


class Distances:
    """d(i, :) = sqrt(clamp(G_xyz(i, :))) + fl(sqrt(clamp(G_feat(i, :))) * gamma)"""

    def __init__(self, xyz, feats, gamma):
        self.gx = Gram(xyz)
        self.gf = Gram(np.zeros((len(xyz), 0), F32) if feats is None else feats)
        self.gamma = F32(gamma)

    def xyz_row(self, i):
        with np.errstate(invalid='ignore'):
            return np.sqrt(clamp0(self.gx.row(i)))

    def row(self, i):
        with np.errstate(invalid='ignore', over='ignore'):
            df = (np.sqrt(clamp0(self.gf.row(i))) * self.gamma).astype(F32)
            return (self.xyz_row(i) + df).astype(F32)


def select(n, m, row_of, temp=None, margins=None):
    """the reference's matrix sampler on rows row_of(old) (n,) -> (m,) int32 picks.  margins: a list that receives, per round,
    (best - runner-up) of the running min-distances"""
    S = opt_n_threads(n)
    temp = np.full(n, 1e10, F32) if temp is None else np.asarray(temp, F32).copy()
    out = np.zeros(m, np.int32)
    if m == 0:
        return out
    old = 0
    nslots = (n + S - 1) // S
    for r in range(1, m):
        d = np.asarray(row_of(old), F32)
        temp = np.fmin(d, temp)
        best = np.full(S, F32(-1), F32)
        besti = np.zeros(S, np.int64)
        for i in range(nslots):
            k = np.arange(S) + i * S
            ok = k < n
            t = np.where(ok, temp[np.minimum(k, n - 1)], F32(-np.inf))
            up = ok & (t > best)
            besti = np.where(up, k, besti)
            best = np.where(up, t, best)
        s = S // 2
        while s >= 1:
            v1, v2, i1, i2 = best[:s], best[s:2 * s], besti[:s], besti[s:2 * s]
            besti = np.concatenate([np.where(v2 > v1, i2, i1), besti[s:]])
            best = np.concatenate([np.fmax(v1, v2), best[s:]])
            s //= 2
        old = int(besti[0])
        out[r] = old
        if margins is not None:
            rest = np.delete(temp, old)
            margins.append(float(temp[old]) - float(rest.max()) if len(rest) else np.inf)
    return out


def fps_features(xyz, feats, m, gamma=1.0, margins=None):
    """one scene: xyz (n, 3), feats (n, C) or None -> (m,) picks of det6d_ext_fps_features"""
    dist = Distances(xyz, feats, gamma)
    return select(len(xyz), m, dist.row, margins=margins)


def fps_matrix(matrix, m, temp=None):
    """one scene of det6d_ext_fps_matrix: (n, n) -> (m,) picks"""
    matrix = np.asarray(matrix, F32)
    return select(matrix.shape[0], m, lambda i: matrix[i], temp)


def rows_of(xyz, feats):
    """(B, n, 3), (B, n, C) -> the kernel's rows (B, n, ld) [xyz | features | 0-pad], ld = round4(3 + C)"""
    b, n, _ = xyz.shape
    c = feats.shape[-1]
    rows = np.zeros((b, n, (3 + c + 3) // 4 * 4), F32)
    rows[..., :3] = xyz
    rows[..., 3:3 + c] = feats
    return rows
