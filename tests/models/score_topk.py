"""Executable CPU model of c-fps (det6d_ext_topk_scores, de6d_amd/csrc/ext/sort_samplers.hip) — TEST INFRASTRUCTURE ONLY.

The reference's c-fps (pointnet2_modules.py:425-430) is scores_slice.sigmoid() ** WEIGHT_GAMMA followed by .topk(npoint).
torch.topk leaves the order of equal values open (its CPU and CUDA forms differ), so the engine fixes one:
  * w[k] = d6_sigmoid_powf(score[k], gamma) (include/det6d_math.h; oracle.ops.sigmoid_pow), the weights S-FPS sees;
  * larger w first; NaN counts as larger than every number, as in torch.topk; among equal w (-0 equals +0) and among NaNs
    the lower index first.
"""
import numpy as np

from oracle import ops

F32 = np.float32


def weights(scores, gamma=1.0):
    return ops.sigmoid_pow(np.ascontiguousarray(scores, F32), gamma)


def order(w):
    """indices of w (n,) in the engine's order: NaNs first, then descending value; ties by ascending index"""
    w = np.asarray(w, F32)
    nan = np.isnan(w)
    value = np.where(nan, F32(0), w)
    # lexsort: last key is the primary one and the sort is stable, so equal (nan, value) pairs stay in index order
    return np.lexsort((-value, ~nan)).astype(np.int32)


def topk_weights(w, m):
    """the rule on given weights (n,) -> (m,) int32"""
    assert 0 <= m <= len(w)
    return order(w)[:m]


def topk_scores(scores, m, gamma=1.0):
    """c-fps of one scene: scores (n,) -> (m,) int32 picks"""
    return topk_weights(weights(scores, gamma), m)
