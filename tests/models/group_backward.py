"""float64 model of the grouped-MLP backward (include/det6d_ext.h: det6d_ext_group_gather, det6d_ext_group_pool_backward,
det6d_ext_group_centre_grad, det6d_ext_vote_backward; de6d_amd/ops/group_backward.py): the four entry points, and a whole radius
group's forward and backward built on tests/models/mlp_backward.py.

A radius group: X0[(c, s)] = [pts[idx[c][s]][:3] - ctr[c] | pts[idx[c][s]][3:k]] -> pointwise layers -> Y; Y *= (cnt[c] > 0);
pooled[c][j] = max_s Y[(c, s)][j].  idx and cnt are constants (ball membership carries no gradient), and so are the points.
Everything is NumPy float64, with one exception that is part of the contract: the gather's subtract is ONE operation in the
precision of its inputs (fp32 inputs give the correctly rounded fp32 difference, the bits the kernel writes)."""
import numpy as np

from . import mlp_backward as mlp

F64 = np.float64


def padded_query(rng, b, n, m, ns, counts=None):
    """a ball query's padded lists without the geometry: cnt (b, m) hits per centre (0 .. ns, the given `counts` first, then
    random), idx (b, m, ns) with the hits in slots [0, cnt) and the FIRST hit repeated in the padding slots; an empty ball's row
    is all zeros, as the query leaves it"""
    cnt = rng.integers(0, ns + 1, size=(b, m)).astype(np.int32)
    flat = cnt.reshape(-1)
    for i, v in enumerate(counts or ()):
        if i < flat.size:
            flat[i] = min(v, ns)
    idx = np.zeros((b, m, ns), np.int32)
    for bi in range(b):
        for c in range(m):
            k = int(cnt[bi, c])
            if k:
                hits = rng.choice(n, size=min(k, n), replace=False)
                hits = np.resize(hits, k)
                idx[bi, c, :k] = hits
                idx[bi, c, k:] = hits[0]
    return cnt, idx


def group_gather(pts, idx, ctr, k=None, ldout=None):
    """pts (b, n, ldp), idx (b, m, ns), ctr (b, m, >= 3) -> (b * m * ns, ldout) float64: [pts[idx][:3] - ctr | pts[idx][3:k] | 0]"""
    b, n, ldp = pts.shape
    _, m, ns = idx.shape
    k = ldp if k is None else k
    ldout = k if ldout is None else ldout
    g = pts[np.arange(b)[:, None, None], idx]                      # (b, m, ns, ldp)
    out = np.zeros((b, m, ns, ldout), F64)
    out[..., :3] = g[..., :3] - np.asarray(ctr)[:, :, None, :3]     # one subtract, in the inputs' precision
    out[..., 3:k] = g[..., 3:k]
    return out.reshape(b * m * ns, ldout)


def winners(y, ns, c):
    """(groups, c): the LOWEST slot whose value equals the maximum over the ns slots of the group"""
    y = np.asarray(y, F64)[:, :c].reshape(-1, ns, c)
    return y.argmax(axis=1), y.max(axis=1)                          # argmax returns the first occurrence


def pool_forward(y, cnt, ns, c):
    _, top = winners(y, ns, c)
    return np.where(np.asarray(cnt).reshape(-1, 1) > 0, top, 0.0)


def pool_backward(y, cnt, g, ns, c, gcol0=0):
    """-> dz (groups * ns, c): g[r][gcol0 + j] at the winning slot of (r, j) when cnt[r] > 0 and the maximum is positive (the
    last layer's ReLU), zeros elsewhere"""
    win, top = winners(y, ns, c)
    groups = win.shape[0]
    passes = (np.asarray(cnt).reshape(-1, 1) > 0) & (top > 0)
    dz = np.zeros((groups, ns, c), F64)
    gi, ji = np.nonzero(passes)
    dz[gi, win[gi, ji], ji] = np.asarray(g, F64)[gi, gcol0 + ji]
    return dz.reshape(groups * ns, c)


def centre_grad(dx, ns):
    dx = np.asarray(dx, F64)[:, :3]
    return -dx.reshape(-1, ns, 3).sum(axis=1)


def vote_points(off, cand, rng):
    r = np.asarray(rng, F64)
    o = np.asarray(off, F64)[:, :3]
    o = np.where(o > -r, o, -r)                                      # the kernel's selects: a NaN ends on -R
    o = np.where(o < r, o, r)
    return np.asarray(cand, F64)[:, :3] + o


def vote_backward(off, rng, dvote):
    r = np.asarray(rng, F64)
    o = np.asarray(off, F64)[:, :3]
    with np.errstate(invalid='ignore'):
        inside = (o >= -r) & (o <= r)                                # a NaN compares false
    return np.where(inside, np.asarray(dvote, F64)[:, :3], 0.0)


def group_forward(pts, idx, cnt, ctr, layers):
    """layers [(W (k, n), shift (n), act)] float64 -> (X0, activations, pooled (b * m, n_last))"""
    ns = idx.shape[2]
    k = layers[0][0].shape[0]
    x0 = group_gather(np.asarray(pts, F64), idx, np.asarray(ctr, F64), k=k)
    acts = mlp.chain_forward(x0, layers)
    return x0, acts, pool_forward(acts[-1], cnt, ns, layers[-1][0].shape[1])


def group_backward(x0, layers, acts, cnt, ns, d_pooled, gcol0=0, win_dz=None):
    """-> (d_ctr (groups, 3), [(dW, dshift)]).  win_dz: a dz of the last layer to use instead of the model's own routing"""
    c = layers[-1][0].shape[1]
    dz = pool_backward(acts[-1], cnt, d_pooled, ns, c, gcol0) if win_dz is None else np.asarray(win_dz, F64)
    dx0, grads = mlp.chain_backward(x0, layers, acts, dz)
    return centre_grad(dx0, ns), grads
