"""CPU checks of the F-FPS model (tests/models/ffps.py): its distances are torch.cdist's within rounding, its picks are the
reference's on tests/golden/ffps_ref.npz, the selection rule's edge cases, and the inequality behind the kernel's skip."""
import os

import numpy as np
import pytest
import torch

from tests.models import ffps

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ffps_ref.npz')


def scene(seed, n, c):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(0, 70.4, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n)], 1).astype(F32)
    return xyz, np.maximum(rng.standard_normal((n, c)), 0).astype(F32)


def brute(n, m, row_of):
    """plain restatement: arg-max of the running min-distances, ties to the smallest (bitrev(k mod S), k)"""
    S = ffps.opt_n_threads(n)
    bits = S.bit_length() - 1
    key = [(int(format(k % S, '0%db' % bits)[::-1], 2) if bits else 0, k) for k in range(n)]
    temp = np.full(n, 1e10, F32)
    out, old = [0], 0
    for _ in range(1, m):
        temp = np.fmin(np.asarray(row_of(old), F32), temp)
        top = temp.max()
        cands = [k for k in range(n) if temp[k] == top]
        old = min(cands, key=lambda k: key[k])
        out.append(old)
    return np.array(out, np.int32)


@pytest.mark.parametrize("c,gamma", [(32, 1.0), (64, 0.5)])
def test_model_distances_match_torch_cdist(oracle_ops, c, gamma):
    xyz, f = scene(3, 300, c)
    x, ft = torch.from_numpy(xyz)[None], torch.from_numpy(f)[None]
    want = (torch.cdist(x, x) + torch.cdist(ft, ft) * gamma)[0].numpy()
    dist = ffps.Distances(xyz, f, gamma)
    for i in (0, 7, 150, 299):
        got = dist.row(i)
        np.testing.assert_allclose(got, want[i], rtol=1e-4, atol=1e-2)


def test_model_picks_equal_the_golden_reference_picks(oracle_ops):
    g = np.load(GOLDEN)
    for si in range(int(g['nscenes'])):
        n, c, m = (int(v) for v in g['meta%d' % si])
        got = ffps.fps_features(g['xyz%d' % si], g['feats%d' % si], m, float(g['gamma%d' % si]))
        np.testing.assert_array_equal(got, g['picks%d' % si], err_msg='scene %d' % si)
        if 'matrix%d' % si in g:
            np.testing.assert_array_equal(ffps.fps_matrix(g['matrix%d' % si], m), g['picks%d' % si])


@pytest.mark.parametrize("case", ["duplicates", "equal_features", "n_1000", "n_40", "m_eq_n", "gamma_0"])
def test_selection_edge_cases_against_brute_force(oracle_ops, case):
    n, c, m, gamma = 300, 16, 60, 1.0
    xyz, f = scene(5, 1000 if case == "n_1000" else 40 if case == "n_40" else n, c)
    if case == "duplicates":
        xyz[1::2], f[1::2] = xyz[0::2], f[0::2]
    if case == "equal_features":
        f[:] = 0.5
    if case == "gamma_0":
        gamma = 0.0
    n = len(xyz)
    if case in ("n_40", "m_eq_n"):
        m = n
    dist = ffps.Distances(xyz, f, gamma)
    got = ffps.fps_features(xyz, f, m, gamma)
    np.testing.assert_array_equal(got, brute(n, m, dist.row))


def test_matrix_rule_on_ties_and_negative_entries(oracle_ops):
    rng = np.random.default_rng(9)
    mat = rng.integers(0, 4, (70, 70)).astype(F32)          # many exact ties
    np.testing.assert_array_equal(ffps.fps_matrix(mat, 70), brute(70, 70, lambda i: mat[i]))
    neg = -np.ones((64, 64), F32) * 3                       # nothing beats -1: every pick is point 0
    assert ffps.fps_matrix(neg, 5).tolist() == [0] * 5
    nan = mat[:64, :64].copy()
    nan[::3] = np.nan                                       # fminf ignores a NaN distance
    np.testing.assert_array_equal(ffps.fps_matrix(nan, 20), brute(64, 20, lambda i: nan[i]))


def test_skip_inequality_holds_on_adversarial_data(oracle_ops):
    """d >= d_xyz in floating point (NaN aside): a point whose min-distance is <= d_xyz keeps it whatever its features"""
    rng = np.random.default_rng(11)
    n = 200
    xyz = (rng.standard_normal((n, 3)) * np.array([1e-3, 1e4, 1.0])).astype(F32)
    f = (rng.standard_normal((n, 8)) * 10.0 ** rng.integers(-30, 30, (n, 1))).astype(F32)
    f[5] = np.inf
    f[6] = np.nan
    xyz[7] = xyz[8]
    for gamma in (0.0, 1e-30, 1.0, 3e38):
        with np.errstate(over='ignore', invalid='ignore'):
            dist = ffps.Distances(xyz, f, gamma)
            for i in (0, 5, 6, 7, 100):
                d, dx = dist.row(i), dist.xyz_row(i)
                assert (np.isnan(d) | (d >= dx)).all(), (gamma, i)
