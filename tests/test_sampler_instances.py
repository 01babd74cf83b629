"""Every kernel instance the sampler launchers can pick, bit for bit.

Each sampler launcher picks one of many template instances from the point count n (S = 2 ** min(10, floor(log2 n)) virtual
threads, ppt = ceil(n / S) points per thread).  The instances differ in exactly what the tie rule (bitrev(k mod S), k) depends
on -- LOG2T, log2vpt, log2pptv, the slot-to-point map, one-wave versus many-wave reduction -- so a mistake in one of them is
invisible to a test of another.  This module

  * restates the three selection rules (launch_fps of csrc/fps.hip, the PPT ladder of csrc/ext/fps_features.hip, the LOGN
    switch of csrc/ext/sort_samplers.hip) as pure functions and checks, WITHOUT a GPU, that the case tables below reach every
    instance the launchers' own tables name, in every form a launcher can give it (test_case_tables_reach_every_instance: a
    size added to a launcher without a case here fails it);
  * runs every case of those tables on the GPU against the oracle (oracle/det6d_oracle.c) or the CPU models (tests/models),
    assert_array_equal throughout: no tolerance anywhere in this file.

Scenes: every D-FPS / S-FPS call carries (a) a KITTI-like cloud with 10 % exact duplicates, (b) a lattice cloud (integer
coordinates in [0, 8)^3: thousands of exact duplicates and exact distance ties, so the picks are decided by the tie rule), and
(c) a cloud whose points are all equal.  m = min(n, 300); sizes up to 2048 run a second time with m = n, whose tail is made of
zero-distance ties only.

Out of scope here (LABNOTES.md, open): non-finite coordinates on the multi-pick and cooperative routes.
"""
import itertools
import math
import os
import re

import numpy as np
import pytest

from tests.models import ffps, pillar_density, score_topk
from tests.util import make_batch

F32 = np.float32
gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'de6d_amd', 'csrc')


# ---- the selection rules, restated ---------------------------------------------------------------------------------------
#: launch_fps: n -> (LOG2T, SLOTS) of the fat-thread kernel that holds exactly n = SLOTS << LOG2T points
FAT = {16384: (9, 32), 8192: (9, 16), 4096: (9, 8), 2048: (7, 16), 1024: (6, 16), 512: (6, 8), 256: (6, 4), 128: (6, 2)}
#: points per thread of the register kernels (fps_reg_kernel, ffps_features_kernel, ffps_matrix_kernel)
PPT_LADDER = (1, 2, 4, 8, 16)
#: det6d_fps_fused: sizes that leave the one-pick family
MULTI_PICK = (16384, 4096)
COOPERATIVE = (32768, 65536)
SORT_MIN_LOG, SORT_MAX_LOG = 8, 14


def log2s(n):
    """fps_opt_n_threads_log2 (csrc/fps_common.h): int(log(n) / log(2)) clamped to [0, 10]"""
    return max(0, min(10, int(math.log(n) / math.log(2.0))))


def points_per_thread(n):
    return -(-n // (1 << log2s(n)))


def fps_instance(n, weighted, fused):
    """the kernel one D-FPS (weighted=False) / S-FPS (True) launch over n points runs: through the reference-shaped wrappers
    (fused=False: det6d_fps, det6d_fps_weights) or through det6d_fps_fused (True; weighted then means "with scores", whose
    free workspace lets the fat-thread kernels score in fp32 with the guarded exact launch behind: 'fastw')"""
    if fused and n in MULTI_PICK:
        return ('multi-pick',)
    if fused and not weighted and n in COOPERATIVE:
        return ('cooperative',)
    form = 'weighted' if weighted else 'plain'
    if n in FAT:
        return ('fat',) + FAT[n] + ('fastw' if weighted and fused else form,)
    ppt = points_per_thread(n)
    for p in PPT_LADDER:
        if ppt <= p:
            return ('reg', p, form)
    return ('mem', form)


def ffps_ppt(n):
    """PPT of ffps_features_kernel / ffps_matrix_kernel (n <= 16384)"""
    assert 0 < n <= 16384
    return next(p for p in PPT_LADDER if points_per_thread(n) <= p)


def sort_logn(n):
    """LOGN of topk_scores_kernel / pillar_weights_kernel (n <= 16384)"""
    assert 0 < n <= 1 << SORT_MAX_LOG
    l = SORT_MIN_LOG
    while (1 << l) < n:
        l += 1
    return l


# ---- the case tables -----------------------------------------------------------------------------------------------------
#: (n, weighted) through farthest_point_sampling_wrapper / furthest_point_sampling_weights_wrapper:
#: reg<1> (32: dead lanes in the 64-thread block), reg<2> with most second slots dead, reg<4>, reg<8>, reg<16>, mem, the fat sizes
FPS_SIZES = (2, 32, 64, 65, 129, 2049, 4097, 8191, 8193, 16383, 16385, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
FPS_CASES = [(n, weighted) for n in FPS_SIZES for weighted in (False, True)]
#: (slice length, with scores) through fused.fps_fused; 3000 is no table size (flags non-null, ignored by the register kernel)
FUSED_CASES = [(n, False) for n in (128, 256, 1024, 2048)] + [(n, True) for n in (128, 256, 512, 1024, 2048, 8192, 3000)]
#: (n, c, m, kind) through ops.ffps.fps_features
FFPS_CASES = [(4097, 16, 200, 'plain'), (8192, 32, 256, 'plain'), (5000, 24, 128, 'slice'), (6000, 16, 128, 'duplicates'),
              (512, 8, 64, 'plain'), (700, 8, 64, 'plain'), (2100, 8, 64, 'plain'), (8200, 8, 64, 'plain')]
#: (n, b, m) through furthest_point_sample_matrix; (8200, 1, 64) is about 270 MB on the device
FFPM_CASES = [(512, 2, 300), (700, 2, 300), (2500, 2, 300), (4200, 2, 300), (8200, 1, 64)]
TOPK_SIZES = (40, 256, 257, 600, 2048, 3000, 4097, 8192, 8193)
PILLAR_SIZES = (256, 257, 600, 2048, 3000, 4097, 8192, 8193)
#: one size per kernel class (fat, register, memory) for the dead branches and the caller-supplied min-distances
CLASS_SIZES = (256, 1000, 16385)


def fps_ms(n):
    """m = min(n, 300) (200 on the memory-resident kernel); up to 2048 points also m = n"""
    first = min(n, 200 if n > 16384 else 300)
    return (first, n) if first < n <= 2048 else (first,)


# ---- host only: the tables against the launchers' sources ----------------------------------------------------------------
def macro_uses(text, name, pattern):
    """the arguments of every use of macro `name` that `pattern` finds; every use but the #define must be found"""
    found = re.findall(pattern, text)
    assert len(re.findall(r'\b%s\(' % name, text)) == len(found) + 1, 'a use of %s( that %r does not read' % (name, pattern)
    return found


def instances_in_sources(csrc=CSRC):
    """what the launchers can pick, read from their own tables"""
    def read(*path):
        with open(os.path.join(csrc, *path)) as f:
            return f.read()
    fps = read('fps.hip')
    feat = read('ext', 'fps_features.hip')
    sort = read('ext', 'sort_samplers.hip')
    fat = {int(n): (int(lt), int(sl))
           for n, lt, sl in macro_uses(fps, 'FPS_FAT', r'if \(n == (\d+)\) FPS_FAT\((\d+), (\d+)\);')}
    body = re.search(r'#define SORT_DISPATCH\(LOG, CASE\)(.*?)\n\n', sort, re.S).group(1)
    labels = re.findall(r'(?:case (\d+)|default): CASE\((\d+)\); break;', body)
    assert len(labels) == len(re.findall(r'CASE\(', body)), 'a line of SORT_DISPATCH that the pattern does not read'
    assert all(lab in ('', arg) for lab, arg in labels), labels
    return {'fat': fat,
            'reg': [int(p) for p in macro_uses(fps, 'FPS_CASE', r'FPS_CASE\((\d+)\);')],
            'mem': len(re.findall(r'hipLaunchKernelGGL\(\(fps_mem_kernel<W>\), grid, block,', fps)),
            'ffps': [int(p) for p in macro_uses(feat, 'FFPS_CASE', r'FFPS_CASE\((\d+)\);')],
            'ffpm': [int(p) for p in macro_uses(feat, 'FFPM_CASE', r'FFPM_CASE\((\d+)\);')],
            'sort': sorted(int(arg) for _, arg in labels)}


def check_tables(csrc=CSRC):
    src = instances_in_sources(csrc)
    # the restated rules use the launchers' tables
    assert src['fat'] == FAT
    assert all(n == sl << lt for n, (lt, sl) in src['fat'].items())
    assert src['reg'] == src['ffps'] == src['ffpm'] == list(PPT_LADDER)
    assert src['mem'] == 1
    assert src['sort'] == list(range(SORT_MIN_LOG, SORT_MAX_LOG + 1))
    # D-FPS / S-FPS: every instance in every form a launcher can give it
    want = set()
    for n in src['fat']:
        for weighted, fused in itertools.product((False, True), repeat=2):
            inst = fps_instance(n, weighted, fused)
            if inst[0] == 'fat':           # 4096 and 16384 through det6d_fps_fused are the multi-pick sampler's
                want.add(inst)
    for form in ('plain', 'weighted'):
        want |= {('reg', p, form) for p in src['reg']} | {('mem', form)}
    reached = {fps_instance(n, weighted, False) for n, weighted in FPS_CASES}
    reached |= {fps_instance(n, scored, True) for n, scored in FUSED_CASES}
    assert not want - reached, 'no case reaches %s' % sorted(want - reached)
    assert ('reg', 4, 'weighted') in {fps_instance(n, s, True) for n, s in FUSED_CASES}     # the non-table length
    # the register kernels of the memory-free classes also run their edges: the smallest and the largest n of reg<8>, reg<16>
    assert {4097, 8191, 8193, 16383, 16385} <= set(FPS_SIZES)
    # F-FPS and the sort samplers
    assert {ffps_ppt(n) for n, _, _, _ in FFPS_CASES} == set(src['ffps'])
    assert {ffps_ppt(n) for n, _, _ in FFPM_CASES} == set(src['ffpm'])
    assert {sort_logn(n) for n in TOPK_SIZES} == set(src['sort'])
    assert {sort_logn(n) for n in PILLAR_SIZES} == set(src['sort'])
    return want, reached


def test_case_tables_reach_every_instance(oracle_ops):
    check_tables()
    sizes = set(FPS_SIZES) | {n for n, _ in FUSED_CASES} | {c[0] for c in FFPS_CASES + FFPM_CASES} | set(TOPK_SIZES + PILLAR_SIZES)
    for n in sorted(sizes | set(CLASS_SIZES)):
        assert oracle_ops.opt_n_threads(n) == ffps.opt_n_threads(n) == 1 << log2s(n), n
    # the rules at the edges of their ranges
    assert fps_instance(2, False, False) == fps_instance(64, False, False) == ('reg', 1, 'plain')
    assert fps_instance(65, True, False) == fps_instance(129, True, False) == ('reg', 2, 'weighted')
    assert fps_instance(2049, False, False) == ('reg', 4, 'plain')
    assert fps_instance(4097, False, False) == fps_instance(8191, False, False) == ('reg', 8, 'plain')
    assert fps_instance(8193, True, False) == fps_instance(16383, True, False) == ('reg', 16, 'weighted')
    assert fps_instance(16385, True, False) == ('mem', 'weighted') and fps_instance(20000, False, True) == ('mem', 'plain')
    assert fps_instance(8192, True, True) == ('fat', 9, 16, 'fastw') and fps_instance(128, True, False) == ('fat', 6, 2, 'weighted')
    assert fps_instance(4096, True, True) == fps_instance(16384, False, True) == ('multi-pick',)
    assert fps_instance(4096, True, False) == ('fat', 9, 8, 'weighted') and fps_instance(65536, False, True) == ('cooperative',)
    assert [ffps_ppt(n) for n in (512, 1024, 1025, 2049, 4097, 8192, 8193, 16384)] == [1, 1, 2, 4, 8, 8, 16, 16]
    assert [sort_logn(n) for n in (1, 40, 256, 257, 2048, 2049, 4097, 8192, 8193, 16384)] == [8, 8, 8, 9, 11, 12, 13, 13, 14, 14]


# ---- inputs --------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lattice(rng, n):
    return rng.integers(0, 8, (n, 3)).astype(F32)


def scenes(seed, n):
    """(3, n, 3): (a) KITTI-like with 10 % exact duplicates, (b) lattice, (c) all points equal"""
    rng = np.random.default_rng(seed)
    cloud = make_batch(seed, 1, n, dup_frac=0.1)[0, :, :3]
    equal = np.tile(np.array([3.5, -2.25, 0.75], F32), (n, 1))
    return np.ascontiguousarray(np.stack([cloud, lattice(rng, n), equal]), F32)


def weights_for(seed, b, n):
    """the recipe of test_fps_weights_bit_exact: zeros and 1e-13 (max(w, 1e-12) in double), equal weights (ties)"""
    rng = np.random.default_rng(seed)
    w = (1.0 / (1.0 + np.exp(-rng.normal(size=(b, n)) * 3))).astype(F32)
    w[:, ::17] = 0.0
    w[:, 5::29] = 1e-13
    w[:, 3::31] = w[:, 2:-1:31][:, :w[:, 3::31].shape[1]]
    return w


def hip_fps(xyz, m, weights=None, temp=None):
    import torch
    from de6d_amd.ops import pointnet2_batch_hip as pn
    b, n, _ = xyz.shape
    t = torch.full((b, n), 1e10, dtype=torch.float32, device='cuda') if temp is None else dev(temp)
    idx = torch.full((b, m), -9, dtype=torch.int32, device='cuda')
    if weights is None:
        pn.farthest_point_sampling_wrapper(b, n, m, dev(xyz), t, idx)
    else:
        pn.furthest_point_sampling_weights_wrapper(b, n, m, dev(xyz), dev(weights), t, idx)
    return idx.cpu().numpy()


def oracle_fps(oracle_ops, xyz, m, weights=None, temp=None):
    temp = None if temp is None else np.array(temp, F32, copy=True, order='C')        # the oracle updates it in place
    return oracle_ops.fps(xyz, m, temp) if weights is None else oracle_ops.fps_weights(xyz, weights, m, temp)


# ---- D-FPS / S-FPS through the reference-shaped wrappers -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,weighted", FPS_CASES)
def test_wrapper_instances_bit_exact(oracle_ops, n, weighted):
    xyz = scenes(1000 + n, n)
    w = weights_for(n, len(xyz), n) if weighted else None
    for m in fps_ms(n):
        np.testing.assert_array_equal(hip_fps(xyz, m, w), oracle_fps(oracle_ops, xyz, m, w),
                                      err_msg='%s, m = %d' % (fps_instance(n, weighted, False), m))


# ---- ... and through det6d_fps_fused -------------------------------------------------------------------------------------
def scored_scenes(seed, n):
    """xyz (6, n, 3) and scores (6, n): the five scenes of test_weighted_sampler_fp32_scoring_and_its_exact_double_fallback
    (ordinary scores; forty -40 logits; one NaN; all -60; all +50) on the three kinds of clouds, and a sixth with ordinary
    scores on equal points.  Scenes 0, 4, 5 keep the fp32 scoring, scenes 1, 2, 3 hand themselves over to the guarded launch."""
    rng = np.random.default_rng(seed)
    a, lat, equal = scenes(seed, n)
    xyz = np.stack([a, lat, make_batch(seed + 1, 1, n, dup_frac=0.1)[0, :, :3], equal, lattice(rng, n), equal]).astype(F32)
    scores = (rng.normal(size=(6, n)) * 3).astype(F32)
    scores[1, rng.choice(n, 40, replace=False)] = -40.0
    scores[2, 17] = np.nan
    scores[3] = -60.0
    scores[4] = 50.0
    return xyz, scores


@gpu
@pytest.mark.parametrize("n,scored", FUSED_CASES)
def test_fused_instances_bit_exact(oracle_ops, n, scored):
    import torch
    from de6d_amd.ops import fused
    lo, tail, off, bias = 37, 19, 3, 1000
    if scored:
        xyz, scores = scored_scenes(2000 + n, n)
    else:
        xyz, scores = scenes(2000 + n, n), None
    b = len(xyz)
    rng = np.random.default_rng(n)
    cloud = rng.uniform(-80, 80, (b, lo + n + tail, 3)).astype(F32)          # the slice [lo, lo + n) of a longer cloud
    cloud[:, lo:lo + n] = xyz
    full = None
    if scored:
        full = (rng.normal(size=(b, lo + n + tail)) * 3).astype(F32)
        full[:, lo:lo + n] = scores
    for gamma in ((1.0, 2.5) if scored else (1.0,)):
        for m in fps_ms(n):
            got = torch.full((b, off + m + 5), -5, dtype=torch.int32, device='cuda')
            fused.fps_fused(dev(cloud), lo, lo + n, m, dev(full) if scored else None, gamma, got, off, idx_bias=bias)
            want = np.full((b, off + m + 5), -5, np.int32)
            oracle_ops.fps_fused(cloud, lo, lo + n, m, full, gamma, want, off)
            want[:, off:off + m] += bias
            np.testing.assert_array_equal(got.cpu().numpy(), want,
                                          err_msg='%s, gamma = %g, m = %d' % (fps_instance(n, scored, True), gamma, m))


# ---- the dead branches of the one-pick kernels ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", CLASS_SIZES)
def test_round_zero_that_finds_nothing_picks_point_zero(oracle_ops, n):
    """weights <= -1 (or NaN) never beat the -1 a thread starts from: "nothing beat -1, pick point 0" for a whole scene, and
    `found ? bj : -1` for the threads of a scene in which others did find something"""
    xyz = np.concatenate([scenes(3000 + n, n), scenes(3001 + n, n)[:1]])
    w = weights_for(n, 4, n)
    w[0] = -2.0
    w[1] = np.nan
    w[2, ::2], w[2, 1::4] = -2.0, np.nan
    w[3, : n - n // 8] = -1.0                         # only the last eighth can win round 0
    got, want = hip_fps(xyz, 16, w), oracle_fps(oracle_ops, xyz, 16, w)
    assert want[0, 0] == 0 and want[1, 0] == 0 and want[3, 0] >= n - n // 8
    np.testing.assert_array_equal(got, want)


@gpu
@pytest.mark.parametrize("kind", ['nan', 'inf'])
@pytest.mark.parametrize("n", CLASS_SIZES)
def test_non_finite_coordinates(oracle_ops, n, kind):
    """the oracle defines both: the distance to a non-finite point is NaN or inf, fminf keeps its 1e10, and once it is the
    last pick no min-distance moves any more: it is picked from then on"""
    xyz = scenes(4000 + n, n)
    if kind == 'nan':
        xyz[0, [n // 3, n // 2 + 1, n - 2], [0, 1, 2]] = np.nan
        xyz[1, n // 2, 1] = np.nan
        xyz[2, n - 1, 0] = np.nan
    else:
        xyz[0, n // 3, 1] = np.inf
        xyz[1, n // 2, 2] = np.inf
        xyz[2, n - 1, 0] = np.inf
    want = oracle_fps(oracle_ops, xyz, 16)
    for s in range(len(xyz)):
        assert not np.isfinite(xyz[s, want[s, 1]]).all() and (want[s, 1:] == want[s, 1]).all()
    np.testing.assert_array_equal(hip_fps(xyz, 16), want)
    w = weights_for(n, len(xyz), n)
    np.testing.assert_array_equal(hip_fps(xyz, 16, w), oracle_fps(oracle_ops, xyz, 16, w))


# ---- caller-supplied min-distances ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", CLASS_SIZES)
def test_initial_min_distances_are_read(oracle_ops, n):
    """`temp` from uniform(0, 4) with every second entry 0 instead of 1e10: the picks follow it.  (What `temp` holds afterwards
    is not asserted: include/det6d_ops.h calls it clobbered scratch.)"""
    xyz = scenes(5000 + n, n)
    temp = np.random.default_rng(n).uniform(0, 4, (len(xyz), n)).astype(F32)
    temp[:, ::2] = 0.0
    m = 64
    want = oracle_fps(oracle_ops, xyz, m, temp=temp)
    assert (want != oracle_fps(oracle_ops, xyz, m)).any()
    np.testing.assert_array_equal(hip_fps(xyz, m, temp=temp), want)
    w = weights_for(n, len(xyz), n)
    np.testing.assert_array_equal(hip_fps(xyz, m, w, temp=temp), oracle_fps(oracle_ops, xyz, m, w, temp=temp))


# ---- F-FPS ---------------------------------------------------------------------------------------------------------------
def feature_scenes(seed, n, c):
    """the three kinds of clouds with features: ReLU noise, small integers on the lattice (ties in both terms), ReLU noise on
    the equal points (the feature term alone decides)"""
    rng = np.random.default_rng(seed)
    xyz = scenes(seed, n)
    feats = np.maximum(rng.standard_normal((3, n, c)), 0).astype(F32)
    feats[1] = rng.integers(0, 3, (n, c)).astype(F32)
    return xyz, feats


@gpu
@pytest.mark.parametrize("n,c,m,kind", FFPS_CASES)
def test_feature_sampler_instances_bit_exact(oracle_ops, n, c, m, kind):
    import torch
    from de6d_amd.ops import ffps as op
    xyz, feats = feature_scenes(6000 + n, n, c)
    if kind == 'duplicates':                                    # every second point a duplicate, features included
        xyz[:, 1::2], feats[:, 1::2] = xyz[:, 0::2], feats[:, 0::2]
    b = len(xyz)
    lo, tail, off, bias = (512, 40, 300, 1000) if kind == 'slice' else (0, 0, 0, 0)
    rng = np.random.default_rng(n)
    rows = np.zeros((b, lo + n + tail, (3 + c + 3) // 4 * 4), F32)
    rows[..., :3 + c] = rng.uniform(0, 4, (b, lo + n + tail, 3 + c))
    rows[:, lo:lo + n] = ffps.rows_of(xyz, feats)
    idx = torch.full((b, off + m + 7), -7, dtype=torch.int32, device='cuda')
    op.fps_features(dev(rows), c, m, 1.0, lo=lo, hi=lo + n, idx_out=idx, idx_offset=off, idx_bias=bias)
    got = idx.cpu().numpy()
    assert (got[:, :off] == -7).all() and (got[:, off + m:] == -7).all()
    for s in range(b):
        np.testing.assert_array_equal(got[s, off:off + m], ffps.fps_features(xyz[s], feats[s], m) + lo + bias,
                                      err_msg='PPT %d, scene %d' % (ffps_ppt(n), s))


@gpu
@pytest.mark.parametrize("n,b,m", FFPM_CASES)
def test_matrix_sampler_instances_bit_exact(oracle_ops, n, b, m):
    from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    mats = np.random.default_rng(n).integers(0, 5, (b, n, n), dtype=np.int8).astype(F32)        # exact ties everywhere
    got = pu.furthest_point_sample_matrix(dev(mats), m).cpu().numpy()
    for s in range(b):
        np.testing.assert_array_equal(got[s], ffps.fps_matrix(mats[s], m), err_msg='PPT %d, scene %d' % (ffps_ppt(n), s))


# ---- the sort samplers ---------------------------------------------------------------------------------------------------
def topk(scores, m, gamma):
    from de6d_amd.ops import sort_samplers as op
    return op.topk_scores(dev(np.ascontiguousarray(scores, F32)), m, gamma).cpu().numpy()


@gpu
@pytest.mark.parametrize("n", TOPK_SIZES)
def test_topk_instances_bit_exact(oracle_ops, n):
    for b, gamma in ((1, 1.0), (3, 2.0)):
        scores = np.random.default_rng(n + b).standard_normal((b, n)).astype(F32)
        scores[:, ::7] = np.round(scores[:, ::7])                 # exact ties among the weights
        want = np.stack([score_topk.topk_scores(s, n, gamma) for s in scores])
        for m in sorted({1, max(n // 3, 1), n}):
            np.testing.assert_array_equal(topk(scores, m, gamma), want[:, :m], err_msg='LOGN %d, b = %d, m = %d' % (sort_logn(n), b, m))


def tie_patterns():
    from tests.test_samplers_model import tie_cases
    return tie_cases()


@gpu
@pytest.mark.parametrize("case", tie_patterns(), ids=lambda c: c[0])
def test_topk_tie_and_nan_patterns_at_8192(oracle_ops, case):
    """the constructed inputs of tie_cases() (tests/test_samplers_model.py pins the model on them at 300 entries), repeated up
    to 8192 entries: LOGN = 13, the instance with four compare-exchange pairs per thread"""
    name, scores, gamma, m_small, _ = case
    n = 8192
    scores = np.resize(np.asarray(scores, F32), n)
    want = score_topk.topk_scores(scores, n, gamma)
    for m in (m_small, n // 3, n):
        np.testing.assert_array_equal(topk(scores[None], m, gamma)[0], want[:m], err_msg='%s, m = %d' % (name, m))


@gpu
@pytest.mark.parametrize("n", PILLAR_SIZES)
def test_pillar_weight_instances_bit_exact(n):
    from de6d_amd.ops import sort_samplers as op
    from tests.test_samplers_gpu import clouds
    for b in (1, 3):
        xyz = clouds(b + n, b, n)
        got = op.pillar_weights(dev(xyz)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (b, n)
        np.testing.assert_array_equal(got, pillar_density.pillar_weights(xyz), err_msg='LOGN %d, b = %d' % (sort_logn(n), b))
