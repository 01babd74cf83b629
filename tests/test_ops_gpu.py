"""GPU parity tests: every C-ABI op of libdet6d_hip.so (through the reference-shaped module
functions) against the CPU oracle on the same seeded inputs.  Bit-exact for indices, masks and
for everything computed with the shared deterministic arithmetic."""
import os

import numpy as np
import pytest
import torch

from tests.util import make_batch, random_boxes

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ext():
    from de6d_amd.ops import pointnet2_batch_hip, iou3d_nms_hip, fused
    return pointnet2_batch_hip, iou3d_nms_hip, fused


def hip_fps(pn, xyz, m, weights=None):
    b, n, _ = xyz.shape
    x = dev(xyz)
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device="cuda")
    idx = torch.zeros((b, m), dtype=torch.int32, device="cuda")
    if weights is None:
        pn.farthest_point_sampling_wrapper(b, n, m, x, temp, idx)
    else:
        pn.furthest_point_sampling_weights_wrapper(b, n, m, x, dev(weights), temp, idx)
    return idx.cpu().numpy()


@pytest.mark.parametrize("b,n,m", [(1, 16384, 4096), (2, 4096, 512), (3, 512, 256), (2, 1000, 100),
                                   (2, 100, 37), (1, 7, 7), (1, 1, 1), (2, 3000, 64), (1, 20000, 50)])
def test_fps_bit_exact(ext, oracle_ops, b, n, m):
    pn = ext[0]
    xyz = make_batch(10, b, n, dup_frac=0.1)[..., :3]
    np.testing.assert_array_equal(hip_fps(pn, xyz, m), oracle_ops.fps(xyz, m))


def test_fps_all_duplicates(ext, oracle_ops):
    """every point identical: the pick is decided purely by the tie rule (bitrev(k mod S), k)"""
    pn = ext[0]
    xyz = np.ones((1, 4096, 3), np.float32)
    np.testing.assert_array_equal(hip_fps(pn, xyz, 64), oracle_ops.fps(xyz, 64))
    xyz = np.ones((1, 300, 3), np.float32)
    np.testing.assert_array_equal(hip_fps(pn, xyz, 20), oracle_ops.fps(xyz, 20))


@pytest.mark.parametrize("b,n,m", [(2, 4096, 512), (2, 512, 256), (1, 16384, 300), (2, 777, 99), (1, 40, 9)])
def test_fps_weights_bit_exact(ext, oracle_ops, b, n, m):
    pn = ext[0]
    xyz = make_batch(20, b, n, dup_frac=0.1)[..., :3]
    rng = np.random.default_rng(5)
    w = (1.0 / (1.0 + np.exp(-rng.normal(size=(b, n)) * 3))).astype(np.float32)
    w[:, ::17] = 0.0          # exercises max(w, 1e-12) in double
    w[:, 5::29] = 1e-13
    w[:, 3::31] = w[:, 2:-1:31][:, :w[:, 3::31].shape[1]]  # equal weights -> ties
    np.testing.assert_array_equal(hip_fps(pn, xyz, m, w), oracle_ops.fps_weights(xyz, w, m))


def test_gather_and_group(ext, oracle_ops):
    pn = ext[0]
    rng = np.random.default_rng(1)
    b, c, n, m, ns = 2, 5, 300, 40, 16
    pts = rng.normal(size=(b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    out = torch.empty((b, c, m), device="cuda")
    pn.gather_points_wrapper(b, c, n, m, dev(pts), dev(idx), out)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle_ops.gather_points(pts, idx))
    gidx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    gout = torch.empty((b, c, m, ns), device="cuda")
    pn.group_points_wrapper(b, c, n, m, ns, dev(pts), dev(gidx), gout)
    np.testing.assert_array_equal(gout.cpu().numpy(), oracle_ops.group_points(pts, gidx))
    # backward scatters: atomic order differs from the sequential oracle -> tolerance
    go = rng.normal(size=(b, c, m)).astype(np.float32)
    gp = torch.zeros((b, c, n), device="cuda")
    pn.gather_points_grad_wrapper(b, c, n, m, dev(go), dev(idx), gp)
    np.testing.assert_allclose(gp.cpu().numpy(), oracle_ops.gather_points_grad(go, idx, n), rtol=1e-5, atol=1e-5)
    ggo = rng.normal(size=(b, c, m, ns)).astype(np.float32)
    ggp = torch.zeros((b, c, n), device="cuda")
    pn.group_points_grad_wrapper(b, c, n, m, ns, dev(ggo), dev(gidx), ggp)
    np.testing.assert_allclose(ggp.cpu().numpy(), oracle_ops.group_points_grad(ggo, gidx, n), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n,m,r_in,r_out,ns", [(16384, 512, 0.0, 0.2, 16), (16384, 512, 0.2, 0.8, 32),
                                               (4096, 1024, 0.8, 1.6, 32), (1024, 512, 1.6, 4.8, 32),
                                               (512, 256, 0.0, 6.4, 32), (100, 30, 0.0, 0.01, 8),
                                               (70, 9, 0.0, 100.0, 128)])
def test_ball_query_variants(ext, oracle_ops, n, m, r_in, r_out, ns):
    pn = ext[0]
    b = 2
    xyz = make_batch(30, b, n, dup_frac=0.05)[..., :3]
    new_xyz = np.ascontiguousarray(xyz[:, :m] + np.float32(0.01))
    new_xyz[:, 0] = 1000.0  # a centre with no neighbours at all
    x, q = dev(xyz), dev(new_xyz)
    # dilated
    cnt = torch.zeros((b, m), dtype=torch.int32, device="cuda")
    idx = torch.zeros((b, m, ns), dtype=torch.int32, device="cuda")
    pn.ball_query_dilated_wrapper(b, n, m, r_in, r_out, ns, q, x, cnt, idx)
    ocnt, oidx = oracle_ops.ball_query_dilated(r_in, r_out, ns, xyz, new_xyz)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ocnt)
    np.testing.assert_array_equal(idx.cpu().numpy(), oidx)
    # cnt
    cnt.zero_(); idx.zero_()
    pn.ball_query_cnt_wrapper(b, n, m, r_out, ns, q, x, cnt, idx)
    ocnt, oidx = oracle_ops.ball_query_cnt(r_out, ns, xyz, new_xyz)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ocnt)
    np.testing.assert_array_equal(idx.cpu().numpy(), oidx)
    # plain
    idx.zero_()
    pn.ball_query_wrapper(b, n, m, r_out, ns, q, x, idx)
    np.testing.assert_array_equal(idx.cpu().numpy(), oracle_ops.ball_query(r_out, ns, xyz, new_xyz))


def test_three_nn_interpolate(ext, oracle_ops):
    pn = ext[0]
    b, n, m, c = 2, 1500, 700, 6
    unknown = make_batch(40, b, n)[..., :3]
    known = np.ascontiguousarray(unknown[:, :m])   # exact zeros + duplicates -> ties
    d2 = torch.empty((b, n, 3), device="cuda")
    idx = torch.empty((b, n, 3), dtype=torch.int32, device="cuda")
    pn.three_nn_wrapper(b, n, m, dev(unknown), dev(known), d2, idx)
    od2, oidx = oracle_ops.three_nn(unknown, known)
    np.testing.assert_array_equal(idx.cpu().numpy(), oidx)
    np.testing.assert_array_equal(d2.cpu().numpy(), od2)
    rng = np.random.default_rng(3)
    feats = rng.normal(size=(b, c, m)).astype(np.float32)
    w = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
    out = torch.empty((b, c, n), device="cuda")
    pn.three_interpolate_wrapper(b, c, m, n, dev(feats), idx, dev(w), out)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle_ops.three_interpolate(feats, oidx, w))
    go = rng.normal(size=(b, c, n)).astype(np.float32)
    gp = torch.zeros((b, c, m), device="cuda")
    pn.three_interpolate_grad_wrapper(b, c, n, m, dev(go), idx, dev(w), gp)
    np.testing.assert_allclose(gp.cpu().numpy(), oracle_ops.three_interpolate_grad(go, oidx, w, m), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 256, 512, 700])
def test_iou_and_nms_bit_exact(ext, oracle_ops, k):
    _, nm, fused = ext
    boxes = random_boxes(k, k, spread=8.0 + k / 8)
    if k > 4:
        boxes[3] = boxes[1]                 # identical boxes
        boxes[4, 3:5] = 0.0                 # zero-area box
    bd = dev(boxes)
    iou = torch.zeros((k, k), device="cuda")
    nm.boxes_iou_bev_gpu(bd, bd, iou)
    np.testing.assert_array_equal(iou.cpu().numpy(), oracle_ops.boxes_iou_bev(boxes, boxes))
    ov = torch.zeros((k, k), device="cuda")
    nm.boxes_overlap_bev_gpu(bd, bd, ov)
    np.testing.assert_array_equal(ov.cpu().numpy(), oracle_ops.boxes_overlap_bev(boxes, boxes))
    for thr in (0.01, 0.1, 0.7):
        keep = torch.zeros(k, dtype=torch.int64)
        num = nm.nms_gpu(bd, keep, thr)
        np.testing.assert_array_equal(keep[:num].numpy(), oracle_ops.nms(boxes, thr))
        num = nm.nms_normal_gpu(bd, keep, thr)
        np.testing.assert_array_equal(keep[:num].numpy(), oracle_ops.nms(boxes, thr, normal=True))
    kd, nd = fused.nms_device(bd, 0.1)
    np.testing.assert_array_equal(kd[:int(nd.item())].cpu().numpy(), oracle_ops.nms(boxes, 0.1))


def nms_chunk_rows(k):
    """rows of the suppression matrix the greedy scan stages per chunk (csrc/iou3d_nms.hip: run_nms), RESTATED here from its
    rule — as many rows of ceil(K / 64) words as fit 96 KB of LDS, K at the most — and not asked of the library"""
    return max(1, min(k, 96 * 1024 // (8 * ((k + 63) // 64))))


def nms_suppressors(mask, keep, k):
    """from the oracle's suppression rows and keep list: (first, last) kept box whose row holds box j's bit, -1 where none"""
    bits = np.unpackbits(mask[keep].view(np.uint8), axis=1, bitorder='little')[:, :k].astype(bool)      # (kept, K)
    bits &= np.arange(k)[None, :] > keep[:, None]          # the scan reads a row from its own box on (the oracle fills the row)
    hit = bits.any(axis=0)
    first = np.where(hit, keep[bits.argmax(axis=0)], -1)
    last = np.where(hit, keep[len(keep) - 1 - bits[::-1].argmax(axis=0)], -1)
    return first, last


@pytest.mark.parametrize("k,spread", [(704, 38.0), (705, 38.0), (877, 42.0), (878, 42.0), (1024, 45.0), (1500, 50.0), (4290, 90.0)])
def test_nms_beyond_one_chunk_of_suppression_rows(ext, oracle_ops, k, spread):
    """det6d_nms / det6d_nms_normal on both sides of the three sizes at which the greedy scan changes (csrc/iou3d_nms.hip:
    run_nms, nms_greedy_kernel): K = 705 is the first launch above the 64 KB default of dynamic LDS (704: 62 040 bytes, 705:
    67 776), K = 878 the first scan in two chunks of staged rows (removal words carried from one chunk into the next), K > 4096
    gives a lane more than one removal word (the `w += 64` loops take a second trip).  Keep lists == the oracle's, through
    nms_gpu, nms_normal_gpu and fused.nms_device.

    That a case bites is asserted on the ORACLE's result, before the GPU runs:
      * K >= 878: removed boxes whose first suppressing keeper lies in an earlier chunk, and among them boxes with NO suppressing
        keeper in their own chunk — a scan that forgot the removal words at a chunk boundary keeps the lowest such box, and
        one that staged another number of rows than it indexes reads another box's row for it;
      * K = 4290: kept and removed boxes from index 4096 on (words 64 .. 67), and among the removed a box all of whose suppressing
        keepers lie 64 words or more below its own word: only the second trip of the update loop ORs their rows into it."""
    _, nm, fused = ext
    boxes = random_boxes(k, k, spread)
    boxes[3] = boxes[1]                     # identical boxes
    boxes[4, 3:5] = 0.0                     # zero-area box
    rows = nms_chunk_rows(k)
    cb = (k + 63) // 64
    lds = (cb + rows * cb) * 8
    assert (lds > 64 * 1024) == (k >= 705) and lds <= 128 * 1024
    assert ((k + rows - 1) // rows >= 2) == (k >= 878)
    bd = dev(boxes)
    for thr in (0.01, 0.3):
        want, mask = oracle_ops.nms(boxes, thr, with_mask=True)
        removed = np.setdiff1d(np.arange(k), want)
        assert 0.1 * k <= len(want) <= 0.6 * k, (len(want), k)          # many kept AND many removed (12 .. 54 % are kept)
        first, last = nms_suppressors(mask, want, k)
        assert (first[want] == -1).all() and (first[removed] >= 0).all() and (last[removed] < removed).all()
        carried = removed[first[removed] // rows < removed // rows]
        only_carried = removed[last[removed] // rows < removed // rows]
        far = removed[(last[removed] >> 6) + 64 <= (removed >> 6)]
        print('nms K=%d thr=%.2f: kept %d, chunks of %d rows, first keeper in an earlier chunk %d, every keeper %d; from 4096 on '
              'kept %d removed %d, every keeper 64 words below %d' % (k, thr, len(want), rows, len(carried), len(only_carried),
                                                                      (want >= 4096).sum(), (removed >= 4096).sum(), len(far)))
        if k >= 878:
            assert len(carried) > 0 and len(only_carried) > 0
        else:
            assert len(carried) == 0
        if k > 4096:
            assert (want >= 4096).any() and (removed >= 4096).any() and len(far) > 0
        keep = torch.full((k,), -1, dtype=torch.int64)
        num = nm.nms_gpu(bd, keep, thr)
        np.testing.assert_array_equal(keep[:num].numpy(), want)
        assert (keep[num:] == -1).all()
        kd, nd = fused.nms_device(bd, thr)
        np.testing.assert_array_equal(kd[:int(nd.item())].cpu().numpy(), want)
        want_n = oracle_ops.nms(boxes, thr, normal=True)
        keep.fill_(-1)
        num = nm.nms_normal_gpu(bd, keep, thr)
        np.testing.assert_array_equal(keep[:num].numpy(), want_n)
        assert (keep[num:] == -1).all()
        kd, nd = fused.nms_device(bd, thr, normal=True)
        np.testing.assert_array_equal(kd[:int(nd.item())].cpu().numpy(), want_n)


@pytest.mark.parametrize("rows,k,n", [(256, 16, 16), (1000, 132, 64), (384, 260, 256), (128, 68, 32),
                                      (4096, 512, 1024), (77, 4, 3), (640, 36, 96)])
def test_linear_rows_bit_exact(ext, oracle_ops, rows, k, n):
    fused = ext[2]
    rng = np.random.default_rng(rows + k)
    lda = (k + 3) // 4 * 4
    ldw = (n + 3) // 4 * 4
    a = rng.normal(size=(rows, lda)).astype(np.float32)
    w = (rng.normal(size=(k, ldw)) / np.sqrt(k)).astype(np.float32)
    shift = rng.normal(size=(n,)).astype(np.float32)
    for act in (0, 1):
        out = torch.zeros((rows, n + 5), device="cuda")
        fused.linear(dev(a), dev(w), dev(shift), act, out, k=k, ncols=n, col0=2)
        ref = np.zeros((rows, n + 5), np.float32)
        oracle_ops.linear(a, w[:, :n], shift, act, k=k, out=ref, col0=2)
        np.testing.assert_array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("n,m,ns,c,n1", [(512, 64, 16, 1, 16), (1024, 96, 32, 64, 64), (300, 40, 32, 128, 128),
                                         (256, 24, 16, 256, 256), (200, 10, 8, 5, 40)])
def test_linear_grouped_pool_bit_exact(ext, oracle_ops, n, m, ns, c, n1):
    fused = ext[2]
    b = 2
    rng = np.random.default_rng(n + m)
    ld = (3 + c + 3) // 4 * 4
    rows = np.zeros((b, n, ld), np.float32)
    rows[..., :3 + c] = rng.normal(size=(b, n, 3 + c))
    ctr = np.zeros((b, m, 4), np.float32)
    ctr[..., :3] = rng.normal(size=(b, m, 3))
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    cnt = rng.integers(0, 3, (b, m)).astype(np.int32)
    w = (rng.normal(size=(ld, n1)) / np.sqrt(ld)).astype(np.float32)
    w[3 + c:] = 0
    shift = rng.normal(size=(n1,)).astype(np.float32)
    # layer 1 unpooled (grouped gather + centre subtraction)
    out = torch.zeros((b * m * ns, n1), device="cuda")
    fused.linear(dev(rows), dev(w), dev(shift), 1, out, idx=dev(idx), ctr=dev(ctr))
    ref = oracle_ops.linear(rows, w, shift, 1, idx=idx, ctr=ctr)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    # pooled + masked
    outp = torch.zeros((b * m, n1 + 4), device="cuda")
    fused.linear(dev(rows), dev(w), dev(shift), 1, outp, idx=dev(idx), ctr=dev(ctr), cnt=dev(cnt), pool=ns, col0=4)
    refp = np.zeros((b * m, n1 + 4), np.float32)
    oracle_ops.linear(rows, w, shift, 1, idx=idx, ctr=ctr, cnt=cnt, pool=ns, out=refp, col0=4)
    np.testing.assert_array_equal(outp.cpu().numpy(), refp)


def test_linear_random_shapes_bit_exact(ext, oracle_ops):
    """seeded sweep over shapes that land on every tile variant, interior and edge tiles, full / short / odd
    K slabs (the buffer-load fast path, its predicated first / last slab, both epilogues)"""
    fused = ext[2]
    rng = np.random.default_rng(2025)
    shapes = [(32768, 132, 128), (33000, 260, 256), (40000, 96, 128), (36864, 64, 96), (32896, 17, 40), (2048, 512, 128),
              (65600, 31, 300), (16384, 16, 1), (70000, 48, 33)]
    shapes += [(int(rng.integers(1, 40000)), int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(10)]
    for rows, k, n in shapes:
        lda, ldw = (k + 3) // 4 * 4 + 4 * int(rng.integers(0, 2)), (n + 3) // 4 * 4
        a = rng.normal(size=(rows, lda)).astype(np.float32)
        a[:, k:] = np.nan                       # columns beyond K must never be read into the result
        w = (rng.normal(size=(k, ldw)) / np.sqrt(k)).astype(np.float32)
        shift = rng.normal(size=(n,)).astype(np.float32)
        act = int(rng.integers(0, 2))
        out = torch.full((rows, n + 3), 7.0, device="cuda")
        fused.linear(dev(a), dev(w), dev(shift), act, out, k=k, ncols=n, col0=1)
        ref = np.full((rows, n + 3), 7.0, np.float32)
        oracle_ops.linear(np.nan_to_num(a), w[:, :n], shift, act, k=k, out=ref, col0=1)
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=str((rows, k, n, lda, act)))


def test_head_elementwise_bit_exact(ext, oracle_ops):
    fused = ext[2]
    rng = np.random.default_rng(9)
    r = 777
    s = (rng.normal(size=(r,)) * 4).astype(np.float32)
    for gamma in (1.0, 0.5, 2.0):
        np.testing.assert_array_equal(fused.sigmoid_pow(dev(s), gamma).cpu().numpy(), oracle_ops.sigmoid_pow(s, gamma))
    off = (rng.normal(size=(r, 4)) * 3).astype(np.float32)
    cand = rng.normal(size=(r, 4)).astype(np.float32) * 10
    vote = torch.zeros((r, 3), device="cuda")
    offo = torch.zeros((r, 3), device="cuda")
    fused.vote_points(dev(off), dev(cand), (3.0, 3.0, 2.0), vote, offo)
    ov, oo = oracle_ops.vote_points(off, cand, (3.0, 3.0, 2.0))
    np.testing.assert_array_equal(vote.cpu().numpy(), ov)
    np.testing.assert_array_equal(offo.cpu().numpy(), oo)
    code = rng.normal(size=(r, 32)).astype(np.float32)
    pts = rng.normal(size=(r, 3)).astype(np.float32) * 20
    thr, fac = np.float32(np.deg2rad(10.0)), np.float32(np.deg2rad(45.0))
    got = fused.decode_boxes(dev(code), dev(pts), 12, True, False, thr, fac).cpu().numpy()
    np.testing.assert_array_equal(got, oracle_ops.decode_boxes(code, pts))


@pytest.mark.parametrize("p,ncls", [(256, 1), (256, 3), (512, 1), (100, 2)])
def test_postprocess_bit_exact(ext, oracle_ops, p, ncls):
    fused = ext[2]
    b = 3
    rng = np.random.default_rng(p + ncls)
    cls = (rng.normal(size=(b * p, ncls)) * 2 - 1).astype(np.float32)
    cls[5] = cls[9]  # equal scores -> stable order
    boxes = np.zeros((b * p, 9), np.float32)
    boxes[:, :7] = random_boxes(1, b * p, spread=40.0)
    boxes[:, 7] = rng.normal(size=b * p) * 0.1
    cls[p:2 * p] = -10.0  # a scene with nothing above threshold
    got = fused.postprocess(dev(cls), dev(boxes), b, 0.1, 512, 100, 0.01)
    ref = oracle_ops.postprocess(cls, boxes, b, 0.1, 512, 100, 0.01)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    assert ref[4][1] == 0 and ref[4][0] > 0


@pytest.mark.parametrize("p,kind", [(1024, "clusters"), (1024, "rows"), (1000, "dense"), (640, "clusters"), (8, "rows"), (1, "dense")])
def test_postprocess_pair_filtered_mask_at_1024_candidates(ext, oracle_ops, p, kind):
    """the two-phase suppression-mask kernel (separated pairs skipped, the rest evaluated from a dense queue: csrc/iou3d_nms.hip)
    at the candidate counts of BASELINE config 5 (1024 per scene) against the oracle, which evaluates EVERY pair: vote-like
    clusters (many near pairs per row), rows of collinear equal boxes (the rule's worst case), one dense blob (nothing skipped:
    the queue holds every pair of a chunk), no score filter so that all p candidates reach the NMS"""
    fused = ext[2]
    b = 3
    rng = np.random.default_rng(p * 7 + len(kind))
    boxes = np.zeros((b * p, 9), np.float32)
    boxes[:, :7] = random_boxes(3, b * p, spread=60.0)
    if kind == "clusters":
        centres = rng.uniform(-50, 50, (40, 2))
        pick = rng.integers(0, 40, b * p)
        boxes[:, 0] = centres[pick, 0] + rng.normal(size=b * p) * 0.7
        boxes[:, 1] = centres[pick, 1] + rng.normal(size=b * p) * 0.7
    elif kind == "rows":
        boxes[:, 3], boxes[:, 4], boxes[:, 6] = 3.9, 1.6, 0.0
        boxes[:, 0] = (np.arange(b * p) % 97) * 1.3
        boxes[:, 1] = ((np.arange(b * p) // 97) % 5) * 1.55
    else:
        boxes[:, 0] = rng.normal(size=b * p) * 2.0
        boxes[:, 1] = rng.normal(size=b * p) * 2.0
    boxes[:, 7] = rng.normal(size=b * p) * 0.1
    cls = (rng.normal(size=(b * p, 1)) * 2 + 1).astype(np.float32)
    for thr in (0.01, 0.3):
        got = fused.postprocess(dev(cls), dev(boxes), b, 0.0, 4096, 100, thr)
        ref = oracle_ops.postprocess(cls, boxes, b, 0.0, 4096, 100, thr)
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g.cpu().numpy(), r)
    assert ref[4].min() > 0


def test_postprocess_cuts_at_pre_max_and_post_max(ext, oracle_ops):
    """det6d_postprocess where both cuts bind (the 65536-point configuration: 1024 candidates per scene, NMS_PRE_MAXSIZE 512):
    more than pre_max candidates pass the score threshold, so only the 512 best reach the NMS, and post_max = 7 cuts the
    survivors.  The vote-like clusters of test_postprocess_pair_filtered_mask_at_1024_candidates (same draw order); all five
    outputs == the oracle's.  That the cuts bind is asserted on the oracle's results."""
    fused = ext[2]
    b, p = 3, 1024
    rng = np.random.default_rng(p * 7 + 8)
    boxes = np.zeros((b * p, 9), np.float32)
    boxes[:, :7] = random_boxes(3, b * p, spread=60.0)
    centres = rng.uniform(-50, 50, (40, 2))
    pick = rng.integers(0, 40, b * p)
    boxes[:, 0] = centres[pick, 0] + rng.normal(size=b * p) * 0.7
    boxes[:, 1] = centres[pick, 1] + rng.normal(size=b * p) * 0.7
    boxes[:, 7] = rng.normal(size=b * p) * 0.1
    cls = (rng.normal(size=(b * p, 1)) * 2 + 1).astype(np.float32)
    passing = (oracle_ops.math_fn("sigmoid", cls).reshape(b, p) >= np.float32(0.1)).sum(axis=1)
    assert (passing > 512).all() and (passing < p).all(), passing                      # 967, 978, 976
    uncut = oracle_ops.postprocess(cls, boxes, b, 0.1, 4096, 100, 0.01)
    for post_max in (100, 7):
        ref = oracle_ops.postprocess(cls, boxes, b, 0.1, 512, post_max, 0.01)
        if post_max == 100:
            assert (ref[4] < post_max).all() and (ref[4] != uncut[4]).all(), (ref[4], uncut[4])   # 53, 54, 58 against 62, 65, 68
            assert not np.array_equal(ref[3], uncut[3])
        else:
            assert (ref[4] == post_max).all()
        got = fused.postprocess(dev(cls), dev(boxes), b, 0.1, 512, post_max, 0.01)
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g.cpu().numpy(), r)


@pytest.mark.parametrize("n,m,sa,sb", [(16384, 700, (0.0, 0.2, 16), (0.2, 0.8, 32)), (4096, 1024, (0.0, 0.8, 16), (0.8, 1.6, 32)),
                                       (512, 256, (0.0, 4.8, 16), (0.0, 6.4, 32)), (100, 7, (0.0, 0.01, 8), (0.0, 50.0, 128)),
                                       (1000, 33, (1.0, 3.0, 5), (0.5, 2.0, 70))])
def test_ball_query_pair_matches_two_queries(ext, oracle_ops, n, m, sa, sb):
    fused = ext[2]
    b = 2
    xyz = make_batch(50, b, n, dup_frac=0.05)[..., :3]
    new_xyz = np.ascontiguousarray(xyz[:, :m] + np.float32(0.01))
    new_xyz[:, 0] = 1000.0
    oca, oia = oracle_ops.ball_query_dilated(sa[0], sa[1], sa[2], xyz, new_xyz)
    ocb, oib = oracle_ops.ball_query_dilated(sb[0], sb[1], sb[2], xyz, new_xyz)
    for grid in (False, True):   # brute-force sweep and grid-hashed search give the same lists
        ca, ia, cb, ib = fused.ball_query_pair(dev(xyz), dev(new_xyz), sa, sb, grid=grid)
        np.testing.assert_array_equal(ca.cpu().numpy(), oca)
        np.testing.assert_array_equal(ia.cpu().numpy(), oia)
        np.testing.assert_array_equal(cb.cpu().numpy(), ocb)
        np.testing.assert_array_equal(ib.cpu().numpy(), oib)


@pytest.mark.parametrize("n,m", [(4096, 512), (512, 256), (16384, 700), (2048, 300), (16384, 2048), (4096, 4096)])
def test_weighted_sampler_fp32_scoring_and_its_exact_double_fallback(ext, oracle_ops, n, m):
    """S-FPS through det6d_fps_fused (round 5): scenes whose weights are all >= 1e-12 are scored with one fp32 multiply per
    point (exactly float(double(t) * double(w)): the product of two floats is exact in double); a scene holding a weight below
    1e-12 (sigmoid(score) ** gamma underflowing it) or a NaN weight hands itself over to the exact-double launch behind.
    Scenes of both kinds in ONE call, against the oracle's restatement of sampling_gpu.cu:419-540.  From round 6 the 16384- and
    4096-point clouds go through the MULTI-PICK score-weighted kernel (fps_seq.hip: fps_seq_w_kernel; (16384, 2048) is the second
    layer of the 65536-point configuration, (4096, 4096) samples every point): records by score, the region bound on scores, the
    box test on min-distances, pick 0 = arg-max of the weights in the reference's tie order, scene 4 = ties everywhere."""
    fused = ext[2]
    b = 5
    pts = make_batch(170 + n, b, n, dup_frac=0.1)
    xyz = np.ascontiguousarray(pts[..., :3])
    rng = np.random.default_rng(n + m)
    scores = (rng.normal(size=(b, n)) * 3).astype(np.float32)
    scores[1, rng.choice(n, 40, replace=False)] = -40.0          # sigmoid -> 4e-18 < 1e-12: clamped in double by the reference
    scores[2, 17] = np.nan                                        # max(NaN, 1e-12) = 1e-12 (sampling_gpu.cu:466)
    scores[3] = -60.0                                             # every weight below the clamp
    scores[4, :] = 50.0                                           # every weight 1.0: ties everywhere -> the reference's tie order
    for gamma in (1.0, 2.5):
        got = torch.full((b, m + 3), -5, dtype=torch.int32, device="cuda")
        fused.fps_fused(dev(xyz), 0, n, m, dev(scores), gamma, got, 3)
        want = np.full((b, m + 3), -5, np.int32)
        oracle_ops.fps_fused(xyz, 0, n, m, scores, gamma, want, 3)
        np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_fused_sampler_and_helpers(ext, oracle_ops):
    """det6d_fps_fused (range slice + sigmoid**gamma + 1e10 init + offset), gather_centres, with_batch_index, pack"""
    fused = ext[2]
    b, n = 2, 4096
    pts = make_batch(70, b, n, dup_frac=0.1)
    xyz = np.ascontiguousarray(pts[..., :3])
    rng = np.random.default_rng(3)
    scores = (rng.normal(size=(b, n)) * 3).astype(np.float32)
    for lo, hi, m, sc, gamma, off in [(0, 4096, 512, None, 1.0, 0), (0, 4096, 512, scores, 1.0, 512), (512, 1024, 256, None, 1.0, 0),
                                      (0, 512, 256, scores, 0.5, 256), (100, 3100, 77, scores, 2.0, 3)]:
        got = torch.full((b, 1100), -5, dtype=torch.int32, device="cuda")
        fused.fps_fused(dev(xyz), lo, hi, m, dev(sc) if sc is not None else None, gamma, got, off)
        want = np.full((b, 1100), -5, np.int32)
        oracle_ops.fps_fused(xyz, lo, hi, m, sc, gamma, want, off)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        # and it equals the unfused reference sequence
        sl = np.ascontiguousarray(xyz[:, lo:hi])
        ref = oracle_ops.fps(sl, m) if sc is None else oracle_ops.fps_weights(sl, oracle_ops.sigmoid_pow(sc[:, lo:hi], gamma), m)
        np.testing.assert_array_equal(want[:, off:off + m], ref + lo)
    idx = rng.integers(0, n, (b, 300)).astype(np.int32)
    rows = torch.full((b, 300, 8), 9.0, device="cuda")
    cx = fused.gather_centres(dev(xyz), dev(idx), rows, 6)
    ox, orows = oracle_ops.gather_centres(xyz, idx, 8, 6)
    np.testing.assert_array_equal(cx.cpu().numpy(), ox)
    r = rows.cpu().numpy()
    np.testing.assert_array_equal(r[..., :3], ox)
    assert (r[..., 3:6] == 9.0).all() and (r[..., 6:] == 0.0).all()
    np.testing.assert_array_equal(fused.with_batch_index(cx, 3).cpu().numpy(), oracle_ops.with_batch_index(ox, 3))
    flat = np.concatenate([np.repeat(np.arange(b, dtype=np.float32), n)[:, None], pts.reshape(b * n, 4)], 1)
    rows2, xyz2 = fused.pack_points(dev(flat), 4)
    orows2, oxyz2 = oracle_ops.pack_points(flat, 4)
    np.testing.assert_array_equal(rows2.cpu().numpy(), orows2)
    np.testing.assert_array_equal(xyz2.cpu().numpy(), oxyz2)


def test_pruned_fps_kernel_is_exact():
    """fps_seq.hip on fps_cells.hip's k-d regions: the multi-pick sampler (16384 points: 16 waves x 16 slots, several picks
    per barrier round) gives the oracle's picks bit for bit, duplicates and all-equal clouds included; the other sizes of the
    first script run the fat-thread kernels.  The one-pick wave-skip sampler of rounds 2-3 (experiments build) likewise."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_cells.py")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if "exact" in l]
    assert len(lines) == 7 and all("exact=True" in l or "exact True" in l for l in lines), out.stdout
    # the 16384-point suites of the round-4 sampler work: ray-cast scenes, every point twice, a lattice of exact ties, far
    # outliers, 32 scenes, m = n
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_seq.py")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "ALL EXACT" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # ... and with the LDS of every CU filled with 0x7F7F0000 (a huge float, an index with high bits set) right before the sampling kernel (experiments build: same kernel
    # source plus the fill hook, DET6D_DBG_POISON_LDS): a sampler must not read LDS it has not written
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_seq.py")],
                         capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, DET6D_EXPERIMENTS_LIB="1", DET6D_DBG_POISON_LDS="0x7F7F0000"))
    assert out.returncode == 0 and "ALL EXACT" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_seq.py")],
                         capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, DET6D_EXPERIMENTS_LIB="1", DET6D_FPS_SEQ="0", DET6D_DBG_POISON_LDS="0x7F7F0000"))
    assert out.returncode == 0 and "ALL EXACT" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_skip_sampler_on_adversarial_clouds():
    """16384-point sampler (fps_seq.hip): more seeds, a lattice with thousands of exact distance ties, collinear points, far
    outliers — always the oracle's indices"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_stress.py")], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL True" in out.stdout, out.stdout


@pytest.mark.parametrize("lda,c1", [(68, 64), (132, 128), (260, 256), (8, 32)])
def test_group_expand_equals_the_gathered_first_layer(ext, oracle_ops, lda, c1):
    """csrc/expand.hip: per-point partial sums (one plain GEMM over the points, coordinate rows zeroed) + three FMAs per
    grouped output == the oracle's first layer over the gathered rows (feature columns first, relative coordinates
    last), dense rows and compact lists, bit for bit"""
    fused = ext[2]
    rng = np.random.default_rng(lda)
    b, n, m, ns = 2, 700, 96, 16
    rows = rng.normal(size=(b, n, lda)).astype(np.float32)
    rows[..., lda - 1] = 0.0                                    # pad column
    ctr = np.ascontiguousarray(rows[:, :m, :3] + rng.normal(size=(b, m, 3)).astype(np.float32) * 0.1)
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    w = (rng.normal(size=(lda, c1)) * 0.2).astype(np.float32)
    w[lda - 1] = 0.0
    shift = rng.normal(size=(c1,)).astype(np.float32)
    ref = oracle_ops.linear(rows, w, shift, 1, idx=idx, ctr=ctr)
    wz = w.copy(); wz[:3] = 0.0
    p = torch.empty((b * n, c1), device='cuda')
    fused.linear(dev(rows).view(b * n, lda), dev(wz), None, 0, p)
    out = torch.full((b * m * ns, c1 + 4), 7.0, device='cuda')
    fused.group_expand(p, 0, dev(w), dev(shift), 1, c1, dev(rows), dev(ctr), out, idx=dev(idx))
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, :c1], ref)
    assert (got[:, c1:] == 0).all()
    # the gathered GEMM of det6d_linear follows the same chain order
    y = torch.empty((b * m * ns, c1), device='cuda')
    fused.linear(dev(rows), dev(w), dev(shift), 1, y, idx=dev(idx), ctr=dev(ctr))
    np.testing.assert_array_equal(y.cpu().numpy(), ref)
    # compact list of the same neighbourhoods: every live row equals the dense row it stands for
    cnt = rng.integers(0, ns + 1, (b, m)).astype(np.int32)
    for bi in range(b):
        for j in range(m):
            c = max(int(cnt[bi, j]), 1)
            idx[bi, j] = np.resize(idx[bi, j, :c], ns)            # cyclic padding like the ball query's
    cr = fused.compact_groups(dev(cnt), dev(idx), n)
    outc = torch.full((cr.capacity, c1), 5.0, device='cuda')
    fused.group_expand(p, 0, dev(w), dev(shift), 1, c1, dev(rows), dev(ctr), outc, compact=cr)
    yc = torch.empty((cr.capacity, c1), device='cuda')
    fused.linear(dev(rows), dev(w), dev(shift), 1, yc, ctr=dev(ctr), compact=cr, gather=True)
    live = int(cr.hdr[0].item())
    tags = cr.crow_c[:live].cpu().numpy()
    a, bb = outc[:live].cpu().numpy(), yc[:live].cpu().numpy()
    np.testing.assert_array_equal(a[tags >= 0], bb[tags >= 0])
    assert (a[tags < 0] == 0).all()


def test_cooperative_sampler_for_large_scenes():
    """csrc/fps_coop.hip: D-FPS of 32768 / 65536-point scenes held in registers by 2 / 4 cooperating workgroups per scene
    (BASELINE config 5): the oracle's picks bit for bit, ties / duplicates / odd batch sizes included; and the
    memory-resident fallback (a scratch too small for the cooperative workspace) still agrees; so does the opt-in same-XCD fast path"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_coop.py")], capture_output=True, text=True,
                         timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL True" in out.stdout, out.stdout
    print(out.stdout)
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_coop.py"), "fallback"], capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL True" in out.stdout and "fallback" in out.stdout, out.stdout
    # DET6D_FPS_COOP_FAST=1: workgroup-scope publishing stores where the placement test and the round-0 handshake allow (the
    # default publishes with agent-scope stores: the memory model's guarantee)
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_coop.py")], capture_output=True, text=True,
                         timeout=1500, env=dict(os.environ, DET6D_FPS_COOP_FAST="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL True" in out.stdout and "fallback" not in out.stdout, out.stdout
    print(out.stdout)
    # the LDS of every CU filled with 0x7F7F0000 (a huge float, an index with high bits set) right before the sampling kernel (experiments build: same kernel source plus
    # the fill hook, DET6D_DBG_POISON_LDS).  Round 4: a record slot never written in a launch leaked into the published candidate count — invisible in a
    # fresh process, where the LDS is zero, and wrong picks in a long-lived one.
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_scripts", "fps_coop.py")], capture_output=True,
                         text=True, timeout=1500, env=dict(os.environ, DET6D_EXPERIMENTS_LIB="1", DET6D_DBG_POISON_LDS="0x7F7F0000"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL True" in out.stdout, out.stdout


def test_cooperative_sampler_call_over_more_scenes_than_the_chip_holds(ext, oracle_ops):
    """one det6d_fps_fused call over 72 scenes of 65536 points = 288 cooperating workgroups on a 256-CU chip: the call samples
    them in chunks of one workgroup per CU (round-4 review: a C-ABI caller could starve itself until the 2 s time-out); picks
    equal the oracle's on a few scenes of every chunk, the status word stays clear"""
    fused = ext[2]
    b, n, m = 72, 65536, 48
    rng = np.random.default_rng(99)
    base = make_batch(640, 3, n)[..., :3]
    xyz = np.ascontiguousarray(base[np.arange(b) % 3] + rng.normal(size=(b, 1, 3)).astype(np.float32) * np.float32(0.01))
    idx = torch.full((b, m), -1, dtype=torch.int32, device="cuda")
    ws = fused.fps_workspace(b, n)
    fused.fps_fused(dev(xyz), 0, n, m, None, 1.0, idx, 0, temp=ws)
    fused.fps_status(b, n, ws)                                   # raises if a workgroup gave up waiting for its partners
    got = idx.cpu().numpy()
    assert (got >= 0).all() and (got < n).all() and (got[:, 0] == 0).all()
    for s in (0, 1, 63, 64, 65, 71):
        np.testing.assert_array_equal(got[s], oracle_ops.fps(xyz[s:s + 1], m)[0], err_msg="scene %d" % s)


def test_ball_query_grid_adversarial(ext, oracle_ops):
    """grid search corner cases: centres outside the cloud, everything in one cell, outliers that stretch
    the bounding box past 128 cells, vertical stacks (the grid is 2-D), non-finite points"""
    fused = ext[2]
    rng = np.random.default_rng(11)
    n, m = 3000, 200
    base = (rng.normal(size=(1, n, 3)) * [8, 8, 1]).astype(np.float32)
    clouds = []
    c0 = base.copy(); clouds.append(c0)
    c1 = base.copy(); c1[0, :5, 0] = [500.0, -400.0, 300.0, 250.0, -350.0]; clouds.append(c1)      # far outliers
    c2 = (base * [0.01, 0.01, 5.0]).astype(np.float32); clouds.append(c2)                         # one cell, tall
    c3 = base.copy(); c3[0, 7] = np.nan; c3[0, 9, 1] = np.inf; clouds.append(c3)
    for xyz in clouds:
        new_xyz = np.ascontiguousarray(xyz[:, :m] + np.float32(0.05))
        new_xyz[0, 0] = (100.0, 100.0, 0.0)
        new_xyz[0, 1] = xyz[0, :, :].min(0) - 0.3 if np.isfinite(xyz).all() else (0, 0, 0)
        for sa, sb in [((0.0, 0.8, 16), (0.8, 1.6, 32)), ((0.0, 4.8, 16), (0.0, 6.4, 32)), ((0.0, 0.05, 8), (0.05, 0.3, 8))]:
            oca, oia = oracle_ops.ball_query_dilated(sa[0], sa[1], sa[2], xyz, new_xyz)
            ocb, oib = oracle_ops.ball_query_dilated(sb[0], sb[1], sb[2], xyz, new_xyz)
            ca, ia, cb, ib = fused.ball_query_pair(dev(xyz), dev(new_xyz), sa, sb, grid=True)
            np.testing.assert_array_equal(ca.cpu().numpy(), oca)
            np.testing.assert_array_equal(ia.cpu().numpy(), oia)
            np.testing.assert_array_equal(cb.cpu().numpy(), ocb)
            np.testing.assert_array_equal(ib.cpu().numpy(), oib)


def test_ball_query_grid_dense_shells(ext, oracle_ops):
    """shells with hundreds of hits per centre (the dense part of a real sweep): the running selection of the nsample
    smallest hit indices is cut back several times per centre (csrc/ball_query_grid.hip: keep_smallest + threshold); point
    order ascending, descending and shuffled inside the cells"""
    fused = ext[2]
    from tests.util import beam_batch
    rng = np.random.default_rng(5)
    n, m = 16384, 900
    beam = beam_batch(4500, 1, n)[..., :3]
    blob = (rng.normal(size=(1, n, 3)) * [2.0, 2.0, 0.3]).astype(np.float32)            # ~1000 points per 0.8 m cell
    clouds = [beam, blob, np.ascontiguousarray(blob[:, ::-1]), np.ascontiguousarray(blob[:, np.argsort(blob[0, :, 0])])]
    for xyz in clouds:
        new_xyz = np.ascontiguousarray(xyz[:, rng.choice(n, m, replace=False)] + np.float32(0.003))
        for sa, sb in [((0.0, 0.2, 16), (0.2, 0.8, 32)), ((0.0, 0.8, 16), (0.0, 0.8, 64))]:
            oca, oia = oracle_ops.ball_query_dilated(sa[0], sa[1], sa[2], xyz, new_xyz)
            ocb, oib = oracle_ops.ball_query_dilated(sb[0], sb[1], sb[2], xyz, new_xyz)
            assert ocb.max() == sb[2]
            ca, ia, cb, ib = fused.ball_query_pair(dev(xyz), dev(new_xyz), sa, sb, grid=True)
            np.testing.assert_array_equal(ca.cpu().numpy(), oca)
            np.testing.assert_array_equal(ia.cpu().numpy(), oia)
            np.testing.assert_array_equal(cb.cpu().numpy(), ocb)
            np.testing.assert_array_equal(ib.cpu().numpy(), oib)


def chain3_case(oracle_ops, c_in, widths, ns, b, n, m, sentinel=0.0):
    """one grouped three-layer MLP: (rows, idx, ctr, cnt) on the host, the layers on the device, and the oracle's three-layer
    sequence pooled into columns 3.. of a (b * m, widths[2] + 3) array pre-filled with `sentinel`"""
    rng = np.random.default_rng(sum(widths))
    ld = (3 + c_in + 3) // 4 * 4
    rows = np.zeros((b, n, ld), np.float32)
    rows[..., :3 + c_in] = rng.normal(size=(b, n, 3 + c_in))
    ctr = rng.normal(size=(b, m, 3)).astype(np.float32)
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    cnt = rng.integers(0, 3, (b, m)).astype(np.int32)
    dims = [ld] + list(widths)
    layers_np, layers_dev = [], []
    for i in range(3):
        kin = dims[i] if i == 0 else (dims[i] + 3) // 4 * 4
        wpad = (dims[i + 1] + 3) // 4 * 4
        w = np.zeros((kin, wpad), np.float32)
        w[:dims[i] if i else 3 + c_in, :dims[i + 1]] = rng.normal(size=(dims[i] if i else 3 + c_in, dims[i + 1])) / np.sqrt(dims[i])
        s = rng.normal(size=(dims[i + 1],)).astype(np.float32)
        layers_np.append((w, s))
        layers_dev.append((dev(w), dev(s), dims[i + 1], 1))
    h = oracle_ops.linear(rows, layers_np[0][0], layers_np[0][1], 1, idx=idx, ctr=ctr)
    h = oracle_ops.linear(np.ascontiguousarray(np.pad(h, ((0, 0), (0, layers_np[1][0].shape[0] - h.shape[1])))), layers_np[1][0], layers_np[1][1], 1)
    h = np.ascontiguousarray(np.pad(h[:, :widths[1]], ((0, 0), (0, layers_np[2][0].shape[0] - widths[1]))))
    ref = np.full((b * m, widths[2] + 3), sentinel, np.float32)
    oracle_ops.linear(h, layers_np[2][0][:, :widths[2]], layers_np[2][1], 1, cnt=cnt, pool=ns, out=ref, col0=3)
    return ld, rows, idx, ctr, cnt, layers_dev, ref


@pytest.mark.parametrize("c_in,widths,ns", [(1, (16, 16, 32), 16), (1, (32, 32, 64), 32), (4, (24, 32, 40), 16), (1, (8, 16, 16), 32),
                                             (64, (64, 64, 128), 16), (64, (64, 96, 128), 32), (64, (64, 96, 128), 16), (64, (64, 64, 128), 32)])
def test_mlp_chain3_equals_three_linears(ext, oracle_ops, c_in, widths, ns):
    """the fused narrow-MLP launch against the oracle's three-layer sequence (and hence against three
    det6d_linear calls, which test_linear_* pins to the same oracle)"""
    fused = ext[2]
    b, n, m = 2, 700, 96
    ld, rows, idx, ctr, cnt, layers_dev, ref = chain3_case(oracle_ops, c_in, widths, ns, b, n, m)
    assert fused.chain_eligible(ld, layers_dev, ns)
    out = torch.zeros((b * m, widths[2] + 3), device="cuda")
    fused.mlp_chain3(dev(rows), dev(idx), dev(ctr), dev(cnt), layers_dev, out, 3)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


SENT = -7.0


@pytest.mark.parametrize("c_in,widths", [(1, (16, 16, 32)), (4, (24, 32, 40)), (64, (64, 64, 128)), (64, (64, 96, 128))])
def test_chain_launch_accepts_exactly_what_its_plan_accepts(ext, oracle_ops, c_in, widths):
    """det6d_mlp_chain3 returns DET6D_OK exactly for the (b, m, ns) det6d_mlp_chain3_plan accepts — the launch routes by the
    function the query answers from — over the row counts at which the routes part: odd m with ns = 16 (two centres of a
    32-row tile in different scenes: LDS kernel for the narrow widths, refusal for the wide ones) and b * m * ns off the tiles.
    Accepted: the oracle's three layers bit for bit around an untouched sentinel; refused (a status before any launch): the
    sentinel everywhere."""
    fused = ext[2]
    L, n = fused.L, 64
    accepted = 0
    for b, m, ns in [(b, m, ns) for b in (1, 2) for m in (1, 2, 3, 6) for ns in (16, 32)]:
        ld, rows, idx, ctr, cnt, layers, ref = chain3_case(oracle_ops, c_in, widths, ns, b, n, m, SENT)
        plan = L.LaunchPlan()
        ok = L.lib().det6d_mlp_chain3_plan(ld, *widths, ns, b, m, 0, 0, plan) == 0
        assert fused.chain_eligible(ld, layers, ns, b, m) == ok
        out = torch.full((b * m, widths[2] + 3), SENT, device="cuda")
        d_rows, d_idx, d_ctr, d_cnt = dev(rows), dev(idx), dev(ctr), dev(cnt)
        (w1, s1, c1, _), (w2, s2, c2, _), (w3, s3, c3, _) = layers
        rc = L.lib().det6d_mlp_chain3(b * m * ns, n, m, ns, L.ptr(d_rows), ld, L.ptr(d_idx), L.ptr(d_ctr), 3, L.ptr(d_cnt), L.ptr(w1),
                                      w1.shape[1], L.ptr(s1), c1, L.ptr(w2), w2.shape[1], L.ptr(s2), c2, L.ptr(w3), w3.shape[1], L.ptr(s3),
                                      c3, L.ptr(out), out.shape[1], 3, L.stream_ptr())
        assert rc == (0 if ok else -1), (b, m, ns, rc, L.CHAIN_ROUTES[plan.route] if ok else None)
        np.testing.assert_array_equal(out.cpu().numpy(), ref if ok else np.full_like(ref, SENT), err_msg=str((b, m, ns)))
        accepted += ok
    assert 0 < accepted < 16


@pytest.mark.parametrize("b,m", [(1, 2), (2, 2), (1, 3), (2, 3)])
def test_group_launch_accepts_exactly_what_its_plan_accepts(ext, oracle_ops, b, m):
    """the same for det6d_mlp_group3 on dense rows, (128, 128, 256) with ns = 16: even m runs (== the oracle's expand + two
    linears), odd m is refused by plan and launch alike"""
    from tests.test_compact_gpu import make_layers, padded_query
    fused = ext[2]
    L, n, ns, c_in, widths = fused.L, 64, 16, 128, (128, 128, 256)
    rng = np.random.default_rng(m)
    ld = (3 + c_in + 3) // 4 * 4
    rows = np.zeros((b, n, ld), np.float32)
    rows[..., :3 + c_in] = rng.normal(size=(b, n, 3 + c_in))
    ctr = rng.normal(size=(b, m, 3)).astype(np.float32)
    cnt, idx = padded_query(rng, b, n, m, ns)
    layers_np, layers = make_layers(rng, ld, c_in, widths)
    ok = L.lib().det6d_mlp_group3_plan(*widths, ns, b, m, 0, 0, L.LaunchPlan()) == 0
    assert ok == (m % 2 == 0) == fused.group_kernel_eligible(layers, ns, False, b, m)
    ref = np.full((b * m, widths[2] + 4), SENT, np.float32)
    if ok:
        h = oracle_ops.linear(rows, layers_np[0][0], layers_np[0][1], 1, idx=idx, ctr=ctr)
        h = oracle_ops.linear(h, layers_np[1][0], layers_np[1][1], 1)
        oracle_ops.linear(h, layers_np[2][0][:, :widths[2]], layers_np[2][1], 1, cnt=cnt, pool=ns, out=ref, col0=4)
    d_rows, d_ctr, d_idx, d_cnt = dev(rows), dev(ctr), dev(idx), dev(cnt)
    wz = layers[0][0].clone()
    wz[:3] = 0
    p = torch.empty((b * n, wz.shape[1]), device="cuda")
    fused.linear(d_rows.view(b * n, ld), wz, None, 0, p)
    out = torch.full((b * m, widths[2] + 4), SENT, device="cuda")
    (w1, s1, c1, _), (w2, s2, c2, _), (w3, s3, c3, _) = layers
    rc = L.lib().det6d_mlp_group3(b * m * ns, L.ptr(p), p.shape[1], 0, L.ptr(w1), w1.shape[1], L.ptr(s1), c1, L.ptr(w2), w2.shape[1],
                                  L.ptr(s2), c2, L.ptr(w3), w3.shape[1], L.ptr(s3), c3, L.ptr(d_rows), ld, L.ptr(d_ctr), 3, L.ptr(d_idx), n,
                                  m, ns, L.ptr(d_cnt), None, None, None, L.ptr(out), out.shape[1], 4, L.stream_ptr())
    assert rc == (0 if ok else -1)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


def test_sa_layer_runs_the_shapes_the_chain_kernels_refuse():
    """dense rows, lda = 68, nsample 16 and THREE caller-supplied centres: the wide chain kernel pairs two centres per tile and
    refuses an odd m; forward_rows asks the plan at its (b, m) and takes the per-layer route (it used to offer the shape to the
    launch, which raised).  == the oracle's layer, bit for bit.  (DET6D_DENSE_ROWS is read at import: a child process.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'tests', 'gpu_scripts', 'sa_odd_centres.py')],
                         env=dict(os.environ, DET6D_DENSE_ROWS='1'), cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'sa_odd_centres ok' in out.stdout


def test_fallback_kernels_via_env_switches(tmp_path):
    """the plain predicated GEMM loader (tensors beyond 32-bit offsets), the LDS chain kernel and the
    three-GEMM route for SA2-sized groups are selected by size / shape at run time; force them with their
    environment switches in a child process and rerun the parity tests that cover them"""
    import subprocess
    import sys
    env = dict(os.environ, DET6D_EXPERIMENTS_LIB='1', DET6D_LINEAR_NO_FAST='1', DET6D_CHAIN_LDS='1', DET6D_CHAIN_NO_WIDE='1')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_ops_gpu.py'), '-q', '-x', '-m', 'gpu',
                          '-k', 'test_linear or (chain3 and not widths4 and not widths5 and not widths6 and not widths7)'], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'passed' in out.stdout


@pytest.mark.parametrize("b,n,m,c", [(2, 16384, 4096, 64), (1, 300, 50, 3), (1, 2048, 16384, 5), (3, 1024, 4093, 7), (2, 5000, 512, 4),
                                     (2, 1024, 4097, 5), (1, 3000, 8192, 1), (2, 2048, 6001, 64), (1, 1500, 16385, 3)])
def test_three_interpolate_shapes(ext, oracle_ops, b, n, m, c):
    """both forms of det6d_three_interpolate (channel rows staged in LDS when four, two or one of them fit 64 KB and n >= 1024,
    the plain gather otherwise; odd m: unaligned rows) against the oracle, bit for bit.  Two rows per workgroup (4096 < m <= 8192):
    m = 4097 with five channels (unaligned rows, the last channel block half full), m = 8192 (exactly 64 KB), m = 6001 (odd);
    m = 16385: one row too long for the LDS, the plain kernel at n >= 1024"""
    pn = ext[0]
    rng = np.random.default_rng(n + m)
    feats = rng.normal(size=(b, c, m)).astype(np.float32)
    idx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
    out = torch.empty((b, c, n), device="cuda")
    pn.three_interpolate_wrapper(b, c, m, n, dev(feats), dev(idx), dev(w), out)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle_ops.three_interpolate(feats, idx, w))


# ---- grid-stride second trips -------------------------------------------------------------------------------------------------
# csrc/points.hip launches at most 8192 workgroups of 256 lanes; beyond that a lane walks further elements by a grid-stride
# loop.  One case per kernel whose element count exceeds the cap by a ragged rest, the inner dimension placed so that the wrap
# falls inside a row.
POINTS_CAP = 8192 * 256
U24 = 2.0 ** -24


def scatter_sum64(index, terms, n):
    """(float64 sum, float64 sum of magnitudes, count) of `terms` (..., L) scattered to `index` (L,) in [0, n)"""
    lead = terms.shape[:-1]
    flat = terms.reshape(-1, terms.shape[-1]).astype(np.float64)
    total = np.stack([np.bincount(index, weights=row, minlength=n) for row in flat]).reshape(lead + (n,))
    mag = np.stack([np.bincount(index, weights=np.abs(row), minlength=n) for row in flat]).reshape(lead + (n,))
    return total, mag, np.bincount(index, minlength=n)


def check_atomic_sum(name, got, total, mag, count):
    """fp32 atomic adds in any order onto a zeroed element: every add rounds a partial sum of magnitude <= sum|terms| once
    (relative 2^-24), a term that is itself a rounded product brings one more, second-order terms one more:
    |got - sum64| <= (L_e + 2) * 2^-24 * sum|terms| with L_e the number of contributions.  Derived, not measured."""
    lim = (count + 2) * U24 * mag
    err = np.abs(got.astype(np.float64) - total)
    ratio = float((err / np.maximum(lim, 1e-300)).max())
    print('%s: contributions per element %d .. %d, largest ratio to the bound %.4f' % (name, count.min(), count.max(), ratio))
    assert np.isfinite(got).all() and (err <= lim).all(), ratio
    assert count.max() < 100 and count.min() >= 0


def test_grid_stride_second_trip_of_the_forward_index_kernels(ext, oracle_ops):
    pn, _, fused = ext
    rng = np.random.default_rng(77)
    # gather_points: 2 x 5 x 210 001 outputs
    b, c, n, m = 2, 5, 300, 210001
    assert POINTS_CAP < b * c * m < 2 * POINTS_CAP and (b * c * m) % POINTS_CAP and POINTS_CAP % m
    pts = rng.normal(size=(b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    out = torch.full((b, c, m), SENT, device="cuda")
    pn.gather_points_wrapper(b, c, n, m, dev(pts), dev(idx), out)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle_ops.gather_points(pts, idx))
    # group_points: 2 x 3 x 11 001 x 32
    b, c, n, m, ns = 2, 3, 300, 11001, 32
    assert POINTS_CAP < b * c * m * ns < 2 * POINTS_CAP and (b * c * m * ns) % POINTS_CAP and POINTS_CAP % (m * ns)
    pts = rng.normal(size=(b, c, n)).astype(np.float32)
    gidx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    gout = torch.full((b, c, m, ns), SENT, device="cuda")
    pn.group_points_wrapper(b, c, n, m, ns, dev(pts), dev(gidx), gout)
    np.testing.assert_array_equal(gout.cpu().numpy(), oracle_ops.group_points(pts, gidx))
    # three_interpolate, plain kernel (n < 1024 points per scene): 2 x 1051 x 999
    b, c, m, n = 2, 1051, 50, 999
    assert POINTS_CAP < b * c * n < 2 * POINTS_CAP and (b * c * n) % POINTS_CAP and POINTS_CAP % n
    feats = rng.normal(size=(b, c, m)).astype(np.float32)
    tidx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
    tout = torch.full((b, c, n), SENT, device="cuda")
    pn.three_interpolate_wrapper(b, c, m, n, dev(feats), dev(tidx), dev(w), tout)
    np.testing.assert_array_equal(tout.cpu().numpy(), oracle_ops.three_interpolate(feats, tidx, w))
    # gather_rows: 2 x 30 001 rows of 35 of 37 columns into rows of 36
    b, n, m, ld_in, ld_out, ncol = 2, 500, 30001, 37, 36, 35
    assert POINTS_CAP < b * m * ncol < 2 * POINTS_CAP and (b * m * ncol) % POINTS_CAP and POINTS_CAP % ncol
    rows_in = rng.normal(size=(b, n, ld_in)).astype(np.float32)
    ridx = rng.integers(0, n, (b, m)).astype(np.int32)
    rout = torch.full((b, m, ld_out), SENT, device="cuda")
    fused.gather_rows(dev(rows_in), dev(ridx), ncol, rout)
    got = rout.cpu().numpy()
    np.testing.assert_array_equal(got[..., :ncol], oracle_ops.gather_rows(rows_in, ridx, ncol, ld_out)[..., :ncol])
    assert (got[..., ncol:] == SENT).all()


def test_grid_stride_second_trip_of_the_atomic_gradients(ext):
    """gather_points_grad, group_points_grad, three_interpolate_grad beyond the launch cap: atomic adds, so the order of a sum is
    free; against the float64 sum within check_atomic_sum's bound, some 30 contributions per element"""
    pn = ext[0]
    rng = np.random.default_rng(78)
    # gather_points_grad: 2 x 5 x 210 001 terms onto 7000 points per (scene, channel)
    b, c, n, m = 2, 5, 7000, 210001
    assert POINTS_CAP < b * c * m < 2 * POINTS_CAP and (b * c * m) % POINTS_CAP and POINTS_CAP % m
    go = rng.normal(size=(b, c, m)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    gp = torch.zeros((b, c, n), device="cuda")
    pn.gather_points_grad_wrapper(b, c, n, m, dev(go), dev(idx), gp)
    got = gp.cpu().numpy()
    for bi in range(b):
        check_atomic_sum('gather_points_grad scene %d' % bi, got[bi], *scatter_sum64(idx[bi], go[bi], n))
    # group_points_grad: 2 x 3 x 11 001 x 32 terms onto 12 000 points
    b, c, n, m, ns = 2, 3, 12000, 11001, 32
    assert POINTS_CAP < b * c * m * ns < 2 * POINTS_CAP and (b * c * m * ns) % POINTS_CAP and POINTS_CAP % (m * ns)
    ggo = rng.normal(size=(b, c, m, ns)).astype(np.float32)
    gidx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    ggp = torch.zeros((b, c, n), device="cuda")
    pn.group_points_grad_wrapper(b, c, n, m, ns, dev(ggo), dev(gidx), ggp)
    got = ggp.cpu().numpy()
    for bi in range(b):
        check_atomic_sum('group_points_grad scene %d' % bi, got[bi], *scatter_sum64(gidx[bi].reshape(-1), ggo[bi].reshape(c, m * ns), n))
    # three_interpolate_grad: 2 x 3 x 350 003 outputs, three terms each (the fp32 product g * w), onto 35 000 points
    b, c, n, m = 2, 3, 350003, 35000
    assert POINTS_CAP < b * c * n < 2 * POINTS_CAP and (b * c * n) % POINTS_CAP and POINTS_CAP % n
    tgo = rng.normal(size=(b, c, n)).astype(np.float32)
    tidx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
    tgp = torch.zeros((b, c, m), device="cuda")
    pn.three_interpolate_grad_wrapper(b, c, n, m, dev(tgo), dev(tidx), dev(w), tgp)
    got = tgp.cpu().numpy()
    for bi in range(b):
        terms = tgo[bi].astype(np.float64)[:, :, None] * w[bi].astype(np.float64)[None]            # (c, n, 3): exact products
        check_atomic_sum('three_interpolate_grad scene %d' % bi, got[bi], *scatter_sum64(tidx[bi].reshape(-1), terms.reshape(c, n * 3), m))
