"""Grouped-MLP backward numbers (de6d_amd/csrc/ext/group_backward.hip and prepare_loss(head=True)).  Prints one JSON line per
result.  On the GPU, in one child process under `timeout`, every call timed with device events on preallocated buffers, median
and quartiles of 200 calls after warm-up (--quick: 20):
  kernels   det6d_ext_group_gather, det6d_ext_group_pool_backward, det6d_ext_group_centre_grad and det6d_ext_vote_backward at
            the KITTI head's shapes (b = 8, m = 256; groups ns = 16, 259 -> 256 -> 256 -> 512 and ns = 32,
            259 -> 256 -> 512 -> 1024), with the bytes each must move and the rate that makes, against the 6.3 TB/s a kernel
            can reach from HBM on this chip
  step      prepare_loss + get_loss + backward of kitti_models/det6d_car_loss.yaml on 8 synthetic scenes of 16384 points, with
            head=True and with towers=True, taking turns call by call

    python scripts/group_backward_measure.py [--quick]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, M, N, K, LD = 8, 256, 16384, 259, 260
GROUPS = ((16, 512), (32, 1024))                                         # (ns, pooled width of the group)
HBM_TBPS = 6.3
SECONDS = 500


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def timed(arms, reps):
    """arms {name: fn} taking turns call by call -> {name: [us]}"""
    import torch
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1))
    return times


def report(what, us, nbytes, **kw):
    q = quartiles(us)
    tbps = nbytes / (q['us_median'] * 1e-6) / 1e12
    print(json.dumps(dict(what=what, bytes=int(nbytes), tb_per_s=round(tbps, 3), of_hbm_rate=round(tbps / HBM_TBPS, 3), **kw, **q)),
          flush=True)


def kernels(reps):
    import torch
    from de6d_amd.ops import group_backward as op
    g = torch.Generator(device='cuda').manual_seed(1)
    pts = torch.randn((B, N, LD), device='cuda', generator=g)
    ctr = torch.randn((B, M, 3), device='cuda', generator=g)
    for ns, c in GROUPS:
        rows = B * M * ns
        idx = torch.randint(0, N, (B, M, ns), device='cuda', generator=g, dtype=torch.int32)
        cnt = torch.randint(0, ns + 1, (B, M), device='cuda', generator=g, dtype=torch.int32)
        x0 = torch.empty((rows, LD), device='cuda')
        y = torch.relu(torch.randn((rows, c), device='cuda', generator=g))
        d_pooled = torch.randn((B * M, 1536), device='cuda', generator=g)
        dz = torch.empty((rows, c), device='cuda')
        dx = torch.randn((rows, 3), device='cuda', generator=g)
        dctr = torch.empty((B * M, 3), device='cuda')
        arms = dict(gather=lambda: op.group_gather(pts, idx, ctr, k=K, out=x0),
                    pool_backward=lambda: op.pool_backward(y, cnt, d_pooled, ns, c, gcol0=0, dz=dz),
                    centre_grad=lambda: op.centre_grad(dx, ns, out=dctr))
        t = timed(arms, reps)
        # gather: a 1036-byte piece of a point row in, a 1040-byte row out, an index per row, a centre per group
        report('group_gather', t['gather'], rows * (K * 4 + LD * 4 + 4) + B * M * 12, ns=ns, rows=rows, k=K, reps=reps)
        # pool_backward: Y once, dz once, d(pooled) and cnt once
        report('group_pool_backward', t['pool_backward'], rows * c * 8 + B * M * (c * 4 + 4), ns=ns, rows=rows, c=c, reps=reps)
        report('group_centre_grad', t['centre_grad'], rows * 12 + B * M * 12, ns=ns, rows=rows, reps=reps)
    rows = B * M
    off = torch.randn((rows, 3), device='cuda', generator=g) * 2.5
    dv = torch.randn((rows, 3), device='cuda', generator=g)
    out = torch.empty((rows, 3), device='cuda')
    t = timed(dict(vote=lambda: op.vote_backward(off, (3.0, 3.0, 2.0), dv, out=out)), reps)
    report('vote_backward', t['vote'], rows * 36, rows=rows, reps=reps)


def step(reps):
    import torch
    from de6d_amd.runtime import load_config, build_model
    from de6d_amd.synthetic import make_batch
    cfg = load_config('kitti_models/det6d_car_loss.yaml')
    net = build_model(cfg, seed=11, device='cuda')
    head = net.point_head
    pts = make_batch(7, B, N)
    flat = np.concatenate([np.repeat(np.arange(B, dtype=np.float32), N)[:, None], pts.reshape(B * N, -1)], 1).astype(np.float32)
    bd = {'batch_size': B, 'points': torch.from_numpy(flat).cuda()}
    with torch.no_grad():
        net(bd)
    vote = bd['point_vote_coords'][:, 1:4].reshape(B, -1, 3)
    gt = torch.zeros((B, 16, 10), device='cuda')
    gt[:, :10, :3] = vote[:, ::25][:, :10]                               # ten boxes per scene around vote points, then zero rows
    gt[:, :10, 3:6] = torch.tensor([4.0, 2.0, 2.0], device='cuda')
    gt[:, :10, 9] = 1.0
    bd['gt_boxes'] = gt

    def run(**kw):
        for p in net.parameters():
            p.grad = None
        head.prepare_loss(bd, requires_grad=True, **kw)
        loss, _ = head.get_loss()
        loss.backward()
        return loss

    t = timed(dict(head=lambda: run(head=True), towers=lambda: run(towers=True)), reps)
    loss = float(run(head=True).detach())
    with_grad = sum(p.grad is not None for p in head.parameters())
    for name, us in t.items():
        print(json.dumps(dict(what='training_step', arm=name, b=B, n=N, reps=reps, loss=round(loss, 5),
                              head_parameters_with_grad=with_grad, **quartiles(us))), flush=True)


def step_gpu(quick):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("group_backward_measure.py needs a GPU")
    reps = 20 if quick else 200
    kernels(reps)
    step(reps)


def main():
    quick = '--quick' in sys.argv
    if '--step' in sys.argv:
        step_gpu(quick)
        return 0
    cmd = ['timeout', '-k', '10', str(SECONDS), sys.executable, os.path.abspath(__file__), '--step', 'gpu']
    rc = subprocess.run(cmd + (['--quick'] if quick else []), cwd=ROOT).returncode
    if rc != 0:
        print(json.dumps(dict(what='failed', step='gpu', exit_status=rc)), flush=True)
    return rc


if __name__ == '__main__':
    sys.exit(main())
