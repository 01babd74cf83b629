"""SASA-loss numbers (de6d_amd/csrc/ext/sasa_loss.hip).  Prints one JSON line per result.
On the GPU, in one child process under `timeout`: labels + loss + backward of the KITTI shape — 8 scenes, SA levels of 4096 and
1024 points with scores and one of 512 without, 64 boxes of which 40 real, BCE with set_ignore_flag and extra_width 0.2 — as
  hip     ops.sasa_loss.forward(labels=True) + ops.sasa_loss.backward (three launches and the allocations of their outputs);
  torch   torch_sasa below: a plain-torch composition of the same semantics, written the way torch is fastest at it (all scenes
          and boxes of a level in one broadcast, no per-scene loop and no host read — the reference's own loop is slower
          still), with autograd for the gradient.
A step is timed with device events; the two arms take turns step by step; median and quartiles over the steps.  Before timing,
the two arms' labels, losses and gradients are compared (labels: the share of rows that differ — fp32 roundings at a face).

    python scripts/sasa_measure.py [--quick]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDS = 300
B, LEVELS, BOXES, REAL = 8, (4096, 1024, 512), 64, 40
WEIGHTS, EXTRA = [0.01, 0.1, 1.0], [0.2, 0.2, 0.2]


def inputs():
    rng = np.random.default_rng(8)
    gt = np.zeros((B, BOXES, 10), np.float32)
    gt[:, :REAL, 0], gt[:, :REAL, 1] = rng.uniform(0, 70, (B, REAL)), rng.uniform(-40, 40, (B, REAL))
    gt[:, :REAL, 2] = rng.uniform(-1.5, 0, (B, REAL))
    gt[:, :REAL, 3:6] = rng.uniform([3.5, 1.5, 1.4], [4.5, 2.0, 1.8], (B, REAL, 3))
    gt[:, :REAL, 6], gt[:, :REAL, 9] = rng.uniform(-np.pi, np.pi, (B, REAL)), 1
    coords, scores = [], []
    for m in LEVELS:
        pts = np.stack([rng.uniform(0, 70, (B, m)), rng.uniform(-40, 40, (B, m)), rng.uniform(-3, 1, (B, m))], -1)
        near = gt[np.arange(B)[:, None], rng.integers(0, REAL, (B, m)), :3] + rng.uniform(-1.2, 1.2, (B, m, 3))
        coords.append(np.where(rng.random((B, m, 1)) < 0.4, near, pts).astype(np.float32))
        scores.append(rng.standard_normal((B * m, 1)).astype(np.float32))
    scores[-1] = None                                        # the last level has no confidence layer
    return coords, scores, gt


def torch_sasa(coords, scores, gt, extra):
    """labels, per-layer losses and the total of PointSASALoss (BCE, set_ignore_flag) in plain torch, all scenes at once"""
    import torch
    import torch.nn.functional as F
    c, s = torch.cos(-gt[:, None, :, 6]), torch.sin(-gt[:, None, :, 6])
    labels, losses = [], []
    for xyz, x, w in zip(coords, scores, WEIGHTS):
        if x is None or w == 0:
            labels.append(None)
            continue
        d = xyz[:, :, None, :] - gt[:, None, :, :3]                        # (B, M, T, 3)
        lx, ly = (d[..., 0] * c + d[..., 1] * (-s)).abs(), (d[..., 0] * s + d[..., 1] * c).abs()
        dz = d[..., 2].abs()

        def inside(dims):
            return ((dz <= dims[..., 2] / 2) & (lx < dims[..., 0] / 2 + 1e-5) & (ly < dims[..., 1] / 2 + 1e-5)).any(-1)
        fg = inside(gt[:, None, :, 3:6])
        ext = inside(gt[:, None, :, 3:6] + extra)
        lab = torch.where(fg, 1, torch.where(ext, -1, 0)).reshape(-1)
        valid = (lab >= 0).float()
        bce = F.binary_cross_entropy_with_logits(x.reshape(-1), (lab > 0).float(), reduction='none')
        losses.append(w * (bce * valid).sum() / valid.sum().clamp(min=1.0))
        labels.append(lab)
    return labels, losses, sum(losses)


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def step_gpu(quick):
    import torch
    from de6d_amd.ops import sasa_loss
    if not torch.cuda.is_available():
        raise RuntimeError("sasa_measure.py needs a GPU")
    reps = 30 if quick else 300
    coords, scores, gt = inputs()
    coords = [torch.from_numpy(x).cuda() for x in coords]
    scores = [None if x is None else torch.from_numpy(x).cuda().requires_grad_(True) for x in scores]
    gt = torch.from_numpy(gt).cuda()
    spec = sasa_loss.SasaSpec('BCE', WEIGHTS, EXTRA, True)
    extra = spec.extra(gt.device)
    one = torch.ones(1, dtype=torch.float32, device='cuda')
    detached = [None if x is None else x.detach() for x in scores]

    def hip():
        sums, labels = sasa_loss.forward(spec, coords, detached, gt, labels=True)
        return labels, sums, sasa_loss.backward(spec, sums, one, coords, detached, gt, labels=labels)

    def plain():
        labels, losses, total = torch_sasa(coords, scores, gt, extra)
        return labels, total, torch.autograd.grad(total, [x for x in scores if x is not None])
    arms = {'hip': hip, 'torch': plain}
    h, t = hip(), plain()
    torch.cuda.synchronize()
    differ = sum(int((a != b).sum()) for a, b in zip(h[0][:2], t[0][:2]))
    print(json.dumps(dict(what='sasa_agreement', rows=B * (LEVELS[0] + LEVELS[1]), labels_that_differ=differ,
                          foreground=int(sum((a == 1).sum() for a in h[0][:2])), ignored=int(sum((a == -1).sum() for a in h[0][:2])),
                          total_hip=float(h[1][-1]), total_torch=float(t[1].detach()),
                          grad_max_abs_diff=max(float((a - b).abs().max()) for a, b in zip(h[2][:2], t[2])))), flush=True)
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1))
    for name, us in times.items():
        print(json.dumps(dict(what='sasa_step', arm=name, scenes=B, levels=list(LEVELS[:2]), boxes=BOXES, reps=reps,
                              **quartiles(us))), flush=True)


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
