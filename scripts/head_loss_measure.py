"""Head-loss numbers (de6d_amd/csrc/ext/head_loss.hip).  Prints one JSON line per result.
  (default)     on the GPU, in one child process under `timeout`: det6d_ext_head_loss_forward (two kernels) and
                det6d_ext_head_loss_backward (one) on preallocated buffers at n = 2048 and n = 20480 rows of the car model's
                shape (one class, 12 bins, ground aware, centerness and corner loss on, half the rows foreground).  Median and
                quartiles of single calls timed with device events, the two arms taking turns call by call.
  --loop N      the program to put under a kernel trace: N times HeadLoss.apply + backward through autograd on n rows
                (--rows, default 2048), after one warm-up pass; prints how many passes it made.
                    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d OUT -o head_loss -- \\
                        python scripts/head_loss_measure.py --loop 20
                the kernel count per get_loss + backward is the trace's calls of each kernel over N + 1.

    python scripts/head_loss_measure.py [--quick]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (2048, 20480)
SECONDS = 300
ORDER = ('vote_preds', 'vote_reg_labels', 'vote_cls_labels', 'cls_preds', 'cls_labels', 'reg_preds', 'reg_labels', 'box_labels')


def inputs(n, nb=12):
    """rows shaped like the car model's: labels as the assignment leaves them, predictions around the labels"""
    rng = np.random.default_rng(n)
    labels = rng.choice([-1, 0, 0, 1, 1, 1], n).astype(np.int64)
    pos = labels > 0
    box = np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(0.5, 5, (n, 3)), rng.uniform(-3, 3, (n, 1)),
                          rng.uniform(-0.5, 0.5, (n, 1)), rng.uniform(-0.3, 0.3, (n, 1))], -1).astype(np.float32)
    points = (box[:, :3] + rng.uniform(-0.4, 0.4, (n, 3)) * box[:, 3:6]).astype(np.float32)
    reg = np.zeros((n, 6 + 2 * nb + 2), np.float32)
    reg[:, :3], reg[:, 3:6] = box[:, :3] - points, np.log(box[:, 3:6])
    k = rng.integers(0, nb, n)
    reg[np.arange(n), 6 + k], reg[np.arange(n), 6 + nb + k] = 1.0, rng.uniform(-0.5, 0.5, n)
    reg[:, 6 + 2 * nb] = box[:, 7] < -0.17
    reg[:, 6 + 2 * nb + 1] = np.where(box[:, 7] < -0.17, (-0.17 - box[:, 7]) / 0.78, 0)
    reg[~pos], box[~pos] = 0, 0
    vcls = (rng.random(n) < 0.4).astype(np.int64)
    return dict(vote_preds=points, vote_reg_labels=np.where(vcls[:, None] > 0, points + 0.3, 0).astype(np.float32),
                vote_cls_labels=vcls, cls_preds=rng.standard_normal((n, 1)).astype(np.float32), cls_labels=labels,
                reg_preds=(reg + 0.15 * rng.standard_normal(reg.shape)).astype(np.float32), reg_labels=reg, box_labels=box)


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def device_inputs(n):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("head_loss_measure.py needs a GPU")
    arrays = inputs(n)
    return [torch.from_numpy(arrays[k]).cuda() for k in ORDER]


def step_gpu(quick):
    import torch
    from de6d_amd import _lib as L
    from de6d_amd.ops import head_loss
    reps = 30 if quick else 300
    spec = head_loss.LossSpec(1, 12, weights={'point_angle_cls_weight': 0.2, 'point_pitch_cls_weight': 0.2})
    for n in SIZES:
        t = device_inputs(n)
        ws_bytes = L.ext_lib().det6d_ext_head_loss_workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        sums = torch.empty(16, dtype=torch.float32, device='cuda')
        g = torch.ones((), dtype=torch.float32, device='cuda')
        grads = [torch.empty_like(t[0]), torch.empty_like(t[3]), torch.empty_like(t[5])]
        head = [n, spec.num_class, spec.angle_bin_num, spec.flags, spec.cfg] + [L.ptr(x) for x in t] + [t[7].shape[1]]
        arms = {   # the C entries on preallocated buffers: the launches alone
            'forward': lambda: L.call_ext("det6d_ext_head_loss_forward", *head, L.ptr(ws), ws_bytes, L.ptr(sums), None, None, None,
                                          L.stream_ptr()),
            'backward': lambda: L.call_ext("det6d_ext_head_loss_backward", *head, L.ptr(sums), L.ptr(g), *[L.ptr(x) for x in grads],
                                           L.stream_ptr()),
        }
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
            print(json.dumps(dict(what='head_loss_call', entry=name, n=n, reps=reps, loss=round(float(sums[0]), 6),
                                  **quartiles(us))), flush=True)


def step_loop(passes, n):
    import torch
    from de6d_amd.ops import head_loss
    spec = head_loss.LossSpec(1, 12, weights={'point_angle_cls_weight': 0.2, 'point_pitch_cls_weight': 0.2})
    t = device_inputs(n)
    leaves = [t[0].requires_grad_(True), t[3].requires_grad_(True), t[5].requires_grad_(True)]
    for _ in range(passes + 1):
        loss, _ = head_loss.HeadLoss.apply(spec, leaves[0], leaves[1], leaves[2], t[1], t[2], t[4], t[6], t[7])
        grads = torch.autograd.grad(loss, leaves)
    torch.cuda.synchronize()
    print(json.dumps(dict(what='head_loss_loop', n=n, passes=passes + 1, loss=round(float(loss), 6),
                          grad_abs_sum=round(float(grads[2].abs().sum()), 6))), flush=True)


def main():
    quick = '--quick' in sys.argv
    if '--loop' in sys.argv:
        rows = int(sys.argv[sys.argv.index('--rows') + 1]) if '--rows' in sys.argv else 2048
        step_loop(int(sys.argv[sys.argv.index('--loop') + 1]), rows)
        return 0
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
