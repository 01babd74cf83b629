"""MLP-backward numbers (de6d_amd/csrc/ext/mlp_backward.hip).  Prints one JSON line per result.
On the GPU, in one child process under `timeout`: each layer of the head's towers at the benchmark shape (2048 rows:
1536 -> 512, 512 -> 128, 128 -> 32, 128 -> 1), three arms taking turns call by call, every call timed with device events
on preallocated buffers:
  backward   det6d_ext_linear_backward (dx with the ReLU mask, dw and dshift: two to four kernels)
  forward    det6d_linear at the same shape; the backward is twice its flops, so the line reports t_bwd / (2 t_fwd)
  matmul     torch.matmul for the same two products (dz @ W^T and x^T @ dz), for scale: no mask, no dshift
Median and quartiles of 200 calls per arm (--quick: 20).

    python scripts/mlp_backward_measure.py [--quick]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2048, 1536, 512), (2048, 512, 128), (2048, 128, 32), (2048, 128, 1))
SECONDS = 300


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def step_gpu(quick):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("mlp_backward_measure.py needs a GPU")
    from de6d_amd import _lib as L
    from de6d_amd.ops import fused
    reps = 20 if quick else 200
    for rows, k, n in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(k + n)
        x = torch.relu(torch.randn((rows, k), device='cuda', generator=g))
        ldw = (n + 3) // 4 * 4
        w = torch.zeros((k, ldw), device='cuda')
        w[:, :n] = torch.randn((k, n), device='cuda', generator=g) / k ** 0.5
        dz = torch.randn((rows, n), device='cuda', generator=g)
        shift = torch.zeros((n,), device='cuda')
        y = torch.empty((rows, n), device='cuda')
        dx, dw, ds = torch.empty((rows, k), device='cuda'), torch.empty((k, n), device='cuda'), torch.empty((n,), device='cuda')
        ws_bytes = int(L.ext_lib().det6d_ext_linear_backward_workspace_bytes(rows, k, n))
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device='cuda')
        wt = w[:, :n].contiguous()

        def backward():
            L.call_ext("det6d_ext_linear_backward", rows, k, n, L.ptr(x), k, 0, L.ptr(w), ldw, 0, L.ptr(dz), n, 1, L.ptr(dx), k, 0,
                       L.ptr(dw), n, L.ptr(ds), L.ptr(ws), ws_bytes, L.stream_ptr())

        def forward():
            fused.linear(x, w, shift, 1, y, ncols=n)

        def matmul():
            torch.matmul(dz, wt.t(), out=dx)
            torch.matmul(x.t(), dz, out=dw)
        arms = dict(backward=backward, forward=forward, matmul=matmul)
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
        backward()
        torch.cuda.synchronize()
        check = round(float(dw.abs().sum()), 3)
        med = {name: float(np.median(us)) for name, us in times.items()}
        for name, us in times.items():
            print(json.dumps(dict(what='mlp_backward_call', arm=name, rows=rows, k=k, n=n, reps=reps, **quartiles(us))), flush=True)
        print(json.dumps(dict(what='mlp_backward_ratio', rows=rows, k=k, n=n, bwd_over_2fwd=round(med['backward'] / (2 * med['forward']), 3),
                              bwd_over_matmul=round(med['backward'] / med['matmul'], 3),
                              bwd_tflops=round(4e-6 * rows * k * n / med['backward'], 3), dw_abs_sum=check)), flush=True)


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
