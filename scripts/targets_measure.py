"""Target-assignment numbers (de6d_amd/csrc/ext/box_targets.hip).  Prints one JSON line per result.
  (default)     on the GPU, in one child process under `timeout`: det6d_ext_assign_targets9 (box index + class labels + 9 box
                columns) and det6d_ext_points_in_boxes9 (box index only) for the head's shape (8 x 256 points, 32 boxes) and
                for whole clouds (8 and 80 x 16384 points, 64 boxes, and 1 box to separate the box loop from the memory
                traffic).  Clouds are uniform over the KITTI range, so nearly every point is outside every box and scans all
                of them: the worst case.  Median and quartiles of single launches timed with device events, the arms taking
                turns launch by launch; bytes = one read of the point rows and one write of the outputs.
  --reference   on the host CPU, authoring machine only (needs the reference checkout, like tests/golden/make_golden*.py): the
                reference's own box_utils.points_in_boxes3d, scene by scene, on the same inputs.

    python scripts/targets_measure.py [--quick] [--reference]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if int(os.environ.get('GPU_MAX_HW_QUEUES', '0')) < 24:
    os.environ['GPU_MAX_HW_QUEUES'] = '24'

SHAPES = [(8, 256, 32), (8, 16384, 64), (80, 16384, 64), (8, 16384, 1), (80, 16384, 1)]
SECONDS = 420


def inputs(b, n, m):
    """stacked rows [scene, x, y, z] of b uniform clouds, (b, m, 10) boxes"""
    rng = np.random.default_rng(b * 100003 + n + m)
    xyz = np.stack([rng.uniform(0, 70.4, (b, n)), rng.uniform(-40, 40, (b, n)), rng.uniform(-3, 1, (b, n))], -1)
    rows = np.concatenate([np.repeat(np.arange(b), n)[:, None], xyz.reshape(-1, 3)], -1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0, 70.4, (b, m, 1)), rng.uniform(-40, 40, (b, m, 1)), rng.uniform(-3, 1, (b, m, 1)),
                            rng.uniform(1.5, 5, (b, m, 1)), rng.uniform(1.4, 2.2, (b, m, 1)), rng.uniform(1.2, 2, (b, m, 1)),
                            rng.uniform(-np.pi, np.pi, (b, m, 1)), rng.uniform(-0.5, 0.5, (b, m, 1)),
                            rng.uniform(-0.3, 0.3, (b, m, 1)), np.ones((b, m, 1))], -1).astype(np.float32)
    return rows, boxes


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def step_gpu(quick):
    import torch
    from de6d_amd import _lib as L
    if not torch.cuda.is_available():
        raise RuntimeError("targets_measure.py needs a GPU")
    reps = 30 if quick else 200
    for b, n, m in SHAPES:
        rows, boxes = inputs(b, n, m)
        rows, boxes = torch.from_numpy(rows).cuda(), torch.from_numpy(boxes).cuda()
        npts = b * n
        idx = torch.empty(npts, dtype=torch.int32, device='cuda')
        cls = torch.empty(npts, dtype=torch.int64, device='cuda')
        lab = torch.empty((npts, 9), dtype=torch.float32, device='cuda')
        arms = {   # the C entries on preallocated outputs: the launch alone, no allocation or fill
            'assign_targets9': (lambda: L.call_ext("det6d_ext_assign_targets9", npts, L.ptr(rows), 4, 1, 0, 1, b, m, L.ptr(boxes), 10,
                                                   None, 9, 1, 10.0, L.ptr(idx), L.ptr(cls), L.ptr(lab), 9, 9, L.stream_ptr()),
                                npts * (16 + 4 + 8 + 36)),
            'points_in_boxes9': (lambda: L.call_ext("det6d_ext_points_in_boxes9", npts, L.ptr(rows), 4, 1, 0, 1, b, m, L.ptr(boxes),
                                                    10, None, L.ptr(idx), L.stream_ptr()), npts * (16 + 4)),
        }
        for fn, _ in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        inside = float((idx >= 0).float().mean())
        times = {k: [] for k in arms}
        for _ in range(reps):
            for name, (fn, _) in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1))
        for name, us in times.items():
            q = quartiles(us)
            nbytes = arms[name][1]
            print(json.dumps(dict(what='targets_launch', entry=name, b=b, n=n, m=m, reps=reps, inside=round(inside, 4), bytes=nbytes,
                                  gb_per_s=round(nbytes / q['us_median'] / 1e3, 1),
                                  ns_per_pair=round(1e3 * q['us_median'] / (npts * m), 4), **q)), flush=True)


def step_reference(quick):
    import importlib.util
    golden = os.path.join(ROOT, 'tests', 'golden')
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.install_reference_stubs()
    sys.path.insert(0, mg.REF)
    from pcdet.utils import box_utils as ref_box_utils
    for b, n, m in SHAPES[:2]:
        rows, boxes = inputs(b, n, m)
        times = []
        for _ in range(2 if quick else 5):
            t0 = time.perf_counter()
            for s in range(b):
                ref_box_utils.points_in_boxes3d(rows[s * n:(s + 1) * n, 1:4], boxes[s, :, :9])
            times.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(what='reference_points_in_boxes3d_host', b=b, n=n, m=m, ms_median=round(float(np.median(times)), 2),
                              ms_min=round(min(times), 2))), flush=True)


def main():
    quick = '--quick' in sys.argv
    if '--reference' in sys.argv:
        step_reference(quick)
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
