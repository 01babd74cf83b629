"""c-fps / df-fps numbers (de6d_amd/csrc/ext/sort_samplers.hip) beside the s-fps launches they replace.  Prints one JSON line
per result.  Two steps, each a child process of its own under `timeout` (a step that fails or hangs ends the run):
  samplers  in ONE process: s-fps (det6d_fps_fused, the baseline), c-fps (det6d_ext_topk_scores), the pillar weights
            (det6d_ext_pillar_weights) and df-fps end to end (weights + slice copy + det6d_fps_weights + offset), at
            4096 -> 512 and 512 -> 256, batches of 1, 8 and 80 scenes.  Median and quartiles of single launches timed with
            device events, the samplers taking turns launch by launch.
  frames    in ONE process: one frame (1 x 16384 points, captured pass) of det6d_car, det6d_car_cfps and det6d_car_dffps, the
            configs taking turns frame by frame.

    python scripts/samplers_measure.py [--quick]
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

STEPS = {'samplers': 420, 'frames': 420}          # seconds each child may take


def quartiles(us):
    q = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(us_median=round(float(q[1]), 2), us_q1=round(float(q[0]), 2), us_q3=round(float(q[2]), 2))


def step_samplers(quick):
    import torch
    from de6d_amd.ops import fused, sort_samplers
    if not torch.cuda.is_available():
        raise RuntimeError("samplers_measure.py needs a GPU")
    reps = 30 if quick else 200
    for b in (1, 8, 80):
        for n, m in ((4096, 512), (512, 256)):
            rng = np.random.default_rng(n + b)
            xyz = np.stack([rng.uniform(0, 70.4, (b, n)), rng.uniform(-40, 40, (b, n)), rng.uniform(-3, 1, (b, n))], -1)
            xyz = torch.from_numpy(xyz.astype(np.float32)).cuda()
            scores = torch.from_numpy(rng.standard_normal((b, n)).astype(np.float32)).cuda()
            idx = torch.empty((b, 2 * m), dtype=torch.int32, device='cuda')
            temp = fused.fps_workspace(b, n, xyz.device)
            arms = {
                's-fps': lambda: fused.fps_fused(xyz, 0, n, m, scores, 1.0, idx, 0, temp),
                'c-fps': lambda: sort_samplers.topk_scores(scores, m, 1.0, 0, n, idx, 0),
                'pillar_weights': lambda: sort_samplers.pillar_weights(xyz, 0, n),
                'df-fps': lambda: sort_samplers.pillar_density_fps(xyz, m, 0, n, idx, m),
            }
            for fn in arms.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(reps):
                for name, fn in arms.items():             # the arms take turns: drift of the clock hits all alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(1e3 * e0.elapsed_time(e1))
            for name, us in times.items():
                print(json.dumps(dict(what='sampler_launch', sampler=name, b=b, n=n, m=m, reps=reps, **quartiles(us))), flush=True)


def step_frames(quick):
    import torch
    from de6d_amd.runtime import load_config, build_model, GraphedDet6D
    from tests.util import make_batch
    if not torch.cuda.is_available():
        raise RuntimeError("samplers_measure.py needs a GPU")
    reps = 10 if quick else 60
    b, n = 1, 16384
    batch = make_batch(5, b, n)
    pts = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.float32), batch.reshape(n, 4)], 1)).cuda()
    names = ('kitti_models/det6d_car.yaml', 'kitti_models/det6d_car_cfps.yaml', 'kitti_models/det6d_car_dffps.yaml')
    runners = {}
    for name in names:
        runners[name] = GraphedDet6D(build_model(load_config(name), seed=7, device='cuda'), b, n)
        for _ in range(3):
            runners[name].launch(pts).finalize()
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for _ in range(reps):
        for name in names:
            t0 = time.perf_counter()
            runners[name].launch(pts).finalize()
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0))
    for name, us in times.items():
        q = quartiles(us)
        print(json.dumps(dict(what='one_frame', cfg=name, reps=reps, ms_median=round(q['us_median'] / 1e3, 3),
                              ms_q1=round(q['us_q1'] / 1e3, 3), ms_q3=round(q['us_q3'] / 1e3, 3))), flush=True)


def main():
    quick = '--quick' in sys.argv
    if '--step' in sys.argv:
        step = sys.argv[sys.argv.index('--step') + 1]
        {'samplers': step_samplers, 'frames': step_frames}[step](quick)
        return 0
    for step, seconds in STEPS.items():
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--step', step]
        rc = subprocess.run(cmd + (['--quick'] if quick else []), cwd=ROOT).returncode
        if rc != 0:
            print(json.dumps(dict(what='failed', step=step, exit_status=rc)), flush=True)
            return rc                                   # nothing more is started on the GPU after a failed step
    return 0


if __name__ == '__main__':
    sys.exit(main())
