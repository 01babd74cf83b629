"""F-FPS numbers (de6d_amd/csrc/ext/fps_features.hip): us per pick and skip rate of the sampler alone, one-frame latency of
det6d_car_ffps beside det6d_car, and scenes/s of det6d_car_ffps through ScenePipeline.  Prints one JSON line per result.

    python scripts/ffps_measure.py [--quick]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if int(os.environ.get('GPU_MAX_HW_QUEUES', '0')) < 24:
    os.environ['GPU_MAX_HW_QUEUES'] = '24'


def sampler(b, n, m, c, reps=10):
    from de6d_amd.ops import ffps
    rng = np.random.default_rng(0)
    rows = np.zeros((b, n, (3 + c + 3) // 4 * 4), np.float32)
    rows[..., 0] = rng.uniform(0, 70.4, (b, n))
    rows[..., 1] = rng.uniform(-40, 40, (b, n))
    rows[..., 2] = rng.uniform(-3, 1, (b, n))
    rows[..., 3:3 + c] = np.maximum(rng.standard_normal((b, n, c)), 0)
    rows = torch.from_numpy(rows).cuda()
    ws = ffps.workspace(b, n)
    idx = torch.empty((b, m), dtype=torch.int32, device='cuda')
    ffps.fps_features(rows, c, m, 1.0, idx_out=idx, ws=ws)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        ffps.fps_features(rows, c, m, 1.0, idx_out=idx, ws=ws)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    evals, wave_evals = ffps.skip_stats(ws, b, n)
    point_rounds = n * (m - 1)
    waves = (min(n, 1024) + 63) // 64
    return dict(what='ffps_sampler', b=b, n=n, m=m, c=c, ms=round(ms, 4), us_per_pick=round(ms * 1e3 / m, 3),
                skip_rate=round(1 - float(evals.sum()) / (b * point_rounds), 4),
                wave_slot_skip_rate=round(1 - float(wave_evals.sum()) / (b * waves * (m - 1) * ((n + 1023) // 1024)), 4))


def one_frame(cfg_name, reps=20):
    from de6d_amd.runtime import load_config, build_model, GraphedDet6D
    from tests.util import make_batch
    cfg = load_config(cfg_name)
    model = build_model(cfg, seed=7, device='cuda')
    b, n = 1, 16384
    batch = make_batch(5, b, n)
    pts = np.concatenate([np.zeros((n, 1), np.float32), batch.reshape(n, 4)], 1)
    pts = torch.from_numpy(pts).cuda()
    runner = GraphedDet6D(model, b, n)
    for _ in range(3):
        runner.launch(pts).finalize()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        runner.launch(pts).finalize()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return dict(what='one_frame', cfg=cfg_name, ms_median=round(1e3 * float(np.median(t)), 3))


def pipeline(cfg_name, steps=60, b=8):
    from de6d_amd.runtime import load_config, build_model, ScenePipeline
    cfg = load_config(cfg_name)
    model = build_model(cfg, seed=7, device='cuda')
    pipe = ScenePipeline(model, b, 16384)
    pipe.run(8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe.run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(what='pipeline', cfg=cfg_name, batch=b, steps=steps, scenes_per_s=round(steps * b / dt, 1))


def main():
    quick = '--quick' in sys.argv
    for b in (8, 80):
        for n, m, c in ((4096, 512, 64), (512, 256, 128)):
            print(json.dumps(sampler(b, n, m, c)), flush=True)
    print(json.dumps(sampler(8, 16384, 2048, 64, reps=3)), flush=True)
    if quick:
        return
    for cfg in ('kitti_models/det6d_car.yaml', 'kitti_models/det6d_car_ffps.yaml'):
        print(json.dumps(one_frame(cfg)), flush=True)
    print(json.dumps(pipeline('kitti_models/det6d_car_ffps.yaml')), flush=True)


if __name__ == '__main__':
    main()
