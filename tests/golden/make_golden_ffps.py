"""Regenerates tests/golden/ffps_ref.npz: the reference's f-fps picks on a few scenes.

Distances are the reference's calc_dist_matrix_for_sampling (pointnet2_utils.py:37-44: torch.cdist(xyz, xyz) +
torch.cdist(f, f) * gamma) on CPU torch; picks are the reference's matrix sampler (sampling_gpu.cu:268-373) applied to that
matrix (tests/models/ffps.py: select).  The engine fixes its own GEMM order for cdist (tests/models/ffps.py), so the two
agree by evidence, not bit for bit: a scene keeps only its first rounds, those whose runner-up margins all exceed twice
the largest difference between the model's distances and torch's.  Inputs: xyz in the KITTI range, ReLU-like features.

    python tests/golden/make_golden_ffps.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.models import ffps  # noqa: E402

F32 = np.float32
#: (n, C, m, gamma, keep the matrix)
SCENES = [(256, 32, 96, 1.0, True), (1024, 32, 128, 1.0, False), (512, 64, 128, 0.5, False)]


def scene(rng, n, c):
    xyz = np.stack([rng.uniform(0, 70.4, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n)], 1).astype(F32)
    feats = np.maximum(rng.standard_normal((n, c)), 0).astype(F32)
    return xyz, feats


def torch_matrix(xyz, feats, gamma):
    x, f = torch.from_numpy(xyz)[None], torch.from_numpy(feats)[None]
    dist = torch.cdist(x, x)
    dist += torch.cdist(f, f) * gamma
    return dist[0].numpy()


def main():
    out = {}
    seed = 100
    for si, (n, c, m, gamma, keep_matrix) in enumerate(SCENES):
        seed += 1
        rng = np.random.default_rng(seed)
        xyz, feats = scene(rng, n, c)
        mat = torch_matrix(xyz, feats, gamma)
        margins = []
        picks = ffps.select(n, m, lambda i: mat[i], margins=margins)
        dist = ffps.Distances(xyz, feats, gamma)
        diff = max(float(np.abs(dist.row(int(i)) - mat[int(i)]).max()) for i in picks[:-1])
        # the first rounds whose runner-up margins all exceed twice the distance difference: picks that cdist's summation
        # order cannot change
        ok = np.asarray(margins) > 2 * diff
        m = int(np.argmin(ok)) + 1 if not ok.all() else m
        picks, margins = picks[:m], margins[:m - 1]
        print("scene %d: n=%d C=%d m=%d seed=%d min margin %.3g, model-vs-torch %.3g" % (si, n, c, m, seed, min(margins), diff))
        out['xyz%d' % si], out['feats%d' % si] = xyz, feats
        out['picks%d' % si] = picks
        out['meta%d' % si] = np.array([n, c, m], np.int32)
        out['gamma%d' % si] = np.array(gamma, F32)
        out['margin%d' % si] = np.array(margins, F32)
        if keep_matrix:
            out['matrix%d' % si] = mat
    np.savez_compressed(os.path.join(HERE, 'ffps_ref.npz'), nscenes=np.array(len(SCENES)), **out)


if __name__ == '__main__':
    main()
