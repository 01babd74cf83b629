"""One set-abstraction layer on DENSE rows whose row count the wide chain kernel refuses: 64 feature channels (lda = 68), groups
[64, 64, 128] and [64, 96, 128] with nsample 16, one scene of 64 points, THREE caller-supplied centres (the kernel pairs two
centres of a scene per 32-row tile).  forward_rows must take the per-layer route and equal oracle/model.py's sa_layer bit for
bit.  DET6D_DENSE_ROWS=1 python tests/gpu_scripts/sa_odd_centres.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from de6d_amd.ops import fused
from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as modules
from oracle import model as omodel

assert not modules.COMPACT_ROWS, "run with DET6D_DENSE_ROWS=1"
b, n, m, c, ns = 1, 64, 3, 64, 16
mlps = [[c, 64, 64, 128], [c, 64, 96, 128]]
torch.manual_seed(3)
sa = modules.PointnetSAModuleFSMSG(npoint_list=[m], sample_range_list=[[0, -1]], sample_method_list=['d-fps'], radii=[0.8, 1.6],
                                   nsamples=[ns, ns], mlps=[list(w) for w in mlps])
for mod in sa.modules():
    if isinstance(mod, torch.nn.BatchNorm2d):      # statistics that make the folded layers differ from the plain convolutions
        mod.running_mean.normal_(0.0, 0.1)
        mod.running_var.uniform_(0.5, 1.5)
        mod.weight.data.uniform_(0.5, 1.5)
        mod.bias.data.normal_(0.0, 0.1)
sa = sa.eval().cuda()
rng = np.random.default_rng(3)
xyz = rng.uniform(-1.0, 1.0, (b, n, 3)).astype(np.float32)
feats = rng.normal(size=(b, c, n)).astype(np.float32)
new_xyz = np.ascontiguousarray(xyz[:, [5, 17, 40]] + np.float32(0.01))

f = sa._prepare(torch.device('cuda', torch.cuda.current_device()))
lda = modules.rows_ld(c)
for layers in f['groups']:
    # counted as chained by its widths, refused at this (b, m), accepted at an even m
    assert fused.chain_eligible(lda, layers, ns) and not fused.chain_eligible(lda, layers, ns, b, m) and fused.chain_eligible(lda, layers, ns, b, m + 1)
assert f['expand'] == []
with torch.no_grad():
    got_xyz, got, scores = sa(torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda(), new_xyz=torch.from_numpy(new_xyz).cuda())
sd = {'sa.' + k: v.detach().cpu().numpy() for k, v in sa.state_dict().items()}
spec = dict(npoint_list=[m], sample_range_list=[[0, -1]], sample_method_list=['d-fps'], radii=[0.8, 1.6], nsamples=[ns, ns],
            n_mlp_layers=3, dilated=False, gamma=1.0, agg=0, conf=None)
_, want, _, aux = omodel.sa_layer(sd, 'sa', spec, xyz, feats, new_xyz=new_xyz)
assert all(cnt.min() > 0 for cnt in aux['idx_cnt'])
assert got.shape == want.shape == (b, 256, m) and scores is None
np.testing.assert_array_equal(got.cpu().numpy(), want)
print('sa_odd_centres ok')
