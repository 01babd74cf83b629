"""Set-abstraction / feature-propagation modules of
core/pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py (PointnetSAModuleFSMSG :497-607 with
the forward of _PointnetSAModuleFSBase :358-494, PointnetFPModule :124-174), re-designed around
the fused HIP ops.

The nn.Conv/BatchNorm children exist only to own parameters under the reference's state-dict
names (`mlps.0.0.weight`, `aggregation_mlp.1.running_var`, ...): they are never called.  At first
use the BN statistics are folded into (K, N) weight matrices + shift vectors that live on the
device, and the whole layer runs as: FPS -> row gather -> ball query -> [gather + 3x(GEMM, shift,
ReLU) + mask + max-pool] per radius group -> aggregation GEMM -> confidence GEMMs.

Internal layout ("rows"): one row per point, `[x, y, z, f_0 .. f_{C-1}, 0-pad]`, row stride a
multiple of 4 floats.  A neighbour gather is then one contiguous row read, and `xyz - centre`
touches only the first three columns.  `forward()` keeps the reference's channel-major
signature by converting at the boundary; `forward_rows()` is the fast path the backbone uses.
"""
from typing import List

import numpy as np
import os

import torch
import torch.nn as nn

from ....ops_backend import ffps, fused, pointnet2_batch_hip as pn2, sort_samplers
from . import pointnet2_utils

round4, rows_ld, run_chain = fused.round4, fused.rows_ld, fused.run_chain     # (their importers find them here too)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def fold_layer(conv, bn, k_rows, k_offset=0):
    """Fold Conv(k=1) [+ BatchNorm(eval)] into W (k_rows, round4(Cout)) and shift (Cout,), fp32.

    y = BN(conv(x)) = x @ (W_conv * s)^T + (beta - mean * s),  s = gamma / sqrt(var + eps);
    rows [k_offset, k_offset + Cin) of W hold the folded weights, every other row is zero
    (xyz columns a layer does not consume, and the row padding).
    """
    w = _np(conv.weight).reshape(conv.weight.shape[0], -1)  # (Cout, Cin)
    cout, cin = w.shape
    if bn is not None:
        scale = _np(bn.weight) / np.sqrt(_np(bn.running_var) + np.float32(bn.eps))
        shift = _np(bn.bias) - _np(bn.running_mean) * scale
        w = w * scale[:, None]
        if conv.bias is not None:
            shift = shift + _np(conv.bias) * scale
    else:
        shift = _np(conv.bias) if conv.bias is not None else np.zeros(cout, np.float32)
    mat = np.zeros((k_rows, round4(cout)), np.float32)
    mat[k_offset:k_offset + cin, :cout] = w.T
    return mat, shift.astype(np.float32), cout


def fold_sequential(seq, k_rows, k_offset=0):
    """[(W, shift, cout, act)] for a Sequential of Conv(/BN/ReLU) blocks; later layers take the
    previous layer's padded width as their K."""
    layers, mods, i = [], list(seq), 0
    while i < len(mods):
        conv = mods[i]
        assert isinstance(conv, (nn.Conv1d, nn.Conv2d))
        bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], (nn.BatchNorm1d, nn.BatchNorm2d)) else None
        j = i + (2 if bn is not None else 1)
        act = 1 if j < len(mods) and isinstance(mods[j], nn.ReLU) else 0
        if act:
            j += 1
        mat, shift, cout = fold_layer(conv, bn, k_rows, k_offset)
        layers.append((mat, shift, cout, act))
        k_rows, k_offset = round4(cout), 0
        i = j
    return layers


def to_device(layers, device):
    return [(torch.from_numpy(m).to(device), torch.from_numpy(s).to(device), c, a) for m, s, c, a in layers]


#: The samplers of a layer run one after the other on the caller's stream.  Forking them onto side streams
#: (DET6D_FORKED_SAMPLERS=1) shortens one pass by ~0.45 ms but costs throughput with many passes in flight
#: (4121 vs 4300 scenes/s at 15 passes: more sampler workgroups resident at once, fork/join in every graph).
SEQUENTIAL_SAMPLERS = fused.L.experiment_switch('DET6D_FORKED_SAMPLERS') is None

#: Grouped MLPs run on compact (ragged) row lists: a ball with cnt < nsample hits is padded by the reference with
#: repetitions of its first cnt hits, so only the first 2^ceil(log2 cnt) slots of a centre are evaluated — the
#: pooled features are identical bit for bit (csrc/compact.hip).  DET6D_DENSE_ROWS=1 restores the reference's
#: dense (B, m, nsample) row space.
COMPACT_ROWS = os.environ.get('DET6D_DENSE_ROWS') is None

#: First layer of a grouped MLP from per-point partial sums (csrc/expand.hip): one plain GEMM over the N points of the
#: layer + 3 FMAs per grouped output instead of a (3 + C)-deep GEMM over every (centre, neighbour) row; identical bits
#: (the chain order of gathered rows puts the relative coordinates last).  DET6D_NO_EXPAND=1: the gathered GEMM instead.
EXPAND_FIRST_LAYER = fused.L.experiment_switch('DET6D_NO_EXPAND') is None


def compact_rows(nsample):
    """does a radius group of this nsample run on a compact row list?"""
    return COMPACT_ROWS and nsample in (4, 8, 16, 32)


def group_route(lda, layers, nsample, compact, expand, b=0, m=0):
    """Which launches evaluate a radius group: the name of one of six routes.

      compact_chain / dense_chain    the whole group in one chain kernel (fused.mlp_chain3_compact / mlp_chain3)
      compact_group / dense_group    first layer from the per-point partial sums, in one group kernel (fused.mlp_group3)
      compact_layers / dense_layers  one launch per layer (group_layers)

    lda: row stride of the point rows; layers: the group's folded chain; compact: compact_rows(nsample); expand: the group
    is in the layer's expand set (its partial sums exist); b, m: scenes and centres per scene.  The library decides what its
    kernels take (fused.chain_compact_eligible, chain_eligible, group_kernel_eligible); compact lists are not asked about
    (b, m).  b = m = 0 asks by the widths alone: that is _prepare's question, which has to settle the expand set before m is
    known.  The consequence: a group chained by its widths is not in the expand set, so where the library refuses its chain
    at this (b, m) — odd m with nsample 16, b * m * nsample off the 32-row tiles — it cannot take the group kernel either
    and runs per layer, its first layer the gathered det6d_linear."""
    if compact:
        if fused.chain_compact_eligible(lda, layers):
            return 'compact_chain'
        return 'compact_group' if expand and fused.group_kernel_eligible(layers, nsample, True) else 'compact_layers'
    if fused.chain_eligible(lda, layers, nsample, b, m):
        return 'dense_chain'
    return 'dense_group' if expand and fused.group_kernel_eligible(layers, nsample, False, b, m) else 'dense_layers'


def neighbour_search(xyz, centres, shells, dilated, want_lists):
    """The ball queries of a layer: shells = [(radius_in, radius_out, nsample)] -> (found = [(cnt (B, m), idx (B, m, ns))]
    per shell, counted).  Two shells go in one launch; with want_lists through the query that also counts the parts of the
    compact lists where the shape qualifies (fused.ball_query_pair_lists): counted are then the two CompactRows for
    fused.compact_groups_pair to place, otherwise None.  Any other number of shells: one query each."""
    if len(shells) == 2:
        fast = fused.ball_query_pair_lists(xyz, centres, shells[0], shells[1]) if want_lists else None
        if fast is not None:
            return [fast[0:2], fast[2:4]], fast[4:]
        ca, ia, cb, ib = fused.ball_query_pair(xyz, centres, shells[0], shells[1])
        return [(ca, ia), (cb, ib)], None
    (b, n, _), m, found = xyz.shape, centres.shape[1], []
    for rin, rout, nsample in shells:
        idx_cnt = torch.zeros((b, m), dtype=torch.int32, device=xyz.device)
        idx = torch.zeros((b, m, nsample), dtype=torch.int32, device=xyz.device)
        if dilated:
            pn2.ball_query_dilated_wrapper(b, n, m, rin, rout, nsample, centres, xyz, idx_cnt, idx)
        else:
            pn2.ball_query_cnt_wrapper(b, n, m, rout, nsample, centres, xyz, idx_cnt, idx)
        found.append((idx_cnt, idx))
    return found, None


def single_list(idx_cnt, idx, n, pooled, col, width):
    """the compact list of one group that the pair builder did not make.  Parts of a centre are combined by an atomic max, so
    the group's slice of `pooled` is cleared first: by the builder itself where the columns allow, by a fill before it else"""
    if fused.COMPACT_SPLIT and (col | width | pooled.shape[1]) % 4 == 0:
        return fused.compact_groups(idx_cnt, idx, n, zero=(pooled, col, width))
    if fused.COMPACT_SPLIT:
        pooled[:, col:col + width].zero_()
    return fused.compact_groups(idx_cnt, idx, n)


def group_layers(rows, ctr, space, idx_cnt, layers, pooled, col, partial=None):
    """A radius group with one launch per layer.  space: the group's row space, the dense idx (B, m, ns) or a CompactRows;
    partial = (P, first column): the first layer from the per-point partial sums (fused.group_expand) instead of the gathered
    GEMM.  The last layer pools into pooled[:, col:] in its epilogue (compact lists by class; dense rows for nsample 8, 16,
    32); for any other nsample it is written out, and mask + max run in their own launch."""
    compact = isinstance(space, fused.CompactRows)
    where = dict(compact=space) if compact else dict(idx=space)
    nsample = space.ns if compact else space.shape[2]
    pool = -1 if compact else nsample if nsample in (8, 16, 32) else 0
    first, later = dict(where, ctr=ctr, gather=compact), (where if compact else {})     # the gathered layer, the plain ones
    x = None
    for li, folded in enumerate(layers):
        kw = first if li == 0 else later
        if li == len(layers) - 1 and pool:
            return fused.layer(rows if li == 0 else x, folded, pooled, col0=col, cnt=idx_cnt, pool=pool, **kw)
        if li == 0 and partial is not None:
            w, shift, cout, act = folded
            x = fused.group_expand(partial[0], partial[1], w, shift, act, cout, rows, ctr, **where)
        else:
            x = fused.layer(rows if li == 0 else x, folded, **kw)
    fused.group_maxpool(x, nsample, layers[-1][2], idx_cnt, pooled, col)


class _PointnetSAModuleFSBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.groupers = None
        self.mlps = None
        self.npoint_list = []
        self.sample_range_list = [[0, -1]]
        self.sample_method_list = ['d-fps']
        self.radii = []
        self.pool_method = 'max_pool'
        self.dilated_radius_group = False
        self.weight_gamma = 1.0
        self.skip_connection = False
        self.aggregation_mlp = None
        self.confidence_mlp = None
        self._folded = None
        self._side_streams = None

    # ---- weight preparation -------------------------------------------------------------
    def invalidate(self):
        self._folded = None

    def _prepare(self, device):
        if self._folded is not None and self._folded['device'] == device:
            return self._folded
        if self.training:
            raise RuntimeError("the HIP set-abstraction path folds BatchNorm: call .eval() first")
        in_ld = rows_ld(self.in_channels)
        groups = [to_device(fold_sequential(seq, in_ld), device) for seq in self.mlps]
        pooled_width = sum(g[-1][2] for g in groups)
        out_channels = pooled_width
        agg = conf = None
        if self.aggregation_mlp is not None:
            agg = to_device(fold_sequential(self.aggregation_mlp, round4(pooled_width)), device)
            out_channels = agg[-1][2]
        if self.confidence_mlp is not None:
            conf = to_device(fold_sequential(self.confidence_mlp, rows_ld(out_channels), k_offset=3), device)
        # groups whose first layer runs as "per-point GEMM + expand" (not the ones a fused chain kernel takes whole)
        expand, pcols, col = [], {}, 0
        for gi, (layers, ns) in enumerate(zip(groups, self.nsamples)):
            chained = group_route(in_ld, layers, ns, compact_rows(ns), False).endswith('_chain')      # by its widths
            if EXPAND_FIRST_LAYER and not chained and len(layers) >= 2 and layers[0][2] % 4 == 0 and in_ld > 4:
                expand.append(gi)
                pcols[gi] = col
                col += layers[0][0].shape[1]
        p_w = None
        if expand:
            p_w = torch.cat([groups[gi][0][0] for gi in expand], dim=1).clone()
            p_w[:3] = 0           # the coordinate rows enter in the expand step; P is the chain over the feature columns
        self._folded = dict(device=device, groups=groups, pooled_width=pooled_width, agg=agg, conf=conf,
                            out_channels=out_channels, expand=expand, pcols=pcols, p_w=p_w)
        return self._folded

    # ---- sampling -----------------------------------------------------------------------
    def _sample_one(self, xyz, scores, lo, hi, method, npoint, idx_out, offset, rows=None):
        """one sampler -> idx_out[:, offset:offset+npoint]; slice, sigmoid**gamma weights, 1e10 init and
        the + lo offset (pointnet2_modules.py:380,415-424,448) all happen inside det6d_fps_fused (d-fps, s-fps) or
        det6d_ext_fps_features (f-fps: cdist(xyz) + cdist(features) * gamma over the layer's rows,
        pointnet2_modules.py:382-387) or det6d_ext_topk_scores (c-fps: the npoint highest weights in descending order, ties
        by ascending index, pointnet2_modules.py:425-430).  df-fps (pointnet2_modules.py:389-414) is two launches:
        det6d_ext_pillar_weights (counted per scene), then the weighted FPS on the slice."""
        hi = xyz.shape[1] if hi == -1 else hi
        if method == 'd-fps':
            fused.fps_fused(xyz, lo, hi, npoint, None, 1.0, idx_out, offset)
        elif method == 's-fps':
            assert scores is not None
            fused.fps_fused(xyz, lo, hi, npoint, scores, self.weight_gamma, idx_out, offset)
        elif method == 'f-fps':
            assert rows is not None, "f-fps samples on the layer's rows [xyz | features]"
            ffps.fps_features(rows, self.in_channels, npoint, self.weight_gamma, lo, hi, idx_out, offset)
        elif method == 'c-fps':
            assert scores is not None
            sort_samplers.topk_scores(scores, npoint, self.weight_gamma, lo, hi, idx_out, offset)
        elif method == 'df-fps':
            sort_samplers.pillar_density_fps(xyz, npoint, lo, hi, idx_out, offset)
        else:
            raise NotImplementedError(
                "sampling method %r is outside the Det6D hot path (SURVEY.md 2.1 #8)" % method)

    def _sample(self, xyz, scores, rows=None):
        """fusion sampling (pointnet2_modules.py:376-450).  The samplers of one layer are independent
        latency chains on one workgroup per scene, so they run concurrently on forked HIP streams
        (also under hipGraph capture, where the fork/join becomes two parallel branches)."""
        jobs = list(zip(self.sample_range_list, self.sample_method_list, self.npoint_list))
        b = xyz.shape[0]
        ctl = fused.SAMPLER_SEGMENTS                                  # capture controller of a pass (runtime.py), or None
        # the controller counts EVERY layer (its index buffers and hoisted samplers are keyed by layer number) ...
        layer = ctl.next_layer() if ctl is not None else -1
        if ctl is not None and not (len(jobs) == 1 or SEQUENTIAL_SAMPLERS):
            # ... but it cannot serve a layer whose samplers run on forked streams (DET6D_FORKED_SAMPLERS=1): its hoisted
            # picks would be recomputed into a private buffer and the group's buffers ignored
            raise RuntimeError("DET6D_FORKED_SAMPLERS=1 cannot be combined with captured passes (GraphedDet6D / Det6DGroup "
                               "hoist the input-only samplers): unset it, or run the model eagerly")
        idx = ctl.index_buffer(layer, b, sum(self.npoint_list)) if ctl is not None else None
        if idx is not None:
            assert tuple(idx.shape) == (b, sum(self.npoint_list)), "index buffer of layer %d has the wrong shape" % layer
        if idx is None:
            idx = torch.empty((b, sum(self.npoint_list)), dtype=torch.int32, device=xyz.device)
        offsets = [sum(self.npoint_list[:i]) for i in range(len(jobs))]
        if len(jobs) == 1 or SEQUENTIAL_SAMPLERS:
            for j, (((lo, hi), method, npoint), off) in enumerate(zip(jobs, offsets)):
                if ctl is not None and ctl.hoisted(layer, j):
                    continue          # launched by the group for all its passes, ahead of this segment (runtime.hoist_plan)
                self._sample_one(xyz, scores, lo, hi, method, npoint, idx, off, rows)
            if ctl is not None:
                ctl.after_samplers(layer, xyz, idx)    # single-graph passes: fork / join of the input-only sampler chain
            return idx
        main = torch.cuda.current_stream()
        if self._side_streams is None or len(self._side_streams) < len(jobs) - 1:
            self._side_streams = [torch.cuda.Stream() for _ in range(len(jobs) - 1)]
        for i, ((lo, hi), method, npoint) in enumerate(jobs[1:], start=1):
            side = self._side_streams[i - 1]
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self._sample_one(xyz, scores, lo, hi, method, npoint, idx, offsets[i], rows)
        (lo, hi), method, npoint = jobs[0]
        self._sample_one(xyz, scores, lo, hi, method, npoint, idx, 0, rows)
        for side in self._side_streams[:len(jobs) - 1]:
            main.wait_stream(side)
        return idx

    # ---- fast path ----------------------------------------------------------------------
    def forward_rows(self, xyz, rows, scores=None, new_xyz=None):
        """
        xyz (B,N,3), rows (B,N,ld) [xyz | features | pad]  ->
        new_xyz (B,M,3), new_rows (B,M,ld') [xyz | new features | pad] or pooled (B,M,sumC) when
        there is no aggregation MLP, new_scores (B,M) or None
        """
        if self.pool_method != 'max_pool' or self.skip_connection:
            raise NotImplementedError("only max_pool without skip connection is on the Det6D path")
        f = self._prepare(rows.device)
        b, n, lda = rows.shape
        new_xyz, new_rows = self._centres(f, xyz, rows, scores, new_xyz)
        m = new_xyz.shape[1]
        pooled = fused.pooled_buffer(b * m, f['pooled_width'], rows.device)
        widths = [layers[-1][2] for layers in f['groups']]
        # both lists of a two-group layer come from one builder when every column offset is a multiple of 4
        paired = COMPACT_ROWS and len(widths) == 2 and (widths[0] | widths[1] | pooled.shape[1]) % 4 == 0
        found, counted = neighbour_search(xyz, new_xyz, self._shells(), self.dilated_radius_group, want_lists=paired)
        lists = [None] * len(found)
        if paired and fused.COMPACT_SPLIT and all(ns in (4, 8, 16, 32) for ns in self.nsamples):
            # (their slices of `pooled` are cleared by the builder)
            lists = fused.compact_groups_pair(found, n, pooled, [(0, widths[0]), (widths[0], widths[1])], counted=counted)
        p_all = None
        if f['expand']:   # per-point partial sums of the first layers of all expand groups: one plain GEMM over the points
            p_all = torch.empty((b * n, f['p_w'].shape[1]), dtype=torch.float32, device=rows.device)
            fused.linear(rows.view(b * n, lda), f['p_w'], None, 0, p_all)
        col = 0
        for gi, ((idx_cnt, idx), nsample, layers, cr) in enumerate(zip(found, self.nsamples, f['groups'], lists)):
            compact, expand = compact_rows(nsample), gi in f['expand']
            route = group_route(lda, layers, nsample, compact, expand, b, m)
            if compact and cr is None:
                cr = single_list(idx_cnt, idx, n, pooled, col, widths[gi])
            if route == 'compact_chain':
                fused.mlp_chain3_compact(rows, cr, new_xyz, layers, pooled, col)
            elif route == 'dense_chain':
                fused.mlp_chain3(rows, idx, new_xyz, idx_cnt, layers, pooled, col)
            elif route == 'compact_group':
                fused.mlp_group3(p_all, f['pcols'][gi], layers, rows, new_xyz, pooled, col, compact=cr)
            elif route == 'dense_group':
                fused.mlp_group3(p_all, f['pcols'][gi], layers, rows, new_xyz, pooled, col, idx=idx, cnt=idx_cnt)
            else:
                group_layers(rows, new_xyz, cr if compact else idx, idx_cnt, layers, pooled, col,
                             partial=(p_all, f['pcols'][gi]) if expand else None)
            col += widths[gi]
        if f['agg'] is None:
            return new_xyz, pooled.view(b, m, -1), None
        if new_rows is None:  # centres supplied by the caller
            new_rows = torch.zeros((b, m, rows_ld(f['out_channels'])), dtype=torch.float32, device=rows.device)
            new_rows[:, :, :3] = new_xyz
        return new_xyz, new_rows, self._aggregate(f, pooled, new_rows)

    def _shells(self):
        """[(radius_in, radius_out, nsample)] of the groups: shells [former radius, radius) when dilated, else plain balls"""
        inner = [0.0] + list(self.radii[:-1]) if self.dilated_radius_group else [0.0] * len(self.radii)
        return list(zip(inner, self.radii, self.nsamples))

    def _centres(self, f, xyz, rows, scores, new_xyz):
        """sample (unless the caller supplies the centres) -> (new_xyz, next level's rows with the centres in or None)"""
        if new_xyz is not None:
            return new_xyz, None
        sample_idx = self._sample(xyz, scores, rows)
        if f['agg'] is None:
            return fused.gather_centres(xyz, sample_idx), None
        # next level's rows: xyz now, features by the aggregation GEMM, pad zeroed
        new_rows = torch.empty((xyz.shape[0], sample_idx.shape[1], rows_ld(f['out_channels'])), dtype=torch.float32, device=rows.device)
        return fused.gather_centres(xyz, sample_idx, new_rows, 3 + f['out_channels']), new_rows

    def _aggregate(self, f, pooled, new_rows):
        """aggregation MLP: pooled -> the feature columns of new_rows; confidence MLP on top of them -> scores (B, M) or None"""
        b, m, _ = new_rows.shape
        rows2d = new_rows.view(b * m, -1)
        conf = f['conf']
        scores = torch.empty((b * m, 1), dtype=torch.float32, device=pooled.device) if conf is not None and conf[-1][2] == 1 else None
        if scores is not None and len(f['agg']) == 1:
            # aggregation + confidence chain in ONE launch (csrc/mlp_rows.hip): the aggregated features go to the next
            # level's rows AND stay in LDS as the input of the confidence layers (whose first three weight rows, the
            # coordinates', are zero: the chain starts at weight row 3)
            spec = (fused.rows_chain(f['agg'], f['pooled_width'], rows2d, ocol0=3)
                    + fused.rows_chain(conf, f['agg'][0][2], scores, wrow0=3))
            if fused.mlp_rows_eligible(f['pooled_width'], [spec]):
                fused.mlp_rows(pooled, 0, [spec])
                return scores.view(b, m)
        run_chain(pooled, f['agg'], out=new_rows, col0=3)
        if conf is None:
            return None
        if scores is not None:   # the last layer writes the (B*M, 1) score column itself
            return run_chain(new_rows, conf, out=scores).view(b, m)
        return run_chain(new_rows, conf)[:, 0].reshape(b, m).contiguous()

    # ---- reference-shaped signature -----------------------------------------------------
    def forward(self, xyz, features=None, new_xyz=None, scores=None):
        """(B,N,3), (B,C,N) -> new_xyz (B,M,3), new_features (B,C',M), new_scores (B,M) | None"""
        b, n, _ = xyz.shape
        c = 0 if features is None else features.shape[1]
        assert c == self.in_channels, "feature channels %d != %d" % (c, self.in_channels)
        rows = torch.zeros((b, n, rows_ld(c)), dtype=torch.float32, device=xyz.device)
        rows[:, :, :3] = xyz
        if c:
            rows[:, :, 3:3 + c] = features.transpose(1, 2)
        f = self._prepare(rows.device)
        new_xyz, out, new_scores = self.forward_rows(xyz.contiguous(), rows, scores, new_xyz)
        if f['agg'] is not None:
            new_features = out[:, :, 3:3 + f['out_channels']]
        else:
            new_features = out[:, :, :f['pooled_width']]
        return new_xyz, new_features.transpose(1, 2).contiguous(), new_scores


class PointnetSAModuleFSMSG(_PointnetSAModuleFSBase):
    """Set abstraction with fusion sampling and multi-scale grouping (keyword signature of the
    reference, pointnet2_modules.py:500-514)."""

    def __init__(self, *, npoint_list: List[int] = None, sample_range_list: List[List[int]] = None,
                 sample_method_list: List[str] = None, radii: List[float], nsamples: List[int],
                 mlps: List[List[int]], bn: bool = True, use_xyz: bool = True, pool_method='max_pool',
                 dilated_radius_group: bool = False, skip_connection: bool = False, weight_gamma: float = 1.0,
                 aggregation_mlp: List[int] = None, confidence_mlp: List[int] = None):
        super().__init__()
        assert npoint_list is None or len(npoint_list) == len(sample_range_list) == len(sample_method_list)
        assert len(radii) == len(nsamples) == len(mlps)
        if not use_xyz:
            raise NotImplementedError("use_xyz=False is not on the Det6D path")
        self.npoint_list = npoint_list
        self.sample_range_list = sample_range_list
        self.sample_method_list = sample_method_list
        self.radii = list(radii)
        self.nsamples = list(nsamples)
        self.pool_method = pool_method
        self.dilated_radius_group = dilated_radius_group
        self.skip_connection = skip_connection
        self.weight_gamma = weight_gamma
        self.in_channels = mlps[0][0]

        self.groupers = nn.ModuleList()  # parameter-free; kept for structural parity
        self.mlps = nn.ModuleList()
        former_radius, out_channels = 0.0, 0
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            if dilated_radius_group:
                self.groupers.append(pointnet2_utils.QueryAndGroupDilated(former_radius, radius, nsample, use_xyz=True))
            else:
                self.groupers.append(pointnet2_utils.QueryWithCntAndGroup(radius, nsample, use_xyz=True))
            former_radius = radius
            widths = [spec[0] + 3] + list(spec[1:])
            block = []
            for cin, cout in zip(widths[:-1], widths[1:]):
                block += [nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU()]
            self.mlps.append(nn.Sequential(*block))
            out_channels += widths[-1]
        if skip_connection:
            out_channels += self.in_channels

        def conv1d_stack(cin, widths):
            block = []
            for cout in widths:
                block += [nn.Conv1d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm1d(cout), nn.ReLU()]
                cin = cout
            return block, cin

        if aggregation_mlp is not None:
            block, out_channels = conv1d_stack(out_channels, aggregation_mlp)
            self.aggregation_mlp = nn.Sequential(*block)
        if confidence_mlp is not None:
            block, last = conv1d_stack(out_channels, confidence_mlp)
            block.append(nn.Conv1d(last, 1, kernel_size=1, bias=True))
            self.confidence_mlp = nn.Sequential(*block)


class PointnetFPModule(nn.Module):
    """Feature propagation: three_nn + inverse-distance three_interpolate + shared MLP
    (pointnet2_modules.py:124-174)."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super().__init__()
        block = []
        for cin, cout in zip(mlp[:-1], mlp[1:]):
            block += [nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU()]
        self.mlp = nn.Sequential(*block)
        self._folded = None

    def invalidate(self):
        self._folded = None

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3), unknow_feats (B,C1,n) | None, known_feats (B,C2,m) -> (B,C',n)"""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight.contiguous())
        else:
            interpolated = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        feats = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        b, c, n = feats.shape
        if self.training:
            raise RuntimeError("the HIP feature-propagation path folds BatchNorm: call .eval() first")
        if self._folded is None or self._folded[0] != feats.device:
            self._folded = (feats.device, to_device(fold_sequential(self.mlp, round4(c)), feats.device))
        x = torch.zeros((b * n, round4(c)), dtype=torch.float32, device=feats.device)
        x[:, :c] = feats.transpose(1, 2).reshape(b * n, c)
        y = run_chain(x, self._folded[1])
        cout = self._folded[1][-1][2]
        return y[:, :cout].reshape(b, n, cout).transpose(1, 2).contiguous()
