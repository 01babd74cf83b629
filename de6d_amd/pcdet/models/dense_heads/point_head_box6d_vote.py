"""PointHeadBox6DVote — the ground-aware vote-based 6-DoF point head
(core/pcdet/models/dense_heads/point_head_box6d_vote.py:14-99 constructor, :778-903 forward),
inference branch, on fused HIP ops:

  candidates = first SAMPLE_RANGE points -> vote FC (GEMM) -> clamp + add (kernel) -> SA layer
  around the votes (ball query + fused grouped GEMMs + max-pool) -> shared / cls / reg FCs (GEMMs)
  -> PointBinResidual6DCoder.decode (kernel).

Target assignment (:171-326, :387-407) exists for the argument combinations Det6D's training forward uses
(set_ignore_flag=False; ASSIGN_METHOD: mask with the ball constraint) as one HIP kernel per assignment
(csrc/ext/box_targets.hip): assign_stack_targets_simple / assign_targets_simple (vote targets),
assign_stack_targets_mask / assign_targets (class, box and encoded regression targets) and
assign_training_targets(batch_dict), which labels the output of an eval forward the way the reference's training
forward (:837-844, :872-876) would.  Nothing in it reads a result on the host: it can be captured into a graph.
The training loss (:101-155, :426-776 with loss_utils.py:10-235) is two launches of csrc/ext/head_loss.hip and one more for
its gradient: build_losses, get_vote_layer_loss, generate_centerness_label, get_cls_layer_loss, get_box_layer_loss,
get_corner_loss_lidar and get_loss(tb_dict=None) under the reference's names, all reading self.forward_ret_dict, which
prepare_loss(batch_dict) fills from an eval forward plus gt_boxes the way the reference's training forward would (:823-876).
get_loss returns a 0-d tensor with a graph: loss.backward() reaches point_vote_coords, point_cls_preds and point_reg_preds of
forward_ret_dict (prepare_loss(batch_dict, requires_grad=True) makes them leaves).
Fine-tuning the towers: prepare_loss(batch_dict, requires_grad=True, towers=True) re-evaluates shared_fc_layer, cls_layers and
reg_layers from the pooled vote features through ops.mlp_backward.FoldedChain (the forward kernels and the cached folded
tensors of the eval forward: the same bits), so that loss.backward() leaves .grad on every parameter of the three stacks
(conv.weight, bn.weight, bn.bias, the last conv.bias) and dL/d(pooled features) on forward_ret_dict['point_pooled_features'].
BatchNorm stays frozen (eval mode: the reference's model.eval() plus grad).  With towers=True alone, vote_layers and everything
before the pooled features get NO gradient: the true gradient of the vote coordinates also flows through the SA layer around the
votes (grouped xyz - new_xyz), and a vote-FC gradient from d_vote alone would silently differ from the reference's.
Fine-tuning the whole head: prepare_loss(batch_dict, requires_grad=True, head=True) also re-evaluates vote_layers, the clamp and
the SA layer around the votes (ops.group_backward: VotePoints, GroupedChain; the ball queries re-run on the vote coordinates,
their membership a constant), so that loss.backward() leaves .grad on every parameter of vote_layers, SA_module.mlps and the
three stacks: the vote coordinates collect the loss's own d_vote and the d(new_xyz) of every radius group.  At a vote offset
exactly on its clamp bound the whole gradient passes (torch's max / min backward passes half).
The SASA loss (:146-155, :733-750, :772-775, :878-887 with loss_utils.py:418-547): with LOSS_CONFIG.LOSS_SASA_CONFIG
(func, layer_weights, extra_width, set_ignore_flag) prepare_loss stores point_sasa_preds / point_sasa_labels, and
get_sasa_layer_loss / get_loss add the layer-wise segmentation loss of the backbone's confidence scores (csrc/ext/sasa_loss.hip:
two launches for the labels, two for the loss, one for its gradient).  prepare_loss(batch_dict, requires_grad=True, sasa=True)
re-evaluates every confidence_mlp of the backbone from the rows of its level (constants), so that loss.backward() leaves .grad
on the confidence layers' parameters — the layers that decide which points the head ever sees.  The labels are yaw-only
(the reference passes gt_boxes[..., 0:7]), and an all-zero padding row of gt_boxes enlarged by extra_width is a small box at the
origin, as in the reference.
The gradient with respect to the input points' features and coordinates (the backbone's SA layers), BatchNorm with batch
statistics and a training-mode forward() stay out of scope.
Differences from the reference, all of them kept on purpose:
  * tb_dict values are 0-d device tensors, not Python floats: nothing is read on the host, the call can be captured;
  * labels are constants.  The reference has no detach at :310, so a gradient leaks from the encoded offset labels back into
    the vote coordinates; here the labels come out of assign_training_targets without a graph;
  * the centerness label turns the frame about z by the LAST column of point_box_labels, which for the nine-column labels is
    rx, not rz.  That is the reference's behaviour (:463) and what its checkpoints were trained against;
  * the corner term is added under the foreground mask with a select, so background rows contribute exactly 0 (the reference
    indexes with a boolean mask under `if reg_weights.sum() > 0`, which reads the device); pitch and roll take no part in it
    (the reference passes [:, 0:7]);
  * the layer methods (get_*_layer_loss, generate_centerness_label, get_corner_loss_lidar) return values without a graph;
    the gradient flows through get_loss.
Out of scope, raising NotImplementedError with the key's name: AXIS_ALIGNED_IOU_LOSS_REGULARIZATION, keys of LOSS_SASA_CONFIG
other than func / layer_weights / extra_width / set_ignore_flag,
LOSS_CLS FocalLoss / WeightedCrossEntropy, LOSS_REG WeightedL1Loss, code_weights, pred_velo, coders other than
PointBinResidual6DCoder, use_mean_size.
forward() in training mode, the set_ignore_flag=True variants of the assign_* methods and ASSIGN_METHOD: iou (:328-385) are not
implemented and raise.
Parameters live under the reference's names (vote_layers, SA_module.mlps, shared_fc_layer,
cls_layers, reg_layers) so reference checkpoints load unchanged."""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_batch import pointnet2_modules
from ...ops.pointnet2.pointnet2_batch.pointnet2_modules import fold_sequential, neighbour_search, to_device
from ...ops_backend import fused
from ....ops import box_targets, group_backward, head_loss, mlp_backward, sasa_loss
from ...utils import box_coder_utils, loss_utils


class PointHeadBox6DVote(nn.Module):
    #: the SASA loss: set by build_losses from LOSS_CONFIG.LOSS_SASA_CONFIG
    enable_sasa = False
    loss_point_sasa = None
    #: set by Det6D.get_training_loss: LOSS_SASA_CONFIG.layer_weights is checked against the backbone's SA levels
    num_sa_levels = None

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.input_channels = input_channels
        self.predict_boxes_when_training = predict_boxes_when_training
        target_cfg = model_cfg.TARGET_CONFIG
        self.box_coder = getattr(box_coder_utils, target_cfg.BOX_CODER)(**target_cfg.BOX_CODER_CONFIG)

        self.vote_cfg = model_cfg.VOTE_CONFIG
        self.vote_layers = self.make_fc_layers(input_channels, 3, self.vote_cfg.VOTE_FC)

        self.sa_cfg = model_cfg.SA_CONFIG
        mlps = [[input_channels] + list(spec) for spec in self.sa_cfg.MLPS]
        self.SA_module = pointnet2_modules.PointnetSAModuleFSMSG(
            radii=self.sa_cfg.RADIUS, nsamples=self.sa_cfg.NSAMPLE, mlps=mlps, use_xyz=True,
            bn=model_cfg.USE_BN)
        channel_in = sum(spec[-1] for spec in mlps)

        shared = []
        for width in model_cfg.SHARED_FC:
            shared += [nn.Conv1d(channel_in, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            channel_in = width
        self.shared_fc_layer = nn.Sequential(*shared)
        loss_cls = model_cfg.get('LOSS_CONFIG', {}).get('LOSS_CLS', None)
        cls_out = num_class + 1 if loss_cls == 'CrossEntropy' else num_class
        self.cls_layers = self.make_fc_layers(channel_in, cls_out, model_cfg.CLS_FC)
        self.reg_layers = self.make_fc_layers(channel_in, self.box_coder.code_size, model_cfg.REG_FC)
        self.init_weights()
        self.forward_ret_dict = None
        self._folded = None
        self._extra_width = None
        self._loss_spec = None

    @staticmethod
    def make_fc_layers(input_channels, output_channels, fc_list):
        layers, pre = [], input_channels
        for width in fc_list:
            layers += [nn.Conv1d(pre, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            pre = width
        layers.append(nn.Conv1d(pre, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    def init_weights(self):
        # xavier-normal like the reference (point_head_box6d_vote.py:80-99)
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def invalidate(self):
        self._folded = None

    def _prepare(self, device):
        if self._folded is not None and self._folded['device'] == device:
            return self._folded
        if self.training:
            raise RuntimeError("the HIP head folds BatchNorm: call .eval() first")
        ld = fused.rows_ld(self.input_channels)
        sa_width = sum(seq[-3].out_channels for seq in self.SA_module.mlps)
        shared = to_device(fold_sequential(self.shared_fc_layer, fused.round4(sa_width)), device)
        k = fused.round4(shared[-1][2])
        self._folded = dict(
            device=device,
            vote=to_device(fold_sequential(self.vote_layers, ld, k_offset=3), device),
            shared=shared,
            cls=to_device(fold_sequential(self.cls_layers, k), device),
            reg=to_device(fold_sequential(self.reg_layers, k), device))
        return self._folded

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("PointHeadBox6DVote on HIP implements the inference branch only")
        batch_size = batch_dict['batch_size']
        stash = batch_dict.get('_det6d_rows', None)
        if stash is not None:
            xyz, rows = stash
        else:  # rebuild the rows layout from the public keys
            coords = batch_dict['point_coords']
            feats = batch_dict['point_features']
            n = coords.shape[0] // batch_size
            xyz = coords[:, 1:4].reshape(batch_size, n, 3).contiguous()
            rows = torch.zeros((batch_size, n, fused.rows_ld(feats.shape[-1])), dtype=torch.float32, device=feats.device)
            rows[:, :, :3] = xyz
            rows[:, :, 3:3 + feats.shape[-1]] = feats.reshape(batch_size, n, -1)
        f = self._prepare(rows.device)
        b, n, ld = rows.shape
        lo, hi = self.model_cfg.SAMPLE_RANGE
        cand_rows = rows[:, lo:hi, :].contiguous()
        p = cand_rows.shape[1]

        # vote offsets -> clamp -> vote points (point_head_box6d_vote.py:815-821)
        off = torch.empty((b * p, fused.round4(f['vote'][-1][2])), dtype=torch.float32, device=rows.device)
        # the chain starts at weight row 3 (rows 0..2: coordinates, zero)
        spec = fused.rows_chain(f['vote'], self.input_channels, off, wrow0=3)
        if fused.mlp_rows_eligible(self.input_channels, [spec]):    # vote FC stack in one launch (csrc/mlp_rows.hip)
            fused.mlp_rows(cand_rows.view(b * p, ld), 3, [spec])
        else:
            off = fused.run_chain(cand_rows, f['vote'])                   # (B*P, 4), cols 0..2 valid
        vote_xyz = torch.empty((b, p, 3), dtype=torch.float32, device=rows.device)
        off_clamped = torch.empty((b * p, 3), dtype=torch.float32, device=rows.device)
        fused.vote_points(off, cand_rows, self.vote_cfg.MAX_TRANSLATION_RANGE, vote_xyz, off_clamped)

        # SA layer around the votes, then the FC towers
        _, pooled, _ = self.SA_module.forward_rows(xyz, rows, new_xyz=vote_xyz)
        shared = fused.run_chain(pooled.view(b * p, -1), f['shared'])
        ncls, ncode = f['cls'][-1][2], f['reg'][-1][2]
        point_cls_preds = torch.empty((b * p, ncls), dtype=torch.float32, device=rows.device)
        kshared = f['shared'][-1][2]
        point_reg_preds = torch.empty((b * p, ncode), dtype=torch.float32, device=rows.device)
        towers = [fused.rows_chain(f['cls'], kshared, point_cls_preds), fused.rows_chain(f['reg'], kshared, point_reg_preds)]
        if shared.shape[1] == kshared and fused.mlp_rows_eligible(kshared, towers):
            fused.mlp_rows(shared, 0, towers)                       # cls and reg towers: two chains, one launch (csrc/mlp_rows.hip)
        else:
            fused.run_chain(shared, f['cls'], out=point_cls_preds)        # the last layer writes the unpadded (B*P, ncls) logits
            reg = fused.run_chain(shared, f['reg'])
            point_reg_preds = reg[:, :ncode].contiguous() if reg.shape[1] != ncode else reg

        vote_flat = vote_xyz.view(b * p, 3)
        boxes = self.box_coder.decode_torch(point_reg_preds, vote_flat)

        cand4 = fused.with_batch_index(cand_rows, 3)
        batch_dict['batch_index'] = cand4[:, 0]
        batch_dict['point_candidate_coords'] = cand4
        batch_dict['point_vote_coords'] = fused.with_batch_index(vote_xyz, 3)
        batch_dict['vote_offsets'] = off_clamped.view(b, p, 3).permute(0, 2, 1)   # (B, 3, P) view, no copy
        batch_dict['point_cls_scores'] = fused.sigmoid_pow(point_cls_preds, 1.0)
        batch_dict['point_box_preds'] = boxes
        batch_dict['batch_cls_preds'] = point_cls_preds
        batch_dict['batch_box_preds'] = boxes
        batch_dict['cls_preds_normalized'] = False
        batch_dict['point_reg_preds'] = point_reg_preds
        self.forward_ret_dict = {'batch_size': batch_size, 'point_cls_preds': point_cls_preds,
                                 'point_reg_preds': point_reg_preds, 'point_box_preds': boxes,
                                 'point_pooled_features': pooled,        # a reference: prepare_loss(towers=True) starts here
                                 'xyz': xyz, 'rows': rows, 'cand_rows': cand_rows}       # references: prepare_loss(head=True)
        return batch_dict

    # ---- target assignment (point_head_box6d_vote.py:171-326, :387-407) ------------------------------------------------
    @staticmethod
    def _check_targets_input(points, gt_boxes):
        assert len(points.shape) == 2 and points.shape[1] == 4, 'points.shape=%s' % str(points.shape)
        assert len(gt_boxes.shape) == 3 and gt_boxes.shape[2] >= 9, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        return points.contiguous(), gt_boxes.contiguous()

    def _extra_width_tensor(self, extra_width, device):
        """the 3 floats of VOTE_EXTRA_WIDTH on the device, uploaded once (an upload cannot be captured into a graph)"""
        if extra_width is None or torch.is_tensor(extra_width):
            return extra_width
        key = (tuple(float(v) for v in extra_width), device)
        if self._extra_width is None or self._extra_width[0] != key:
            self._extra_width = (key, torch.tensor(key[0], dtype=torch.float32, device=device))
        return self._extra_width[1]

    def _assign_simple(self, points, gt_boxes, extra_width):
        points, gt_boxes = self._check_targets_input(points, gt_boxes)
        _, cls_labels, reg_labels = box_targets.assign_targets9(
            points, gt_boxes, extra_width=self._extra_width_tensor(extra_width, points.device), n_cols=3)
        return {'point_cls_labels': cls_labels, 'point_reg_labels': reg_labels}

    def assign_stack_targets_simple(self, points, gt_boxes, extend_gt_boxes=None, set_ignore_flag=True):
        """vote targets (:171-226).  points (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 9 + 1) ->
        point_cls_labels (N,) int64: 1 inside a box, else 0; point_reg_labels (N, 3): the centre of that box, else 0"""
        if set_ignore_flag or extend_gt_boxes is not None:
            raise NotImplementedError("assign_stack_targets_simple: set_ignore_flag=True / extend_gt_boxes is not used by "
                                      "Det6D's training forward and is not implemented")
        return self._assign_simple(points, gt_boxes, None)

    def assign_targets_simple(self, points, gt_boxes, extra_width=None, set_ignore_flag=True):
        """:228-253: assign_stack_targets_simple on the boxes enlarged by extra_width (box_utils.enlarge_box3d; the kernel adds
        it to dx, dy, dz itself)"""
        if set_ignore_flag:
            raise NotImplementedError("assign_targets_simple: set_ignore_flag=True is not used by Det6D's training forward "
                                      "and is not implemented")
        return self._assign_simple(points, gt_boxes, extra_width)

    def assign_stack_targets_mask(self, points, gt_boxes, extend_gt_boxes=None, set_ignore_flag=True,
                                  use_ball_constraint=False, central_radius=2.0):
        """:255-326 with set_ignore_flag=False, use_ball_constraint=True.  A point inside a box and closer than
        central_radius to its centre is foreground; inside but not closer: label -1.  -> point_cls_labels (N,) int64,
        point_reg_labels (N, code_size) = box_coder.encode_torch(box, point), point_box_labels (N, C - 1) = the box
        without its class column; both zero for every point that is not foreground."""
        assert set_ignore_flag != use_ball_constraint, 'Choose one only!'
        if set_ignore_flag:
            # the reference calls the yaw-only roiaware_pool3d op with 9-wide boxes here (:289): it cannot have run
            raise NotImplementedError("assign_stack_targets_mask: set_ignore_flag=True (yaw-only roiaware_pool3d boxes) is "
                                      "not implemented")
        if not central_radius > 0:
            raise ValueError("assign_stack_targets_mask: central_radius = %r must be positive" % (central_radius,))
        points, gt_boxes = self._check_targets_input(points, gt_boxes)
        assert gt_boxes.shape[2] >= 10, 'gt_boxes.shape=%s (the last column is the class)' % str(gt_boxes.shape)
        ncol = gt_boxes.shape[2] - 1
        box_idx, cls_labels, box_labels = box_targets.assign_targets9(
            points, gt_boxes, class_col=ncol, num_class=self.num_class, central_radius=central_radius, n_cols=ncol)
        fg = ((box_idx >= 0) & (cls_labels != -1)).unsqueeze(-1)
        # encode EVERY row and mask: the reference's boolean indexing would read the number of foreground points on the host.
        # encode_torch clamps the sizes of its argument in place; like the reference (:310-318) the box labels keep that clamp.
        code = self.box_coder.encode_torch(box_labels, points[:, 1:4])[..., :self.box_coder.code_size]
        zero = code.new_zeros(())
        return {'point_cls_labels': cls_labels,
                'point_reg_labels': torch.where(fg, code, zero),
                'point_box_labels': torch.where(fg, box_labels, zero)}

    def assign_targets(self, input_dict):
        """:387-407: the targets of the vote points, by TARGET_CONFIG.ASSIGN_METHOD (only 'mask')"""
        target_cfg = self.model_cfg.TARGET_CONFIG
        if target_cfg.get('ASSIGN_METHOD', None) is None:
            raise KeyError("TARGET_CONFIG.ASSIGN_METHOD is not set (the target assignment needs it: 'mask')")
        if target_cfg.ASSIGN_METHOD != 'mask':
            raise NotImplementedError("TARGET_CONFIG.ASSIGN_METHOD: %s is not implemented (only 'mask')" % target_cfg.ASSIGN_METHOD)
        points = input_dict['point_vote_coords']
        gt_boxes = input_dict['gt_boxes']
        assert points.shape.__len__() == 2, 'points.shape=%s' % str(points.shape)
        assert gt_boxes.shape.__len__() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        return self.assign_stack_targets_mask(points=points, gt_boxes=gt_boxes, set_ignore_flag=False, use_ball_constraint=True,
                                              central_radius=target_cfg.get('GT_CENTRAL_RADIUS', 2.0))

    def assign_training_targets(self, batch_dict):
        """The labels the reference's training forward puts into forward_ret_dict (:837-844, :872-876), for the batch_dict an
        eval forward returned plus batch_dict['gt_boxes'] (B, M, 9 + 1): vote_cls_labels / vote_reg_labels of the candidate
        points, point_cls_labels / point_reg_labels / point_box_labels of the vote points."""
        extra_width = self.model_cfg.TARGET_CONFIG.get('VOTE_EXTRA_WIDTH', None)
        vote = self.assign_targets_simple(points=batch_dict['point_candidate_coords'], gt_boxes=batch_dict['gt_boxes'],
                                          extra_width=extra_width, set_ignore_flag=False)
        point = self.assign_targets(batch_dict)
        return {'vote_cls_labels': vote['point_cls_labels'], 'vote_reg_labels': vote['point_reg_labels'],
                'point_cls_labels': point['point_cls_labels'], 'point_reg_labels': point['point_reg_labels'],
                'point_box_labels': point['point_box_labels']}

    # ---- training loss (point_head_box6d_vote.py:101-155, :426-776) ----------------------------------------------------
    def build_losses(self, losses_cfg):
        """validates LOSS_CONFIG and keeps its scalars as the host array the kernels read; what is out of scope raises
        NotImplementedError naming the key"""
        if losses_cfg is None:
            raise KeyError("LOSS_CONFIG is not set")
        coder = self.box_coder
        if not isinstance(coder, box_coder_utils.PointBinResidual6DCoder):
            raise NotImplementedError("TARGET_CONFIG.BOX_CODER: %s (the loss is implemented for PointBinResidual6DCoder)"
                                      % type(coder).__name__)
        if getattr(coder, 'use_mean_size', False):
            raise NotImplementedError("BOX_CODER_CONFIG.use_mean_size is not supported")
        if getattr(coder, 'pred_velo', False):
            raise NotImplementedError("BOX_CODER_CONFIG.pred_velo is not supported")
        loss_cls = losses_cfg.get('LOSS_CLS', None)
        if loss_cls not in ('WeightedBinaryCrossEntropyLoss', 'WeightedBinaryCrossEntropyLossWithCenterness'):
            raise NotImplementedError("LOSS_CLS: %s is not implemented (WeightedBinaryCrossEntropyLoss[WithCenterness])" % loss_cls)
        if losses_cfg.get('LOSS_REG', None) != 'WeightedSmoothL1Loss':
            raise NotImplementedError("LOSS_REG: %s is not implemented (WeightedSmoothL1Loss)" % losses_cfg.get('LOSS_REG', None))
        loss_point_sasa = self._build_sasa_loss(losses_cfg.get('LOSS_SASA_CONFIG', None))
        if losses_cfg.get('AXIS_ALIGNED_IOU_LOSS_REGULARIZATION', False):
            raise NotImplementedError("AXIS_ALIGNED_IOU_LOSS_REGULARIZATION is not implemented")
        weights = losses_cfg.get('LOSS_WEIGHTS', None) or {}
        if weights.get('code_weights', None) is not None:
            raise NotImplementedError("LOSS_WEIGHTS.code_weights is not implemented")
        corner = bool(losses_cfg.get('CORNER_LOSS_REGULARIZATION', False))
        needed = [k for k in head_loss.WEIGHT_KEYS if k != 'point_corner_weight' or corner]
        if not coder.ground_aware:
            needed.remove('point_pitch_cls_weight')
        missing = [k for k in needed if k not in weights]
        if missing:
            raise KeyError("LOSS_CONFIG.LOSS_WEIGHTS lacks %s" % ', '.join(missing))
        reg_cfg = dict(losses_cfg.get('LOSS_REG_CONFIG', None) or {})
        unknown = sorted(set(reg_cfg) - {'beta'})
        if unknown:
            raise NotImplementedError("LOSS_REG_CONFIG: %s is not implemented (beta)" % ', '.join(unknown))
        cls_cfg = losses_cfg.get('LOSS_CLS_CONFIG', None)
        centerness = 'WithCenterness' in loss_cls
        self._loss_spec = head_loss.LossSpec(
            self.num_class, coder.angle_bin_num, ground_aware=coder.ground_aware, centerness=centerness, corner=corner,
            weights={k: weights[k] for k in head_loss.WEIGHT_KEYS if k in weights}, beta=reg_cfg.get('beta', 1.0 / 9.0),
            centerness_min=cls_cfg['centerness_min'] if cls_cfg is not None else 0.0,
            centerness_max=cls_cfg['centerness_max'] if cls_cfg is not None else 1.0)
        self.enable_sasa = loss_point_sasa is not None
        self.__dict__['loss_point_sasa'] = loss_point_sasa     # it has no parameters: kept out of the registered submodules
        return self._loss_spec

    SASA_KEYS = ('func', 'layer_weights', 'extra_width', 'set_ignore_flag')

    def _build_sasa_loss(self, sasa_cfg):
        """LOSS_SASA_CONFIG (:146-155) -> loss_utils.PointSASALoss or None"""
        if sasa_cfg is None:
            return None
        unknown = sorted(set(sasa_cfg) - set(self.SASA_KEYS))
        if unknown:
            raise NotImplementedError("LOSS_SASA_CONFIG: %s is not implemented (%s)" % (', '.join(unknown), ', '.join(self.SASA_KEYS)))
        if sasa_cfg.get('layer_weights', None) is None:
            raise KeyError("LOSS_SASA_CONFIG lacks layer_weights")
        weights = list(sasa_cfg['layer_weights'])
        if self.num_sa_levels is not None and len(weights) > self.num_sa_levels:
            raise ValueError("LOSS_SASA_CONFIG.layer_weights lists %d layers, the backbone has %d" % (len(weights), self.num_sa_levels))
        extra_width = sasa_cfg.get('extra_width', None)
        return loss_utils.PointSASALoss(func=sasa_cfg.get('func', 'BCE'), layer_weights=weights,
                                        extra_width=None if extra_width is None else list(extra_width),
                                        set_ignore_flag=bool(sasa_cfg.get('set_ignore_flag', False)))

    def _loss_inputs(self):
        if self._loss_spec is None:
            self.build_losses(self.model_cfg.get('LOSS_CONFIG', None))
        ret = self.forward_ret_dict
        if ret is None or 'point_cls_labels' not in ret:
            raise RuntimeError("the loss reads forward_ret_dict: call prepare_loss(batch_dict) after an eval forward")
        return self._loss_spec, (ret['point_vote_coords'], ret['vote_reg_labels'], ret['vote_cls_labels'],
                                 ret['point_cls_preds'].view(-1, self.num_class), ret['point_cls_labels'].view(-1),
                                 ret['point_reg_preds'], ret['point_reg_labels'], ret['point_box_labels'])

    def _loss_forward(self):
        spec, tensors = self._loss_inputs()
        return head_loss.forward(spec, *(t.detach().contiguous() for t in tensors), per_point=True)

    def prepare_loss(self, batch_dict, requires_grad=False, towers=False, head=False, sasa=False, sa_modules=None):
        """Fills forward_ret_dict with what the reference's training forward puts there (:823-876), for the batch_dict an eval
        forward returned plus batch_dict['gt_boxes'] (B, M, 9 + 1): the five labels of assign_training_targets,
        point_candidate_coords and point_vote_coords as (N, 3), beside the predictions forward() left.
        requires_grad=True makes point_vote_coords, point_cls_preds and point_reg_preds leaves, so that get_loss()[0].backward()
        leaves dL/d(prediction) in their .grad.
        towers=True re-evaluates shared_fc_layer, cls_layers and reg_layers from point_pooled_features (made a leaf) with a graph
        to their parameters and stores those predictions — the bits of the eval forward — in place of the leaves: backward()
        then leaves .grad on every parameter of the three stacks and on point_pooled_features; point_vote_coords stays a
        leaf, vote_layers and the backbone get nothing (see the module docstring).
        head=True implies the towers' graph and re-evaluates what lies before it as well, from the references forward() kept
        (xyz, rows, cand_rows): vote_layers, the clamp, the ball queries around the votes (constants) and SA_module.mlps.
        point_vote_coords is then the (N, 3) view of the re-evaluated votes, a non-leaf in which the loss's d_vote and the SA
        layer's d(new_xyz) add up, and point_pooled_features the re-evaluated tensor — all of them the bits of the eval
        forward.  backward() leaves .grad on every parameter of the head; the backbone gets nothing.
        With LOSS_SASA_CONFIG, point_sasa_preds (the backbone's point_scores_list; leaves with requires_grad=True) and
        point_sasa_labels (:878-887) are stored as well.  sasa=True (with sa_modules = the backbone's SA_modules, which
        Det6D.get_training_loss passes) re-evaluates every weighted level's confidence_mlp from that level's rows — a constant:
        nothing flows into the aggregated features — with a graph to its parameters and stores those scores, the bits of the
        eval forward, instead: backward() then leaves .grad on every parameter of those confidence_mlp stacks and on nothing
        else of the backbone.  The rows are not kept by the inference forward (it is left exactly as it is): the SA layers up
        to the last weighted level run again, without a graph, at the centres the forward sampled (forward_rows with new_xyz:
        the forward's own kernels, the same bits) and the rows are stored as point_sasa_rows.  Combines freely with towers /
        head."""
        ret = self.forward_ret_dict
        if ret is None or 'point_reg_preds' not in ret:
            raise RuntimeError("prepare_loss needs the forward_ret_dict of an eval forward")
        towers = towers or head
        if (towers or sasa) and self.training:
            raise RuntimeError("the HIP head folds BatchNorm: call .eval() first")
        if self._loss_spec is None:
            self.build_losses(self.model_cfg.get('LOSS_CONFIG', None))
        if sasa and not self.enable_sasa:
            raise RuntimeError("prepare_loss(sasa=True) needs LOSS_CONFIG.LOSS_SASA_CONFIG")
        if head:
            for key in ('xyz', 'rows', 'cand_rows'):
                if key not in ret:
                    raise RuntimeError("prepare_loss(head=True) needs forward_ret_dict['%s'] of an eval forward" % key)
        ret.update(self.assign_training_targets(batch_dict))
        ret['point_candidate_coords'] = batch_dict['point_candidate_coords'][:, 1:4].contiguous()
        ret['point_vote_coords'] = batch_dict['point_vote_coords'][:, 1:4].contiguous()
        for key in ('point_vote_coords', 'point_cls_preds', 'point_reg_preds'):
            ret[key] = ret[key].detach().requires_grad_(requires_grad)
        if head:
            # Let go of the previous step's graph BEFORE the new one is built: the pooled tensor of an earlier head=True call is
            # a non-leaf, and while it lives the AccumulateGrad nodes of vote_layers and SA_module.mlps live too and are reused
            # — with the stream of the step that created them.  A step captured on another stream would then make autograd
            # synchronise the capture stream with that stream: a fork onto the default stream inside the capture.
            ret['point_pooled_features'] = ret['point_pooled_features'].detach()
            with torch.set_grad_enabled(requires_grad):
                vote, pooled = self._reevaluate_votes(ret)
            ret['point_vote_coords'] = vote.view(-1, 3)
            ret['point_pooled_features'] = pooled
        if towers:
            pooled = ret['point_pooled_features']
            if not head:
                pooled = pooled.detach().requires_grad_(requires_grad)
                ret['point_pooled_features'] = pooled
            f = self._prepare(pooled.device)
            k0 = sum(seq[-3].out_channels for seq in self.SA_module.mlps)
            with torch.set_grad_enabled(requires_grad):
                chains = [mlp_backward.folded_params(seq, f[key]) for seq, key in
                          ((self.shared_fc_layer, 'shared'), (self.cls_layers, 'cls'), (self.reg_layers, 'reg'))]
                cls, reg = mlp_backward.folded_chain(pooled.view(-1, pooled.shape[-1]), chains[0], chains[1:], k0=k0)
            ret['point_cls_preds'], ret['point_reg_preds'] = cls, reg
        if self.enable_sasa:
            ret.pop('point_sasa_preds', None)      # let go of the previous step's graph before the new one is built (see head=True)
            ret.update(self._prepare_sasa(batch_dict, requires_grad, sasa, sa_modules))
        return ret

    def _prepare_sasa(self, batch_dict, requires_grad, reevaluate, sa_modules):
        """point_sasa_preds and point_sasa_labels of forward_ret_dict (:878-887)"""
        scores = list(batch_dict['point_scores_list'])
        spec = self.loss_point_sasa.spec
        n = len(spec.layer_weights)
        if n > len(scores):
            raise ValueError("LOSS_SASA_CONFIG.layer_weights lists %d layers, the backbone has %d" % (n, len(scores)))
        out = {}
        if reevaluate:
            if sa_modules is None:
                raise RuntimeError("prepare_loss(sasa=True) needs sa_modules, the backbone's SA_modules (Det6D.get_training_loss "
                                   "passes them)")
            live = [i for i in range(n) if not spec.skipped(i, scores)]
            level_rows = self._level_rows(batch_dict, sa_modules, max(live) + 1 if live else 0)
            for i in live:
                sa, rows = sa_modules[i], level_rows[i]
                b, m, ld = rows.shape
                with torch.set_grad_enabled(requires_grad):
                    chain = mlp_backward.folded_params(sa.confidence_mlp, sa._prepare(rows.device)['conf'], k_offset=3)
                    scores[i], = mlp_backward.folded_chain(rows.view(b * m, ld), chain)
            out['point_sasa_rows'] = level_rows + [None] * (len(scores) - len(level_rows))
        else:
            scores = [None if s is None else s.detach().requires_grad_(requires_grad) for s in scores]
        labels = self.loss_point_sasa(batch_dict['point_coords_list'], scores, batch_dict['gt_boxes'])
        out.update({'point_sasa_preds': scores, 'point_sasa_labels': labels})
        return out

    @staticmethod
    @torch.no_grad()
    def _level_rows(batch_dict, sa_modules, levels):
        """the rows [xyz | aggregated features | pad] (B, M, ld) of the first `levels` SA levels, as the eval forward computed
        them: the points packed again and every SA layer run again at the centres the forward sampled"""
        if levels == 0:
            return []
        b = batch_dict['batch_size']
        points = batch_dict['points'].contiguous()
        ld = pointnet2_modules.rows_ld(points.shape[1] - 4)
        rows, xyz = fused.pack_points(points, ld)
        rows, xyz = rows.view(b, -1, ld), xyz.view(b, -1, 3)
        coords = batch_dict['point_coords_list']
        out = []
        for i, sa in enumerate(list(sa_modules)[:levels]):
            if sa.training:
                raise RuntimeError("the HIP set-abstraction path folds BatchNorm: call .eval() first")
            if sa.aggregation_mlp is None:
                raise NotImplementedError("prepare_loss(sasa=True): an SA level without an aggregation MLP has no rows to re-evaluate")
            centres = coords[i][:, 1:4].reshape(b, -1, 3).contiguous()
            xyz, rows, _ = sa.forward_rows(xyz, rows, new_xyz=centres)
            out.append(rows)
        return out

    def get_sasa_layer_loss(self, tb_dict=None):
        """:733-750 -> (point_loss_sasa or None, tb_dict): two launches on the labels prepare_loss stored, and one more when the
        loss's backward() runs; (None, None) without LOSS_SASA_CONFIG or when every layer is skipped.
        tb_dict['point_loss_sasa_layer_%d'] and tb_dict['point_loss_sasa'] are 0-d device tensors"""
        if self._loss_spec is None:
            self.build_losses(self.model_cfg.get('LOSS_CONFIG', None))
        if not self.enable_sasa:
            return None, None
        ret = self.forward_ret_dict
        if ret is None or 'point_sasa_labels' not in ret:
            raise RuntimeError("the loss reads forward_ret_dict: call prepare_loss(batch_dict) after an eval forward")
        spec = self.loss_point_sasa.spec
        preds, labels = ret['point_sasa_preds'], ret['point_sasa_labels']
        if all(spec.skipped(i, preds) for i in range(len(spec.layer_weights))):
            return None, None
        loss, sums = sasa_loss.SasaLoss.apply(spec, None, None, labels, *preds)
        tb_dict = {} if tb_dict is None else tb_dict
        for i in range(len(spec.layer_weights)):
            if labels[i] is not None:
                tb_dict['point_loss_sasa_layer_%d' % i] = sums[4 * i]
        tb_dict['point_loss_sasa'] = sums[-1]
        return loss, tb_dict

    def _reevaluate_votes(self, ret):
        """vote_layers -> clamp -> ball queries -> SA_module.mlps -> max-pool, dense and layer by layer, with a graph to the
        parameters -> (vote (B, P, 3), pooled (B, P, round4(sum C))): the bits forward() computed on its fused routes"""
        sa = self.SA_module
        if sa.dilated_radius_group or sa.pool_method != 'max_pool' or sa.skip_connection:
            raise NotImplementedError("prepare_loss(head=True): dilated groups, pooling other than max_pool and skip connections "
                                      "have no backward")
        xyz, rows, cand_rows = ret['xyz'], ret['rows'], ret['cand_rows']
        f, f_sa = self._prepare(rows.device), sa._prepare(rows.device)
        b, p, ld = cand_rows.shape
        # the whole candidate rows enter the first layer: the folded weight's three coordinate rows are zero (their dW reaches
        # no parameter) — run_chain(cand_rows, f['vote']) of forward()
        vote_chain = mlp_backward.folded_params(self.vote_layers, f['vote'], k_offset=3)
        off, = mlp_backward.folded_chain(cand_rows.view(b * p, ld), vote_chain)
        vote = group_backward.VotePoints.apply(off, cand_rows, tuple(self.vote_cfg.MAX_TRANSLATION_RANGE))
        centres = vote.detach()
        found, _ = neighbour_search(xyz, centres, sa._shells(), False, want_lists=False)       # dense padded lists
        groups = [mlp_backward.folded_params(seq, layers) for seq, layers in zip(sa.mlps, f_sa['groups'])]
        pooled = group_backward.grouped_chain(rows, vote, found, groups, f_sa['pooled_width'])
        return vote, pooled.view(b, p, -1)

    def get_vote_layer_loss(self, tb_dict=None):
        """:426-446 -> (vote_loss_reg, tb_dict); tb_dict['vote_loss_reg'] is a 0-d device tensor"""
        sums, _ = self._loss_forward()
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'vote_loss_reg': sums[head_loss.VOTE]})
        return sums[head_loss.VOTE], tb_dict

    @torch.no_grad()
    def generate_centerness_label(self, point_base, point_box_labels, pos_mask, epsilon=1e-6):
        """:448-482.  The frame is turned about z by the last column of point_box_labels, as in the reference."""
        if epsilon != 1e-6:
            raise NotImplementedError("generate_centerness_label: epsilon = %r (the kernel clamps at 1e-6)" % (epsilon,))
        return head_loss.centerness_labels(point_base.contiguous(), point_box_labels.contiguous(), pos_mask.contiguous())

    def get_corner_loss_lidar(self, pred_boxes, gt_boxes):
        """:515-540 for (N, 7) boxes -> (N,)"""
        assert pred_boxes.shape[0] == gt_boxes.shape[0]
        if pred_boxes.shape[1] != 7 or gt_boxes.shape[1] != 7:
            raise NotImplementedError("get_corner_loss_lidar takes (N, 7) boxes: pitch and roll take no part in the corner loss")
        return head_loss.corner_loss(pred_boxes.detach().contiguous(), gt_boxes.detach().contiguous())

    def get_cls_layer_loss(self, tb_dict=None):
        """:542-576 -> (point_loss_cls (N,), cls_weights (N,), tb_dict); tb_dict['point_pos_num'] is a 0-d device tensor"""
        sums, (loss_cls, _, _) = self._loss_forward()
        labels = self.forward_ret_dict['point_cls_labels'].view(-1)
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_pos_num': sums[head_loss.N_POS]})
        return loss_cls, (labels >= 0).float(), tb_dict

    def get_box_layer_loss(self, tb_dict=None):
        """:578-731 -> (point_loss_box (N,), reg_weights (N,), tb_dict)"""
        _, (_, loss_box, _) = self._loss_forward()
        labels = self.forward_ret_dict['point_cls_labels'].view(-1)
        return loss_box, (labels > 0).float(), ({} if tb_dict is None else tb_dict)

    def get_loss(self, tb_dict=None):
        """:752-776 -> (point_loss, tb_dict): two launches, and one more when point_loss.backward() runs.  tb_dict holds 0-d
        device tensors under the reference's keys."""
        spec, t = self._loss_inputs()
        loss, sums = head_loss.HeadLoss.apply(spec, t[0], t[3], t[5], t[1], t[2], t[4], t[6], t[7])
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_loss_vote': sums[head_loss.VOTE], 'point_loss_cls': sums[head_loss.CLS],
                        'point_loss_box': sums[head_loss.BOX], 'vote_loss_reg': sums[head_loss.VOTE],
                        'point_pos_num': sums[head_loss.N_POS]})
        loss_sasa, tb_sasa = self.get_sasa_layer_loss()
        if loss_sasa is not None:
            tb_dict.update(tb_sasa)
            loss = loss + loss_sasa
        return loss, tb_dict
