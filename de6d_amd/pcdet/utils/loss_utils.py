"""PointSASALoss of core/pcdet/utils/loss_utils.py:418-547 on the device: the layer-wise foreground / background segmentation
loss that trains the backbone's confidence layers.  Labels, loss and gradient are launches of csrc/ext/sasa_loss.hip
(ops/sasa_loss.py); signatures and return shapes are the reference's.  Nothing reads a result on the host.
The other loss classes of the reference's file live inside csrc/ext/head_loss.hip (ops/head_loss.py) and have no class here."""
import torch.nn as nn

from ..ops_backend import sasa_loss


class PointSASALoss(nn.Module):
    """
    Layer-wise point segmentation loss, used for SASA.
    """

    def __init__(self, func: str = 'BCE', layer_weights: list = None, extra_width: list = None, set_ignore_flag: bool = False):
        super(PointSASALoss, self).__init__()
        self.layer_weights = layer_weights
        if func not in sasa_loss.FUNCS:
            raise NotImplementedError
        assert not set_ignore_flag or (set_ignore_flag and extra_width is not None)
        self.func = func
        self.extra_width = extra_width
        self.set_ignore_flag = set_ignore_flag
        self.spec = sasa_loss.SasaSpec(func, layer_weights, extra_width, set_ignore_flag)

    def _one_layer(self):
        return sasa_loss.SasaSpec(self.func, [1.0], self.extra_width, self.set_ignore_flag)

    def assign_target(self, points, gt_boxes):
        """
        Args:
            points: (N1 + N2 + N3 + ..., 4) [bs_idx, x, y, z], every scene holding the same number of consecutive rows
            gt_boxes: (B, M, 8)
        Returns:
            point_cls_labels: (N1 + N2 + N3 + ...) int64, 0: bg, 1: fg, -1: ignore
        """
        assert len(points.shape) == 2 and points.shape[1] == 4, 'points.shape=%s' % str(points.shape)
        assert len(gt_boxes.shape) == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        points = points.detach().contiguous()
        scores = points.new_zeros((points.shape[0], 1))       # the labels do not depend on them
        return sasa_loss.assign(self._one_layer(), [points], [scores], gt_boxes.detach().contiguous())[0]

    def forward(self, l_points, l_scores, gt_boxes):
        """
        Args:
            l_points: List of points, [(N, 4): bs_idx, x, y, z]
            l_scores: List of points, [(N, 1): predicted point scores]
            gt_boxes: (B, M, 8)
        Returns:
            l_labels: List of labels: [(N,): assigned segmentation labels], None where the layer has no scores or a weight of 0
        """
        coords = [None if self.spec.skipped(i, l_scores) else l_points[i].detach().contiguous() for i in range(len(self.layer_weights))]
        scores = [None if s is None else s.detach().contiguous() for s in l_scores]
        return sasa_loss.assign(self.spec, coords, scores, gt_boxes.detach().contiguous())

    def loss_forward(self, l_scores, l_labels):
        """
        Args:
            l_scores: List of points, [(N, 1): predicted point scores]
            l_labels: List of points, [(N,): assigned segmentation labels]
        Returns:
            l_loss: List of segmentation loss, 0-d device tensors (None for a skipped layer); the gradient reaches l_scores
        """
        n = len(self.layer_weights)
        scores = [None if (i >= len(l_scores) or l_labels[i] is None) else l_scores[i] for i in range(n)]
        if all(self.spec.skipped(i, scores) for i in range(n)):
            return [None] * n
        sums = sasa_loss.SasaLayerLosses.apply(self.spec, l_labels, *scores)
        return [None if self.spec.skipped(i, scores) else sums[4 * i] for i in range(n)]
