"""Det6D detector (core/pcdet/models/detectors/det6d.py:4-30): backbone_3d -> point_head ->
post_processing.  forward() is inference only.  get_training_loss(batch_dict) (:24-30) gives the point head's loss for the
batch_dict of an eval forward plus gt_boxes; with towers=True its backward reaches the parameters of the head's three FC stacks,
with head=True every parameter of the head, with sasa=True (and LOSS_SASA_CONFIG) the backbone's confidence layers
(PointHeadBox6DVote.prepare_loss).  The backward of the backbone's SA layers is out of scope."""
from ...ops_backend import fused
from .detector3d_template import Detector3DTemplate


class Det6D(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError('Det6D on HIP is an inference engine: call .eval() (training is out of scope)')
        for module in self.module_list:
            batch_dict = module(batch_dict)
        out = self.post_processing(batch_dict)
        if fused.PENDING_FPS_STATUS:       # eager launches of the cooperative 32768 / 65536-point sampler: did one give up?
            fused.check_fps_status()       # (post_processing has synchronised already)
        return out

    def forward_async(self, batch_dict):
        """enqueue one full pass on the current stream without blocking the host; pair with
        finalize().  Needs the fused post-processing route (class-agnostic nms_gpu, <= 512 boxes)."""
        for module in self.module_list:
            batch_dict = module(batch_dict)
        return self.post_processing_async(batch_dict)

    def get_training_loss(self, batch_dict, requires_grad=False, towers=False, head=False, sasa=False):
        """(loss, tb_dict, disp_dict) of :24-30 for the batch_dict forward() or forward_async() filled, plus
        batch_dict['gt_boxes'] (B, M, 9 + 1).  The reference reads the labels its training forward stored; here
        PointHeadBox6DVote.prepare_loss assigns them first.  loss and the tb_dict values are 0-d device tensors; nothing is
        read on the host.  requires_grad / towers / head: as prepare_loss takes them (towers=True: loss.backward() leaves .grad on
        the parameters of shared_fc_layer, cls_layers and reg_layers; head=True: on those of vote_layers and SA_module.mlps too;
        sasa=True, with LOSS_SASA_CONFIG: on those of the backbone's confidence_mlp stacks, through the SASA loss)."""
        disp_dict = {}
        sa_modules = list(self.backbone_3d.SA_modules)
        self.point_head.num_sa_levels = len(sa_modules)       # LOSS_SASA_CONFIG.layer_weights is checked against it
        self.point_head.prepare_loss(batch_dict, requires_grad=requires_grad, towers=towers, head=head, sasa=sasa,
                                     sa_modules=sa_modules)
        loss_point, tb_dict = self.point_head.get_loss()
        return loss_point, tb_dict, disp_dict
