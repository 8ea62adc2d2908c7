"""VoxelRCNN (reference pcdet/models/detectors/voxel_rcnn.py:4-34): a voxel backbone, a dense-head RPN (AnchorHeadSingle or
CenterHead) and VoxelRCNNHead refining its proposals from the multi-scale sparse features."""
from .detector3d_template import Detector3DTemplate


class VoxelRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {"loss": loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {"loss_rpn": loss_rpn.detach(), **tb_dict}
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_rcnn, tb_dict, {}
