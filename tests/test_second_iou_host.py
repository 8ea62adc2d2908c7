"""SECOND-IoU on the host: both configurations build, the RoI head's parameter names are the reference's, the CPU grid pool and
the roi sampler reproduce the reference fixtures (tests/golden/capture_second_head.py), unregistered RoI heads still refuse."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "{}.yaml")
GOLDEN = os.path.join(ROOT, "tests", "golden")

TARGET_CONFIG = dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=32, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                     CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                     HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)


def head_cfg(in_channel=8, dp_ratio=0.0):
    """The small SECONDHead of the fixtures."""
    from toda_amd.pcdet.config import AttrDict

    nms = dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)
    return AttrDict(dict(
        NAME="SECONDHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], IOU_FC=[16, 16], DP_RATIO=dp_ratio,
        NMS_CONFIG=dict(TRAIN=dict(nms, NMS_POST_MAXSIZE=512, NMS_THRESH=0.8), TEST=nms),
        ROI_GRID_POOL=dict(GRID_SIZE=7, IN_CHANNEL=in_channel, DOWNSAMPLE_RATIO=4),
        TARGET_CONFIG=TARGET_CONFIG,
        LOSS_CONFIG=dict(IOU_LOSS="BinaryCrossEntropy", LOSS_WEIGHTS=dict(rcnn_iou_weight=1.0, code_weights=[1.0] * 7))))


def load_cfg(name):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file

    cfg = AttrDict()
    cfg_from_yaml_file(CFG.format(name), cfg)
    return cfg


def build(cfg):
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network

    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    torch.manual_seed(0)
    return build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)


@pytest.mark.parametrize("name,backbone", [("second_iou_kitti", "VoxelBackBone8x"), ("toda_stage1_secondiou_targetmix", "VoxelResBackBone8x")])
def test_second_iou_configs_build_on_the_cpu(name, backbone):
    from toda_amd.pcdet.models.detectors import SECONDNetIoU
    from toda_amd.pcdet.models.roi_heads import SECONDHead

    cfg = load_cfg(name)
    net = build(cfg)
    assert isinstance(net, SECONDNetIoU) and isinstance(net.roi_head, SECONDHead)
    assert type(net.backbone_3d).__name__ == backbone
    assert net.dense_head.predict_boxes_when_training
    assert net.roi_head.num_class == 1                                   # CLASS_AGNOSTIC
    assert net.module_list[-1] is net.roi_head
    sd = net.roi_head.state_dict()
    assert tuple(sd["shared_fc_layer.0.weight"].shape) == (256, 512 * 49, 1)
    assert tuple(sd["iou_layers.7.weight"].shape) == (1, 256, 1) and tuple(sd["iou_layers.7.bias"].shape) == (1,)
    full = net.state_dict()
    assert "roi_head.shared_fc_layer.0.weight" in full and "roi_head.iou_layers.0.weight" in full
    # DP_RATIO 0.3: a Dropout between the two shared layers and after the first IoU layer, as make_fc_layers / shared_fc_list
    assert [type(m).__name__ for m in net.roi_head.shared_fc_layer] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout", "Conv1d", "BatchNorm1d", "ReLU"]
    assert [type(m).__name__ for m in net.roi_head.iou_layers] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout", "Conv1d", "BatchNorm1d", "ReLU", "Conv1d"]


def test_roi_head_keys_and_shapes_equal_the_reference_fixture():
    from toda_amd.pcdet.models.roi_heads import SECONDHead

    g = np.load(os.path.join(GOLDEN, "second_head_head.npz"))
    head = SECONDHead(input_channels=8, model_cfg=head_cfg(), num_class=1)
    sd = head.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for k, v in sd.items():
        assert tuple(v.shape) == g[f"state.{k}"].shape, k


def test_cpu_grid_pool_matches_reference_fixture():
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.roi_heads import SECONDHead

    g = np.load(os.path.join(GOLDEN, "second_head_pool.npz"))
    min_x, min_y, vx, vy, ds, grid = g["geometry"]
    head = SECONDHead(input_channels=16, model_cfg=head_cfg(in_channel=16), num_class=1)
    dcfg = AttrDict(dict(POINT_CLOUD_RANGE=[min_x, min_y, -3.0, 6.0, 5.0, 1.0],
                         DATA_PROCESSOR=[dict(NAME="transform_points_to_voxels", VOXEL_SIZE=[vx, vy, 0.1])]))
    feat = torch.from_numpy(g["feat"]).requires_grad_(True)
    out = head.roi_grid_pool({"batch_size": 2, "rois": torch.from_numpy(g["rois"]), "spatial_features_2d": feat, "dataset_cfg": dcfg})
    assert out.shape == g["out"].shape and not out.requires_grad
    np.testing.assert_allclose(out.numpy(), g["out"], rtol=0, atol=1e-6)
    assert float(out[9 + 2].abs().max()) == 0.0                           # a roi entirely outside the map pools zeros


def test_host_subsampling_reproduces_reference_draws():
    """Given the fixture's max-IoU tables and seeds, the sampler draws the reference's rois (np.random.permutation, torch.randint
    on the CPU generator, in the reference's order)."""
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer

    g = np.load(os.path.join(GOLDEN, "second_head_targets.npz"))
    ptl = ProposalTargetLayer(AttrDict(TARGET_CONFIG))
    seed = int(g["seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    for b in range(g["max_iou"].shape[0]):
        picks = ptl.subsample_rois(torch.from_numpy(g["max_iou"][b]))
        assert picks.dtype == torch.int64
        np.testing.assert_array_equal(picks.numpy(), g["picks"][b])


def test_fg_only_sample_draws_with_np_random_rand():
    """Every roi above the fg threshold: ROI_PER_IMAGE draws floor(U * n_fg) from np.random.rand (the reference's branch, whose
    final concatenation with an empty Python list fails there)."""
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer

    ptl = ProposalTargetLayer(AttrDict(TARGET_CONFIG))
    ious = torch.tensor([0.9, 0.2, 0.8, 0.95, 0.7, 0.99], dtype=torch.float32)
    ious[1] = 0.6                                                         # all six >= 0.55
    np.random.seed(3)
    picks = ptl.subsample_rois(ious)
    np.random.seed(3)
    want = np.floor(np.random.rand(32) * 6).astype(np.int64)
    np.testing.assert_array_equal(picks.numpy(), want)


def test_unregistered_roi_heads_still_refuse():
    cfg = load_cfg("second_iou_kitti")
    cfg.MODEL.ROI_HEAD.NAME = "PVRCNNHead"
    with pytest.raises(NotImplementedError, match="PVRCNNHead"):
        build(cfg)
    cfg = load_cfg("second_iou_kitti")
    cfg.MODEL.PFE = {"NAME": "VoxelSetAbstraction"}
    with pytest.raises(NotImplementedError):
        build(cfg)


def test_cpu_head_forward_matches_reference_eval_fixture():
    """Eval-mode SECONDHead on CPU tensors (given rois: no NMS): the restated pool and the fc layers run as row matmuls give the
    reference's batch_cls_preds."""
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.roi_heads import SECONDHead

    g = np.load(os.path.join(GOLDEN, "second_head_head.npz"))
    head = SECONDHead(input_channels=8, model_cfg=head_cfg(), num_class=1)
    head.load_state_dict({k: torch.from_numpy(g[f"state.{k}"]) for k in head.state_dict()})
    head.eval()
    dcfg = AttrDict(dict(POINT_CLOUD_RANGE=[-4.0, -5.0, -3.0, 6.0, 5.0, 1.0],
                         DATA_PROCESSOR=[dict(NAME="transform_points_to_voxels", VOXEL_SIZE=[0.1, 0.1, 0.1])]))
    bd = {"batch_size": 3, "rois": torch.from_numpy(g["rois"]), "roi_scores": torch.from_numpy(g["roi_scores"]),
          "roi_labels": torch.from_numpy(g["roi_labels"]), "spatial_features_2d": torch.from_numpy(g["feat"]), "dataset_cfg": dcfg}
    with torch.no_grad():
        out = head(bd)
    np.testing.assert_allclose(out["batch_cls_preds"].numpy(), g["eval_cls"], rtol=1e-4, atol=1e-5)
    assert out["batch_box_preds"] is bd["rois"] and out["cls_preds_normalized"] is False
