"""csu -- MI355X-native CSWin-(SimAM-)UNet training path.

Drop-in for the model/training API of TrungMasterChef/CSWin-SimAM-UNet
(train_cswinunet_segmentation.py, train_unet_segmentation.py): same class/function names,
constructor arguments and state_dict keys; compute runs in hand-written gfx950 kernels
(libcsu_hip.so, C ABI in include/csu.h).  Import with ``cswin-simam-unet_amd`` on sys.path.
"""
from .model import (CARAFE, CARAFE4, CSWinBlock, CSWinTransformer, DropPath, LePEAttention, Merge_Block, Mlp,
                    img2windows, windows2img)
from .simam import SimAM, simam
from .unet import DoubleConv, Down, UNet, Up
from .train import (bce_loss, dice_coefficient, evaluate_model, iou_score, make_optimizer, make_scheduler,
                    train_model, train_step)
from .losses import (BoundarySegLoss, MultiClassSegLoss, SegLoss, bce_dice_loss, boundary_loss, ce_dice_boundary_loss,
                     ce_dice_loss, ce_loss, dice_loss, linear_ramp, multiclass_dice_loss, tversky_loss,
                     HardExampleSegLoss, dice_focal_loss, dice_topk_loss, focal_loss, topk_ce_loss,
                     LovaszSegLoss, ce_lovasz_loss, lovasz_softmax_loss, reference_lovasz_softmax)
from .optim import FusedAdam, FusedAdamW
from .ema import WeightEMA
from .infer import (SlidingWindowPredictor, evaluate_full_res, plan_axis, plan_tiles, reference_predict, window_1d)
from .metrics import (SurfaceMetrics, distance_transform_edt, reference_distance_transform_edt,
                      reference_surface_metrics, surface_metrics)
from .boundary import reference_signed_distance_map, signed_distance_map
from .components import (PostProcess, connected_components, postprocess_labels, reference_connected_components,
                         reference_postprocess_labels)
from .augment import SpatialAugment, reference_augment
from .patches import PatchLoader, PatchPool, PatchSampler, reference_patch_sample
from . import rng
from .rng import manual_seed

__all__ = ["UNet", "DoubleConv", "Down", "Up", "CARAFE", "CARAFE4", "CSWinBlock", "CSWinTransformer", "DropPath", "LePEAttention", "Merge_Block", "Mlp",
           "img2windows", "windows2img", "SimAM", "simam", "bce_loss", "dice_coefficient", "evaluate_model",
           "iou_score", "make_optimizer", "make_scheduler", "train_model", "train_step", "FusedAdamW", "FusedAdam",
           "rng", "manual_seed", "SegLoss", "dice_loss", "bce_dice_loss", "tversky_loss",
           "MultiClassSegLoss", "ce_loss", "ce_dice_loss", "multiclass_dice_loss", "WeightEMA",
           "SlidingWindowPredictor", "reference_predict", "evaluate_full_res", "plan_axis", "plan_tiles", "window_1d",
           "SurfaceMetrics", "surface_metrics", "reference_surface_metrics", "distance_transform_edt",
           "reference_distance_transform_edt", "connected_components", "postprocess_labels", "PostProcess",
           "reference_connected_components", "reference_postprocess_labels", "SpatialAugment", "reference_augment",
           "BoundarySegLoss", "boundary_loss", "ce_dice_boundary_loss", "linear_ramp", "signed_distance_map",
           "reference_signed_distance_map", "HardExampleSegLoss", "focal_loss", "dice_focal_loss", "topk_ce_loss",
           "dice_topk_loss", "PatchPool", "PatchSampler", "PatchLoader", "reference_patch_sample",
           "LovaszSegLoss", "lovasz_softmax_loss", "ce_lovasz_loss", "reference_lovasz_softmax"]
