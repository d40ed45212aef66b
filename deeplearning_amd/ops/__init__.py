from ._ext import ext, has_ext, use_hip
from .activations import GELU, SiLU, add_relu, gelu, silu
from .batchnorm import BatchNorm2d, FrozenBatchNorm2d
from .conv1x1 import conv1x1_bn, conv_bn, conv_bn_add_relu
from .boxes import (batched_nms, bbox_iou_aligned, box_area, box_iou,
                    clip_boxes_to_image, generalized_box_iou, nms,
                    remove_small_boxes)
from .drop import DropPath, drop_path
from .dwconv import DepthwiseConv2d, can_use_dwconv, depthwise_conv2d
from .ema import ModelEMA
from .layernorm import LayerNorm, LayerNorm2d, layer_norm
from .losses import (CrossEntropyLoss, cross_entropy, dense_cross_entropy,
                     sigmoid_focal_loss, soft_target_cross_entropy)
from .roi_align import MultiScaleRoIAlign, roi_align
from .stem import bn_relu_maxpool, can_fuse_stem
from .window import (roll_and_window_partition, window_merge_and_roll,
                     window_partition_eager, window_reverse_eager)

__all__ = [
    "ext", "has_ext", "use_hip",
    "gelu", "silu", "add_relu", "GELU", "SiLU",
    "BatchNorm2d", "FrozenBatchNorm2d",
    "conv_bn", "conv1x1_bn", "conv_bn_add_relu",
    "bn_relu_maxpool", "can_fuse_stem",
    "depthwise_conv2d", "can_use_dwconv", "DepthwiseConv2d",
    "box_iou", "generalized_box_iou", "bbox_iou_aligned", "box_area", "nms",
    "batched_nms", "clip_boxes_to_image", "remove_small_boxes",
    "DropPath", "drop_path", "ModelEMA",
    "LayerNorm", "LayerNorm2d", "layer_norm",
    "CrossEntropyLoss", "cross_entropy", "soft_target_cross_entropy",
    "sigmoid_focal_loss", "dense_cross_entropy",
    "MultiScaleRoIAlign", "roi_align",
    "roll_and_window_partition", "window_merge_and_roll",
    "window_partition_eager", "window_reverse_eager",
]
