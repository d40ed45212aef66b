"""Fused ResNet stem tail: train-mode BatchNorm2d(relu=True) followed by a
3x3 / stride 2 / padding 1 max-pool, as one apply+pool kernel forward and two
gather kernels backward (csrc/batchnorm.hip).

The BN output (the largest activation of the network) is never written, no
int64 pooling indices exist, and backward needs no full-size pooling
gradient: saved are the raw conv output, one uint8 window slot per pooled
element and the per-channel vectors. The pooled output is bit-identical to
F.max_pool2d(BatchNorm2d(relu=True)(x), 3, 2, 1).

Reference parity: the conv1 -> bn1 -> relu -> maxpool stem of
classification/resnet/models/networks.py (ResNet:127).
"""
from __future__ import annotations

import os

import torch
from torch import nn

from ._ext import ext, use_hip


class _BNReluMaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps):
        pooled, slots, mean, rstd, scale, shift = ext().bn_relu_maxpool_fwd(
            x, weight, bias, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(x, slots, weight, mean, rstd, scale, shift)
        return pooled

    @staticmethod
    def backward(ctx, dpool):
        x, slots, weight, mean, rstd, scale, shift = ctx.saved_tensors
        dx, dw, db = ext().bn_relu_maxpool_bwd(dpool, x, slots, weight, mean,
                                               rstd, scale, shift)
        return dx, dw, db, None, None, None, None


def _fused_stem_disabled() -> bool:
    return os.environ.get("DLA_NO_FUSED_STEM", "0") == "1"  # A/B runs


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def can_fuse_stem(x: torch.Tensor, bn, pool) -> bool:
    """True when pool(bn(x)) can run as the fused BN+ReLU+max-pool: GPU,
    train mode, channels_last bf16/fp16/fp32 with C a multiple of the
    16-byte vector, ops.BatchNorm2d(relu=True), and exactly
    MaxPool2d(3, stride=2, padding=1)."""
    from .batchnorm import BatchNorm2d

    if _fused_stem_disabled() or not use_hip(x):
        return False
    if type(bn) is not BatchNorm2d or not bn.relu or not bn.training:
        return False
    if type(pool) is not nn.MaxPool2d or pool.ceil_mode or \
            pool.return_indices:
        return False
    if (_pair(pool.kernel_size), _pair(pool.stride), _pair(pool.padding),
            _pair(pool.dilation)) != ((3, 3), (2, 2), (1, 1), (1, 1)):
        return False
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        return False
    if x.dim() != 4 or x.numel() == 0 or \
            x.shape[1] % (16 // x.element_size()) != 0:
        return False
    if x.shape[0] * x.shape[2] * x.shape[3] >= 2 ** 31:
        return False
    # channels_last proper: a tensor that is also NCHW-contiguous takes the
    # plain route, as BatchNorm2d itself would treat it as NCHW
    return x.is_contiguous(memory_format=torch.channels_last) and \
        not x.is_contiguous()


def bn_relu_maxpool(x: torch.Tensor, bn, pool) -> torch.Tensor:
    """pool(bn(x)) for a BatchNorm2d(relu=True) and MaxPool2d(3, 2, 1):
    fused when can_fuse_stem allows it, else the two modules as they are."""
    if not can_fuse_stem(x, bn, pool):
        return pool(bn(x))
    if bn.running_mean.dtype != torch.float32:
        bn.running_mean.data = bn.running_mean.data.float()
        bn.running_var.data = bn.running_var.data.float()
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BNReluMaxPoolFn.apply(x, bn.weight, bn.bias, bn.running_mean,
                                  bn.running_var, bn._eaf(), bn.eps)
