"""BatchNorm2d backed by the HIP kernels (csrc/batchnorm.hip): training-mode
batch statistics with optional fused ReLU, and FrozenBatchNorm2d.

Reference parity: nn.BatchNorm2d everywhere; FrozenBatchNorm2d
(detection/fasterRcnn/models/backbone/resnet50_fpn.py:5, FPN/fpn_model.py:8).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._ext import dense, ext, use_hip


def _mask_from_y() -> bool:
    return os.environ.get("DLA_BN_MASK_FROM_Y", "0") == "1"  # A/B runs


def save_bn_for_backward(ctx, x, y, weight, mean, rstd, scale, shift, relu):
    """Save what batchnorm_bwd_ex needs. The ReLU mask comes from x through
    the forward's own scale/shift where the extension's rule allows it
    (channels_last), so y is not saved there; otherwise, or with
    DLA_BN_MASK_FROM_Y=1, from the stored y as before."""
    ctx.relu = relu
    ctx.mask_from_x = bool(relu and not _mask_from_y() and
                           ext().bn_relu_mask_from_x(x))
    if ctx.mask_from_x:
        ctx.save_for_backward(x, weight, mean, rstd, scale, shift)
    elif relu:
        ctx.save_for_backward(x, weight, mean, rstd, y)
    else:
        ctx.save_for_backward(x, weight, mean, rstd)


RELU_X, JOIN, JOIN_DUAL = 1, 2, 3  # BwdMode of csrc/conv1x1.hip


def bwd_stats_epilogue_disabled() -> bool:
    """DLA_NO_BWD_STATS_EPILOGUE=1 (A/B runs) keeps pass 1 of every BN
    backward a kernel of its own; DLA_NO_FUSED_JOIN=1 implies it."""
    return (os.environ.get("DLA_NO_BWD_STATS_EPILOGUE", "0") == "1" or
            os.environ.get("DLA_NO_FUSED_JOIN", "0") == "1")


class BwdStatsLink:
    """Hand-over between a BN producer (BatchNorm2d(relu=True), the residual
    joins) and the 1x1 conv that consumes its output, for the backward.

    The producer's forward fills in what pass 1 of its backward reads (x_raw,
    mean, rstd; scale/shift for the ReLU mask; the second BN of a dual join).
    The consuming conv's backward takes these out, runs its dgrad GEMM with
    the backward-stats epilogue and leaves the masked gradient g and the
    partial-sum slab here. The producer's backward claims them, but only if
    the gradient autograd hands it IS g (same storage, geometry and version:
    no second consumer, hook or accumulation in between), and then runs the
    dx pass alone. Each hand-over empties the link, so it holds no tensor
    after a backward and a second backward through a retained graph takes
    the two-pass route."""

    __slots__ = ("mode", "operands", "g", "slab", "g_version")

    def __init__(self, mode, **operands):
        self.mode = mode
        self.operands = operands
        self.g = self.slab = self.g_version = None

    def take_operands(self):
        ops, self.operands = self.operands, None
        return ops

    def offer(self, g, slab):
        self.g, self.slab, self.g_version = g, slab, g._version

    def claim(self, dy, like):
        """The slab, if dy is the tensor the epilogue wrote (laid out like
        the producer's output `like`); else None."""
        g, slab, version = self.g, self.slab, self.g_version
        self.g = self.slab = self.g_version = None
        if g is None or dy is None or not dy.is_cuda:
            return None
        same = (dy.dtype == g.dtype and dy.shape == like.shape and
                dy.stride() == like.stride() and dy.storage_offset() == 0 and
                dy.data_ptr() == g.data_ptr() and
                dy.untyped_storage().data_ptr() ==
                g.untyped_storage().data_ptr() and dy._version == version)
        return slab if same else None


def link_eligible(x) -> bool:
    """Shapes the conv1x1 dgrad epilogue serves: bf16 channels_last, C % 64."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and
            x.shape[1] % 64 == 0 and
            x.is_contiguous(memory_format=torch.channels_last))


def relu_x_epilogue_enabled() -> bool:
    """The BN+ReLU (bn2 <- conv3 dgrad) mode is opt-in: measured per call it
    gains nothing over the separate pass 1, which reads only dy and x
    (profiles/bwdstats_epilogue_ab.txt). DLA_BWD_STATS_RELU_X=1 routes it."""
    return os.environ.get("DLA_BWD_STATS_RELU_X", "0") == "1"


def attach_relu_link(y):
    """After a BatchNorm2d(relu=True) forward built on save_bn_for_backward:
    hang a RELU_X link on the output for a consuming 1x1 conv to find."""
    fn = y.grad_fn
    if fn is None or not getattr(fn, "mask_from_x", False) or \
            not relu_x_epilogue_enabled() or bwd_stats_epilogue_disabled():
        return y
    x, _, mean, rstd, scale, shift = fn.saved_tensors
    if link_eligible(x):
        fn.link = y._dla_bwd_link = BwdStatsLink(
            RELU_X, x_raw=x, mean=mean, rstd=rstd, scale=scale, shift=shift)
    return y


def bn_backward(ctx, dy):
    """(dx, dweight, dbias) from what save_bn_for_backward kept."""
    x, weight, mean, rstd, *rest = ctx.saved_tensors
    link = getattr(ctx, "link", None)
    if link is not None:
        slab = link.claim(dy, x)
        if slab is not None:  # pass 1 ran in the consumer's dgrad epilogue
            return ext().bn_bwd_dx_from_slab(dy, slab, x, weight, mean, rstd)
    y = scale = shift = None
    if ctx.mask_from_x:
        scale, shift = rest
    elif ctx.relu:
        y, = rest
    return ext().batchnorm_bwd_ex(dy, x, y, weight, mean, rstd, scale, shift,
                                  ctx.relu)


class _BNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu):
        x = dense(x)
        y, mean, rstd, scale, shift = ext().batchnorm_fwd(
            x, weight, bias, running_mean, running_var, momentum, eps, relu)
        save_bn_for_backward(ctx, x, y, weight, mean, rstd, scale, shift, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db = bn_backward(ctx, dy)
        return dx, dw, db, None, None, None, None, None


class BatchNorm2d(nn.BatchNorm2d):
    """Drop-in BatchNorm2d; optional fused ReLU via `relu=True`.

    GPU train mode uses the HIP kernel; eval mode uses the fused scale/shift
    apply kernel; CPU uses eager F.batch_norm. State-dict compatible with
    nn.BatchNorm2d.
    """

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True,
                         track_running_stats=True)
        self.relu = relu

    def _eaf(self) -> float:
        """Exponential average factor; momentum=None means cumulative average
        (torch semantics — what SWA's update_bn relies on)."""
        if self.momentum is not None:
            return self.momentum
        if self.training and self.num_batches_tracked is not None:
            return 1.0 / float(max(int(self.num_batches_tracked), 1))
        return 0.0

    def forward(self, x):
        if not use_hip(x):
            if self.training and self.momentum is None and \
                    self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
            y = F.batch_norm(x, self.running_mean, self.running_var, self.weight,
                             self.bias, self.training, self._eaf(), self.eps)
            return torch.relu(y) if self.relu else y
        if self.running_mean.dtype != torch.float32:
            # .to(bf16) on the module converts buffers; the HIP kernel keeps
            # running statistics in fp32 — restore them once.
            self.running_mean.data = self.running_mean.data.float()
            self.running_var.data = self.running_var.data.float()
        if self.training:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
            y = _BNFn.apply(x, self.weight, self.bias, self.running_mean,
                            self.running_var, self._eaf(), self.eps,
                            self.relu)
            return attach_relu_link(y) if self.relu else y
        rstd = torch.rsqrt(self.running_var.float() + self.eps)
        scale = self.weight.float() * rstd
        shift = self.bias.float() - self.running_mean.float() * scale
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
            y = x * scale.reshape(1, -1, 1, 1).to(x.dtype) + shift.reshape(1, -1, 1, 1).to(x.dtype)
            return torch.relu(y) if self.relu else y
        return ext().bn_apply(dense(x), scale, shift, self.relu)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm with fixed affine + stats (detection backbones)."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        rstd = torch.rsqrt(self.running_var.float() + self.eps)
        scale = self.weight.float() * rstd
        shift = self.bias.float() - self.running_mean.float() * scale
        if use_hip(x) and not (torch.is_grad_enabled() and x.requires_grad):
            return ext().bn_apply(dense(x), scale, shift, False)
        sc = scale.reshape(1, -1, 1, 1).to(x.dtype)
        sh = shift.reshape(1, -1, 1, 1).to(x.dtype)
        return x * sc + sh
