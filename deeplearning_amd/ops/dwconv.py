"""Depthwise 2-D convolution on the hand-written NHWC kernels of
csrc/dwconv.hip: forward, dgrad and wgrad (+ dbias) for square K in {3, 5, 7},
stride 1 or 2, padding (K-1)/2, dilation 1, groups == Cin == Cout.

`DepthwiseConv2d` is a drop-in `nn.Conv2d`: same constructor, parameters,
state-dict keys and init. Its forward takes the HIP route when
`can_use_dwconv` allows it and `nn.Conv2d.forward` otherwise, so CPU runs,
NCHW inputs and unsupported geometries behave exactly as before.

Switch `DLA_DWCONV` (read at call time): `0` never routes, `1` routes every
supported (K, stride) family, unset routes the families of `_DEFAULT_ON`.

Reference parity: the depthwise nn.Conv2d(groups=C) call sites of ConvNeXt,
EfficientNet MBConv, ShuffleNet, CoAtNet, Xception and YOLOv5.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn

from ._ext import ext, use_hip

_KERNELS = (3, 5, 7)
_STRIDES = (1, 2)
_DTYPES = (torch.bfloat16, torch.float16, torch.float32)

# (K, stride) families routed when DLA_DWCONV is unset. A family is listed
# only if its summed fwd + dgrad + wgrad time over the shapes of
# tools/bench_dwconv.py is no slower than aten's and the model step is not
# slower with it on (profiles/dwconv_bench.txt, profiles/dwconv_model_ab.txt).
# Measured: every family those shapes contain wins. 7x7 stride 2 occurs in
# none of them, so it stays opt-in behind DLA_DWCONV=1.
_DEFAULT_ON = frozenset({(3, 1), (3, 2), (5, 1), (5, 2), (7, 1)})


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _family_enabled(k: int, stride: int) -> bool:
    mode = os.environ.get("DLA_DWCONV")
    if mode == "0":
        return False
    if mode == "1":
        return True
    return (k, stride) in _DEFAULT_ON


def _supported(x: torch.Tensor, weight: torch.Tensor, stride, padding,
               dilation, groups) -> bool:
    """The routing rule on raw arguments (shared by can_use_dwconv and
    depthwise_conv2d)."""
    if x.dim() != 4 or weight.dim() != 4 or x.numel() == 0:
        return False
    c = x.shape[1]
    k = weight.shape[2]
    if weight.shape[0] != c or weight.shape[1] != 1 or groups != c or \
            weight.shape[3] != k or k not in _KERNELS:
        return False
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if isinstance(padding[0], str):
        return False
    if stride[0] != stride[1] or stride[0] not in _STRIDES or \
            padding != ((k - 1) // 2,) * 2 or dilation != (1, 1):
        return False
    if not _family_enabled(k, stride[0]) or not use_hip(x, weight):
        return False
    if x.dtype not in _DTYPES or weight.dtype not in (x.dtype, torch.float32):
        return False
    if c % (16 // x.element_size()) != 0:
        return False
    if x.shape[0] * x.shape[2] * x.shape[3] >= 2 ** 31:
        return False
    # channels_last proper: a tensor that is also NCHW-contiguous keeps the
    # plain route (its consumers treat it as NCHW)
    return x.is_contiguous(memory_format=torch.channels_last) and \
        not x.is_contiguous()


def can_use_dwconv(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """True when conv(x) can run on the HIP depthwise kernels: GPU, the
    (K, stride) family enabled by DLA_DWCONV / the default table, square K in
    {3, 5, 7}, stride 1 or 2, padding (K-1)/2, dilation 1, zero padding mode,
    groups == Cin == Cout, bf16/fp16/fp32 with C a multiple of the 16-byte
    vector, B*H*W < 2^31 and a channels_last (not also NCHW-contiguous) x."""
    if conv.padding_mode != "zeros" or conv.in_channels != conv.out_channels:
        return False
    if conv.bias is not None and \
            conv.bias.dtype not in (x.dtype, torch.float32):
        return False
    return _supported(x, conv.weight, conv.stride, conv.padding,
                      conv.dilation, conv.groups)


class _DepthwiseConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        # fp32 parameters (autocast) go to the kernels as they are; the
        # kernels round them to x's dtype while staging the taps, so the
        # result is that of casting here without the cast launches
        y = ext().dwconv_fwd(x, weight.contiguous(),
                             None if bias is None else bias.contiguous(),
                             stride)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.b_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dy = dy.contiguous(memory_format=torch.channels_last)
        if ctx.needs_input_grad[0]:
            dx = ext().dwconv_dgrad(dy, weight.contiguous(), x.shape[2],
                                    x.shape[3], ctx.stride)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # dbias rides the wgrad pass: dy is being read anyway
            dw, db = ext().dwconv_wgrad(dy, x, weight.shape[2], ctx.stride,
                                        weight.dtype == torch.float32)
            if not ctx.needs_input_grad[1]:
                dw = None
            if not ctx.needs_input_grad[2]:
                db = None
            elif db.dtype != ctx.b_dtype:
                db = db.to(ctx.b_dtype)
        return dx, dw, db, None


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor, bias=None,
                     stride=1, padding=None) -> torch.Tensor:
    """Depthwise conv2d of x [B,C,H,W] with weight [C,1,K,K]; padding defaults
    to (K-1)/2. HIP kernels when the route applies (see can_use_dwconv),
    F.conv2d(..., groups=C) otherwise."""
    if padding is None:
        padding = (weight.shape[2] - 1) // 2, (weight.shape[3] - 1) // 2
    c = x.shape[1]
    bias_ok = bias is None or (bias.is_cuda and
                               bias.dtype in (x.dtype, torch.float32))
    if bias_ok and _supported(x, weight, stride, padding, 1, c):
        return _DepthwiseConvFn.apply(x, weight, bias, _pair(stride)[0])
    return F.conv2d(x, weight, bias, stride, padding, 1, c)


class DepthwiseConv2d(nn.Conv2d):
    """nn.Conv2d whose forward runs the HIP depthwise kernels when
    can_use_dwconv(x, self) holds, and nn.Conv2d.forward otherwise."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if can_use_dwconv(x, self):
            return _DepthwiseConvFn.apply(x, self.weight, self.bias,
                                          self.stride[0])
        return super().forward(x)
