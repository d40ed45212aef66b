"""1x1 convolution on the hand-written implicit-GEMM MFMA kernel
(csrc/conv1x1.hip) and its fusion with train-mode BatchNorm.

This is the BASELINE.json north-star conv path: NHWC 1x1 conv IS the GEMM
C[M,N] = A[M,K] @ W[N,K]^T on CDNA4 matrix cores. The same kernel computes
forward (A=x, B=W) and dgrad (A=dy, B=W^T); wgrad is a separate M-contraction
kernel. The forward epilogue can accumulate per-channel sum/sumsq so the
following BatchNorm needs no separate stats pass over the conv output, and in
eval mode the whole conv+BN(+ReLU) chain is ONE kernel (scale/shift epilogue).

Reference parity: nn.Conv2d 1x1 call sites — ResNet Bottleneck conv1/conv3
and downsample (classification/resnet/models/networks.py:78-133).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn

from ._ext import ext, use_hip
from .batchnorm import (JOIN, JOIN_DUAL, RELU_X, BwdStatsLink,
                        attach_relu_link, bn_backward,
                        bwd_stats_epilogue_disabled, link_eligible,
                        save_bn_for_backward)


def _flatten_nhwc(x: torch.Tensor) -> torch.Tensor:
    """[B,C,H,W] channels_last -> [B*H*W, C] view (no copy)."""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C)


def _unflatten_nhwc(y2d: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """[B*H*W, N] -> [B,N,H,W] channels_last view."""
    return y2d.view(B, H, W, -1).permute(0, 3, 1, 2)


class _Conv1x1Fn(torch.autograd.Function):
    """y2d[M,N] = x2d[M,K] @ w[N,K]^T with optional fused epilogue.

    Inputs are 2D bf16 (the NHWC flattening happens in the callers). The
    optional second output is the per-channel {sum, sumsq} of the raw conv
    output (fp32 [n_blocks, 2N] partial slab) for the downstream BatchNorm —
    non-differentiable.

    pass_input=True hands x2d back as a last, differentiable output (an
    alias, not a copy). A residual branch hung off that alias delivers its
    gradient to THIS node, which folds it into the dgrad GEMM's residual
    epilogue (dx = dy @ W + d_alias in the store pass) — autograd no longer
    sums the block input's two gradients with a separate add kernel.

    link: the BwdStatsLink of the BN or join that produced x2d. The dgrad
    GEMM then also runs pass 1 of that producer's backward in its store pass
    (mask, store g, partial sums) and hands g and the slab over through the
    link; g is a valid gradient for x2d either way, because masking twice is
    masking once.
    """

    @staticmethod
    def forward(ctx, x2d, w, bias, scale, shift, residual, relu, want_stats,
                pass_input=False, link=None):
        xb = x2d if x2d.dtype == torch.bfloat16 else x2d.to(torch.bfloat16)
        # the join modes mask from xb, which must be the producer's output
        ctx.link = link if xb is x2d else None
        wb = w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)
        wb = wb.contiguous()
        y2d, sums = ext().conv1x1_fwd(xb, wb, bias, scale, shift, residual,
                                      relu, want_stats)
        ctx.save_for_backward(xb, wb)
        ctx.x_dtype = x2d.dtype
        ctx.w_dtype = w.dtype
        ctx.pass_input = pass_input
        outs = (y2d,)
        if want_stats:
            ctx.mark_non_differentiable(sums)
            outs += (sums,)
        if pass_input:
            # either branch may be unused downstream: receive None, not zeros
            ctx.set_materialize_grads(False)
            outs += (x2d,)
        return outs if len(outs) > 1 else y2d

    @staticmethod
    def backward(ctx, dy2d, *rest):
        xb, wb = ctx.saved_tensors
        d_alias = rest[-1] if ctx.pass_input else None
        if d_alias is not None:
            d_alias = d_alias.contiguous()
        dx = dw = db = None
        if dy2d is None:  # only the pass-through output was used
            if d_alias is not None and ctx.needs_input_grad[0]:
                dx = d_alias.to(ctx.x_dtype)
            return dx, None, None, None, None, None, None, None, None, None
        dy2d = dy2d.contiguous()
        if dy2d.dtype != torch.bfloat16:
            dy2d = dy2d.to(torch.bfloat16)
        if ctx.needs_input_grad[0]:
            # LDS-tiled transpose kernel (torch's strided copy is ~15x slower)
            wt = ext().transpose2d(wb)  # [K,N] bf16
            if d_alias is not None and d_alias.dtype != torch.bfloat16:
                d_alias = d_alias.to(torch.bfloat16)
            link = ctx.link
            ops = link.take_operands() if link is not None else None
            if ops is not None and ops["x_raw"].numel() == xb.numel() and \
                    ops["x_raw"].shape[1] == xb.shape[1]:
                dx, slab = ext().conv1x1_dgrad_bwdstats(
                    dy2d, wt, d_alias, link.mode,
                    None if link.mode == RELU_X else xb, ops["x_raw"],
                    ops.get("scale"), ops.get("shift"), ops["mean"],
                    ops["rstd"], ops.get("xd_raw"), ops.get("mean_d"),
                    ops.get("rstd_d"))
                link.offer(dx, slab)
            else:
                dx, _ = ext().conv1x1_fwd(dy2d, wt, None, None, None,
                                          d_alias, False, False)
            if dx.dtype != ctx.x_dtype:
                dx = dx.to(ctx.x_dtype)
        if ctx.needs_input_grad[1]:
            dw = ext().conv1x1_wgrad(dy2d, xb)  # fp32 [N,K]
            if dw.dtype != ctx.w_dtype:
                dw = dw.to(ctx.w_dtype)
        if ctx.needs_input_grad[2]:
            # bias rides the fused epilogue in forward; its grad is the
            # per-channel column sum of dy
            db = dy2d.float().sum(0)
        return dx, dw, db, None, None, None, None, None, None, None


class _BNFromStatsFn(torch.autograd.Function):
    """Train-mode BN whose stats pass was fused into the producing conv
    kernel: forward = finalize + apply (one read of x instead of two),
    backward = the full batchnorm_bwd (including the d-mean/d-var terms)."""

    @staticmethod
    def forward(ctx, x, weight, bias, sums, running_mean, running_var,
                momentum, eps, relu):
        y, mean, rstd, scale, shift = ext().batchnorm_fwd_from_sums(
            x, weight, bias, sums, running_mean, running_var, momentum, eps,
            relu)
        save_bn_for_backward(ctx, x, y, weight, mean, rstd, scale, shift,
                             relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db = bn_backward(ctx, dy)
        return dx, dw, db, None, None, None, None, None, None


class _Stride2Fn(torch.autograd.Function):
    """Stride-2 NHWC subsample via coalesced row-copy kernels; backward is a
    single-pass scatter that zero-fills unsampled rows (torch's strided
    slicing assign ran ~700us per call on these shapes)."""

    @staticmethod
    def forward(ctx, x):
        ctx.ihw = (x.shape[2], x.shape[3])
        return ext().stride2_gather(x)

    @staticmethod
    def backward(ctx, dy):
        if not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.contiguous(memory_format=torch.channels_last)
        return ext().stride2_scatter(dy, *ctx.ihw)


def _conv1x1_disabled() -> bool:
    return os.environ.get("DLA_NO_CONV1X1", "0") == "1"


def can_fuse_conv1x1(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """True when the HIP conv1x1 GEMM path applies to this call."""
    if _conv1x1_disabled() or not use_hip(x):
        return False
    if x.dtype != torch.bfloat16:
        return False
    if conv.kernel_size != (1, 1) or conv.groups != 1:
        return False
    if conv.padding != (0, 0) or conv.dilation != (1, 1):
        return False
    if conv.stride not in ((1, 1), (2, 2)):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    if cin % 64 != 0 or cout % 64 != 0:
        return False
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


def _prep(x: torch.Tensor, conv: nn.Conv2d):
    """Subsample for stride 2 (autograd scatters the grad back), flatten
    NHWC; the bf16 weight cast happens inside _Conv1x1Fn so fp32 weight
    leaves get their fp32 wgrad directly."""
    stride = conv.stride[0]
    if stride == 2:
        x = _Stride2Fn.apply(x)
    B, C, H, W = x.shape
    x2d = _flatten_nhwc(x)
    w2d = conv.weight.reshape(conv.weight.shape[0], conv.weight.shape[1])
    bias = conv.bias.float() if conv.bias is not None else None
    return x2d, w2d, bias, (B, H, W)


def conv1x1(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """Plain 1x1 conv through the MFMA GEMM kernel (bias fused)."""
    x2d, wb, bias, (B, H, W) = _prep(x, conv)
    y2d = _Conv1x1Fn.apply(x2d, wb, bias, None, None, None, False, False)
    return _unflatten_nhwc(y2d, B, H, W)


def _fp32_running_stats(bn) -> None:
    if bn.running_mean.dtype != torch.float32:
        bn.running_mean.data = bn.running_mean.data.float()
        bn.running_var.data = bn.running_var.data.float()


def _conv1x1_train_stats(x: torch.Tensor, conv: nn.Conv2d, bn,
                         pass_input: bool = False):
    """Train-mode front half shared by conv1x1_bn and the fused join: conv
    GEMM with the stats epilogue plus the BN bookkeeping. Returns (raw conv
    output NHWC 4D, [n_blocks, 2C] stats partials, momentum, x alias|None)."""
    # the backward-stats link of x's producer, if this conv may serve it: x
    # itself is the GEMM operand (stride 1, bf16), and a join's output has no
    # other consumer than this conv and the identity that rides its dgrad
    link = getattr(x, "_dla_bwd_link", None)
    if link is not None and (
            bwd_stats_epilogue_disabled() or conv.stride != (1, 1) or
            x.dtype != torch.bfloat16 or
            (link.mode != RELU_X and not pass_input)):
        link = None
    x2d, wb, bias, (B, H, W) = _prep(x, conv)
    _fp32_running_stats(bn)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    momentum = bn._eaf() if hasattr(bn, "_eaf") else (bn.momentum or 0.0)
    outs = _Conv1x1Fn.apply(x2d, wb, bias, None, None, None, False, True,
                            pass_input, link)
    alias = _unflatten_nhwc(outs[2], B, H, W) if pass_input else None
    return _unflatten_nhwc(outs[0], B, H, W), outs[1], momentum, alias


def conv1x1_bn(x: torch.Tensor, conv: nn.Conv2d, bn,
               pass_input: bool = False):
    """Fused conv1x1 + BatchNorm2d(+ReLU) chain.

    train: conv GEMM with fused channel-stats epilogue -> BN finalize+apply
           (skips the stats read pass over the conv output entirely)
    eval (no grad): ONE kernel — conv GEMM with scale/shift(+ReLU) epilogue.

    pass_input=True (train, stride 1) returns (y, x_alias): route a residual
    branch through x_alias and its gradient rides the dgrad GEMM epilogue.
    """
    relu = bool(getattr(bn, "relu", False))
    if bn.training:
        # conv + fused stats, then BN finalize/apply straight from the
        # per-block partial slab
        y_raw, partials, momentum, alias = _conv1x1_train_stats(
            x, conv, bn, pass_input)
        y = _BNFromStatsFn.apply(y_raw, bn.weight, bn.bias, partials,
                                 bn.running_mean, bn.running_var, momentum,
                                 bn.eps, relu)
        if relu:
            attach_relu_link(y)
        return (y, alias) if pass_input else y
    if pass_input:
        raise ValueError("conv1x1_bn: pass_input needs train mode")

    x2d, wb, bias, (B, H, W) = _prep(x, conv)
    _fp32_running_stats(bn)

    if not bn.training:
        rstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight.float() * rstd
        shift = bn.bias.float() - bn.running_mean * scale
        if not (torch.is_grad_enabled() and
                (x.requires_grad or conv.weight.requires_grad or
                 bn.weight.requires_grad)):
            y2d, _ = ext().conv1x1_fwd(
                x2d.to(torch.bfloat16), wb.to(torch.bfloat16).contiguous(),
                bias, scale.contiguous(), shift.contiguous(), None, relu,
                False)
            return _unflatten_nhwc(y2d, B, H, W)
        # eval with grad: conv kernel + differentiable scale/shift
        y2d = _Conv1x1Fn.apply(x2d, wb, bias, None, None, None, False, False)
        y = _unflatten_nhwc(y2d, B, H, W)
        y = y * scale.reshape(1, -1, 1, 1).to(y.dtype) + \
            shift.reshape(1, -1, 1, 1).to(y.dtype)
        return torch.relu(y) if relu else y


class _BNJoinFn(torch.autograd.Function):
    """out = relu(bn(x_raw) + identity) in one pass over memory; the BN is
    finalized from the producing conv's stats partials and its output is
    never materialised. Backward: pass 1 masks (g = dy*[out>0]) and reduces,
    pass 2 writes dx_raw; the identity gradient is g itself."""

    @staticmethod
    def forward(ctx, x_raw, weight, bias, partials, running_mean,
                running_var, momentum, eps, identity):
        out, mean, rstd = ext().bn_add_relu_fwd_from_sums(
            x_raw, weight, bias, partials, running_mean, running_var,
            momentum, eps, identity)
        ctx.save_for_backward(x_raw, out, weight, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dy):
        x_raw, out, weight, mean, rstd = ctx.saved_tensors
        link = getattr(ctx, "link", None)
        slab = link.claim(dy, out) if link is not None else None
        if slab is not None:  # dy is g: the next conv1's dgrad ran pass 1
            g = dy
            dx, dw, db = ext().bn_bwd_dx_from_slab(g, slab, x_raw, weight,
                                                   mean, rstd)
        else:
            g, dx, dw, db = ext().bn_add_relu_bwd(dy, out, x_raw, weight,
                                                  mean, rstd)
        return dx, dw, db, None, None, None, None, None, g


class _BNJoinDualFn(torch.autograd.Function):
    """First block of a stage: out = relu(bn(x_raw) + bn_d(xd_raw)), both
    operands raw conv outputs with their own BN (same C, same rows)."""

    @staticmethod
    def forward(ctx, x_raw, weight, bias, partials, running_mean,
                running_var, momentum, eps, xd_raw, weight_d, bias_d,
                partials_d, running_mean_d, running_var_d, momentum_d, eps_d):
        out, mean, rstd, mean_d, rstd_d = \
            ext().bn_add_relu_dual_fwd_from_sums(
                x_raw, weight, bias, partials, running_mean, running_var,
                momentum, eps, xd_raw, weight_d, bias_d, partials_d,
                running_mean_d, running_var_d, momentum_d, eps_d)
        ctx.save_for_backward(x_raw, xd_raw, out, weight, mean, rstd,
                              weight_d, mean_d, rstd_d)
        return out

    @staticmethod
    def backward(ctx, dy):
        (x_raw, xd_raw, out, weight, mean, rstd, weight_d, mean_d,
         rstd_d) = ctx.saved_tensors
        link = getattr(ctx, "link", None)
        slab = link.claim(dy, out) if link is not None else None
        if slab is not None:
            dx, dxd, dw, db, dwd, dbd = \
                ext().bn_join_dual_bwd_dx_from_slab(
                    dy, slab, x_raw, weight, mean, rstd, xd_raw, weight_d,
                    mean_d, rstd_d)
        else:
            dx, dxd, dw, db, dwd, dbd = ext().bn_add_relu_dual_bwd(
                dy, out, x_raw, weight, mean, rstd, xd_raw, weight_d,
                mean_d, rstd_d)
        return (dx, dw, db, None, None, None, None, None,
                dxd, dwd, dbd, None, None, None, None, None)


def _fused_join_disabled() -> bool:
    return os.environ.get("DLA_NO_FUSED_JOIN", "0") == "1"  # A/B runs


def _dual_epilogue_disabled() -> bool:
    # the three-sum epilogue of the dual join (see docs/KERNELS.md)
    return os.environ.get("DLA_NO_BWD_STATS_DUAL", "0") == "1"


def _attach_join_link(out: torch.Tensor) -> torch.Tensor:
    """Hang a JOIN / JOIN_DUAL link on a join output that autograd tracks.
    Whether it is used is the consumer's decision (a pass_input conv1)."""
    fn = out.grad_fn
    if fn is None or bwd_stats_epilogue_disabled():
        return out
    saved = fn.saved_tensors
    if len(saved) == 5:
        x_raw, _, _, mean, rstd = saved
        if link_eligible(x_raw):
            fn.link = out._dla_bwd_link = BwdStatsLink(
                JOIN, x_raw=x_raw, mean=mean, rstd=rstd)
    elif not _dual_epilogue_disabled():
        x_raw, xd_raw, _, _, mean, rstd, _, mean_d, rstd_d = saved
        if link_eligible(x_raw):
            fn.link = out._dla_bwd_link = BwdStatsLink(
                JOIN_DUAL, x_raw=x_raw, mean=mean, rstd=rstd, xd_raw=xd_raw,
                mean_d=mean_d, rstd_d=rstd_d)
    return out


def _join_bn_ok(conv: nn.Conv2d, bn) -> bool:
    from .batchnorm import BatchNorm2d

    return (type(bn) is BatchNorm2d and bn.training and
            not getattr(bn, "relu", False) and conv.bias is None)


def can_pass_input(x: torch.Tensor, conv: nn.Conv2d, bn) -> bool:
    """True when conv1x1_bn(x, conv, bn, pass_input=True) applies: the
    identity gradient of a residual block can ride this conv's dgrad."""
    from .batchnorm import BatchNorm2d

    return (not _fused_join_disabled() and can_fuse_conv1x1(x, conv) and
            conv.stride == (1, 1) and type(bn) is BatchNorm2d and
            bn.training and torch.is_grad_enabled() and x.requires_grad)


def can_fuse_join(x: torch.Tensor, conv: nn.Conv2d, bn, identity=None,
                  x_down=None, downsample=None) -> bool:
    """True when conv -> bn -> (+identity | +downsample(x_down)) -> relu can
    run as conv+stats GEMM(s) and ONE join kernel."""
    if _fused_join_disabled() or not can_fuse_conv1x1(x, conv) or \
            not _join_bn_ok(conv, bn):
        return False
    if downsample is not None:
        if not (isinstance(downsample, nn.Sequential) and
                len(downsample) == 2 and
                isinstance(downsample[0], nn.Conv2d)):
            return False
        return (x_down is not None and
                can_fuse_conv1x1(x_down, downsample[0]) and
                _join_bn_ok(downsample[0], downsample[1]) and
                downsample[0].out_channels == conv.out_channels)
    return (identity is not None and use_hip(identity) and
            identity.dtype == torch.bfloat16 and identity.dim() == 4 and
            identity.is_contiguous(memory_format=torch.channels_last))


def conv_bn_add_relu(x: torch.Tensor, conv: nn.Conv2d, bn, identity=None,
                     x_down=None, downsample=None) -> torch.Tensor:
    """The residual join relu(bn(conv(x)) + branch), where branch is
    `identity`, or `downsample(x_down)` when a downsample module is given.

    Fused route (GPU, bf16, channels_last, channels % 64, train-mode
    BatchNorm2d, 1x1 convs): conv GEMM(s) with stats epilogue, then one
    kernel that finalizes, normalises, adds and applies ReLU. Anything else
    runs the plain composition conv_bn -> add_relu."""
    if can_fuse_join(x, conv, bn, identity, x_down, downsample):
        y_raw, partials, momentum, _ = _conv1x1_train_stats(x, conv, bn)
        if downsample is None:
            if identity.shape != y_raw.shape:
                raise ValueError("conv_bn_add_relu: identity shape mismatch")
            return _attach_join_link(_BNJoinFn.apply(
                y_raw, bn.weight, bn.bias, partials, bn.running_mean,
                bn.running_var, momentum, bn.eps, identity))
        conv_d, bn_d = downsample[0], downsample[1]
        yd_raw, partials_d, momentum_d, _ = _conv1x1_train_stats(
            x_down, conv_d, bn_d)
        if yd_raw.shape != y_raw.shape:
            raise ValueError("conv_bn_add_relu: downsample shape mismatch")
        return _attach_join_link(_BNJoinDualFn.apply(
            y_raw, bn.weight, bn.bias, partials, bn.running_mean,
            bn.running_var, momentum, bn.eps, yd_raw, bn_d.weight, bn_d.bias,
            partials_d, bn_d.running_mean, bn_d.running_var, momentum_d,
            bn_d.eps))
    from .activations import add_relu

    out = conv_bn(x, conv, bn)
    if downsample is not None:
        if (isinstance(downsample, nn.Sequential) and len(downsample) == 2
                and isinstance(downsample[0], nn.Conv2d)):
            identity = conv_bn(x_down, downsample[0], downsample[1])
        else:
            identity = downsample(x_down)
    return add_relu(out, identity)


def conv_bn(x: torch.Tensor, conv: nn.Conv2d, bn) -> torch.Tensor:
    """conv -> bn chain, routed through the fused MFMA path when it applies
    (1x1 any stride, or 3x3 s1p1; GPU, bf16, channels_last, channels % 64);
    otherwise eager."""
    from .batchnorm import BatchNorm2d

    if isinstance(bn, BatchNorm2d):
        if can_fuse_conv1x1(x, conv):
            return conv1x1_bn(x, conv, bn)
        if can_fuse_conv3x3(x, conv):
            return conv3x3_bn(x, conv, bn)
    return bn(conv(x))


class _Conv3x3Fn(torch.autograd.Function):
    """3x3 s1 p1 conv: forward on the TAPS=9 implicit-GEMM MFMA kernel
    (beats MIOpen fwd on 3 of 4 ResNet shapes, up to 2.75x, and can fuse
    the BN-stats epilogue); dgrad reuses the SAME kernel with the flipped,
    channel-transposed weight; wgrad is the TAPS=9 variant of the
    M-contraction wgrad kernel — conv2d 3x3 is hand-written end to end."""

    @staticmethod
    def forward(ctx, x4d, w, want_stats):
        B, C, H, W = x4d.shape
        xb = x4d if x4d.dtype == torch.bfloat16 else x4d.to(torch.bfloat16)
        wb = w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)
        a = _flatten_nhwc(xb)
        w9 = wb.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()
        y2d, sums = ext().conv3x3_fwd(a, w9, H, W, None, None, None, None,
                                      False, want_stats)
        ctx.save_for_backward(xb, wb)
        ctx.w_dtype = w.dtype
        ctx.x_dtype = x4d.dtype
        y = _unflatten_nhwc(y2d, B, H, W)
        if want_stats:
            ctx.mark_non_differentiable(sums)
            return y, sums
        return y

    @staticmethod
    def backward(ctx, dy, *unused):
        xb, wb = ctx.saved_tensors
        B, C, H, W = xb.shape
        if not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.contiguous(memory_format=torch.channels_last)
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        dy2d = _flatten_nhwc(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # dgrad IS the same TAPS=9 kernel: conv3x3 of dy with the
            # spatially-flipped, channel-transposed weight
            wd = wb.flip(2, 3).transpose(0, 1)       # [Ci, Co, 3, 3]
            wd9 = wd.permute(0, 2, 3, 1).reshape(C, -1).contiguous()
            dx2d, _ = ext().conv3x3_fwd(dy2d, wd9, H, W, None, None, None,
                                        None, False, False)
            dx = _unflatten_nhwc(dx2d, B, H, W)
            if dx.dtype != ctx.x_dtype:
                dx = dx.to(ctx.x_dtype)
        if ctx.needs_input_grad[1]:
            dw9 = ext().conv3x3_wgrad(dy2d, _flatten_nhwc(xb), H, W)
            dw = dw9.view(wb.shape[0], 3, 3, C).permute(0, 3, 1, 2)
            if dw.dtype != ctx.w_dtype:
                dw = dw.to(ctx.w_dtype)
            else:
                dw = dw.contiguous()
        return dx, dw, None


def _conv3x3_enabled() -> bool:
    # measured round 2: the TAPS=9 fwd kernel beats MIOpen fwd on 3 of 4
    # ResNet shapes in isolation (to 2.75x), but the integrated train step
    # regressed 7403 -> 7192 img/s (library-backward/permute overheads eat
    # the fwd win). Routed opt-in until the hand-written 3x3 dgrad/wgrad
    # land; the kernel stays fully tested either way.
    return os.environ.get("DLA_CONV3X3", "0") == "1"


def can_fuse_conv3x3(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    if _conv1x1_disabled() or not _conv3x3_enabled() or not use_hip(x):
        return False
    if x.dtype != torch.bfloat16:
        return False
    if conv.kernel_size != (3, 3) or conv.groups != 1:
        return False
    if conv.padding != (1, 1) or conv.dilation != (1, 1) or \
            conv.stride != (1, 1) or conv.bias is not None:
        return False
    if conv.in_channels % 64 != 0 or conv.out_channels % 64 != 0:
        return False
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


def conv3x3_bn(x: torch.Tensor, conv: nn.Conv2d, bn) -> torch.Tensor:
    """Fused 3x3 conv + BatchNorm(+ReLU): train fuses the stats epilogue
    into the conv (no separate stats pass); eval is one kernel."""
    relu = bool(getattr(bn, "relu", False))
    B, C, H, W = x.shape
    if bn.running_mean.dtype != torch.float32:
        bn.running_mean.data = bn.running_mean.data.float()
        bn.running_var.data = bn.running_var.data.float()
    if not bn.training:
        rstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight.float() * rstd
        shift = bn.bias.float() - bn.running_mean * scale
        if not (torch.is_grad_enabled() and
                (x.requires_grad or conv.weight.requires_grad or
                 bn.weight.requires_grad)):
            xb = x.to(torch.bfloat16)
            wb = conv.weight.to(torch.bfloat16)
            w9 = wb.permute(0, 2, 3, 1).reshape(wb.shape[0], -1).contiguous()
            y2d, _ = ext().conv3x3_fwd(_flatten_nhwc(xb), w9, H, W, None,
                                       scale.contiguous(), shift.contiguous(),
                                       None, relu, False)
            return _unflatten_nhwc(y2d, B, H, W)
        y = _Conv3x3Fn.apply(x, conv.weight, False)
        y = y * scale.reshape(1, -1, 1, 1).to(y.dtype) + \
            shift.reshape(1, -1, 1, 1).to(y.dtype)
        return torch.relu(y) if relu else y
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    momentum = bn._eaf() if hasattr(bn, "_eaf") else (bn.momentum or 0.0)
    y_raw, partials = _Conv3x3Fn.apply(x, conv.weight, True)
    return _BNFromStatsFn.apply(y_raw, bn.weight, bn.bias, partials,
                                bn.running_mean, bn.running_var, momentum,
                                bn.eps, relu)
