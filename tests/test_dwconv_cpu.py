"""Depthwise conv op and module without a GPU: the CPU route is F.conv2d
itself, DepthwiseConv2d is state-dict compatible with nn.Conv2d, and the zoo's
depthwise call sites use it without changing parameter names, shapes or init.
"""
import importlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from deeplearning_amd import ops
from deeplearning_amd.models import build_model
from deeplearning_amd.ops import (DepthwiseConv2d, can_use_dwconv,
                                  depthwise_conv2d)


def _inputs(C=8, K=3, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, C, 9, 7, generator=g)
    w = torch.randn(C, 1, K, K, generator=g)
    b = torch.randn(C, generator=g) if bias else None
    return x, w, b


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("bias", [False, True])
def test_function_equals_conv2d_on_cpu(K, stride, bias):
    x, w, b = _inputs(K=K, bias=bias)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)
              if t is not None]
    ref_leaves = [t.clone().requires_grad_(True) for t in (x, w, b)
                  if t is not None]
    y = depthwise_conv2d(*leaves, stride=stride) if bias else \
        depthwise_conv2d(leaves[0], leaves[1], None, stride=stride)
    ref = F.conv2d(ref_leaves[0], ref_leaves[1],
                   ref_leaves[2] if bias else None, stride, (K - 1) // 2, 1,
                   x.shape[1])
    assert torch.equal(y, ref)
    dy = torch.randn_like(ref)
    y.backward(dy)
    ref.backward(dy)
    for a, r in zip(leaves, ref_leaves):
        assert torch.equal(a.grad, r.grad)


def test_function_explicit_padding_on_cpu():
    x, w, b = _inputs(K=3)
    assert torch.equal(depthwise_conv2d(x, w, b, stride=1, padding=0),
                       F.conv2d(x, w, b, 1, 0, 1, x.shape[1]))


def test_module_equals_conv2d_on_cpu():
    torch.manual_seed(3)
    m = DepthwiseConv2d(8, 8, 5, 2, 2, groups=8)
    plain = nn.Conv2d(8, 8, 5, 2, 2, groups=8)
    plain.load_state_dict(m.state_dict())
    x, _, _ = _inputs()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = m(xa), plain(xb)
    assert torch.equal(ya, yb)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(m.weight.grad, plain.weight.grad)
    assert torch.equal(m.bias.grad, plain.bias.grad)


def test_can_use_dwconv_false_on_cpu(monkeypatch):
    monkeypatch.setenv("DLA_DWCONV", "1")
    m = DepthwiseConv2d(8, 8, 3, 1, 1, groups=8).to(torch.bfloat16)
    x = torch.randn(2, 8, 6, 6).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    assert can_use_dwconv(x, m) is False


@pytest.mark.parametrize("bias", [False, True])
def test_state_dict_matches_conv2d(bias):
    torch.manual_seed(11)
    a = DepthwiseConv2d(16, 16, 7, padding=3, groups=16, bias=bias)
    torch.manual_seed(11)
    b = nn.Conv2d(16, 16, 7, padding=3, groups=16, bias=bias)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k])
    a.load_state_dict(sb, strict=True)
    b.load_state_dict(sa, strict=True)


# model, module holding the class, number of depthwise convs
_MODELS = [
    ("convnext_tiny", "classification.convnext", 18),
    ("efficientnet_b0", "classification.efficientnet", 16),
    ("shufflenet_v2_x1_0", "classification.shufflenet", 19),
    ("coatnet_0", "classification.coatnet", 5),
    ("xception", "classification.zoo_tail", 34),
]


def _is_depthwise(m):
    return isinstance(m, nn.Conv2d) and m.groups > 1 and \
        m.groups == m.in_channels == m.out_channels


@pytest.mark.parametrize("name,modname,n_dw", _MODELS,
                         ids=[m[0] for m in _MODELS])
def test_models_keep_plain_conv_state_dict(name, modname, n_dw, monkeypatch):
    torch.manual_seed(0)
    model = build_model(name, num_classes=10)
    dws = [m for m in model.modules() if _is_depthwise(m)]
    assert len(dws) == n_dw
    assert all(type(m) is DepthwiseConv2d for m in dws)

    # the same construction with a plain nn.Conv2d at every depthwise site
    mod = importlib.import_module("deeplearning_amd.models." + modname)
    monkeypatch.setattr(mod, "DepthwiseConv2d", nn.Conv2d)
    torch.manual_seed(0)
    plain = build_model(name, num_classes=10)
    assert not any(isinstance(m, DepthwiseConv2d) for m in plain.modules())
    sa, sb = model.state_dict(), plain.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape, k
        assert torch.equal(sa[k], sb[k]), k  # same init RNG order
    plain.load_state_dict(sa, strict=True)


def test_convnext_dwconv_keys():
    sd = build_model("convnext_tiny", num_classes=10).state_dict()
    assert tuple(sd["stages.0.0.dwconv.weight"].shape) == (96, 1, 7, 7)
    assert tuple(sd["stages.0.0.dwconv.bias"].shape) == (96,)


def test_yolov5_depthwise_conv_site():
    from deeplearning_amd.models.detection.yolov5 import Conv

    assert type(Conv(16, 16, 3, 1, g=16).conv) is DepthwiseConv2d
    assert type(Conv(16, 32, 3, 1).conv) is nn.Conv2d


def test_ops_exports():
    for name in ("depthwise_conv2d", "can_use_dwconv", "DepthwiseConv2d"):
        assert name in ops.__all__ and hasattr(ops, name)
