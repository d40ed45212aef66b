"""Residual-join fusion, CPU side: the new entry points reduce to the eager
composition bit for bit, and the ResNet-50 state dict is unchanged."""
import copy

import torch
from torch import nn

from deeplearning_amd.models import build_model
from deeplearning_amd.ops import BatchNorm2d, conv_bn_add_relu
from deeplearning_amd.ops.conv1x1 import can_fuse_join, can_pass_input


def _mods(cin, cout, stride=1, seed=0):
    torch.manual_seed(seed)
    conv = nn.Conv2d(cin, cout, 1, stride=stride, bias=False)
    bn = BatchNorm2d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
    return conv, bn


def test_single_join_is_eager_composition_on_cpu():
    conv, bn = _mods(64, 128)
    conv_r, bn_r = copy.deepcopy(conv), copy.deepcopy(bn)
    x = torch.randn(2, 64, 5, 7).requires_grad_(True)
    idt = torch.randn(2, 128, 5, 7).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    idr = idt.detach().clone().requires_grad_(True)

    assert not can_fuse_join(x, conv, bn, identity=idt)
    assert not can_pass_input(x, conv, bn)
    out = conv_bn_add_relu(x, conv, bn, identity=idt)
    ref = torch.relu(bn_r(conv_r(xr)) + idr)
    assert torch.equal(out, ref)

    out.square().mean().backward()
    ref.square().mean().backward()
    assert torch.equal(x.grad, xr.grad)
    assert torch.equal(idt.grad, idr.grad)
    assert torch.equal(conv.weight.grad, conv_r.weight.grad)
    assert torch.equal(bn.weight.grad, bn_r.weight.grad)
    assert torch.equal(bn.bias.grad, bn_r.bias.grad)
    assert torch.equal(bn.running_mean, bn_r.running_mean)
    assert torch.equal(bn.running_var, bn_r.running_var)
    assert int(bn.num_batches_tracked) == int(bn_r.num_batches_tracked)


def test_dual_join_is_eager_composition_on_cpu():
    conv, bn = _mods(64, 128, seed=1)
    conv_d, bn_d = _mods(256, 128, stride=2, seed=2)
    down = nn.Sequential(conv_d, bn_d)
    conv_r, bn_r, down_r = (copy.deepcopy(m) for m in (conv, bn, down))
    x = torch.randn(2, 64, 4, 3)
    xd = torch.randn(2, 256, 8, 6)

    assert not can_fuse_join(x, conv, bn, x_down=xd, downsample=down)
    out = conv_bn_add_relu(x, conv, bn, x_down=xd, downsample=down)
    ref = torch.relu(bn_r(conv_r(x)) + down_r(xd))
    assert torch.equal(out, ref)
    for a, b in ((bn, bn_r), (bn_d, down_r[1])):
        assert torch.equal(a.running_mean, b.running_mean)
        assert torch.equal(a.running_var, b.running_var)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked)


def test_bottleneck_block_on_cpu_matches_manual_composition():
    torch.manual_seed(3)
    model = build_model("resnet50", num_classes=10)
    for block, cin, hw in ((model.layer2[0], 256, 8), (model.layer2[1], 512, 4)):
        ref_b = copy.deepcopy(block)
        x = torch.randn(2, cin, hw, hw)
        out = block(x)
        r = ref_b.bn1(ref_b.conv1(x))
        r = ref_b.bn2(ref_b.conv2(r))
        r = ref_b.bn3(ref_b.conv3(r))
        idt = x if ref_b.downsample is None else ref_b.downsample(x)
        assert torch.equal(out, torch.relu(r + idt))


def test_resnet50_state_dict_keys_and_param_count_unchanged():
    model = build_model("resnet50", num_classes=1000)
    sd = model.state_dict()
    # torchvision-compatible ResNet-50: 161 parameter tensors, 53 BNs with
    # three buffers each
    assert len(sd) == 161 + 3 * 53
    assert sum(p.numel() for p in model.parameters()) == 25_557_032
    for key in ("conv1.weight", "bn1.running_mean",
                "layer1.0.conv1.weight", "layer1.0.bn3.weight",
                "layer1.0.bn3.num_batches_tracked",
                "layer1.0.downsample.0.weight",
                "layer1.0.downsample.1.running_var",
                "layer3.5.conv3.weight", "layer4.2.bn3.bias", "fc.bias"):
        assert key in sd, key
    per_block = {k.split(".")[2] for k in sd if k.startswith("layer3.1.")}
    assert per_block == {"conv1", "bn1", "conv2", "bn2", "conv3", "bn3"}
