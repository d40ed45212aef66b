"""Fused ResNet stem tail on the GPU: train-mode BatchNorm2d(relu=True) +
MaxPool2d(3, 2, 1) as one apply+pool kernel and a two-pass gather backward.
References: the unfused route (DLA_NO_FUSED_STEM=1: bn kernels + aten pool)
and eager fp32 autograd.

Inputs on the integer lattice -3..3 give many exact ties inside a window, at
zero (after ReLU) and at positive values, in bf16 and fp32 alike, so the
first-maximum routing of the fp32 reference equals the bf16 one. The affine
has negative weights, which reverse the order within a channel.

Tolerances: tests/test_join_fusion_gpu.py's 5e-2 forward / 8e-2 gradients of
max|ref| against fp32 eager; against the unfused route the pooled output is
bit-identical, dbias is exact for integer dpool (every sum is exact in fp32
and bf16), and dx differs only by the order of the fp32 atomic sum(g*xhat):
one bf16 ulp, |a-b| <= 2^-7 max(|a|,|b|).
"""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

# (B, C, H, W): smallest vector width, odd H and W, every window on a border
# / the stem's C with even sizes / several blocks and two row runs per image
SHAPES = [(2, 8, 7, 9), (3, 64, 12, 10), (2, 64, 17, 16)]
EPS, MOM = 1e-5, 0.1


def _rel_err(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1.0))


def _scaled_err(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-12))


def _within_one_bf16_ulp(a, b):
    a, b = a.float(), b.float()
    return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()))
                .all())


def _x(B, C, H, W, kind, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(7 * C + H)
    if kind == "lattice":
        x = torch.randint(-3, 4, (B, C, H, W), device="cuda", generator=g)
    else:
        # normal, on a grid of 1/8: sum and sum of squares are then exact in
        # fp32 whatever order the atomics take, so two forward runs derive
        # the very same scale/shift and bit-equality is a fair demand
        x = torch.randn(B, C, H, W, device="cuda", generator=g) * 1.5 + 0.3
        x = (x.clamp(-6, 6) * 8).round() / 8
    return x.to(dtype).contiguous(memory_format=torch.channels_last)


def _affine(C):
    g = torch.Generator(device="cuda").manual_seed(C)
    w = torch.rand(C, device="cuda", generator=g) + 0.5
    w[1::3] *= -1.0
    b = torch.randn(C, device="cuda", generator=g) * 0.2
    return w, b


def _dpool(B, C, H, W, integer, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(3 * C + W)
    shape = (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    d = torch.randint(-3, 4, shape, device="cuda", generator=g).float() \
        if integer else torch.randn(shape, device="cuda", generator=g)
    return d.to(dtype).contiguous(memory_format=torch.channels_last)


def _bn(C, w, b, train=True):
    from deeplearning_amd.ops import BatchNorm2d

    bn = BatchNorm2d(C, relu=True).cuda()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    return bn.train(train)


def _route(x, w, b, dpool, fused, pool=None, train=True, expect=None):
    """bn_relu_maxpool forward (+ backward when dpool is given); `fused`
    False sets DLA_NO_FUSED_STEM=1."""
    from deeplearning_amd.ops import bn_relu_maxpool, can_fuse_stem

    os.environ["DLA_NO_FUSED_STEM"] = "0" if fused else "1"
    try:
        torch.manual_seed(5)
        bn = _bn(x.shape[1], w, b, train)
        pool = pool or nn.MaxPool2d(3, stride=2, padding=1)
        xr = x.clone().requires_grad_(True)
        assert can_fuse_stem(xr, bn, pool) == (fused if expect is None
                                               else expect)
        out = bn_relu_maxpool(xr, bn, pool)
        res = {"out": out.detach(), "rmean": bn.running_mean.clone(),
               "rvar": bn.running_var.clone(),
               "nbt": int(bn.num_batches_tracked)}
        if dpool is not None:
            out.backward(dpool)
            res.update(dx=xr.grad, dweight=bn.weight.grad,
                       dbias=bn.bias.grad)
        torch.cuda.synchronize()
        return res
    finally:
        os.environ["DLA_NO_FUSED_STEM"] = "0"


def _eager(x, w, b, dpool, pool_kw=None, train=True):
    """fp32 eager BN -> ReLU -> max_pool2d and its autograd."""
    torch.manual_seed(5)
    bn = _bn(x.shape[1], w, b, train)  # same running-stat start values
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    xr = x.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = torch.relu(F.batch_norm(xr, rm, rv, wr, br, train, MOM, EPS))
    out = F.max_pool2d(y, 3, 2, 1, **(pool_kw or {}))
    out.backward(dpool.float())
    return {"out": out.detach(), "rmean": rm, "rvar": rv, "dx": xr.grad,
            "dweight": wr.grad, "dbias": br.grad}


@pytest.mark.parametrize("kind", ["lattice", "normal"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_forward_is_bit_identical_to_bn_then_pool(B, C, H, W, kind):
    x = _x(B, C, H, W, kind)
    w, b = _affine(C)
    fused = _route(x, w, b, None, True)
    torch.manual_seed(5)
    bn = _bn(C, w, b)
    ref = F.max_pool2d(bn(x), 3, 2, 1)
    assert fused["out"].dtype == x.dtype and fused["out"].shape == ref.shape
    assert fused["out"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(fused["out"], ref)
    assert fused["nbt"] == 1 and int(bn.num_batches_tracked) == 1
    for k, r in (("rmean", bn.running_mean), ("rvar", bn.running_var)):
        err = _rel_err(fused[k], r)
        print(f"{k}: rel err {err:.4g}")
        assert err < 5e-2, k


def test_forward_fp32_is_bit_identical():
    B, C, H, W = 2, 8, 7, 9  # fp32 vectors are 4 channels wide
    x = _x(B, C, H, W, "normal", torch.float32)
    w, b = _affine(C)
    fused = _route(x, w, b, None, True)
    unfused = _route(x, w, b, None, False)
    assert torch.equal(fused["out"], unfused["out"])


@pytest.mark.parametrize("kind", ["lattice", "normal"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_backward_routing_and_mask_exact(B, C, H, W, kind):
    x = _x(B, C, H, W, kind)
    w, b = _affine(C)
    dpool = _dpool(B, C, H, W, integer=True)
    fused = _route(x, w, b, dpool, True)
    unfused = _route(x, w, b, dpool, False)
    assert torch.equal(fused["out"], unfused["out"])
    assert torch.equal(fused["dbias"], unfused["dbias"])
    d = (fused["dx"].float() - unfused["dx"].float()).abs().max()
    print(f"dx max |fused - unfused| {float(d):.4g}")
    assert _within_one_bf16_ulp(fused["dx"], unfused["dx"])
    assert _within_one_bf16_ulp(fused["dweight"], unfused["dweight"])


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_vs_fp32_eager_autograd(B, C, H, W):
    x = _x(B, C, H, W, "lattice")
    w, b = _affine(C)
    dpool = _dpool(B, C, H, W, integer=False)
    fused = _route(x, w, b, dpool, True)
    unfused = _route(x, w, b, dpool, False)
    ref = _eager(x, w, b, dpool)
    for k in ("out", "rmean", "rvar", "dx", "dweight", "dbias"):
        tol = 5e-2 if k in ("out", "rmean", "rvar") else 8e-2
        ef, eu = _scaled_err(fused[k], ref[k]), _scaled_err(unfused[k], ref[k])
        print(f"{k}: fused err {ef:.4g} unfused err {eu:.4g}")
        assert _rel_err(fused[k], ref[k]) < tol, k
        assert ef <= 1.5 * eu, \
            f"{k}: fused err {ef:.4g} > 1.5 x unfused err {eu:.4g}"


@pytest.mark.parametrize("name", ["nchw", "ceil_mode", "c6", "eval", "env"])
def test_fallbacks_take_the_old_path_and_match_eager(name):
    B, C, H, W = 2, (6 if name == "c6" else 8), 7, 9
    x = _x(B, C, H, W, "lattice")
    if name == "nchw":
        x = x.contiguous()
    w, b = _affine(C)
    train = name != "eval"
    pool_kw = {"ceil_mode": True} if name == "ceil_mode" else {}
    pool = nn.MaxPool2d(3, stride=2, padding=1, **pool_kw)
    with torch.no_grad():
        shape = pool(x.float()).shape
    g = torch.Generator(device="cuda").manual_seed(9)
    dpool = torch.randn(shape, device="cuda", generator=g).to(x.dtype)
    got = _route(x, w, b, dpool, fused=(name != "env"), pool=pool,
                 train=train, expect=False)
    ref = _eager(x, w, b, dpool, pool_kw, train)
    assert got["out"].shape == ref["out"].shape
    assert got["nbt"] == (1 if train else 0)
    for k in ("out", "rmean", "rvar", "dx", "dweight", "dbias"):
        err = _rel_err(got[k], ref[k])
        print(f"fallback {name} {k}: rel err {err:.4g}")
        assert err < (5e-2 if k in ("out", "rmean", "rvar") else 8e-2), k


def test_resnet18_fused_vs_unfused_stem():
    from deeplearning_amd.models import build_model
    from deeplearning_amd.ops import cross_entropy

    def run(fused):
        os.environ["DLA_NO_FUSED_STEM"] = "0" if fused else "1"
        try:
            torch.manual_seed(3)
            model = build_model("resnet18", num_classes=10).cuda() \
                .to(memory_format=torch.channels_last).train()
            x = torch.randn(2, 3, 32, 32, device="cuda") \
                .contiguous(memory_format=torch.channels_last)
            t = torch.tensor([1, 7], device="cuda")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = cross_entropy(model(x), t)
            loss.backward()
            torch.cuda.synchronize()
            assert int(model.bn1.num_batches_tracked) == 1
            return loss.detach().float(), model.conv1.weight.grad.float()
        finally:
            os.environ["DLA_NO_FUSED_STEM"] = "0"

    loss_f, g_f = run(True)
    loss_u, g_u = run(False)
    print(f"loss fused {float(loss_f):.6f} unfused {float(loss_u):.6f}; "
          f"conv1.weight.grad rel err {_scaled_err(g_f, g_u):.4g}")
    assert _rel_err(loss_f, loss_u) < 5e-2
    assert _scaled_err(g_f, g_u) < 8e-2
