"""BatchNorm2d(relu=True) backward with the ReLU mask recomputed from x
(fma(x, scale, shift) > 0 with the forward's own scale/shift) instead of read
from the stored y. References: the y route (DLA_BN_MASK_FROM_Y=1) and eager
fp32 autograd.

Bounds: dy is integer valued, so sum(dy * mask) is exact in fp32 and dbias
must equal the mask of the stored y exactly. Against the y route everything
but the order of the fp32 atomics is the same arithmetic: one bf16 ulp,
|a-b| <= 2^-7 max(|a|,|b|). Against fp32 eager: the project's 8e-2 of
max|ref| for gradients (tests/test_join_fusion_gpu.py).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from deeplearning_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

# (B, C, H, W): 16-byte vectors / odd sizes / V=2 fallback / V=1 fallback
SHAPES = [(2, 64, 7, 7), (3, 16, 5, 9), (2, 6, 4, 4), (2, 5, 3, 3)]
EPS, MOM = 1e-5, 0.1


def _rel_err(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1.0))


def _within_one_bf16_ulp(a, b):
    a, b = a.float(), b.float()
    return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()))
                .all())


def _inputs(B, C, H, W, dtype, nhwc):
    g = torch.Generator(device="cuda").manual_seed(100 + C)
    # normal, on a grid of 1/8: the batch sums are exact in fp32 in any
    # order, so both routes' forwards derive the same scale/shift and y
    x = torch.randn(B, C, H, W, device="cuda", generator=g) * 1.5 + 0.3
    x = ((x.clamp(-6, 6) * 8).round() / 8).to(dtype)
    dy = torch.randint(-3, 4, (B, C, H, W), device="cuda", generator=g) \
        .to(dtype)
    w = torch.rand(C, device="cuda", generator=g) + 0.5
    w[::3] *= -1.0
    b = torch.randn(C, device="cuda", generator=g) * 0.2
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
        dy = dy.contiguous(memory_format=torch.channels_last)
    return x, dy, w, b


def _run(x, dy, w, b, from_y):
    from deeplearning_amd.ops import BatchNorm2d

    os.environ["DLA_BN_MASK_FROM_Y"] = "1" if from_y else "0"
    try:
        bn = BatchNorm2d(x.shape[1], relu=True).cuda()
        with torch.no_grad():
            bn.weight.copy_(w)
            bn.bias.copy_(b)
        xr = x.clone().requires_grad_(True)
        y = bn(xr)
        saved = y.grad_fn.saved_tensors
        y.backward(dy)
        torch.cuda.synchronize()
        return {"y": y.detach(), "dx": xr.grad, "dweight": bn.weight.grad,
                "dbias": bn.bias.grad, "saved": saved}
    finally:
        os.environ["DLA_BN_MASK_FROM_Y"] = "0"


def _eager(x, dy, w, b):
    xr = x.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    C = x.shape[1]
    y = torch.relu(F.batch_norm(
        xr, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), wr,
        br, True, MOM, EPS))
    y.backward(dy.float())
    return {"y": y.detach(), "dx": xr.grad, "dweight": wr.grad,
            "dbias": br.grad}


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_mask_from_x_nhwc_bf16(B, C, H, W):
    x, dy, w, b = _inputs(B, C, H, W, torch.bfloat16, True)
    assert ext().bn_relu_mask_from_x(x)
    new = _run(x, dy, w, b, from_y=False)
    old = _run(x, dy, w, b, from_y=True)
    ref = _eager(x, dy, w, b)

    # the x route keeps scale/shift and not y; the y route keeps y
    y_ptr = new["y"].data_ptr()
    assert len(new["saved"]) == 6
    assert all(t.data_ptr() != y_ptr for t in new["saved"])
    assert any(t.data_ptr() == old["y"].data_ptr() for t in old["saved"])
    assert torch.equal(new["y"], old["y"])

    frac = float((new["y"] <= 0).float().mean())
    assert 0.2 < frac < 0.8, f"mask should be about half zero, got {frac}"
    exact = torch.where(new["y"] > 0, dy, torch.zeros_like(dy)).float() \
        .sum((0, 2, 3))
    assert torch.equal(new["dbias"], exact)

    for k in ("dx", "dweight", "dbias"):
        print(f"{k}: x route vs y route max |diff| "
              f"{float((new[k].float() - old[k].float()).abs().max()):.4g}, "
              f"vs fp32 eager rel err {_rel_err(new[k], ref[k]):.4g}")
        assert _within_one_bf16_ulp(new[k], old[k]), k
        assert _rel_err(new[k], ref[k]) < 8e-2, k


def test_nchw_fp32_keeps_the_y_route():
    x, dy, w, b = _inputs(2, 16, 5, 9, torch.float32, False)
    assert not ext().bn_relu_mask_from_x(x)
    got = _run(x, dy, w, b, from_y=False)
    ref = _eager(x, dy, w, b)
    assert any(t.data_ptr() == got["y"].data_ptr() for t in got["saved"])
    for k in ("y", "dx", "dweight", "dbias"):
        err = _rel_err(got[k], ref[k])
        print(f"{k}: rel err {err:.4g}")
        assert err < 1e-3, k  # fp32 on both sides, summation order only


def test_old_entry_point_still_masks_from_y():
    """batchnorm_bwd with today's signature, on the forward's own y."""
    x, dy, w, b = _inputs(3, 16, 5, 9, torch.bfloat16, True)
    y, mean, rstd, scale, shift = ext().batchnorm_fwd(
        x, w, b, None, None, MOM, EPS, True)
    old = ext().batchnorm_bwd(dy, x, y, w, mean, rstd, True)
    new = ext().batchnorm_bwd_ex(dy, x, None, w, mean, rstd, scale, shift,
                                 True)
    torch.cuda.synchronize()
    for a, r in zip(new, old):
        assert _within_one_bf16_ulp(a, r)
    with pytest.raises(RuntimeError):
        ext().batchnorm_bwd(dy, x, None, w, mean, rstd, True)
