"""Residual-join fusion on the GPU: relu(bn(conv(x)) + identity) as conv GEMM
plus ONE join kernel, its two-pass backward, and the identity gradient riding
the conv1 dgrad epilogue. Reference: eager fp32 PyTorch and its autograd.

Tolerances follow tests/test_conv1x1_gpu.py::test_conv1x1_bn_train_parity:
5e-2 forward, 8e-2 gradients, relative to max|ref|.
"""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from deeplearning_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

# (B, H, W, C): 98 rows with 8 lanes per row (fewer rows than the row
# stride) / odd row count (row-loop tail) / several blocks
SHAPES = [(2, 7, 7, 64), (3, 5, 9, 128), (2, 14, 14, 256)]
EPS, MOM = 1e-5, 0.1


def _rel_err(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1.0))


def _assert_close(got, ref, rtol=2e-2, msg=""):
    err = _rel_err(got, ref)
    print(f"{msg}: rel err {err:.4g}")
    assert err < rtol, f"{msg}: rel err {err:.4g}"


def _nhwc(B, C, H, W, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(B, C, H, W, device="cuda", generator=g) * scale + shift
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _slab(x, parts):
    """[parts, 2C] per-chunk {sum, sumsq} partials, as the conv epilogue
    leaves them."""
    rows = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).float()
    return torch.stack([torch.cat([c.sum(0), (c * c).sum(0)])
                        for c in torch.tensor_split(rows, parts)]).contiguous()


def _affine(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.rand(C, device="cuda", generator=g) + 0.5
    b = torch.randn(C, device="cuda", generator=g) * 0.2
    return w, b


def _smooth_dy(pre, seed):
    """Random upstream gradient that fades to zero where the pre-activation
    crosses zero, so a mask bit decided by the last fp32 ulp cannot move the
    result; masked positions still carry non-zero dy."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.randn(pre.shape, device="cuda", generator=g)
    return (r * pre.detach().abs().clamp(max=1.0)).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_join_kernels_vs_fp32_eager(B, H, W, C, dual):
    x = _nhwc(B, C, H, W, 1, scale=1.5, shift=0.3)
    other = _nhwc(B, C, H, W, 2, scale=(2.0 if dual else 1.0), shift=-0.2)
    w, b = _affine(C, 3)
    wd, bd = _affine(C, 4)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    rmd, rvd = rm.clone(), rv.clone()

    # fp32 eager reference
    xr = x.float().requires_grad_(True)
    orf = other.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    wdr, bdr = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    rm_r, rv_r, rmd_r, rvd_r = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    branch = F.batch_norm(orf, rmd_r, rvd_r, wdr, bdr, True, MOM, EPS) \
        if dual else orf
    pre = F.batch_norm(xr, rm_r, rv_r, wr, br, True, MOM, EPS) + branch
    out_r = torch.relu(pre)
    frac = float((pre <= 0).float().mean())
    assert 0.3 < frac < 0.7, f"mask should be about half zero, got {frac}"
    dy = _smooth_dy(pre, 5)
    out_r.backward(dy.float())

    slab = _slab(x, 5)
    if dual:
        out, mean, rstd, mean_d, rstd_d = \
            ext().bn_add_relu_dual_fwd_from_sums(
                x, w, b, slab, rm, rv, MOM, EPS, other, wd, bd,
                _slab(other, 3), rmd, rvd, MOM, EPS)
        dx, dxd, dw, db, dwd, dbd = ext().bn_add_relu_dual_bwd(
            dy, out, x, w, mean, rstd, other, wd, mean_d, rstd_d)
    else:
        out, mean, rstd = ext().bn_add_relu_fwd_from_sums(
            x, w, b, slab, rm, rv, MOM, EPS, other)
        g, dx, dw, db = ext().bn_add_relu_bwd(dy, out, x, w, mean, rstd)
    torch.cuda.synchronize()

    assert out.dtype == torch.bfloat16
    assert out.is_contiguous(memory_format=torch.channels_last)
    _assert_close(out, out_r.detach(), 5e-2, "out")
    _assert_close(dx, xr.grad, 8e-2, "dx_raw")
    _assert_close(dw, wr.grad, 8e-2, "dweight")
    _assert_close(db, br.grad, 8e-2, "dbias")
    _assert_close(rm, rm_r, 5e-2, "running_mean")
    _assert_close(rv, rv_r, 5e-2, "running_var")
    if dual:
        _assert_close(dxd, orf.grad, 8e-2, "dxd_raw")
        _assert_close(dwd, wdr.grad, 8e-2, "dweight_d")
        _assert_close(dbd, bdr.grad, 8e-2, "dbias_d")
        _assert_close(rmd, rmd_r, 5e-2, "running_mean_d")
        _assert_close(rvd, rvd_r, 5e-2, "running_var_d")
        assert dbd.data_ptr() != db.data_ptr()  # two params, two buffers
    else:
        _assert_close(g, orf.grad, 8e-2, "identity grad")
        # g is exactly dy under the mask of the stored output
        assert torch.equal(g, torch.where(out > 0, dy, torch.zeros_like(dy)))


def test_finalize_reads_slab_like_presummed_vector():
    """[n_parts, 2C] slab and its [2C] column sum finalize alike (up to the
    fp32 summation order), including a slab deeper than the row lanes."""
    B, H, W, C = 3, 5, 9, 128
    x = _nhwc(B, C, H, W, 11, scale=2.0, shift=1.0)
    idt = _nhwc(B, C, H, W, 12)
    w, b = _affine(C, 13)
    res = []
    for sums in (_slab(x, 1)[0].contiguous(), _slab(x, 2), _slab(x, 131)):
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        out, mean, rstd = ext().bn_add_relu_fwd_from_sums(
            x, w, b, sums, rm, rv, MOM, EPS, idt)
        res.append((out.float(), mean, rstd, rm, rv))
    for other in res[1:]:
        # out: at most one bf16 ulp (2^-7 relative); statistics: fp32 order
        assert torch.allclose(other[0], res[0][0], rtol=1e-2, atol=1e-3)
        for a, r in zip(other[1:], res[0][1:]):
            assert torch.allclose(a, r, rtol=1e-4, atol=1e-5)


def _op_case(B, H, W, C, dual, fused):
    """conv_bn_add_relu fwd+bwd through the public entry point; `fused`
    False runs the previous route (bn apply + add_relu + autograd add)."""
    from deeplearning_amd.ops import BatchNorm2d, conv_bn_add_relu
    from deeplearning_amd.ops.conv1x1 import can_fuse_join

    os.environ["DLA_NO_FUSED_JOIN"] = "0" if fused else "1"
    try:
        torch.manual_seed(21)
        cin = 64
        conv = nn.Conv2d(cin, C, 1, bias=False).cuda()
        bn = BatchNorm2d(C).cuda()
        conv_d = nn.Conv2d(128, C, 1, bias=False).cuda()
        bn_d = BatchNorm2d(C).cuda()
        with torch.no_grad():
            for m in (bn, bn_d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
        x = _nhwc(B, cin, H, W, 22).requires_grad_(True)
        idt = _nhwc(B, C, H, W, 23).requires_grad_(True)
        xd = _nhwc(B, 128, H, W, 24).requires_grad_(True)
        down = nn.Sequential(conv_d, bn_d) if dual else None
        assert can_fuse_join(x, conv, bn, identity=idt, x_down=xd,
                             downsample=down) == fused
        out = conv_bn_add_relu(x, conv, bn, identity=idt, x_down=xd,
                               downsample=down)
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        got = {"out": out.detach(), "dx": x.grad, "dconv": conv.weight.grad,
               "dweight": bn.weight.grad, "dbias": bn.bias.grad,
               "rmean": bn.running_mean, "rvar": bn.running_var}
        if dual:
            got.update({"dxd": xd.grad, "dconv_d": conv_d.weight.grad,
                        "dweight_d": bn_d.weight.grad,
                        "dbias_d": bn_d.bias.grad,
                        "rmean_d": bn_d.running_mean,
                        "rvar_d": bn_d.running_var})
        else:
            got["didentity"] = idt.grad
        assert int(bn.num_batches_tracked) == 1
        assert int(bn_d.num_batches_tracked) == (1 if dual else 0)

        # fp32 eager reference on the same inputs and parameters
        xr = x.detach().float().requires_grad_(True)
        ir = idt.detach().float().requires_grad_(True)
        xdr = xd.detach().float().requires_grad_(True)
        ps = [p.detach().clone().requires_grad_(True) for p in
              (conv.weight, bn.weight, bn.bias, conv_d.weight, bn_d.weight,
               bn_d.bias)]
        cw, w, b, cwd, wd, bd = ps
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        rmd, rvd = rm.clone(), rv.clone()
        branch = F.batch_norm(F.conv2d(xdr, cwd), rmd, rvd, wd, bd, True,
                              MOM, EPS) if dual else ir
        ref_out = torch.relu(F.batch_norm(F.conv2d(xr, cw), rm, rv, w, b,
                                          True, MOM, EPS) + branch)
        ref_out.square().mean().backward()
        ref = {"out": ref_out.detach(), "dx": xr.grad, "dconv": cw.grad,
               "dweight": w.grad, "dbias": b.grad, "rmean": rm, "rvar": rv}
        if dual:
            ref.update({"dxd": xdr.grad, "dconv_d": cwd.grad,
                        "dweight_d": wd.grad, "dbias_d": bd.grad,
                        "rmean_d": rmd, "rvar_d": rvd})
        else:
            ref["didentity"] = ir.grad
        return {k: (got[k], ref[k]) for k in got}
    finally:
        os.environ["DLA_NO_FUSED_JOIN"] = "0"


def _scaled_err(got, ref):
    """Error relative to max|ref| with no floor: the gradients of a mean
    loss are far below 1, and fused and unfused must be compared in the
    quantity's own scale."""
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-12))


@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_join_op_vs_fp32_eager_and_vs_unfused(B, H, W, C, dual):
    fused = _op_case(B, H, W, C, dual, True)
    unfused = _op_case(B, H, W, C, dual, False)
    fwd = ("out", "rmean", "rvar", "rmean_d", "rvar_d")
    for k, (got, ref) in fused.items():
        _assert_close(got, ref, 5e-2 if k in fwd else 8e-2, f"fused {k}")
    for k, (got, ref) in fused.items():
        ef = _scaled_err(got, ref)
        eu = _scaled_err(*unfused[k])
        print(f"{k}: fused err {ef:.4g} unfused err {eu:.4g}")
        assert ef <= 1.5 * eu, \
            f"{k}: fused err {ef:.4g} > 1.5 x unfused err {eu:.4g}"


@pytest.fixture(scope="module")
def bottleneck_runs():
    """resnet50 layer3[0] (dual, stride 2) and layer3[1] (plain, with the
    dgrad-residual route), fused vs DLA_NO_FUSED_JOIN=1."""
    from deeplearning_amd.models import build_model

    def run(fused):
        os.environ["DLA_NO_FUSED_JOIN"] = "0" if fused else "1"
        try:
            torch.manual_seed(7)
            model = build_model("resnet50", num_classes=10).cuda() \
                .to(memory_format=torch.channels_last)
            res = {}
            for idx, cin, hw in ((0, 512, 28), (1, 1024, 14)):
                block = model.layer3[idx]
                x = torch.randn(4, cin, hw, hw, device="cuda") \
                    .to(torch.bfloat16) \
                    .contiguous(memory_format=torch.channels_last) \
                    .requires_grad_(True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = block(x)
                y.float().square().mean().backward()
                r = {"y": y.detach().float(), "dx": x.grad.detach().float(),
                     "dw1": block.conv1.weight.grad.detach().float(),
                     "dw3": block.conv3.weight.grad.detach().float()}
                if block.downsample is not None:
                    r["dwd"] = block.downsample[0].weight.grad.detach().float()
                assert int(block.bn3.num_batches_tracked) == 1
                res[idx] = r
            torch.cuda.synchronize()
            return res
        finally:
            os.environ["DLA_NO_FUSED_JOIN"] = "0"

    return run(True), run(False)


@pytest.mark.parametrize("idx", [0, 1], ids=["layer3_0_dual", "layer3_1_plain"])
def test_bottleneck_fused_vs_unfused(bottleneck_runs, idx):
    fused, unfused = bottleneck_runs
    assert set(fused[idx]) == set(unfused[idx])
    assert ("dwd" in fused[idx]) == (idx == 0)
    for name, got in fused[idx].items():
        ref = unfused[idx][name]
        err = (got - ref).abs().max() / ref.abs().max().clamp(min=1e-3)
        print(f"layer3[{idx}] {name}: rel err {float(err):.4g}")
        assert err < 8e-2, f"layer3[{idx}] {name} rel err {err:.4g}"


def test_pass_through_is_alias_and_tolerates_unused_branches():
    from deeplearning_amd.ops import BatchNorm2d
    from deeplearning_amd.ops.conv1x1 import can_pass_input, conv1x1_bn

    torch.manual_seed(31)
    conv = nn.Conv2d(128, 64, 1, bias=False).cuda()
    bn = BatchNorm2d(64, relu=True).cuda()

    def fresh():
        conv.weight.grad = None
        return _nhwc(3, 128, 5, 9, 32).requires_grad_(True)

    x = fresh()
    assert can_pass_input(x, conv, bn)
    y, alias = conv1x1_bn(x, conv, bn, pass_input=True)
    assert alias.data_ptr() == x.data_ptr() and alias.shape == x.shape
    assert alias.is_contiguous(memory_format=torch.channels_last)
    # identity gradient None: the pass-through output is left unused
    y.float().square().mean().backward()
    dx_unused, dw_unused = x.grad.clone(), conv.weight.grad.clone()

    x = fresh()
    conv1x1_bn(x, conv, bn).float().square().mean().backward()
    # same kernels on both sides; the atomic sums of BN backward and wgrad
    # leave fp32-order noise, at most a bf16 ulp after rounding
    assert _scaled_err(dx_unused, x.grad) < 1e-2
    assert _scaled_err(dw_unused, conv.weight.grad) < 1e-3

    # both branches used: dx = dgrad + identity gradient, in one GEMM
    x = fresh()
    y, alias = conv1x1_bn(x, conv, bn, pass_input=True)
    gi = _nhwc(3, 128, 5, 9, 33, scale=0.01)
    (y.float().square().mean() + (alias.float() * gi.float()).sum()).backward()
    _assert_close(x.grad.float() * 100, (dx_unused.float() + gi.float()) * 100,
                  8e-2, "dx with identity gradient")

    # only the pass-through used: the conv branch's gradient is None
    x = fresh()
    _, alias = conv1x1_bn(x, conv, bn, pass_input=True)
    (alias.float() * gi.float()).sum().backward()
    assert torch.equal(x.grad, gi)
    assert conv.weight.grad is None


def _fallback_case(name):
    from deeplearning_amd.ops import BatchNorm2d

    torch.manual_seed(41)
    cin, C, dtype, nchw, train = 64, 128, torch.bfloat16, False, True
    if name == "c72":
        C = 72
    elif name == "fp32":
        dtype = torch.float32
    elif name == "eval":
        train = False
    elif name == "nchw":
        nchw = True
    conv = nn.Conv2d(cin, C, 1, bias=False).cuda()
    bn = BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    bn.train(train)
    x = torch.randn(3, cin, 5, 9, device="cuda").to(dtype)
    idt = torch.randn(3, C, 5, 9, device="cuda").to(dtype)
    if not nchw:
        x = x.contiguous(memory_format=torch.channels_last)
        idt = idt.contiguous(memory_format=torch.channels_last)
    return conv, bn, x, idt, train


@pytest.mark.parametrize("name", ["c72", "fp32", "eval", "nchw"])
def test_fallbacks_take_the_old_path_and_match_eager(name):
    from deeplearning_amd.ops import conv_bn_add_relu
    from deeplearning_amd.ops.conv1x1 import can_fuse_join

    conv, bn, x, idt, train = _fallback_case(name)
    assert not can_fuse_join(x, conv, bn, identity=idt)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        ref = torch.relu(F.batch_norm(
            F.conv2d(x.float(), conv.weight.float()), rm, rv,
            bn.weight.float(), bn.bias.float(), train, MOM, bn.eps)
            + idt.float())
        with torch.autocast("cuda", dtype=torch.bfloat16,
                            enabled=x.dtype == torch.bfloat16):
            out = conv_bn_add_relu(x, conv, bn, identity=idt)
    assert out.shape == ref.shape and out.dtype == x.dtype
    _assert_close(out, ref, 1e-3 if name == "fp32" else 5e-2,
                  f"fallback {name}")
    _assert_close(bn.running_mean, rm, 5e-2, "running_mean")
    _assert_close(bn.running_var, rv, 5e-2, "running_var")
