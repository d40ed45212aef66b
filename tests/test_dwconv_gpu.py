"""Depthwise conv kernels (csrc/dwconv.hip) on the GPU against
F.conv2d(..., groups=C) in float64 on the CPU and its autograd.

Exact cases: x and dy are integers in -3..3, weights and bias lie on a grid of
1/8 in [-1, 1]. Every product and partial sum is then exactly representable in
fp32 in any summation order (|y| <= 49*3 + 1 in multiples of 1/8, |dW| <=
9*B*OH*OW in integers), so the tolerance is zero: fp32 results equal the fp64
reference bit for bit, bf16/fp16 results equal the reference rounded once to
the storage type.

Rounding cases: |got - ref| <= 2^-8 |ref| + n 2^-23 S element-wise, S the same
convolution / reduction over absolute values and n the number of summed terms
(K^2 for y and dx, B*OH*OW for dW and dbias): one rounding to the bf16 storage
type plus twice the worst-case fp32 summation bound. Results stored in fp32
(gradients of fp32 parameters) have 2^-23 |ref| as the first term.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import deeplearning_amd.ops.dwconv as dw
from deeplearning_amd.models import build_model
from deeplearning_amd.ops import (DepthwiseConv2d, can_use_dwconv,
                                  depthwise_conv2d)
from deeplearning_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

# (B, C, H, W)
# one bf16 vector, H below a 7-tap window, batch stride / three vectors, odd x
# even, longer than a W strip / ConvNeXt's C (not a multiple of 64)
SHAPES_16 = [(3, 8, 5, 9), (2, 24, 17, 16), (2, 96, 12, 10)]
SHAPE_32 = (2, 4, 7, 6)  # the fp32 vector width
# more wgrad partial slabs (17) than finalize row lanes (16)
SHAPE_SLABS = (2, 128, 20, 52)
# fp32: more (b, row, strip) items than the capped forward grid covers in one
# trip, and more than the capped wgrad grid's 512 slabs
SHAPE_STRIDE_LOOP = (4, 64, 128, 260)


@pytest.fixture(autouse=True)
def _route_all(monkeypatch):
    monkeypatch.setenv("DLA_DWCONV", "1")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _exact_case(shape, K, stride, bias):
    """Inputs on the exact grid and the fp64 CPU reference (y, dx, dW, db)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(hash((shape, K, stride)) % (2 ** 31))
    x = torch.randint(-3, 4, shape, generator=g).double()
    w = torch.randint(-8, 9, (C, 1, K, K), generator=g).double() / 8
    b = torch.randint(-8, 9, (C,), generator=g).double() / 8 if bias else None
    leaves = [t.requires_grad_(True) for t in (x, w, b) if t is not None]
    y = F.conv2d(x, w, b, stride, (K - 1) // 2, 1, C)
    dy = torch.randint(-3, 4, y.shape, generator=g).double()
    grads = torch.autograd.grad(y, leaves, dy)
    return (x.detach(), w.detach(), None if b is None else b.detach(), dy,
            y.detach(), grads[0], grads[1], grads[2] if bias else None)


def _run_exact(shape, K, stride, bias, dtype, pdtype):
    x, w, b, dy, y_ref, dx_ref, dw_ref, db_ref = _exact_case(shape, K, stride,
                                                             bias)
    xg = _cl(x.to("cuda", dtype)).requires_grad_(True)
    wg = w.to("cuda", pdtype).requires_grad_(True)
    bg = b.to("cuda", pdtype).requires_grad_(True) if bias else None
    y = depthwise_conv2d(xg, wg, bg, stride=stride)
    assert y.dtype == dtype and y.shape == y_ref.shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(_cl(dy.to("cuda", dtype)))
    assert torch.equal(y.detach().cpu(), y_ref.to(dtype)), "y"
    assert xg.grad.dtype == dtype
    assert torch.equal(xg.grad.cpu(), dx_ref.to(dtype)), "dx"
    assert wg.grad.dtype == pdtype and wg.grad.shape == wg.shape
    assert torch.equal(wg.grad.cpu(), dw_ref.to(pdtype)), "dW"
    if bias:
        assert bg.grad.dtype == pdtype and bg.grad.shape == bg.shape
        assert torch.equal(bg.grad.cpu(), db_ref.to(pdtype)), "dbias"


@pytest.mark.parametrize("pdtype", ["fp32", "same"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES_16, ids=str)
def test_exact_16bit(shape, K, stride, bias, dtype, pdtype):
    _run_exact(shape, K, stride, bias, dtype,
               torch.float32 if pdtype == "fp32" else dtype)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_exact_fp32(K, stride, bias):
    _run_exact(SHAPE_32, K, stride, bias, torch.float32, torch.float32)


@pytest.mark.parametrize("K,stride", [(3, 1), (7, 2)])
def test_exact_many_slabs(K, stride):
    _run_exact(SHAPE_SLABS, K, stride, True, torch.bfloat16, torch.float32)


def test_exact_grid_stride_loop():
    _run_exact(SHAPE_STRIDE_LOOP, 3, 1, True, torch.float32, torch.float32)


# ---- rounding ---------------------------------------------------------------
def _ref64(x, w, b, dy, stride):
    """fp64 CPU conv and gradients of (x, w, b) for upstream dy."""
    C, K = x.shape[1], w.shape[2]
    leaves = [t.detach().double().cpu().requires_grad_(True)
              for t in (x, w, b) if t is not None]
    y = F.conv2d(leaves[0], leaves[1], leaves[2] if b is not None else None,
                 stride, (K - 1) // 2, 1, C)
    grads = torch.autograd.grad(y, leaves, dy.detach().double().cpu())
    return (y.detach(), grads[0], grads[1],
            grads[2] if b is not None else None)


def _check_bound(got, ref, mag, n, name):
    first = 2.0 ** -23 if got.dtype == torch.float32 else 2.0 ** -8
    err = (got.detach().double().cpu() - ref).abs()
    bound = first * ref.abs() + n * 2.0 ** -23 * mag
    worst = float((err - bound).max())
    print(f"{name}: max err {float(err.max()):.4g}, max(err - bound) "
          f"{worst:.4g}")
    assert bool((err <= bound).all()), f"{name}: exceeds bound by {worst:.4g}"


def _check_all(x, w, b, dy, stride, y, dx, dw, db):
    K = w.shape[2]
    y_ref, dx_ref, dw_ref, db_ref = _ref64(x, w, b, dy, stride)
    absb = None if b is None else b.abs()
    y_mag, dx_mag, dw_mag, db_mag = _ref64(x.abs(), w.abs(), absb, dy.abs(),
                                           stride)
    n_red = dy.shape[0] * dy.shape[2] * dy.shape[3]
    _check_bound(y, y_ref, y_mag, K * K, "y")
    _check_bound(dx, dx_ref, dx_mag, K * K, "dx")
    _check_bound(dw, dw_ref, dw_mag, n_red, "dW")
    if b is not None:
        _check_bound(db, db_ref, db_mag, n_red, "dbias")


def _randn_cl(shape, seed, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _cl(torch.randn(shape, device="cuda", generator=g).to(dtype))


@pytest.mark.parametrize("K,stride", [(7, 1), (5, 2)])
def test_rounding_bf16(K, stride):
    B, C, H, W = 2, 24, 17, 16
    x = _randn_cl((B, C, H, W), 1).requires_grad_(True)
    g = torch.Generator(device="cuda").manual_seed(2)
    w = torch.randn(C, 1, K, K, device="cuda", generator=g) \
        .to(torch.bfloat16).requires_grad_(True)
    b = torch.randn(C, device="cuda", generator=g) \
        .to(torch.bfloat16).requires_grad_(True)
    y = depthwise_conv2d(x, w, b, stride=stride)
    dy = _randn_cl(y.shape, 3)
    y.backward(dy)
    assert w.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    _check_all(x, w, b, dy, stride, y, x.grad, w.grad, b.grad)


@pytest.mark.parametrize("K,stride", [(7, 1), (5, 2)])
def test_autocast_fp32_params(K, stride):
    B, C, H, W = 2, 24, 17, 16
    torch.manual_seed(5)
    m = DepthwiseConv2d(C, C, K, stride, (K - 1) // 2, groups=C).cuda()
    with torch.no_grad():
        m.bias.normal_()
    x = _randn_cl((B, C, H, W), 6).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert can_use_dwconv(x, m)
        y = m(x)
    assert y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    dy = _randn_cl(y.shape, 7)
    y.backward(dy)
    assert m.weight.grad.dtype == torch.float32
    assert m.weight.grad.shape == m.weight.shape
    assert m.bias.grad.dtype == torch.float32
    assert m.bias.grad.shape == m.bias.shape
    # the parameters enter the convolution cast to bf16, as autocast casts
    _check_all(x, m.weight.to(torch.bfloat16), m.bias.to(torch.bfloat16), dy,
               stride, y, x.grad, m.weight.grad, m.bias.grad)


def test_wgrad_bit_reproducible():
    x = _randn_cl(SHAPE_SLABS, 8)
    dy = _randn_cl(SHAPE_SLABS, 9)
    dw1, db1 = ext().dwconv_wgrad(dy, x, 7, 1, True)
    dw2, db2 = ext().dwconv_wgrad(dy, x, 7, 1, True)
    assert dw1.dtype == torch.float32 and float(dw1.abs().max()) > 0
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


def test_needs_input_grad():
    C = 24
    m = DepthwiseConv2d(C, C, 3, 1, 1, groups=C).cuda().to(torch.bfloat16)
    x = _randn_cl((2, C, 9, 8), 10)
    assert can_use_dwconv(x, m)
    m(x).float().sum().backward()  # x needs no gradient
    assert x.grad is None and m.weight.grad is not None
    assert m.bias.grad is not None

    m.zero_grad(set_to_none=True)
    m.requires_grad_(False)  # frozen weights
    x.requires_grad_(True)
    m(x).float().sum().backward()
    assert x.grad is not None and m.weight.grad is None
    assert m.bias.grad is None


# ---- routing ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES_16, ids=str)
def test_can_use_supported(shape, K, stride, dtype):
    C = shape[1]
    m = DepthwiseConv2d(C, C, K, stride, (K - 1) // 2, groups=C).cuda()
    assert can_use_dwconv(_randn_cl(shape, 1, dtype), m)
    assert can_use_dwconv(_randn_cl(shape, 1, dtype), m.to(dtype))


def test_can_use_supported_fp32():
    C = SHAPE_32[1]
    m = DepthwiseConv2d(C, C, 3, 1, 1, groups=C).cuda()
    assert can_use_dwconv(_randn_cl(SHAPE_32, 1, torch.float32), m)


def _conv(cin, cout, k, **kw):
    return DepthwiseConv2d(cin, cout, k, bias=False, **kw)


# name -> (module factory, input shape, channels_last input?, DLA_DWCONV)
_UNROUTED = {
    "nchw_input": (lambda: _conv(24, 24, 3, padding=1, groups=24),
                   (2, 24, 9, 8), False, "1"),
    "c12_bf16": (lambda: _conv(12, 12, 3, padding=1, groups=12),
                 (2, 12, 9, 8), True, "1"),
    "dilation2": (lambda: _conv(24, 24, 3, padding=1, dilation=2, groups=24),
                  (2, 24, 9, 8), True, "1"),
    "padding0_k3": (lambda: _conv(24, 24, 3, padding=0, groups=24),
                    (2, 24, 9, 8), True, "1"),
    "k9": (lambda: _conv(24, 24, 9, padding=4, groups=24),
           (2, 24, 9, 8), True, "1"),
    "k3x5": (lambda: _conv(24, 24, (3, 5), padding=(1, 2), groups=24),
             (2, 24, 9, 8), True, "1"),
    "groups_half": (lambda: _conv(24, 24, 3, padding=1, groups=12),
                    (2, 24, 9, 8), True, "1"),
    "cout_2c": (lambda: _conv(24, 48, 3, padding=1, groups=24),
                (2, 24, 9, 8), True, "1"),
    "env_off": (lambda: _conv(24, 24, 3, padding=1, groups=24),
                (2, 24, 9, 8), True, "0"),
}


@pytest.mark.parametrize("case", sorted(_UNROUTED))
def test_unrouted_still_matches_reference(case, monkeypatch):
    make, shape, cl, env = _UNROUTED[case]
    monkeypatch.setenv("DLA_DWCONV", env)
    torch.manual_seed(12)
    m = make().cuda().to(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16)
    x = _cl(x) if cl else x.contiguous()
    assert can_use_dwconv(x, m) is False
    y = m(x)
    xd, wd = (t.detach().double().cpu() for t in (x, m.weight))
    args = (None, m.stride, m.padding, m.dilation, m.groups)
    ref = F.conv2d(xd, wd, *args)
    mag = F.conv2d(xd.abs(), wd.abs(), *args)
    n = m.weight[0].numel()  # summed terms per output
    _check_bound(y, ref, mag, n, case)


# ---- model level ------------------------------------------------------------
def _model_step(model, x, stages, env, monkeypatch):
    monkeypatch.setenv("DLA_DWCONV", env)
    layouts = []
    hooks = [s.register_forward_hook(
        lambda _m, _i, out: layouts.append(
            out.is_contiguous(memory_format=torch.channels_last)))
        for s in stages]
    model.zero_grad(set_to_none=True)
    torch.manual_seed(21)  # drop-path / dropout masks
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(x)
    logits.float().square().mean().backward()
    for h in hooks:
        h.remove()
    grads = {n: p.grad for n, p in model.named_parameters()}
    return logits.detach().float(), layouts, grads


@pytest.mark.parametrize("name,stages_attr", [("convnext_tiny", "stages"),
                                              ("efficientnet_b0", "blocks")])
def test_model_routes_agree(name, stages_attr, monkeypatch):
    """One train step per route from the same seed: stage outputs stay
    channels_last, logits agree within 5e-2 of max|ref|, gradients are finite.

    efficientnet_b0 misses the logit bound at this batch and is left failing:
    with 2 x 2x2 = 8 samples per channel in the last BatchNorms the train-mode
    network amplifies one-ulp bf16 differences. Measured on an MI355X, same
    weights, input and seed: DLA_DWCONV=1 against =0 gave 0.10, 0.078 and
    0.055 in three processes, while =0 against a second run of =0 gave 0.055
    (the BatchNorm sums are float atomics) and either bf16 route is 0.7 away
    from the fp32 run. The routes themselves agree: 6.9e-6 in fp32 train mode,
    bit-identical logits in bf16 eval mode, and the batch-64 train loss is the
    same to four digits (profiles/dwconv_model_ab.txt). convnext_tiny
    (LayerNorm) gives 5.7e-3.
    """
    # other tests leave cudnn.benchmark on for the whole session; keep this
    # one on the library's default algorithm choice, whatever ran before it
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    torch.manual_seed(20)
    model = build_model(name, num_classes=10).cuda() \
        .to(memory_format=torch.channels_last).train()
    stages = list(getattr(model, stages_attr))
    x = _randn_cl((2, 3, 64, 64), 22, torch.float32)

    routed = []  # one entry per forward that took the HIP route

    class _Counting:
        def __getattr__(self, attr):
            if attr == "dwconv_fwd":
                routed.append(1)
            return getattr(ext(), attr)

    monkeypatch.setattr(dw, "ext", lambda: _Counting())
    got, lay1, grads1 = _model_step(model, x, stages, "1", monkeypatch)
    n_routed = len(routed)
    ref, lay0, _ = _model_step(model, x, stages, "0", monkeypatch)
    assert n_routed > 0 and len(routed) == n_routed

    assert len(lay1) == len(stages) and all(lay1), lay1
    assert len(lay0) == len(stages) and all(lay0), lay0
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{name}: {n_routed} routed convs, logits rel err {err:.4g}")
    assert err < 5e-2
    for n, g in grads1.items():
        assert g is not None and bool(torch.isfinite(g).all()), n
