"""BN backward pass 1 inside the conv1x1 dgrad epilogue: the entry points,
two chained Bottlenecks with and without DLA_NO_BWD_STATS_EPILOGUE=1, and the
cases that must land on the two-pass route.

References and tolerances are those of tests/test_join_fusion_gpu.py: fp32
eager autograd, gradients within 8e-2 of max|ref|, and the new route's error
at most 1.5 x the two-pass route's error against the same reference. Upstream
gradients fade to zero where the pre-activation crosses zero (_smooth_dy), so
a mask bit decided in the last ulp cannot move a result.
"""
import gc
import os
import weakref

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from deeplearning_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

RELU_X, JOIN, JOIN_DUAL = 1, 2, 3
MODES = {"relu_x": RELU_X, "join": JOIN, "join_dual": JOIN_DUAL}
# M = 98 (less than one 128-row block) / 135 (tail rows) / 392 (several)
BHW = [(2, 7, 7), (3, 5, 9), (2, 14, 14)]
# dgrad (K, N): BN=64 / BN=64 deep K / BN=128 BK=32 / BN=128 BK=64 / BN=256
KN = [(64, 64), (256, 64), (128, 128), (256, 128), (64, 256)]
EPS, MOM = 1e-5, 0.1
ENV = "DLA_NO_BWD_STATS_EPILOGUE"


def _nhwc(B, C, H, W, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(B, C, H, W, device="cuda", generator=g) * scale + shift
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _affine(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.rand(C, device="cuda", generator=g) + 0.5
    b = torch.randn(C, device="cuda", generator=g) * 0.2
    return w, b


def _slab(x, parts):
    rows = _rows(x).float()
    return torch.stack([torch.cat([c.sum(0), (c * c).sum(0)])
                        for c in torch.tensor_split(rows, parts)]).contiguous()


def _scaled_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-12))


def _entry_case(mode, B, H, W, K, N):
    """Forward of the producer through the extension, then the dgrad GEMM
    today's way (plain output + the producer's two-pass backward) and the new
    way (epilogue + dx-only entry) on the same inputs."""
    e = ext()
    M = B * H * W
    x = _nhwc(B, N, H, W, 1, scale=1.5, shift=0.3)
    xd = _nhwc(B, N, H, W, 2, scale=2.0 if mode == JOIN_DUAL else 1.0,
               shift=-0.2)
    w, b = _affine(N, 3)
    wd, bd = _affine(N, 4)
    rm, rv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    if mode == RELU_X:
        out, mean, rstd, scale, shift = e.batchnorm_fwd(
            x, w, b, rm, rv, MOM, EPS, True)
        pre = x.float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        # the kernels mask from bn_pre(x) > 0, which is out > 0 for every
        # pre-activation above bf16's smallest subnormal
        mask = out > 0
    elif mode == JOIN:
        out, mean, rstd = e.bn_add_relu_fwd_from_sums(
            x, w, b, _slab(x, 5), rm, rv, MOM, EPS, xd)
        pre = F.batch_norm(x.float(), None, None, w, b, True, MOM, EPS) + \
            xd.float()
        mask = out > 0
    else:
        out, mean, rstd, mean_d, rstd_d = e.bn_add_relu_dual_fwd_from_sums(
            x, w, b, _slab(x, 5), rm, rv, MOM, EPS, xd, wd, bd, _slab(xd, 3),
            rm.clone(), rv.clone(), MOM, EPS)
        pre = F.batch_norm(x.float(), None, None, w, b, True, MOM, EPS) + \
            F.batch_norm(xd.float(), None, None, wd, bd, True, MOM, EPS)
        mask = out > 0
    frac = float((~mask).float().mean())
    assert 0.3 < frac < 0.7, f"mask should be 30-70 % zero, got {frac}"

    # dgrad operands: a smooth gradient for the GEMM to reproduce in the
    # mean (dy @ wt ~ fade * noise), an identity gradient as the residual
    gen = torch.Generator(device="cuda").manual_seed(5)
    fade = _rows(pre.abs().clamp(max=1.0))
    dy = (torch.randn(M, K, device="cuda", generator=gen)).to(torch.bfloat16)
    wt = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5) \
        .to(torch.bfloat16)
    res = (torch.randn(M, N, device="cuda", generator=gen) * fade) \
        .to(torch.bfloat16)
    residual = res if mode != RELU_X else None

    plain, _ = e.conv1x1_fwd(dy, wt, None, None, None, residual, False, False)
    plain4 = plain.view(B, H, W, N).permute(0, 3, 1, 2)

    def fused():
        return e.conv1x1_dgrad_bwdstats(
            dy, wt, residual, mode, None if mode == RELU_X else out, x,
            scale if mode == RELU_X else None,
            shift if mode == RELU_X else None, mean, rstd,
            xd if mode == JOIN_DUAL else None,
            mean_d if mode == JOIN_DUAL else None,
            rstd_d if mode == JOIN_DUAL else None)

    g, slab = fused()
    g2, slab2 = fused()
    g4 = g.view(B, H, W, N).permute(0, 3, 1, 2)
    r = {"g": g, "g_ref": torch.where(_rows(mask), plain,
                                     torch.zeros_like(plain)),
         "slab": slab, "slab2": slab2, "g2": g2, "x": x, "xd": xd,
         "mean": mean, "rstd": rstd}
    if mode == RELU_X:
        r["old"] = e.batchnorm_bwd_ex(plain4, x, None, w, mean, rstd, scale,
                                      shift, True)
        r["new"] = e.bn_bwd_dx_from_slab(g4, slab, x, w, mean, rstd)
    elif mode == JOIN:
        r["old"] = e.bn_add_relu_bwd(plain4, out, x, w, mean, rstd)[1:]
        r["new"] = e.bn_bwd_dx_from_slab(g4, slab, x, w, mean, rstd)
    else:
        r["mean_d"], r["rstd_d"] = mean_d, rstd_d
        r["old"] = e.bn_add_relu_dual_bwd(plain4, out, x, w, mean, rstd, xd,
                                          wd, mean_d, rstd_d)
        r["new"] = e.bn_join_dual_bwd_dx_from_slab(
            g4, slab, x, w, mean, rstd, xd, wd, mean_d, rstd_d)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("B,H,W", BHW)
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_entry_points(mode, B, H, W, K, N):
    m = MODES[mode]
    r = _entry_case(m, B, H, W, K, N)
    M = B * H * W
    ns = 3 if m == JOIN_DUAL else 2
    assert r["slab"].shape == ((M + 127) // 128, ns * N)
    # g is today's dgrad output under the mask, bit for bit
    assert torch.equal(r["g"], r["g_ref"])
    # two calls: identical bits
    assert torch.equal(r["g"], r["g2"])
    assert torch.equal(r["slab"], r["slab2"])
    sums = ext().bn_slab_reduce(r["slab"])
    assert torch.equal(sums, ext().bn_slab_reduce(r["slab2"]))

    # sums against fp64 over that g; today's pass-1 sums (dbias = sum g and
    # dweight = sum g*xhat of the two-pass entry) set the error allowed
    g64 = r["g"].double()
    xh = (_rows(r["x"]).double() - r["mean"].double()) * r["rstd"].double()
    ref = [g64.sum(0), (g64 * xh).sum(0)]
    old = [r["old"][-1 if m != JOIN_DUAL else 3],
           r["old"][-2 if m != JOIN_DUAL else 2]]
    if m == JOIN_DUAL:
        xhd = (_rows(r["xd"]).double() - r["mean_d"].double()) * \
            r["rstd_d"].double()
        ref.append((g64 * xhd).sum(0))
        old.append(r["old"][4])
    for s, (want, was) in enumerate(zip(ref, old)):
        got = sums[s * N:(s + 1) * N]
        e_new, e_old = _scaled_err(got, want), _scaled_err(was, want)
        print(f"sum {s}: epilogue err {e_new:.3g} two-pass err {e_old:.3g}")
        assert e_new <= 1.5 * e_old, \
            f"sum {s}: err {e_new:.3g} > 1.5 x two-pass err {e_old:.3g}"

    # dx-only entry against the two-pass entry on the same inputs: the same
    # dx kernel on the same g, with sums that differ in fp32 order only, so
    # a result may move by one bf16 rounding (2^-7 relative to max|dx|)
    assert len(r["new"]) == len(r["old"])
    for i, (got, was) in enumerate(zip(r["new"], r["old"])):
        err = _scaled_err(got, was)
        print(f"output {i}: rel diff {err:.3g}")
        assert got.shape == was.shape and got.dtype == was.dtype
        assert err <= 2.0 ** -7, f"output {i}: rel diff {err:.3g}"


def test_deep_slab_reduce_is_fixed_order_and_exact_enough():
    """A slab deeper than the single-stage reduce (two stages) against fp64,
    bit-identical across calls, with a ragged last group."""
    g = torch.Generator(device="cuda").manual_seed(9)
    for parts, cols in ((513, 192), (1568, 128), (700, 72)):
        slab = torch.randn(parts, cols, device="cuda", generator=g)
        a = ext().bn_slab_reduce(slab)
        b = ext().bn_slab_reduce(slab)
        assert torch.equal(a, b)
        ref = slab.double().sum(0)
        # fp32 sums of `parts` unit normals: error far below parts * 2^-24
        # * sqrt(parts); allow that bound
        bound = parts ** 1.5 * 2.0 ** -24
        assert float((a.double() - ref).abs().max()) < bound


# ---- two chained Bottlenecks ------------------------------------------------

class _GradTap:
    """Records the gradient tensors the join backward entries receive or
    return as g, without touching them."""

    def __init__(self):
        self.names = ("bn_add_relu_bwd", "bn_add_relu_dual_bwd",
                      "bn_bwd_dx_from_slab", "bn_join_dual_bwd_dx_from_slab")
        self.calls = []

    def __enter__(self):
        e = ext()
        self.orig = {n: getattr(e, n) for n in self.names}
        for n in self.names:
            def wrap(*a, _n=n):
                outs = self.orig[_n](*a)
                self.calls.append((_n, a[0].detach().clone(),
                                   [o.detach().clone() for o in outs]))
                return outs
            setattr(e, n, wrap)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(ext(), n, f)


def _set_env(off):
    os.environ[ENV] = "1" if off else "0"


def _chain_run(off, mutate=None, backwards=1, relu_x=False):
    """layer3[0:3] of resnet50 at batch 4: a dual join into a plain block and
    a plain join into another plain block. relu_x also routes the opt-in
    bn2 <- conv3 dgrad mode."""
    from deeplearning_amd.models import build_model

    _set_env(off)
    os.environ["DLA_BWD_STATS_RELU_X"] = "1" if relu_x else "0"
    # The library 3x3 convs are not reproducible run to run by default: two
    # runs of the two-pass route alone then sit up to 7.6e-2 apart (y 3e-3),
    # two of the new route 1.8e-1. With deterministic algorithms the two-pass
    # route repeats bit for bit and the comparison sees the routes only.
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(7)
        model = build_model("resnet50", num_classes=10).cuda() \
            .to(memory_format=torch.channels_last)
        blocks = model.layer3[0:3]
        x = torch.randn(4, 512, 28, 28, device="cuda").to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with _GradTap() as tap:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if mutate is None:
                    y = blocks(x)
                    extra = 0.0
                else:
                    y, extra = mutate(blocks, x)
            loss = y.float().square().mean() + extra
            grads = []
            for i in range(backwards):
                for p in blocks.parameters():
                    p.grad = None
                x.grad = None
                loss.backward(retain_graph=i + 1 < backwards)
                r = {"y": y.detach().float(), "dx": x.grad.detach().float()}
                for n, p in blocks.named_parameters():
                    r["d" + n] = p.grad.detach().float()
                grads.append(r)
        torch.cuda.synchronize()
        return grads, tap.calls
    finally:
        _set_env(False)
        os.environ.pop("DLA_BWD_STATS_RELU_X")
        torch.backends.cudnn.deterministic = det


def _chain_ref():
    """fp32 eager run of the same blocks on the same input and weights."""
    from deeplearning_amd.models import build_model

    os.environ["DLA_FORCE_EAGER"] = "1"
    try:
        torch.manual_seed(7)
        model = build_model("resnet50", num_classes=10).cuda()
        blocks = model.layer3[0:3].float()
        x = torch.randn(4, 512, 28, 28, device="cuda").to(torch.bfloat16) \
            .float().requires_grad_(True)
        y = blocks(x)
        y.square().mean().backward()
        r = {"y": y.detach(), "dx": x.grad.detach()}
        for n, p in blocks.named_parameters():
            r["d" + n] = p.grad.detach()
        return r
    finally:
        os.environ["DLA_FORCE_EAGER"] = "0"


@pytest.fixture(scope="module")
def warm():
    """One uncounted run, so that no compared run is the first to meet a
    library conv shape."""
    _chain_run(True)


@pytest.fixture(scope="module")
def chain(warm):
    on, on_calls = _chain_run(False)
    off, off_calls = _chain_run(True)
    return on[0], on_calls, off[0], off_calls, _chain_ref()


def _short_calls(calls):
    return [c[0] for c in calls if c[0].endswith("from_slab")]


def test_chain_takes_the_short_route(chain):
    on, on_calls, off, off_calls, _ = chain
    # the joins of blocks 0 (dual) and 1 (the join of block 2 ends the
    # chain: its gradient comes from the loss)
    assert sorted(_short_calls(on_calls)) == [
        "bn_bwd_dx_from_slab", "bn_join_dual_bwd_dx_from_slab"]
    assert _short_calls(off_calls) == []


def test_chain_with_relu_x_mode(chain):
    """DLA_BWD_STATS_RELU_X=1 adds bn2 of the three blocks."""
    off = chain[2]
    on, on_calls = _chain_run(False, relu_x=True)
    names = _short_calls(on_calls)
    assert names.count("bn_bwd_dx_from_slab") == 4 and \
        names.count("bn_join_dual_bwd_dx_from_slab") == 1, names
    for name in off:
        err = _scaled_err(on[0][name], off[name])
        print(f"{name}: rel diff {err:.4g}")
        assert err < 8e-2, f"{name}: rel diff {err:.4g}"


def test_chain_matches_switched_off_run(chain):
    on, on_calls, off, off_calls, _ = chain
    assert set(on) == set(off)
    for name in on:
        err = _scaled_err(on[name], off[name])
        print(f"{name}: rel diff {err:.4g}")
        assert err < 8e-2, f"{name}: rel diff {err:.4g}"
    # the g tensors are equal: what the short route consumed for block 1's
    # join is what pass 1 of the two-pass route wrote for it (the dgrad
    # operands are the same bits in both runs: everything upstream of block
    # 2's conv1 dgrad runs the same kernels)
    g_off_single = [outs[0] for n, first, outs in off_calls
                    if n == "bn_add_relu_bwd"]
    joins_on = [first for n, first, outs in on_calls
                if n == "bn_bwd_dx_from_slab"]
    # switched off, the join backwards run for blocks 2, 1, 0 in that order
    assert len(joins_on) == 1 and len(g_off_single) == 2
    g_new, g_old = joins_on[0], g_off_single[1]
    frac = float((g_old == 0).float().mean())
    assert 0.3 < frac < 0.7, f"mask should be 30-70 % zero, got {frac}"
    assert torch.equal(g_new, g_old)


def test_chain_error_against_fp32_eager(chain):
    on, _, off, _, ref = chain
    for name in ref:
        e_on, e_off = _scaled_err(on[name], ref[name]), \
            _scaled_err(off[name], ref[name])
        print(f"{name}: epilogue err {e_on:.4g} two-pass err {e_off:.4g}")
        assert e_on <= 1.5 * e_off, \
            f"{name}: err {e_on:.4g} > 1.5 x two-pass err {e_off:.4g}"


# ---- fallbacks --------------------------------------------------------------

def _second_consumer(blocks, x):
    mid = blocks[0](x)
    y = blocks[2](blocks[1](mid))
    return y, mid.float().mean() * 0.01


def _hook_new_tensor(blocks, x):
    mid = blocks[0](x)
    mid.register_hook(lambda g: g.clone())
    return blocks[2](blocks[1](mid)), 0.0


@pytest.mark.parametrize("mutate", [_second_consumer, _hook_new_tensor],
                         ids=["second_consumer", "hook_new_tensor"])
def test_join_output_used_twice_or_hooked_takes_two_passes(warm, mutate):
    on, on_calls = _chain_run(False, mutate)
    off, _ = _chain_run(True, mutate)
    # block 0's (dual) join must not have taken the short route
    assert "bn_join_dual_bwd_dx_from_slab" not in _short_calls(on_calls)
    assert any(c[0] == "bn_add_relu_dual_bwd" for c in on_calls)
    for name in on[0]:
        err = _scaled_err(on[0][name], off[0][name])
        assert err < 8e-2, f"{name}: rel diff {err:.4g}"


def test_retain_graph_two_backwards(warm):
    on, on_calls = _chain_run(False, backwards=2)
    off, _ = _chain_run(True, backwards=2)
    for i in range(2):
        for name in on[i]:
            err = _scaled_err(on[i][name], off[i][name])
            assert err < 8e-2, f"backward {i} {name}: rel diff {err:.4g}"
    # the second backward found the links empty
    assert len(_short_calls(on_calls)) == 2


@pytest.mark.parametrize("name", ["eval", "fp32", "nchw", "c72"])
def test_unsupported_cases_attach_nothing_and_match(name):
    from deeplearning_amd.ops import BatchNorm2d, conv_bn_add_relu

    def run(off):
        _set_env(off)
        try:
            torch.manual_seed(41)
            C = 72 if name == "c72" else 128
            dtype = torch.float32 if name == "fp32" else torch.bfloat16
            conv = nn.Conv2d(64, C, 1, bias=False).cuda()
            bn = BatchNorm2d(C).cuda()
            bn.train(name != "eval")
            x = torch.randn(3, 64, 5, 9, device="cuda").to(dtype)
            idt = torch.randn(3, C, 5, 9, device="cuda").to(dtype)
            if name != "nchw":
                x = x.contiguous(memory_format=torch.channels_last)
                idt = idt.contiguous(memory_format=torch.channels_last)
            x.requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16,
                                enabled=dtype == torch.bfloat16):
                out = conv_bn_add_relu(x, conv, bn, identity=idt)
            assert getattr(out, "_dla_bwd_link", None) is None
            out.float().square().mean().backward()
            return out.detach().float(), x.grad.float(), \
                conv.weight.grad.float()
        finally:
            _set_env(False)

    for a, b in zip(run(False), run(True)):
        # the same kernels both times; NCHW BatchNorm sums with atomics
        assert _scaled_err(a, b) < (1e-5 if name == "fp32" else 2.0 ** -7)


def test_link_holds_no_tensor_after_backward_and_none_without_grad():
    from deeplearning_amd.models import build_model

    _set_env(False)
    torch.manual_seed(3)
    model = build_model("resnet50", num_classes=10).cuda() \
        .to(memory_format=torch.channels_last)
    blocks = model.layer3[1:3]
    x = torch.randn(2, 1024, 14, 14, device="cuda").to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        mid = blocks[0](x)
    assert getattr(mid, "_dla_bwd_link", None) is None

    x.requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        mid = blocks[0](x)
        link = mid._dla_bwd_link
        x_raw_ref = weakref.ref(link.operands["x_raw"])
        y = blocks[1](mid)
    y.float().square().mean().backward()
    assert link.operands is None and link.g is None and link.slab is None
    del mid, y
    gc.collect()
    assert x_raw_ref() is None
