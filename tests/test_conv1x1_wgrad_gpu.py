"""Tests for the atomic-free 1x1-conv weight-gradient kernel
(conv1x1_wgrad2_kernel in csrc/conv1x1.hip), called through
ext().conv1x1_wgrad on seeded bf16 inputs of unit scale.

Reference: dy.double().t() @ x.double(). Products of bf16 values are exact
in fp32, so the only error is the order of the fp32 summation; the bound is
elementwise |dw - ref| <= 2 * M * 2^-24 * (|dy|^T |x|), twice the standard
gamma_M bound to cover the MFMA's undocumented internal accumulation.
"""
import functools

import pytest
import torch

from deeplearning_amd.ops._ext import ext

gpu = pytest.mark.gpu

# (M, K, N): which tile instantiation <BCO over N, BCI over K> and which
# split path each shape is for
SHAPES = [
    (49, 64, 64),        # <64,64>, 1 split: fewer rows than one 64-row step
    (64, 64, 64),        # <64,64>, 1 split: exactly one step, no tail
    (300, 192, 128),     # <128,64>, 1 split: full steps then a 44-row tail
    (1000, 128, 192),    # <64,128>, 3 splits: N % 128 != 0, tail in a step;
                         # finalize with 1 split group
    (6152, 64, 256),     # <128,64>, 2 tiles x 20 splits, ragged last chunk
                         # of 72 rows; finalize with 4 split groups
    (6152, 256, 64),     # <64,128>, same the other way round
    (4096 + 8, 256, 256),  # <128,128>, 4 tiles x 8 splits, last chunk 72
                           # rows; finalize with 2 split groups
]
MULTI_SPLIT = (6152, 64, 256)
SINGLE_SPLIT = (300, 192, 128)


@functools.lru_cache(maxsize=None)
def _inputs(m, k, n):
    """Seeded CPU bf16 (dy [m,n], x [m,k]); shared, never modified."""
    g = torch.Generator().manual_seed(1000 * m + k + n)
    dy = torch.randn(m, n, generator=g).to(torch.bfloat16)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    return dy, x


def _ref_and_bound(dy, x):
    m = dy.shape[0]
    ref = dy.double().t() @ x.double()
    bound = 2.0 * m * 2.0 ** -24 * (dy.double().abs().t() @ x.double().abs())
    return ref, bound


@functools.lru_cache(maxsize=None)
def _gpu_case(m, k, n):
    dy, x = _inputs(m, k, n)
    dy, x = dy.cuda(), x.cuda()
    return (dy, x) + _ref_and_bound(dy, x)


def _check(dw, ref, bound, what):
    assert dw.dtype == torch.float32 and dw.shape == ref.shape
    assert torch.isfinite(dw).all(), f"{what}: non-finite dW"
    ratio = ((dw.double() - ref).abs() / bound).max().item()
    print(f"{what}: max |dw-ref|/bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f}x the bound"


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_dropped_row_exceeds_bound_cpu(m, k, n):
    """The bound is tight enough to catch a dropped (or doubled) row: zeroing
    one row of x moves the reference by more than the bound somewhere."""
    dy, x = _inputs(m, k, n)
    ref, bound = _ref_and_bound(dy, x)
    for r in (0, m // 2, m - 1):
        x0 = x.clone()
        x0[r] = 0
        moved = (dy.double().t() @ x0.double() - ref).abs()
        assert (moved / bound).max().item() > 1.0, f"row {r}"


@gpu
@pytest.mark.parametrize("m,k,n", SHAPES)
def test_wgrad_within_summation_bound(m, k, n):
    dy, x, ref, bound = _gpu_case(m, k, n)
    _check(ext().conv1x1_wgrad(dy, x), ref, bound, f"wgrad {m}x{k}x{n}")


@gpu
@pytest.mark.parametrize("m,k,n", SHAPES)
def test_wgrad_never_reads_past_m(m, k, n):
    """NaN rows directly behind the M rows passed in must not be read."""
    dy, x, ref, bound = _gpu_case(m, k, n)
    dyp = torch.full((m + 64, n), float("nan"), device="cuda",
                     dtype=torch.bfloat16)
    xp = torch.full((m + 64, k), float("nan"), device="cuda",
                    dtype=torch.bfloat16)
    dyp[:m] = dy
    xp[:m] = x
    assert dyp[:m].is_contiguous() and xp[:m].is_contiguous()
    _check(ext().conv1x1_wgrad(dyp[:m], xp[:m]), ref, bound,
           f"NaN tail {m}x{k}x{n}")


@gpu
@pytest.mark.parametrize("m,k,n", [MULTI_SPLIT, SINGLE_SPLIT])
def test_wgrad_bit_reproducible(m, k, n):
    dy, x, _, _ = _gpu_case(m, k, n)
    a = ext().conv1x1_wgrad(dy, x)
    b = ext().conv1x1_wgrad(dy, x)
    assert torch.equal(a, b)


@gpu
def test_wgrad_v1_switch(monkeypatch):
    """DLA_C1X1_WGRAD_V1=1 routes to the old atomicAdd kernel, which meets
    the same bound."""
    m, k, n = MULTI_SPLIT
    dy, x, ref, bound = _gpu_case(m, k, n)
    monkeypatch.setenv("DLA_C1X1_WGRAD_V1", "1")
    _check(ext().conv1x1_wgrad(dy, x), ref, bound, "v1 route")


@gpu
def test_autograd_weight_grad():
    """_Conv1x1Fn at N=2, C=64->128, 9x9 channels-last (M = 162 rows): the
    weight gradient against fp32 autograd, by the rule of
    test_conv1x1_gpu.test_autograd_function_end_to_end."""
    from deeplearning_amd.ops.conv1x1 import _Conv1x1Fn, _flatten_nhwc

    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, 64, 9, 9, device="cuda", generator=g) \
        .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = torch.randn(128, 64, device="cuda", generator=g,
                    requires_grad=True)
    x2d = _flatten_nhwc(x)
    y = _Conv1x1Fn.apply(x2d, w, None, None, None, None, False, False)
    (y.float() ** 2).mean().backward()

    w32 = w.detach().clone().requires_grad_(True)
    yr = x2d.float() @ w32.t()
    (yr ** 2).mean().backward()
    assert w.grad.dtype == torch.float32
    denom = w32.grad.abs().max().clamp(min=1.0)
    err = ((w.grad - w32.grad).abs().max() / denom).item()
    assert err < 4e-2, f"wgrad rel err {err:.4g}"
