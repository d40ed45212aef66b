"""Fused per-pixel cross-entropy (csrc/dense_ce.hip) against an fp64 CPU
reference computed from the exact (upcast) input values.

Tolerances (derived, not tuned):
  - losses, any input dtype: the inputs upcast exactly and the arithmetic is
    fp32, so rtol = atol = 1e-5, the project's fp32 CE tolerance.
  - gradients, elementwise: atol = 1e-5 * max|ref|; rtol = 1e-5 for fp32 and
    one output ulp with a factor of two for the 16-bit types (2^-7 bf16,
    2^-10 fp16). Below the output type's smallest normal the ulp no longer
    shrinks with the value (fp16: 2^-24 under 2^-14), so the relative term is
    taken of max(|ref|, smallest normal). This matters for fp16 only: a `mean`
    gradient over 3x64x64 pixels is ~4e-4 * softmax, mostly fp16 subnormals,
    where correct rounding alone is up to 2^-25 off: 6.9x the bound without
    that floor (measured, nchw 64x64 C=2 fp16 mean), 0.5x with it.
Labels outside [0, C) are remapped to ignore_index before the reference call:
the fused op counts them as ignored, the eager GPU op would device-assert.
"""
import pytest
import torch
import torch.nn.functional as F

from deeplearning_amd import ops
from deeplearning_amd.engine.cli_seg import seg_criterion
from deeplearning_amd.models.segmentation import OhemCrossEntropy

pytestmark = pytest.mark.gpu

IGNORE = 255
LOSS_TOL = 1e-5
GRAD_RTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -7,
             torch.float16: 2.0 ** -10}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
FN_NAME = "_DenseCEFnBackward"


# ---- inputs and reference ------------------------------------------------------
def make_inputs(B, C, spatial, dtype, seed=0, scale=3.0):
    """CPU logits in `dtype`, target with ~30 % ignore_index and a few labels
    at -1, C and 254, and a per-class weight."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, C, *spatial, generator=g) * scale).to(dtype)
    target = torch.randint(0, C, (B, *spatial), generator=g)
    target[torch.rand(B, *spatial, generator=g) < 0.3] = IGNORE
    flat = target.view(-1)
    n = flat.numel()
    for k, bad in enumerate((-1, C, 254)):
        flat[(7 + 13 * k) % n] = bad
        flat[(n - 3 - 5 * k) % n] = bad
    weight = torch.rand(C, generator=g) + 0.5
    return logits, target, weight


def reference(logits, target, weight, reduction, gout=None, mult=1.0):
    """fp64 CPU loss and dlogits; gout is the per-pixel upstream grad of
    `none`, mult the factor applied to a reduced loss before backward."""
    C = logits.shape[1]
    z = logits.detach().cpu().double().requires_grad_()
    t = target.detach().cpu().clone()
    t[(t < 0) | (t >= C)] = IGNORE
    w = None if weight is None else weight.detach().cpu().double()
    if reduction == "mean":
        valid = t != IGNORE
        denom = (w[t[valid]].sum() if w is not None else valid.sum())
        if float(denom) == 0:  # the op's convention: 0, not NaN
            return torch.zeros((), dtype=torch.float64), torch.zeros_like(z)
    loss = F.cross_entropy(z, t, weight=w, ignore_index=IGNORE,
                           reduction=reduction)
    if reduction == "none":
        loss.backward(gout.detach().cpu().double())
    else:
        (loss * mult).backward()
    return loss.detach(), z.grad


def to_layout(x, layout):
    """Move CPU logits to the GPU in the requested memory layout."""
    x = x.cuda()
    if layout == "nchw":
        return x.contiguous()
    if layout == "cl":
        return x.contiguous(memory_format=torch.channels_last)
    raise ValueError(layout)


def same_format(grad, x):
    return grad.dtype == x.dtype and grad.shape == x.shape and (
        grad.stride() == x.stride() or not _dense(x))


def _dense(x):
    return x.is_contiguous() or (
        x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))


def assert_loss(got, ref, what):
    assert got.dtype == torch.float32, what
    assert torch.isfinite(got).all(), what
    err = (got.detach().cpu().double() - ref).abs()
    bound = LOSS_TOL + LOSS_TOL * ref.abs()
    print(f"{what}: loss max err {float(err.max()):.3e} "
          f"(bound at it {float(bound.flatten()[err.argmax()]):.3e})")
    assert bool((err <= bound).all()), what


def assert_grad(got, ref, dtype, what):
    assert torch.isfinite(got).all(), what
    err = (got.detach().cpu().double() - ref).abs()
    floor = torch.finfo(dtype).smallest_normal
    bound = (1e-5 * ref.abs().max()
             + GRAD_RTOL[dtype] * ref.abs().clamp(min=floor))
    print(f"{what}: grad max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


def run_all_reductions(x_cpu, x_gpu_src, target, weight, what):
    """none (random upstream grad), sum, mean and weighted mean (x 3.7) on
    x_gpu_src; x_cpu holds the same values for the reference."""
    tg = target.cuda()
    wg = weight.cuda()
    dtype = x_gpu_src.dtype
    g = torch.Generator().manual_seed(11)
    gout = torch.randn(target.shape, generator=g)
    for reduction, w, mult in (("none", None, 1.0), ("sum", None, 1.0),
                               ("mean", None, 3.7), ("mean", weight, 3.7),
                               ("none", weight, 1.0)):
        x = x_gpu_src.detach().requires_grad_()
        loss = ops.dense_cross_entropy(
            x, tg, weight=None if w is None else wg, ignore_index=IGNORE,
            reduction=reduction)
        assert type(loss.grad_fn).__name__ == FN_NAME
        ref_loss, ref_grad = reference(x_cpu, target, w, reduction, gout, mult)
        tag = f"{what} {reduction}{' weighted' if w is not None else ''}"
        assert loss.shape == ref_loss.shape, tag
        assert_loss(loss, ref_loss, tag)
        if reduction == "none":
            loss.backward(gout.cuda())
        else:
            (loss * mult).backward()
        assert same_format(x.grad, x), tag
        assert_grad(x.grad, ref_grad, dtype, tag)


# ---- the layout x shape x class-count x dtype matrix ---------------------------
# 7x9: under one wave, odd, no vector alignment. 17x23: several waves with a
# tail, misaligned planes. 64x64: aligned fast path, several blocks, a
# multi-row slab. C: even and odd LDS row strides.
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [2, 5, 19, 21, 32, 33])
@pytest.mark.parametrize("spatial", [(7, 9), (17, 23), (64, 64)],
                         ids=["7x9", "17x23", "64x64"])
@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_matches_reference(layout, spatial, C, dtype):
    logits, target, weight = make_inputs(3, C, spatial, dtype)
    run_all_reductions(logits, to_layout(logits, layout), target, weight,
                       f"{layout} {spatial} C={C} {dtype}")


# 8- and 4-byte NCHW accesses: P = 4 * odd (8 B for bf16, 16 B for fp32) and
# P = 2 * odd (4 B for bf16, 8 B for fp32)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("spatial", [(4, 23), (2, 23)], ids=["4x23", "2x23"])
def test_nchw_narrower_vectors(spatial, dtype):
    logits, target, weight = make_inputs(3, 5, spatial, dtype, seed=2)
    run_all_reductions(logits, logits.cuda(), target, weight,
                       f"nchw {spatial} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("L", [391, 64])
def test_3d_logits(L, dtype):
    logits, target, weight = make_inputs(3, 5, (L,), dtype, seed=3)
    run_all_reductions(logits, logits.cuda(), target, weight, f"3d L={L}")


def test_nchw_many_classes():
    logits, target, weight = make_inputs(3, 300, (7, 9), torch.bfloat16, seed=4)
    run_all_reductions(logits, logits.cuda(), target, weight, "nchw C=300")


# channels_last tiles of 64 and 128 pixels, and the tile above 64 KiB of LDS
@pytest.mark.parametrize("C,dtype", [(150, torch.bfloat16), (64, torch.float32),
                                     (255, torch.float32), (256, torch.float32),
                                     (256, torch.float16)],
                         ids=["150bf16", "64fp32", "255fp32", "256fp32",
                              "256fp16"])
def test_channels_last_wide_rows(C, dtype):
    logits, target, weight = make_inputs(3, C, (17, 23), dtype, seed=5)
    run_all_reductions(logits, to_layout(logits, "cl"), target, weight,
                       f"cl C={C} {dtype}")


def test_channels_last_above_limit_is_eager():
    """C = 300 in channels_last takes F.cross_entropy itself."""
    logits, target, _ = make_inputs(3, 300, (7, 9), torch.float32, seed=6)
    C = 300
    target[(target < 0) | (target >= C)] = IGNORE  # eager asserts on those
    tg = target.cuda()
    x = to_layout(logits, "cl").requires_grad_()
    y = to_layout(logits, "cl").requires_grad_()
    got = ops.dense_cross_entropy(x, tg)
    ref = F.cross_entropy(y, tg, ignore_index=IGNORE)
    assert type(got.grad_fn) is type(ref.grad_fn)
    ref_loss, ref_grad = reference(logits, target, None, "mean")
    assert_loss(got, ref_loss, "cl C=300")
    got.backward()
    assert_grad(x.grad, ref_grad, torch.float32, "cl C=300")


def test_sliced_view():
    """A non-dense view takes one .contiguous(); values and grads match."""
    big, _, weight = make_inputs(3, 7, (19, 26), torch.bfloat16, seed=7)
    logits = big[:, 1:6, ::2, 3:]
    _, target, _ = make_inputs(3, 5, tuple(logits.shape[2:]), torch.bfloat16,
                               seed=8)
    src = big.cuda()[:, 1:6, ::2, 3:]
    assert not _dense(src)
    run_all_reductions(logits, src, target, weight[:5].contiguous(), "sliced")


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_misaligned_storage(layout, dtype):
    """Dense logits and target that start one element into their storage:
    the kernels must drop to accesses the pointers allow."""
    logits, target, weight = make_inputs(3, 5, (8, 8), dtype, seed=9)
    buf = torch.empty(logits.numel() + 1, dtype=dtype, device="cuda")
    if layout == "nchw":
        src = buf[1:].view(logits.shape)
    else:
        src = buf[1:].view(3, 8, 8, 5).permute(0, 3, 1, 2)
    src.copy_(logits)
    assert _dense(src) and src.data_ptr() % 16 != 0
    tbuf = torch.empty(target.numel() + 1, dtype=torch.long, device="cuda")
    tg = tbuf[1:].view(target.shape)
    tg.copy_(target)
    x = src.detach().requires_grad_()
    assert x.data_ptr() == src.data_ptr()
    for reduction in ("none", "mean"):
        x.grad = None
        loss = ops.dense_cross_entropy(x, tg, weight=weight.cuda(),
                                       reduction=reduction)
        ref_loss, ref_grad = reference(logits, target, weight, reduction,
                                       torch.ones(target.shape))
        assert_loss(loss, ref_loss, f"misaligned {layout} {reduction}")
        loss.sum().backward()
        assert_grad(x.grad, ref_grad, dtype, f"misaligned {layout} {reduction}")


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_grid_stride(layout):
    """More work items than the capped grid covers in one step: odd P (scalar
    NCHW path) with B * P above 2048 * 256."""
    logits, target, weight = make_inputs(3, 5, (419, 419), torch.bfloat16,
                                         seed=10)
    assert target.numel() > 2048 * 256
    tg, wg = target.cuda(), weight.cuda()
    x = to_layout(logits, layout).requires_grad_()
    loss = ops.dense_cross_entropy(x, tg, weight=wg)
    ref_loss, ref_grad = reference(logits, target, weight, "mean", mult=3.7)
    assert_loss(loss, ref_loss, f"grid stride {layout}")
    (loss * 3.7).backward()
    assert_grad(x.grad, ref_grad, torch.bfloat16, f"grid stride {layout}")


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_offsets_past_2_31(layout):
    """2 x 33 x 5712 x 5712 bf16 logits: 2.15e9 elements, so element offsets
    in the second image pass 2^31. Reference: the same op on each image alone
    (1.08e9 elements, all offsets below 2^31); the per-pixel arithmetic does
    not depend on the batch index, so the results are bit-identical."""
    B, C, H, W = 2, 33, 5712, 5712
    assert B * C * H * W > 2 ** 31 > C * H * W
    torch.manual_seed(0)
    if layout == "nchw":
        x = torch.randn(B, C, H, W, dtype=torch.bfloat16, device="cuda")
    else:
        x = torch.randn(B, H, W, C, dtype=torch.bfloat16,
                        device="cuda").permute(0, 3, 1, 2)
    t = torch.randint(0, C, (B, H, W), device="cuda")
    t[:, ::3, 5::7] = IGNORE
    x.requires_grad_()
    loss = ops.dense_cross_entropy(x, t, reduction="none")
    loss.sum().backward()
    assert x.grad.stride() == x.stride()
    for b in range(B):
        xb = x.detach()[b:b + 1].requires_grad_()
        lb = ops.dense_cross_entropy(xb, t[b:b + 1], reduction="none")
        lb.sum().backward()
        assert torch.equal(loss.detach()[b:b + 1], lb.detach()), b
        assert torch.equal(x.grad[b:b + 1], xb.grad), b
        del xb, lb


# ---- edge cases ----------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_all_ignored(layout, reduction):
    logits, target, weight = make_inputs(3, 5, (17, 23), torch.bfloat16)
    target.fill_(IGNORE)
    target.view(-1)[::7] = -1
    target.view(-1)[3::11] = 5
    x = to_layout(logits, layout).requires_grad_()
    loss = ops.dense_cross_entropy(x, target.cuda(), weight=weight.cuda(),
                                   reduction=reduction)
    assert torch.isfinite(loss).all()
    assert bool((loss == 0).all())
    (loss.sum() * 3.7).backward()
    assert torch.isfinite(x.grad).all()
    assert bool((x.grad == 0).all())


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_large_magnitude_logits(layout):
    """fp32 rows that contain +1e4 and -1e4: nothing overflows and the loss
    still matches (it is formed as (max - z_t) + log(sum), without the
    cancellation of lse - z_t at lse ~ 1e4)."""
    logits, target, _ = make_inputs(3, 5, (17, 23), torch.float32, seed=12)
    g = torch.Generator().manual_seed(13)
    hi = torch.randint(0, 5, (3, 1, 17, 23), generator=g)
    lo = (hi + 1 + torch.randint(0, 4, hi.shape, generator=g)) % 5
    logits.scatter_(1, hi, 1e4)
    logits.scatter_(1, lo, -1e4)
    assert bool((logits.amax(1) == 1e4).all() and (logits.amin(1) == -1e4).all())
    for reduction in ("none", "mean"):
        x = to_layout(logits, layout).requires_grad_()
        loss = ops.dense_cross_entropy(x, target.cuda(), reduction=reduction)
        ref_loss, _ = reference(logits, target, None, reduction,
                                torch.ones(target.shape))
        assert_loss(loss, ref_loss, f"1e4 {layout} {reduction}")
        loss.sum().backward()
        assert torch.isfinite(x.grad).all()


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_bit_reproducible(layout, reduction):
    logits, target, weight = make_inputs(3, 21, (64, 64), torch.bfloat16,
                                         seed=14)
    tg, wg = target.cuda(), weight.cuda()
    src = to_layout(logits, layout)
    gout = torch.randn(target.shape, device="cuda")
    out = []
    for _ in range(2):
        x = src.detach().requires_grad_()
        loss = ops.dense_cross_entropy(x, tg, weight=wg, reduction=reduction)
        loss.backward(gout if reduction == "none" else None)
        out.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_no_fp32_logit_sized_temporaries(layout):
    """One fwd+bwd may allocate dlogits (S), lse and slack: <= 1.5 S above
    the inputs. The eager chain needs more than 4 S."""
    logits = torch.randn(4, 21, 256, 256, device="cuda").bfloat16()
    if layout == "cl":
        logits = logits.contiguous(memory_format=torch.channels_last)
    target = torch.randint(0, 21, (4, 256, 256), device="cuda")
    x = logits.requires_grad_()
    S = x.numel() * x.element_size()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = ops.dense_cross_entropy(x, target)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"{layout}: peak rise {rise / S:.3f} S")
    assert type(loss.grad_fn).__name__ == FN_NAME
    assert rise <= 1.5 * S


# ---- routing -------------------------------------------------------------------
def _graph_names(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return set()
    seen.add(fn)
    names = {type(fn).__name__}
    for nxt, _ in fn.next_functions:
        names |= _graph_names(nxt, seen)
    return names


def _seg_case():
    out, target, _ = make_inputs(2, 5, (17, 23), torch.bfloat16, seed=20)
    aux = make_inputs(2, 5, (17, 23), torch.bfloat16, seed=21)[0]
    return out, aux, target


def _seg_reference(out, aux, target):
    l1, g1 = reference(out, target, None, "mean")
    l2, g2 = reference(aux, target, None, "mean", mult=0.5)
    return l1 + 0.5 * l2, g1, g2


def test_seg_criterion_routes_to_fused():
    out, aux, target = _seg_case()
    a = out.cuda().requires_grad_()
    b = aux.cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = seg_criterion({"out": a, "aux": b}, target.cuda())
    assert FN_NAME in _graph_names(loss.grad_fn)
    ref, g1, g2 = _seg_reference(out, aux, target)
    assert_loss(loss, ref, "seg_criterion")
    loss.backward()
    assert a.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    assert_grad(a.grad, g1, torch.bfloat16, "seg_criterion out")
    assert_grad(b.grad, g2, torch.bfloat16, "seg_criterion aux")


def test_ops_cross_entropy_routes_dense_logits():
    out, _, target = _seg_case()
    x = out.cuda().requires_grad_()
    loss = ops.cross_entropy(x, target.cuda(), ignore_index=IGNORE)
    assert type(loss.grad_fn).__name__ == FN_NAME
    assert_loss(loss, reference(out, target, None, "mean")[0], "cross_entropy")
    crit = ops.CrossEntropyLoss(ignore_index=IGNORE)
    assert type(crit(x, target.cuda()).grad_fn).__name__ == FN_NAME
    # smoothing on dense logits keeps the eager op
    t = target.clone()
    t[(t < 0) | (t >= 5)] = IGNORE
    sm = ops.cross_entropy(x, t.cuda(), smoothing=0.1, ignore_index=IGNORE)
    assert FN_NAME not in _graph_names(sm.grad_fn)


def _ohem_case():
    """fp32 logits whose kept set is decided with a margin: no valid pixel's
    target probability lies within 1e-4 of the threshold."""
    logits, target, _ = make_inputs(2, 5, (17, 23), torch.float32, seed=30,
                                    scale=2.0)
    target[(target < 0) | (target >= 5)] = IGNORE
    mask = target.view(-1) != IGNORE
    t = target.clone()
    t[t == IGNORE] = 0
    p = F.softmax(logits.double(), 1).gather(1, t.unsqueeze(1)).view(-1)[mask]
    p = p.sort()[0]
    threshold = max(float(p[50]), 0.7)
    assert threshold == 0.7  # more than min_kept pixels are hard
    assert float((p - threshold).abs().min()) > 1e-4
    assert 0 < int((p < threshold).sum()) < p.numel()
    return logits, target


def test_ohem_gpu_matches_cpu_module():
    logits, target = _ohem_case()
    crit = OhemCrossEntropy(min_kept=50)
    z = logits.double().requires_grad_()
    ref = crit(z, target)
    ref.backward()
    x = logits.cuda().requires_grad_()
    loss = crit(x, target.cuda())
    assert FN_NAME in _graph_names(loss.grad_fn)
    assert_loss(loss, ref.detach(), "ohem")
    loss.backward()
    assert_grad(x.grad, z.grad, torch.float32, "ohem")


def test_gate_off_takes_eager(monkeypatch):
    monkeypatch.setenv("DLA_DENSE_CE", "0")
    out, aux, target = _seg_case()
    target[(target < 0) | (target >= 5)] = IGNORE  # eager asserts on those
    a = out.cuda().requires_grad_()
    b = aux.cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = seg_criterion({"out": a, "aux": b}, target.cuda())
        tg = target.cuda()
        ref = (F.cross_entropy(a, tg, ignore_index=IGNORE)
               + 0.5 * F.cross_entropy(b, tg, ignore_index=IGNORE))
    names = _graph_names(loss.grad_fn)
    assert FN_NAME not in names and "LogSoftmaxBackward0" in names
    # the same eager op twice: only its own summation order may differ
    torch.testing.assert_close(loss, ref, rtol=LOSS_TOL, atol=LOSS_TOL)

    logits, t2 = _ohem_case()
    x = logits.cuda().requires_grad_()
    ohem = OhemCrossEntropy(min_kept=50)(x, t2.cuda())
    names = _graph_names(ohem.grad_fn)
    assert FN_NAME not in names and "LogSoftmaxBackward0" in names
