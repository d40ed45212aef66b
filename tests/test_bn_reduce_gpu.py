"""The atomic-free NHWC BatchNorm reductions of csrc/batchnorm.hip: each block
of bn_stats_nhwc / bn_bwd_stats_nhwc / bn_join_bwd_stats_nhwc /
bn_relu_maxpool_bwd_stats_nhwc stores one row of a [n_parts, NS*C] slab, and
bn_slab_reduce_kernel (backward) or bn_finalize_parts_kernel (forward) sums
the slab rows in a fixed order.

Exact inputs. The kernels take mean, rstd, scale and shift as inputs, so the
sums can be made independent of the summation order: x in [-4, 4] and dy in
[-3, 3] integer valued, integer mean, rstd and weight powers of two in
[1/2, 2], scale = 1 and shift = k + 0.5 (the pre-activation x + k + 0.5 is
exact and never 0). Every term dy, dy * (x - mean) * rstd is then a multiple
of 1/2 of magnitude <= 36, every partial sum over <= 7688 rows a multiple of
1/2 below 2^19 < 2^24: fp32 holds all of them exactly, so dbias and dweight
must EQUAL the fp64 reference, whatever the order. A dropped, doubled or
uninitialised slab element cannot hide in a tolerance.

dx = weight * rstd * (g - sum_g / n - xhat * sum_gxh / n) is not exact (1 / n
is rounded). It must lie within one bf16 ulp, 2^-7 max(|dx|, |ref|), of the
fp64 value; where the three terms cancel to less than 2^-17 of their size the
fp32 evaluation itself (rounded 1 / n, two products, two differences: at most
4 * 2^-24 of the terms' magnitudes) is larger than an ulp of the result, so
that evaluation error of the terms is added to the bound. It is 2^-15 of one
bf16 ulp of the terms.

Forward. With an exact sum and sumsq, mean = sum / n is one division: exact
when n is a power of two, else within 2 fp32 ulps (the division is correctly
rounded; 2 leaves room for a reciprocal-multiply lowering). var = sumsq / n
- mean^2 has an absolute error of at most 2u * sumsq / n + u * var, u =
2^-24, i.e. a relative (2k + 1) u with k = (sumsq / n) / (var + eps). The
inputs keep k <= 2 (asserted; shapes with fewer than 64 rows mirror their
rows, x[n-1-i] = -x[i], so that mean^2 stays small against var; a single row
gives sumsq / n = mean^2 and var = 0 exactly), so var is
within 5u, rstd = rsqrtf(var + eps) within 5u / 2 + 2u (rsqrtf) < 5u, the
unbiased variance within 7u, and running_var = (1 - m) * 1 + m * unbiased
within 10u, running_mean = m * mean within 2u: all below 2^-20 = 16u.

Random inputs: unit-scale randn, the true mean and rstd; every sum must lie
within gamma_(n+3) * sum |term| of the fp64 sum of the same terms (n + 3:
the n - 1 additions and the roundings inside one term), gamma_k = k u /
(1 - k u). A sum kept in bf16 or fp16 misses that by orders of magnitude.
"""
import functools

import pytest
import torch

from deeplearning_amd.ops._ext import ext

gpu = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
U = 2.0 ** -24

# (B, H, W, C), the smallest shapes at which the (channel chunk, row split)
# grid can go wrong
BN_SHAPES = [
    (1, 1, 1, 8),       # one row, one lane
    (1, 1, 3, 2048),    # 3 rows, 256 lanes per row: 8 chunks, row-lanes idle
    (2, 7, 7, 64),      # 98 rows, ragged against 32 row-lanes per block
    (3, 5, 9, 24),      # 3 lanes per row, 85 row-lanes, one thread idle
    (2, 3, 3, 4096),    # a row wider than a block: 16 chunks
    (1, 5, 5, 6),       # V = 2
    (1, 5, 5, 5),       # V = 1
    (4, 32, 32, 128),   # 4096 rows, a power of two; 32 parts
    (8, 31, 31, 64),    # 7688 rows: 31 parts, ragged last rows
]
JOIN_SHAPES = [s for s in BN_SHAPES if s[3] % 8 == 0] + [
    (3, 5, 9, 128), (8, 31, 31, 256)]
DUAL_SHAPES = JOIN_SHAPES + [(2, 3, 3, 2048)]
DTYPE_SHAPE = (2, 7, 7, 64)
NO_ROWS_SHAPES = [(1, 1, 3, 2048), (2, 3, 3, 4096)]  # threads without rows
MULTI_PART = (8, 31, 31, 64)


def _cl(t):
    """[B, H, W, C] contiguous -> the same memory as channels-last [B,C,H,W]."""
    return t.permute(0, 3, 1, 2)


def _rows(t):
    """channels-last [B, C, H, W] -> fp64 [rows, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double()


@functools.lru_cache(maxsize=None)
def _int_inputs(shape, dtype=torch.bfloat16):
    """Seeded CPU tensors of the exact construction; shared, never modified."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(7 + 131 * B + 17 * H + 3 * W + C)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    pow2 = lambda: 2.0 ** ri(-1, 1, C).float()
    x = ri(-4, 4, B, H, W, C)
    n = B * H * W
    if n < 64:  # see the module docstring, Forward
        flat = x.reshape(n, C)
        for i in range(n // 2):
            flat[n - 1 - i] = -flat[i]
    d = {
        "x": x.to(dtype), "xd": ri(-4, 4, B, H, W, C).to(dtype),
        "dy": ri(-3, 3, B, H, W, C).to(dtype),
        "out": ri(-2, 2, B, H, W, C).to(dtype),
        "mean": ri(-2, 2, C).float(), "rstd": pow2(),
        "weight": pow2() * (1 - 2 * ri(0, 1, C)).float(),
        "mean_d": ri(-2, 2, C).float(), "rstd_d": pow2(),
        "weight_d": pow2() * (1 - 2 * ri(0, 1, C)).float(),
        "scale": torch.ones(C), "shift": ri(-2, 2, C).float() + 0.5,
        "bias": ri(-2, 2, C).float(),
    }
    return d


@functools.lru_cache(maxsize=None)
def _rand_inputs(shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(99 + B + H + W + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = {k: rn(B, H, W, C).to(torch.bfloat16) for k in ("x", "xd", "dy", "out")}
    for k, src in (("", "x"), ("_d", "xd")):
        f = d[src].double().reshape(-1, C)
        d["mean" + k] = f.mean(0).float()
        d["rstd" + k] = (f.var(0, unbiased=False) + EPS).rsqrt().float()
        d["weight" + k] = rn(C) * 0.5 + 1.0
    d["bias"] = rn(C) * 0.2
    d["scale"] = d["weight"] * d["rstd"]
    d["shift"] = d["bias"] - d["mean"] * d["scale"]
    return d


def _gpu(d):
    return {k: (_cl(v.cuda()) if v.dim() == 4 else v.cuda())
            for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _int_gpu(shape, dtype=torch.bfloat16):
    return _gpu(_int_inputs(shape, dtype))


@functools.lru_cache(maxsize=None)
def _rand_gpu(shape):
    return _gpu(_rand_inputs(shape))


def _bwd_ref(g, x, mean, rstd, weight):
    """fp64: sum g, sum g*xhat [C], their |term| sums, dx [rows, C] and the
    magnitude of dx's three terms."""
    g, x = _rows(g), _rows(x)
    n = g.shape[0]
    mean, rstd, weight = mean.double(), rstd.double(), weight.double()
    xh = (x - mean) * rstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    a0, a1 = g.abs().sum(0), (g * xh).abs().sum(0)
    dx = weight * rstd * (g - s0 / n - xh * s1 / n)
    mag = (weight * rstd).abs() * (g.abs() + (s0 / n).abs()
                                   + (xh * s1 / n).abs())
    return s0, s1, a0, a1, dx, mag


def _check_dx(dx, ref, mag, what):
    dx = _rows(dx)
    assert torch.isfinite(dx).all(), f"{what}: non-finite dx"
    bound = 2.0 ** -7 * torch.maximum(dx.abs(), ref.abs()) + 4 * U * mag
    worst = ((dx - ref).abs() / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max |dx-ref|/bound = {worst:.4f}")
    assert ((dx - ref).abs() <= bound).all(), f"{what}: {worst:.3f}x the bound"


def _gamma(k):
    return k * U / (1 - k * U)


def _check_sum(got, ref, absum, n, exact, what):
    assert got.dtype == torch.float32
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    if exact:
        assert torch.equal(got, ref.float()), \
            f"{what}: max |diff| {(got.double() - ref).abs().max().item()}"
        return
    bound = _gamma(n + 3) * absum
    worst = ((got.double() - ref).abs() / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max |sum-ref|/bound = {worst:.4f}")
    assert ((got.double() - ref).abs() <= bound).all(), \
        f"{what}: {worst:.3f}x the summation bound"


# ---- the entry points, on a dict of inputs ---------------------------------
def _call_bn_bwd(d, relu):
    if relu and not ext().bn_relu_mask_from_x(d["x"]):
        # H = W = 1 is NCHW and channels-last at once and takes the NCHW
        # route, whose mask is the stored y = relu(x * scale + shift)
        sc, sh = (d[k].view(1, -1, 1, 1) for k in ("scale", "shift"))
        y = torch.relu(d["x"].float() * sc + sh).to(d["x"].dtype)
        return ext().batchnorm_bwd_ex(d["dy"], d["x"], y, d["weight"],
                                      d["mean"], d["rstd"], None, None, True)
    return ext().batchnorm_bwd_ex(
        d["dy"], d["x"], None, d["weight"], d["mean"], d["rstd"],
        d["scale"] if relu else None, d["shift"] if relu else None, relu)


def _call_join(d):
    return ext().bn_add_relu_bwd(d["dy"], d["out"], d["x"], d["weight"],
                                 d["mean"], d["rstd"])


def _call_dual(d):
    return ext().bn_add_relu_dual_bwd(
        d["dy"], d["out"], d["x"], d["weight"], d["mean"], d["rstd"], d["xd"],
        d["weight_d"], d["mean_d"], d["rstd_d"])


def _call_fwd(d):
    C = d["x"].shape[1]
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    out = ext().batchnorm_fwd(d["x"], d["weight"], d["bias"], rm, rv, MOM, EPS,
                              False)
    return list(out) + [rm, rv]


def _check_bn_bwd(d, relu, exact, what):
    dx, dw, db = _call_bn_bwd(d, relu)
    g = d["dy"]
    if relu:
        pre = d["x"].double() * d["scale"].double().view(1, -1, 1, 1) \
            + d["shift"].double().view(1, -1, 1, 1)
        g = torch.where(pre > 0, d["dy"], torch.zeros_like(d["dy"]))
    s0, s1, a0, a1, ref, mag = _bwd_ref(g, d["x"], d["mean"], d["rstd"],
                                        d["weight"])
    n = ref.shape[0]
    _check_sum(db, s0, a0, n, exact, what + " dbias")
    _check_sum(dw, s1, a1, n, exact, what + " dweight")
    _check_dx(dx, ref, mag, what)


def _check_join(d, exact, what):
    g, dx, dw, db = _call_join(d)
    gref = torch.where(d["out"] > 0, d["dy"], torch.zeros_like(d["dy"]))
    assert torch.equal(g, gref), what + ": g"
    s0, s1, a0, a1, ref, mag = _bwd_ref(gref, d["x"], d["mean"], d["rstd"],
                                        d["weight"])
    n = ref.shape[0]
    _check_sum(db, s0, a0, n, exact, what + " dbias")
    _check_sum(dw, s1, a1, n, exact, what + " dweight")
    _check_dx(dx, ref, mag, what)


def _check_dual(d, exact, what):
    dx, dxd, dw, db, dwd, dbd = _call_dual(d)
    gref = torch.where(d["out"] > 0, d["dy"], torch.zeros_like(d["dy"]))
    s0, s1, a0, a1, ref, mag = _bwd_ref(gref, d["x"], d["mean"], d["rstd"],
                                        d["weight"])
    _, s1d, _, a1d, refd, magd = _bwd_ref(gref, d["xd"], d["mean_d"],
                                          d["rstd_d"], d["weight_d"])
    n = ref.shape[0]
    _check_sum(db, s0, a0, n, exact, what + " dbias")
    _check_sum(dbd, s0, a0, n, exact, what + " dbias_d")
    _check_sum(dw, s1, a1, n, exact, what + " dweight")
    _check_sum(dwd, s1d, a1d, n, exact, what + " dweight_d")
    _check_dx(dx, ref, mag, what + " dx")
    _check_dx(dxd, refd, magd, what + " dxd")


def _ulp32(t):
    """Spacing of fp32 at |t| (fp64 tensor), 0 where t == 0."""
    e = torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -126)))
    return torch.where(t == 0, torch.zeros_like(t), 2.0 ** (e - 23))


# ---- CPU: why exact equality catches a dropped or doubled row --------------
@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_zeroed_row_moves_the_reference_cpu(shape):
    """On the integer-valued inputs, zeroing any one row moves the fp64
    reference of some channel, so a kernel that drops (or doubles) a row
    cannot equal it. Zeroing row r of dy moves sum(dy) by dy[r], zeroing row
    r of x moves sumsq by x[r]^2: every row needs one non-zero entry."""
    d = _int_inputs(shape)
    C = shape[3]
    dy, x = d["dy"].double().reshape(-1, C), d["x"].double().reshape(-1, C)
    for r in range(min(dy.shape[0], 3)):  # spelled out for three rows
        dy0 = dy.clone()
        dy0[r] = 0
        assert (dy0.sum(0) != dy.sum(0)).any(), f"row {r}"
    assert (dy.abs().sum(1) > 0).all() and ((x * x).sum(1) > 0).all()


# ---- exact sums --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_bn_bwd_exact_sums(shape, relu):
    _check_bn_bwd(_int_gpu(shape), relu, True, f"bn_bwd {shape} relu={relu}")


@gpu
@pytest.mark.parametrize("shape", JOIN_SHAPES, ids=str)
def test_join_bwd_exact_sums(shape):
    _check_join(_int_gpu(shape), True, f"join {shape}")


@gpu
@pytest.mark.parametrize("shape", DUAL_SHAPES, ids=str)
def test_dual_join_bwd_exact_sums(shape):
    _check_dual(_int_gpu(shape), True, f"dual {shape}")


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=str)
def test_exact_sums_other_dtypes(dtype):
    d = _int_gpu(DTYPE_SHAPE, dtype)
    for relu in (False, True):
        _check_bn_bwd(d, relu, True, f"bn_bwd {dtype} relu={relu}")
    _check_join(d, True, f"join {dtype}")
    _check_dual(d, True, f"dual {dtype}")
    _check_fwd_exact(d, DTYPE_SHAPE, f"fwd {dtype}")


def _check_fwd_exact(d, shape, what):
    """Bounds: module docstring, Forward."""
    y, mean, rstd, scale, shift, rm, rv = _call_fwd(d)
    x = _rows(d["x"])
    n = x.shape[0]
    s, q = x.sum(0), (x * x).sum(0)
    mu = s / n
    var = q / n - mu * mu
    k = ((q / n) / (var + EPS)).max().item()
    assert n == 1 or k <= 2.0, f"{what}: test inputs have k = {k}"
    for t in (y, mean, rstd, scale, shift, rm, rv):
        assert torch.isfinite(t).all(), what
    err = (mean.double() - mu).abs()
    if n & (n - 1) == 0:
        assert torch.equal(mean, mu.float()), f"{what}: mean, n = {n}"
    else:
        assert (err <= 2 * _ulp32(mu)).all(), \
            f"{what}: mean off by {(err / _ulp32(mu).clamp(min=1e-300)).max()} ulp"
    unb = var * n / max(n - 1, 1)
    for name, got, ref in (("rstd", rstd, (var + EPS).rsqrt()),
                           ("running_mean", rm, MOM * mu),
                           ("running_var", rv, (1 - MOM) + MOM * unb)):
        rel = ((got.double() - ref).abs()
               / ref.abs().clamp(min=1e-300)).max().item()
        print(f"{what}: {name} max rel err {rel / U:.2f} u")
        assert ((got.double() - ref).abs() <= 2.0 ** -20 * ref.abs()).all(), \
            f"{what}: {name} rel err {rel:.3g}"


@gpu
@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_bn_fwd_exact_sums(shape):
    _check_fwd_exact(_int_gpu(shape), shape, f"fwd {shape}")


# ---- random inputs: the summation bound ------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(2, 7, 7, 64), MULTI_PART,
                                   (2, 3, 3, 2048)], ids=str)
def test_random_inputs_within_summation_bound(shape):
    d = _rand_gpu(shape)
    _check_bn_bwd(d, True, False, f"bn_bwd rand {shape}")
    _check_join(d, False, f"join rand {shape}")
    _check_dual(d, False, f"dual rand {shape}")
    # forward: mean = sum / n, and sumsq through rstd
    y, mean, rstd, *_ = _call_fwd(d)
    x = _rows(d["x"])
    n = x.shape[0]
    mu, q = x.sum(0) / n, (x * x).sum(0) / n
    gam = _gamma(n + 3)
    b_mu = gam * x.abs().sum(0) / n
    assert ((mean.double() - mu).abs() <= b_mu).all(), "fwd mean"
    var = q - mu * mu
    b_var = gam * q + 2 * mu.abs() * b_mu + b_mu ** 2
    b_rstd = 0.5 * b_var / (var + EPS) + 2.0 ** -20
    rel = (rstd.double() * (var + EPS).sqrt() - 1).abs()
    print(f"fwd rand {shape}: rstd max rel/bound {(rel / b_rstd).max():.4f}")
    assert (rel <= b_rstd).all(), "fwd rstd"


# ---- never reads past the tensor -------------------------------------------
def _nan_tailed(d):
    """Every 4D input becomes the first B images of a (B+1)-image
    channels-last buffer whose last image is NaN."""
    out = dict(d)
    for k, v in d.items():
        if v.dim() != 4:
            continue
        B, C, H, W = v.shape
        buf = torch.full((B + 1, H, W, C), float("nan"), device="cuda",
                         dtype=v.dtype)
        buf[:B] = v.permute(0, 2, 3, 1)
        out[k] = _cl(buf)[:B]
        assert out[k].is_contiguous(memory_format=torch.channels_last) \
            or B == 1
    return out


def _all_calls(d):
    return [*_call_bn_bwd(d, False), *_call_bn_bwd(d, True), *_call_join(d),
            *_call_dual(d), *_call_fwd(d)]


def _assert_same_finite(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all(), f"{what}: output {i} not finite"
        assert torch.equal(a, b), f"{what}: output {i} changed"


@gpu
@pytest.mark.parametrize("shape", [(1, 1, 3, 2048), (2, 7, 7, 64),
                                   (3, 5, 9, 24), MULTI_PART], ids=str)
def test_never_reads_past_the_tensor(shape):
    d = _int_gpu(shape)
    _assert_same_finite(_all_calls(_nan_tailed(d)), _all_calls(d),
                        f"NaN tail {shape}")


# ---- every slab element that is read was written ----------------------------
def _poison_allocator():
    """Leave the caching allocator holding only NaN-filled free blocks, of
    every size class up to 8 MiB (the largest slab here is 48 KiB), so the
    next torch::empty hands out poisoned memory."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    blocks = [torch.full((2 ** p,), float("nan"), device="cuda")
              for p in range(7, 22)]
    del blocks
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("shape", NO_ROWS_SHAPES + [MULTI_PART], ids=str)
def test_every_slab_element_read_was_written(shape):
    d = _int_gpu(shape)
    calls = [lambda: _call_bn_bwd(d, False), lambda: _call_bn_bwd(d, True),
             lambda: _call_join(d), lambda: _call_dual(d),
             lambda: _call_fwd(d)]
    try:
        for i, call in enumerate(calls):
            ref = call()
            _poison_allocator()
            _assert_same_finite(call(), ref, f"poisoned {shape} call {i}")
    finally:  # hand the NaN-filled free blocks back, not on to later tests
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- reproducibility ----------------------------------------------------------
@gpu
def test_bit_reproducible():
    d = _rand_gpu(MULTI_PART)
    for i, call in enumerate([lambda: _call_bn_bwd(d, True),
                              lambda: _call_join(d), lambda: _call_dual(d),
                              lambda: _call_fwd(d)]):
        _assert_same_finite(call(), call(), f"repeat of call {i}")

    g = torch.Generator().manual_seed(3)
    x = _cl((torch.randn(2, 16, 16, 64, generator=g) * 1.5 + 0.3)
            .to(torch.bfloat16).cuda())
    dpool = _cl(torch.randn(2, 8, 8, 64, generator=g).to(torch.bfloat16)
                .cuda())
    w = (torch.rand(64, generator=g) + 0.5).cuda()
    b = (torch.randn(64, generator=g) * 0.2).cuda()

    def stem():
        rm, rv = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
        pooled, slots, mean, rstd, scale, shift = ext().bn_relu_maxpool_fwd(
            x, w, b, rm, rv, MOM, EPS)
        bwd = ext().bn_relu_maxpool_bwd(dpool, x, slots, w, mean, rstd, scale,
                                        shift)
        return [pooled, slots, mean, rstd, scale, shift, rm, rv, *bwd]

    _assert_same_finite(stem(), stem(), "stem fwd+bwd")
