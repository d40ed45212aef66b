"""CPU tests for the attention routing table (ops.attention._attn_route):
which of the resident, streaming and eager implementations serves a shape,
decided by arithmetic alone."""
import pytest
import torch

from deeplearning_amd.ops.attention import (_attn_route, _eager_attention,
                                            _resident_bwd_lds_bytes,
                                            fused_attention)

BF16 = torch.bfloat16
LDS_LIMIT = 163840  # 160 KiB per CU


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("DLA_ATTN_STREAM", raising=False)
    monkeypatch.delenv("DLA_FORCE_EAGER", raising=False)


# (N, d) -> (fwd, bwd) on the plain bf16 path. d = 64 leaves the resident
# backward at N = 225 (lds_kv = 178 176 B at Npad = 256); d = 32 fits up to 256.
PLAIN = [
    (197, 32, ("resident", "resident")),
    (197, 64, ("resident", "resident")),
    (224, 32, ("resident", "resident")),
    (224, 64, ("resident", "resident")),
    (225, 32, ("resident", "resident")),
    (225, 64, ("resident", "stream")),
    (256, 32, ("resident", "resident")),
    (256, 64, ("resident", "stream")),
    (257, 32, ("stream", "stream")),
    (257, 64, ("stream", "stream")),
    (4096, 32, ("stream", "stream")),
    (4096, 64, ("stream", "stream")),
]


@pytest.mark.parametrize("N,d,want", PLAIN)
def test_plain_route(N, d, want):
    assert _attn_route(N, d, BF16, False, True) == want


@pytest.mark.parametrize("d", [32, 64])
def test_small_shapes_stay_resident(d):
    # every shape that launches today keeps its kernels
    for N in (1, 16, 49, 50, 96, 97, 144, 197, 224):
        assert _attn_route(N, d, BF16, False, True) == \
            ("resident", "resident"), N


@pytest.mark.parametrize("d", [32, 64])
def test_bias_mask_rows(d):
    for N in (49, 144, 197, 224, 225, 256):
        assert _attn_route(N, d, BF16, True, True) == \
            ("resident", "resident"), N
    for N in (257, 577, 4096, 4097):
        assert _attn_route(N, d, BF16, True, True) == ("eager", "eager"), N


def test_eager_rows():
    eager = ("eager", "eager")
    assert _attn_route(4097, 64, BF16, False, True) == eager
    assert _attn_route(577, 64, torch.float16, False, True) == eager
    assert _attn_route(577, 64, torch.float32, False, True) == eager
    assert _attn_route(197, 64, torch.float32, False, True) == eager
    assert _attn_route(577, 48, BF16, False, True) == eager
    assert _attn_route(197, 128, BF16, False, True) == eager
    assert _attn_route(577, 64, BF16, False, False) == eager  # CPU / forced
    assert _attn_route(197, 64, BF16, False, False) == eager


def test_stream_switch(monkeypatch):
    monkeypatch.setenv("DLA_ATTN_STREAM", "1")
    for N in (1, 197, 256, 577, 4096):
        for d in (32, 64):
            assert _attn_route(N, d, BF16, False, True) == \
                ("stream", "stream")
    # only where streaming is legal
    assert _attn_route(197, 64, BF16, True, True) == ("resident", "resident")
    assert _attn_route(577, 64, BF16, True, True) == ("eager", "eager")
    assert _attn_route(4097, 64, BF16, False, True) == ("eager", "eager")
    assert _attn_route(577, 64, torch.float32, False, True) == \
        ("eager", "eager")
    assert _attn_route(577, 64, BF16, False, False) == ("eager", "eager")


def test_lds_formula_values():
    # the figures of the launch code, worked by hand
    assert _resident_bwd_lds_bytes(256, 64) == (178176, 144384)
    assert _resident_bwd_lds_bytes(224, 64) == (160768, 131072)
    assert max(_resident_bwd_lds_bytes(224, 64)) <= LDS_LIMIT
    assert max(_resident_bwd_lds_bytes(225, 64)) > LDS_LIMIT
    assert max(_resident_bwd_lds_bytes(256, 32)) <= LDS_LIMIT


def test_lds_formula_equals_launch_code():
    """The Python byte counts are those attn_bwd launches with."""
    from deeplearning_amd.ops import ext
    for N in (1, 96, 97, 197, 224, 225, 240, 256, 257, 4096):
        for d in (32, 64):
            assert list(_resident_bwd_lds_bytes(N, d)) == \
                list(ext().attn_bwd_lds_bytes(N, d)), (N, d)


def test_fused_attention_cpu_is_eager_above_256():
    torch.manual_seed(0)
    B, N, H, d = 1, 300, 2, 32
    qkv = torch.randn(B, N, 3 * H * d)
    out = fused_attention(qkv, H, d ** -0.5)
    ref = _eager_attention(qkv, H, d ** -0.5)
    assert torch.equal(out, ref)
    qkv_b = qkv.bfloat16()
    assert torch.equal(fused_attention(qkv_b, H, d ** -0.5),
                       _eager_attention(qkv_b, H, d ** -0.5))
