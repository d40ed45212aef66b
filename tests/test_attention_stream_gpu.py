"""GPU numerics tests for the streaming attention kernels
(csrc/attention_stream.hip, N > 256) against a plain fp32 PyTorch reference
and against the resident kernels where both launch.

Tolerances are the project's bf16 attention ones at unit input scale:
forward max abs error < 0.02, backward max abs error < 0.05 * max(|ref
grad|max, 1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 0.02
BWD_TOL = 0.05

# (B, N, H, d): one key in the tail panel and one row in the last query
# block; a tail tile on a 16-row boundary; exact panels; ViT-B/16 at 384^2;
# a 448^2 input; more than four 256-key panels and nine query blocks.
SHAPES = [(2, 257, 2, 64), (2, 272, 3, 32), (1, 512, 2, 64),
          (1, 577, 2, 64), (1, 785, 2, 32), (1, 1025, 1, 64)]


def eager_ref_f32(qkv, H, scale):
    B, N, _ = qkv.shape
    qkv = qkv.float().reshape(B, N, 3, H, -1).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, -1)


def make_qkv(B, N, H, d, ramp=False, seed=0):
    torch.manual_seed(seed)
    qkv = torch.randn(B, N, 3, H, d, device="cuda")
    if ramp:
        # K rows grow along N: every row's maximum moves into later panels,
        # so the online rescale is exercised and a dropped panel shows
        qkv[:, :, 1] *= torch.linspace(0.25, 4.0, N, device="cuda") \
            .view(1, N, 1, 1)
    return qkv.reshape(B, N, 3 * H * d).bfloat16()


def check_fwd_bwd(qkv, H, scale, seed=1):
    """fused_attention forward and backward against fp32; returns the errors
    (printed before asserting so a run shows the figures)."""
    from deeplearning_amd.ops.attention import fused_attention
    qkv_f = qkv.clone().requires_grad_()
    qkv_r = qkv.clone().float().requires_grad_()
    out = fused_attention(qkv_f, H, scale)
    ref = eager_ref_f32(qkv_r, H, scale)
    torch.manual_seed(seed)
    g = torch.randn_like(ref)
    out.float().backward(g)
    ref.backward(g)
    ferr = (out.float() - ref).abs().max().item()
    berr = (qkv_f.grad.float() - qkv_r.grad).abs().max().item()
    mag = qkv_r.grad.abs().max().item()
    print(f"N={qkv.shape[1]} fwd err {ferr:.5f}  bwd err {berr:.5f} "
          f"(bound {BWD_TOL * max(mag, 1.0):.4f})")
    assert torch.isfinite(out).all() and torch.isfinite(qkv_f.grad).all()
    assert ferr < FWD_TOL, f"fwd err {ferr}"
    assert berr < BWD_TOL * max(mag, 1.0), \
        f"bwd err {berr} vs ref magnitude {mag}"


@pytest.mark.parametrize("ramp", [False, True], ids=["randn", "ramp"])
@pytest.mark.parametrize("B,N,H,d", SHAPES)
def test_stream_fwd_bwd_matches_fp32(B, N, H, d, ramp):
    check_fwd_bwd(make_qkv(B, N, H, d, ramp=ramp), H, d ** -0.5)


@pytest.mark.parametrize("hot", ["last", "first_panel"])
@pytest.mark.parametrize("B,N,H,d", [(2, 257, 2, 64), (1, 1025, 1, 64)])
def test_hot_key(B, N, H, d, hot):
    """One key j* takes every row's softmax mass: in the one-key tail panel
    (j* = N-1, all earlier panels must be rescaled away) or in the first
    panel (j* = 3, all later panels must add next to nothing)."""
    from deeplearning_amd.ops.attention import fused_attention
    js = N - 1 if hot == "last" else 3
    scale = d ** -0.5
    torch.manual_seed(0)
    qkv5 = torch.randn(B, N, 3, H, d, device="cuda")
    qkv5[:, :, 0] = 2.0 + 0.5 * qkv5[:, :, 0]   # q = 2 + noise
    qkv5[:, :, 1] *= 0.25                        # cold keys: small
    qkv5[:, js, 1] = 4.0                         # the hot key
    qkv = qkv5.reshape(B, N, 3 * H * d).bfloat16()

    # conditions on the input, checked on the fp32 reference
    q, k, v = qkv.float().reshape(B, N, 3, H, d).permute(2, 0, 3, 1, 4) \
        .unbind(0)
    logits = (q @ k.transpose(-2, -1)) * scale          # B,H,N,N
    others = logits.clone()
    others[..., js] = -float("inf")
    margin = (logits[..., js] - others.max(-1).values).min().item()
    assert margin >= 16.0, margin
    mass = logits.softmax(-1)[..., js].min().item()
    assert mass > 0.99, mass

    qkv_f = qkv.clone().requires_grad_()
    out = fused_attention(qkv_f, H, scale)
    ref = eager_ref_f32(qkv, H, scale)
    ferr = (out.float() - ref).abs().max().item()
    torch.manual_seed(1)
    g = torch.randn_like(ref)
    out.float().backward(g)
    dv_hot = qkv_f.grad.float().reshape(B, N, 3, H, d)[:, js, 2]  # B,H,d
    colsum = g.reshape(B, N, H, d).sum(1)                          # B,H,d
    berr = (dv_hot - colsum).abs().max().item()
    bound = BWD_TOL * max(colsum.abs().max().item(), 1.0)
    print(f"hot key {js}/{N}: margin {margin:.1f} fwd err {ferr:.5f} "
          f"dV err {berr:.5f} (bound {bound:.4f})")
    assert ferr < FWD_TOL, f"fwd err {ferr}"
    assert berr < bound, f"dV[j*] err {berr} vs bound {bound}"


@pytest.mark.parametrize("B,N,H,d", [(2, 197, 3, 64), (2, 224, 2, 32)])
def test_stream_matches_resident(B, N, H, d):
    """Where both launch, the streaming kernels reproduce the resident ones:
    the row maximum is the same MFMA sequence and the same fp32 max, so it is
    bitwise equal; l is an fp32 sum of positive __expf terms (bound ~1e-5)."""
    from deeplearning_amd.ops import ext
    qkv = make_qkv(B, N, H, d)
    scale = d ** -0.5
    out_s, st_s = ext().attn_fwd_stream(qkv, H, scale, True)
    out_r, st_r = ext().attn_fwd(qkv, H, scale, None, None, False, True)
    assert st_s.shape == st_r.shape == (2, B, H, N)
    assert torch.equal(st_s[0], st_r[0]), "row maxima differ"
    torch.testing.assert_close(st_s[1], st_r[1], rtol=1e-4, atol=0.0)
    ferr = (out_s.float() - out_r.float()).abs().max().item()
    assert ferr < FWD_TOL, f"fwd stream vs resident {ferr}"

    torch.manual_seed(1)
    dout = torch.randn(B, N, H * d, device="cuda").bfloat16()
    drow = (dout.float() * out_r.float()).view(B, N, H, d).sum(-1) \
        .permute(0, 2, 1).contiguous()
    (dq_s,) = ext().attn_bwd_stream(qkv, dout, st_r, drow, H, scale)
    (dq_r,) = ext().attn_bwd(qkv, dout, st_r, drow, H, scale)
    berr = (dq_s.float() - dq_r.float()).abs().max().item()
    mag = dq_r.float().abs().max().item()
    print(f"N={N} stream vs resident: fwd {ferr:.5f} bwd {berr:.5f}")
    assert berr < BWD_TOL * max(mag, 1.0), f"bwd stream vs resident {berr}"


def test_stream_is_deterministic():
    from deeplearning_amd.ops.attention import fused_attention
    B, N, H, d = 1, 577, 2, 64
    qkv = make_qkv(B, N, H, d)
    torch.manual_seed(1)
    g = torch.randn(B, N, H * d, device="cuda").bfloat16()
    runs = []
    for _ in range(2):
        x = qkv.clone().requires_grad_()
        out = fused_attention(x, H, d ** -0.5)
        out.backward(g)
        runs.append((out.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_routing_is_real():
    """N = 577 runs the fused Function, and its forward never allocates
    anything the size of a [B,H,N,N] score tensor."""
    from deeplearning_amd.ops.attention import fused_attention
    B, N, H, d = 8, 577, 12, 64
    qkv = make_qkv(B, N, H, d).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fused_attention(qkv, H, d ** -0.5)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert type(out.grad_fn).__name__.startswith("_AttnFusedBwdFn"), \
        out.grad_fn
    scores_bytes = B * H * N * N * 4
    print(f"forward peak {peak / 2**20:.1f} MiB, one fp32 score tensor "
          f"{scores_bytes / 2**20:.1f} MiB")
    assert peak < scores_bytes, (peak, scores_bytes)


@pytest.mark.parametrize("B,N,H,d", [(2, 256, 2, 64), (2, 240, 2, 64)])
def test_resident_backward_lds_hole(B, N, H, d):
    """d = 64 with 225 <= N <= 256: the resident backward's LDS does not fit
    160 KiB, so the backward takes the streaming kernels."""
    check_fwd_bwd(make_qkv(B, N, H, d), H, d ** -0.5)


def test_vit_above_256_tokens_matches_eager(monkeypatch):
    """A small ViT at 272^2 (N = 290) under bf16 autocast: the fused route
    against the same model with DLA_FORCE_EAGER=1."""
    import torch.nn.functional as F
    from deeplearning_amd.models.classification.vit import VisionTransformer

    torch.manual_seed(0)
    model = VisionTransformer(img_size=272, patch_size=16, num_classes=10,
                              embed_dim=128, depth=2, num_heads=2).cuda()
    x = torch.randn(2, 3, 272, 272, device="cuda")
    y = torch.tensor([3, 7], device="cuda")
    w = model.blocks[0].attn.qkv.weight

    def run():
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x)
        F.cross_entropy(logits.float(), y).backward()
        return logits.detach().float(), w.grad.detach().float().clone()

    monkeypatch.delenv("DLA_FORCE_EAGER", raising=False)
    logits_f, grad_f = run()
    monkeypatch.setenv("DLA_FORCE_EAGER", "1")
    logits_e, grad_e = run()
    monkeypatch.delenv("DLA_FORCE_EAGER")

    lerr = (logits_f - logits_e).abs().max().item()
    gerr = (grad_f - grad_e).abs().max().item()
    gmag = grad_e.abs().max().item()
    print(f"vit N=290: logits err {lerr:.5f}, qkv.weight grad err {gerr:.3e} "
          f"of max {gmag:.3e}")
    assert gmag > 0
    assert lerr < 0.05, f"logits {lerr}"
    assert gerr < 0.05 * gmag, f"qkv.weight grad {gerr} vs {gmag}"
