"""CPU behaviour of the dense (per-pixel) cross-entropy: off the GPU it is
F.cross_entropy itself, and the segmentation call sites compute what they
computed before."""
import pytest
import torch
import torch.nn.functional as F

from deeplearning_amd import ops
from deeplearning_amd.engine.cli_seg import seg_criterion
from deeplearning_amd.models.segmentation import OhemCrossEntropy
from deeplearning_amd.ops.losses import dense_ce_fused


def _case(seed=0, B=2, C=5, H=7, W=9):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g) * 3
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.3] = 255
    weight = torch.rand(C, generator=g) + 0.5
    return logits, target, weight


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True])
def test_eager_path_is_f_cross_entropy(reduction, weighted):
    logits, target, weight = _case()
    w = weight if weighted else None
    assert not dense_ce_fused(logits, target)
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    got = ops.dense_cross_entropy(a, target, weight=w, ignore_index=255,
                                  reduction=reduction)
    ref = F.cross_entropy(b, target, weight=w, ignore_index=255,
                          reduction=reduction)
    assert torch.equal(got, ref)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(1))
    got.backward(gout)
    ref.backward(gout)
    assert torch.equal(a.grad, b.grad)


def test_default_ignore_index_is_255():
    logits, target, _ = _case()
    assert torch.equal(ops.dense_cross_entropy(logits, target),
                       F.cross_entropy(logits, target, ignore_index=255))


def test_bad_reduction_raises():
    logits, target, _ = _case()
    with pytest.raises(ValueError):
        ops.dense_cross_entropy(logits, target, reduction="avg")


def test_ops_cross_entropy_4d_is_f_cross_entropy():
    logits, target, _ = _case()
    target[target == 255] = -100
    assert torch.equal(ops.cross_entropy(logits, target),
                       F.cross_entropy(logits, target))
    assert torch.equal(ops.cross_entropy(logits, target, smoothing=0.1),
                       F.cross_entropy(logits, target, label_smoothing=0.1))
    crit = ops.CrossEntropyLoss(ignore_index=3)
    assert torch.equal(crit(logits, target.clamp(min=0)),
                       F.cross_entropy(logits, target.clamp(min=0),
                                       ignore_index=3))
    # 3-D [B, C, L]
    l3, t3 = logits.flatten(2), target.flatten(1)
    assert torch.equal(ops.cross_entropy(l3, t3), F.cross_entropy(l3, t3))


def test_seg_criterion_cpu_unchanged():
    logits, target, _ = _case()
    aux = _case(seed=3)[0]
    got = seg_criterion({"out": logits, "aux": aux}, target, aux_weight=0.4)
    ref = (F.cross_entropy(logits, target, ignore_index=255)
           + 0.4 * F.cross_entropy(aux, target, ignore_index=255))
    assert torch.equal(got, ref)


def _ohem_expected(logits, target, ignore, thresh, min_kept):
    """The OHEM rule written out: keep the valid pixels whose target-class
    probability is below max(thresh, the min_kept-th smallest probability)."""
    prob = F.softmax(logits, dim=1)
    losses = F.cross_entropy(logits, target, ignore_index=ignore,
                             reduction="none").view(-1)
    mask = target.view(-1) != ignore
    t = target.clone()
    t[t == ignore] = 0
    p = prob.gather(1, t.unsqueeze(1)).squeeze(1).view(-1)[mask]
    p, ind = p.sort()
    threshold = max(p[min(min_kept, p.numel() - 1)], thresh)
    return losses[mask][ind][p < threshold].mean()


@pytest.mark.parametrize("min_kept", [5, 60])
def test_ohem_cpu_unchanged(min_kept):
    logits, target, _ = _case(seed=5)
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    got = OhemCrossEntropy(min_kept=min_kept)(a, target)
    ref = _ohem_expected(b, target, 255, 0.7, min_kept)
    assert torch.equal(got, ref)
    got.backward()
    ref.backward()
    assert torch.equal(a.grad, b.grad)
