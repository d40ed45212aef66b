#!/usr/bin/env python3
"""Dense (per-pixel) cross-entropy A/B: the fused op (csrc/dense_ce.hip)
against the eager chain (F.cross_entropy under bf16 autocast, the route of
DLA_DENSE_CE=0), alternating rounds in one process: forward, forward+backward,
the peak memory of one forward+backward, and the achieved bytes/s against the
byte floors (S = the logits' bytes: forward reads S, backward reads S and
writes S). Both layouts, then an OHEM call. --e2e adds one segmentation train
step with the gate off and on. Prints to stdout and to --out.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch
import torch.nn.functional as F

from deeplearning_amd.models.segmentation import OhemCrossEntropy
from deeplearning_amd.ops import dense_cross_entropy

SHAPES = [  # (tag, B, C, H, W)
    ("voc_480", 8, 21, 480, 480),
    ("cityscapes_512x1024", 4, 19, 512, 1024),
]
OHEM_SHAPE = SHAPES[1]


def timeit(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(fns, iters, rounds, warmup=5):
    """fns: {name: callable}. Returns {name: [ms per round]}, the versions
    taking turns inside every round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timeit(fn, iters))
    return out


def fmt(ts):
    return (f"{statistics.median(ts):8.3f} ms (min {min(ts):.3f} "
            f"max {max(ts):.3f})")


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def gated(on, fn):
    def run():
        os.environ["DLA_DENSE_CE"] = "1" if on else "0"
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return fn()
    return run


def make(B, C, H, W, layout):
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device="cuda").bfloat16()
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, C, (B, H, W), device="cuda")
    t[torch.rand(B, H, W, device="cuda") < 0.1] = 255
    return x, t


def e2e(say, model_name, iters, rounds):
    from deeplearning_amd.engine.cli_seg import seg_criterion
    from deeplearning_amd.models import build_model

    torch.manual_seed(0)
    model = build_model(model_name, num_classes=21).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=0.0, momentum=0.9)
    x = torch.randn(8, 3, 480, 480, device="cuda")
    y = torch.randint(0, 21, (8, 480, 480), device="cuda")

    def step():
        loss = seg_criterion(model(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    r = alternate({"fused": gated(True, step), "eager": gated(False, step)},
                  iters, rounds, warmup=3)
    say(f"{model_name} train step B=8 480x480 bf16  DLA_DENSE_CE=1 "
        f"{fmt(r['fused'])}  DLA_DENSE_CE=0 {fmt(r['eager'])}  "
        f"{statistics.median(r['eager']) / statistics.median(r['fused']):.3f}x")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--e2e", default="",
                   help="model for one train-step pair, e.g. fcn_resnet50")
    p.add_argument("--out", default=str(
        Path(__file__).resolve().parents[1] / "profiles" / "dense_ce_ab.txt"))
    args = p.parse_args()
    assert torch.cuda.is_available()
    os.environ.pop("DLA_FORCE_EAGER", None)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_dense_ce.py, one process, {args.rounds} alternating "
        f"rounds of {args.iters} iterations (median, min, max), bf16 logits.")
    say("# eager = F.cross_entropy under bf16 autocast (DLA_DENSE_CE=0). "
        "S = the logits' bytes; floors: fwd S, bwd 2S.")

    for tag, B, C, H, W in SHAPES:
        for layout in ("nchw", "channels_last"):
            x, t = make(B, C, H, W, layout)
            S = x.numel() * x.element_size()

            def train():
                q = x.detach().requires_grad_()
                dense_cross_entropy(q, t).backward()

            def infer():
                with torch.no_grad():
                    dense_cross_entropy(x, t)

            hdr = f"{tag} {B}x{C}x{H}x{W} {layout} S={S / 2 ** 20:.0f} MiB"
            fb = alternate({"fused": gated(True, train),
                            "eager": gated(False, train)},
                           args.iters, args.rounds)
            f = alternate({"fused": gated(True, infer),
                           "eager": gated(False, infer)},
                          args.iters, args.rounds)
            mf, me = (statistics.median(f[k]) for k in ("fused", "eager"))
            mfb, meb = (statistics.median(fb[k]) for k in ("fused", "eager"))
            say(f"{hdr} fwd      fused {fmt(f['fused'])}  eager "
                f"{fmt(f['eager'])}  {me / mf:.2f}x")
            say(f"{hdr} fwd+bwd  fused {fmt(fb['fused'])}  eager "
                f"{fmt(fb['eager'])}  {meb / mfb:.2f}x")
            say(f"{hdr} fused bytes/s at the floor: fwd {S / mf / 1e9:.2f} TB/s"
                f", fwd+bwd {3 * S / mfb / 1e9:.2f} TB/s, bwd alone "
                f"{2 * S / max(mfb - mf, 1e-9) / 1e9:.2f} TB/s")
            say(f"{hdr} peak of one fwd+bwd: fused "
                f"{peak_mib(gated(True, train)):.0f} MiB "
                f"({peak_mib(gated(True, train)) * 2 ** 20 / S:.2f} S), eager "
                f"{peak_mib(gated(False, train)):.0f} MiB "
                f"({peak_mib(gated(False, train)) * 2 ** 20 / S:.2f} S)")
            del x, t

    tag, B, C, H, W = OHEM_SHAPE
    ohem = OhemCrossEntropy(min_kept=100000)
    for layout in ("nchw", "channels_last"):
        x, t = make(B, C, H, W, layout)

        def train():
            q = x.detach().requires_grad_()
            ohem(q, t).backward()

        r = alternate({"fused": gated(True, train),
                       "eager": gated(False, train)}, args.iters, args.rounds)
        hdr = f"OHEM {tag} {B}x{C}x{H}x{W} {layout}"
        say(f"{hdr} fwd+bwd  fused {fmt(r['fused'])}  eager {fmt(r['eager'])}"
            f"  {statistics.median(r['eager']) / statistics.median(r['fused']):.2f}x")
        say(f"{hdr} peak of one fwd+bwd: fused "
            f"{peak_mib(gated(True, train)):.0f} MiB, eager "
            f"{peak_mib(gated(False, train)):.0f} MiB")
        del x, t

    if args.e2e:
        e2e(say, args.e2e, max(args.iters // 4, 3), args.rounds)
    os.environ.pop("DLA_DENSE_CE", None)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
