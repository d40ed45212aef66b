#!/usr/bin/env python3
"""Streaming-attention A/B (N > 256): fused_attention forward+backward
against the eager chain (the route these shapes took before the streaming
kernels), alternating rounds in one process, with the peak memory of one
forward+backward; then the forward key-panel size (DLA_ATTN_STREAM_PANEL
128 against 256) and, at ViT-B's N = 197, the resident kernels against the
streaming ones (DLA_ATTN_STREAM=1). No convs, starts in seconds.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from deeplearning_amd.ops.attention import _eager_attention, fused_attention

SHAPES = [  # (tag, B, N, H, d)
    ("vit_b16_384", 64, 577, 12, 64),
    ("vit_b16_448", 32, 785, 12, 64),
]


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available()
    for k in ("DLA_ATTN_STREAM", "DLA_ATTN_STREAM_PANEL", "DLA_FORCE_EAGER"):
        os.environ.pop(k, None)

    for tag, B, N, H, d in SHAPES:
        torch.manual_seed(0)
        qkv = torch.randn(B, N, 3 * H * d, device="cuda").bfloat16()
        g = torch.randn(B, N, H * d, device="cuda").bfloat16()
        scale = d ** -0.5

        def train(attn):
            def run():
                q = qkv.detach().requires_grad_()
                attn(q, H, scale).backward(g)
            return run

        def infer(attn):
            def run():
                with torch.no_grad():
                    attn(qkv, H, scale)
            return run

        hdr = f"{tag} B={B} N={N} H={H} d={d}"
        r = alternate({"stream": train(fused_attention),
                       "eager": train(_eager_attention)},
                      args.iters, args.rounds)
        print(f"{hdr} fwd+bwd  stream {fmt(r['stream'])}  "
              f"eager {fmt(r['eager'])}  "
              f"{statistics.median(r['eager']) / statistics.median(r['stream']):.2f}x")
        r = alternate({"stream": infer(fused_attention),
                       "eager": infer(_eager_attention)},
                      args.iters, args.rounds)
        print(f"{hdr} fwd      stream {fmt(r['stream'])}  "
              f"eager {fmt(r['eager'])}  "
              f"{statistics.median(r['eager']) / statistics.median(r['stream']):.2f}x")
        print(f"{hdr} peak of one fwd+bwd: stream "
              f"{peak_mib(train(fused_attention)):.0f} MiB, eager "
              f"{peak_mib(train(_eager_attention)):.0f} MiB")

        def panel(n):
            run = infer(fused_attention)

            def f():
                os.environ["DLA_ATTN_STREAM_PANEL"] = str(n)
                run()
            return f

        r = alternate({"p256": panel(256), "p128": panel(128)},
                      args.iters, args.rounds)
        os.environ.pop("DLA_ATTN_STREAM_PANEL", None)
        print(f"{hdr} fwd panel 256 {fmt(r['p256'])}  "
              f"panel 128 {fmt(r['p128'])}")

    # the resident domain: what forcing the streaming kernels costs there
    B, N, H, d = 256, 197, 12, 64
    qkv = torch.randn(B, N, 3 * H * d, device="cuda").bfloat16()
    g = torch.randn(B, N, H * d, device="cuda").bfloat16()

    def route(force):
        def run():
            os.environ["DLA_ATTN_STREAM"] = "1" if force else "0"
            q = qkv.detach().requires_grad_()
            fused_attention(q, H, d ** -0.5).backward(g)
        return run

    r = alternate({"resident": route(False), "stream": route(True)},
                  args.iters, args.rounds)
    os.environ.pop("DLA_ATTN_STREAM", None)
    print(f"vit_b16_224 B={B} N={N} H={H} d={d} fwd+bwd  "
          f"resident {fmt(r['resident'])}  stream {fmt(r['stream'])}")


if __name__ == "__main__":
    main()
