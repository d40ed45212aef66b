#!/usr/bin/env python3
"""Microbenchmark: conv1x1 MFMA kernel vs MIOpen nn.Conv2d on the ResNet-50
1x1 shapes (batch 256, bf16, channels_last), plus the fused conv+BN chain
vs conv + separate BN, and CE old-vs-new launch overhead.

Run on a GPU box:  python tools/bench_conv1x1.py [--quick]
                   python tools/bench_conv1x1.py --wgrad-ab   (wgrad only: old
                   route DLA_C1X1_WGRAD_V1=1 against new, with the byte floor)
                   python tools/bench_conv1x1.py --bwdstats-ab   (dgrad with
                   the BN backward-stats epilogue against the separate pass 1)
"""
import argparse
import os
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from deeplearning_amd.ops._ext import ext  # noqa: E402


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms


# ResNet-50 1x1 conv shapes at batch 256 / 224^2: (HW, Cin, Cout)
SHAPES = [
    (56 * 56, 256, 64),
    (56 * 56, 64, 256),
    (28 * 28, 512, 128),
    (28 * 28, 128, 512),
    (14 * 14, 1024, 256),
    (14 * 14, 256, 1024),
    (7 * 7, 2048, 512),
    (7 * 7, 512, 2048),
]


# best measured unique-byte rate of the forward kernel (802816x256x64 in
# profiles/conv1x1_bench.txt): the yardstick for the wgrad byte floor
FLOOR_GBPS = 5144.0


def wgrad_ab(B, iters):
    """wgrad only, old route (DLA_C1X1_WGRAD_V1=1: scatter staging + fp32
    atomics + zero fill) against the default one in the same process. The
    switch is read at every call. Unique bytes = 2*M*(N+K): each operand
    read once; floor = those bytes at FLOOR_GBPS."""
    print(f"batch={B}  wgrad A/B, {iters} calls per timing, best of 3 "
          "alternating rounds")
    print(f"{'shape MxKxN':>24} {'v1 ms':>8} {'v2 ms':>8} {'v1/v2':>6} "
          f"{'v2 GB/s':>8} {'floor ms':>9} {'v2/floor':>9}")
    for HW, K, N in SHAPES:
        M = B * HW
        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        best = {"1": float("inf"), "0": float("inf")}
        for _ in range(3):
            for v in ("1", "0"):
                os.environ["DLA_C1X1_WGRAD_V1"] = v
                t = timeit(lambda: ext().conv1x1_wgrad(dy, x), iters)
                best[v] = min(best[v], t)
        os.environ.pop("DLA_C1X1_WGRAD_V1")
        nbytes = 2 * M * (N + K)
        floor = nbytes / (FLOOR_GBPS * 1e9) * 1e3
        gbps = nbytes / (best["0"] * 1e-3) / 1e9
        print(f"{f'{M}x{K}x{N}':>24} {best['1']:8.3f} {best['0']:8.3f} "
              f"{best['1'] / best['0']:6.2f} {gbps:8.0f} {floor:9.3f} "
              f"{best['0'] / floor:9.2f}")


def bwdstats_ab(B, iters):
    """BN backward pass 1 in the dgrad epilogue against a pass of its own,
    per ResNet-50 shape. relu_x: conv3 dgrad feeding bn2 (N = width); join /
    join_dual: the next block's conv1 dgrad feeding a residual join (N = 4 *
    width), with the identity gradient as the GEMM's residual.
      dgrad   the plain dgrad GEMM alone
      old     dgrad + today's two-pass BN backward entry (pass 1, slab
              reduce, dx pass)
      epi     the dgrad GEMM with the epilogue alone
      red     the slab reduce alone (its slab has M/128 rows)
      new     epi + the dx-only entry (slab reduce, dx pass)
    old - new is what a step gains per call. floor: the unique bytes the
    epilogue GEMM moves (A, the [M,N] reads and the g write) at FLOOR_GBPS."""
    e = ext()
    print(f"batch={B}  backward-stats epilogue A/B, {iters} calls per timing, "
          "best of 3 alternating rounds, ms")
    print(f"{'mode':>9} {'shape MxKxN':>20} {'dgrad':>7} {'old':>7} "
          f"{'epi':>7} {'red':>7} {'new':>7} {'old-new':>8} {'epi floor':>9}")
    widths = [(56 * 56, 64), (28 * 28, 128), (14 * 14, 256), (7 * 7, 512)]
    for mode, name in ((1, "relu_x"), (2, "join"), (3, "join_dual")):
        for HW, wd in widths:
            K, N = (4 * wd, wd) if mode == 1 else (wd, 4 * wd)
            M, H = B * HW, int(HW ** 0.5)

            def nhwc(scale=1.0):
                t = torch.randn(M, N, device="cuda") * scale
                return t.to(torch.bfloat16).view(B, H, H, N) \
                    .permute(0, 3, 1, 2)

            x, xd, out = nhwc(), nhwc(), nhwc()
            dy = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            wt = (torch.randn(N, K, device="cuda") / K ** 0.5) \
                .to(torch.bfloat16)
            res = None if mode == 1 else \
                torch.randn(M, N, device="cuda").to(torch.bfloat16)
            w = torch.rand(N, device="cuda") + 0.5
            mean = torch.randn(N, device="cuda") * 0.1
            rstd = torch.rand(N, device="cuda") + 0.5
            scale, shift = w * rstd, -mean * w * rstd

            def as4(t):
                return t.view(B, H, H, N).permute(0, 3, 1, 2)

            def dgrad():
                return e.conv1x1_fwd(dy, wt, None, None, None, res, False,
                                     False)[0]

            def epi():
                return e.conv1x1_dgrad_bwdstats(
                    dy, wt, res, mode, None if mode == 1 else out, x,
                    scale if mode == 1 else None,
                    shift if mode == 1 else None, mean, rstd,
                    xd if mode == 3 else None, mean if mode == 3 else None,
                    rstd if mode == 3 else None)

            def old():
                d = as4(dgrad())
                if mode == 1:
                    return e.batchnorm_bwd_ex(d, x, None, w, mean, rstd,
                                              scale, shift, True)
                if mode == 2:
                    return e.bn_add_relu_bwd(d, out, x, w, mean, rstd)
                return e.bn_add_relu_dual_bwd(d, out, x, w, mean, rstd, xd,
                                              w, mean, rstd)

            def new():
                g, slab = epi()
                if mode == 3:
                    return e.bn_join_dual_bwd_dx_from_slab(
                        as4(g), slab, x, w, mean, rstd, xd, w, mean, rstd)
                return e.bn_bwd_dx_from_slab(as4(g), slab, x, w, mean, rstd)

            slab = epi()[1]
            fns = {"dgrad": dgrad, "old": old, "epi": epi,
                   "red": lambda: e.bn_slab_reduce(slab), "new": new}
            best = {k: float("inf") for k in fns}
            for _ in range(3):
                for k, fn in fns.items():
                    best[k] = min(best[k], timeit(fn, iters))
            tensors = {1: 2, 2: 4, 3: 5}[mode]  # [M,N] reads + the g write
            nbytes = 2 * M * (K + tensors * N)
            floor = nbytes / (FLOOR_GBPS * 1e9) * 1e3
            print(f"{name:>9} {f'{M}x{K}x{N}':>20} {best['dgrad']:7.3f} "
                  f"{best['old']:7.3f} {best['epi']:7.3f} {best['red']:7.3f} "
                  f"{best['new']:7.3f} {best['old'] - best['new']:8.3f} "
                  f"{floor:9.3f}")
    print("slab reduce alone (fixed order, two stages above 512 rows):")
    for rows, cols in ((6272, 512), (6272, 768), (1568, 1024), (392, 2048)):
        slab = torch.randn(rows, cols, device="cuda")
        t = min(timeit(lambda: e.bn_slab_reduce(slab), iters)
                for _ in range(3))
        print(f"  {rows} x {cols}: {t * 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--bwdstats-ab", action="store_true",
                    help="time the dgrad backward-stats epilogue against "
                         "the separate pass 1")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--wgrad-ab", action="store_true",
                    help="time only wgrad, old route against new")
    args = ap.parse_args()
    if args.wgrad_ab:
        wgrad_ab(args.batch, 50 if args.quick else 200)
        return
    if args.bwdstats_ab:
        bwdstats_ab(args.batch, 30 if args.quick else 100)
        return
    iters = 20 if args.quick else 50
    B = args.batch
    torch.backends.cudnn.benchmark = True

    print(f"batch={B}  (GEMM M = B*HW)")
    print(f"{'shape':>24} {'miopen':>9} {'dla':>9} {'ratio':>6} "
          f"{'dla GB/s':>9} {'dla TF':>7}")
    for HW, K, N in SHAPES:
        M = B * HW
        a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        w = torch.randn(N, K, device="cuda").to(torch.bfloat16)
        # 4d view for the conv: [B, K, H, W] channels_last
        H = int(HW ** 0.5)
        x4 = a.view(B, H, H, K).permute(0, 3, 1, 2)
        conv = torch.nn.Conv2d(K, N, 1, bias=False).cuda() \
            .to(memory_format=torch.channels_last).to(torch.bfloat16)
        conv.weight.data.copy_(w.view(N, K, 1, 1))

        t_miopen = timeit(lambda: conv(x4), iters)
        t_dla = timeit(
            lambda: ext().conv1x1_fwd(a, w, None, None, None, None, False,
                                      False), iters)
        t_dla_stats = timeit(
            lambda: ext().conv1x1_fwd(a, w, None, None, None, None, False,
                                      True), iters)
        bytes_moved = (M * K + M * N + N * K) * 2
        gbps = bytes_moved / (t_dla * 1e-3) / 1e9
        tf = 2 * M * K * N / (t_dla * 1e-3) / 1e12
        print(f"{f'{M}x{K}x{N}':>24} {t_miopen:9.3f} {t_dla:9.3f} "
              f"{t_miopen / t_dla:6.2f} {gbps:9.0f} {tf:7.1f}"
              f"   (+stats {t_dla_stats:.3f})")

        # wgrad
        dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        t_wg = timeit(lambda: ext().conv1x1_wgrad(dy, a), iters)
        # MIOpen wgrad via autograd on weight only
        x4g = x4.detach()
        wref = conv.weight
        def miopen_wgrad():
            wref.grad = None
            y = torch.nn.functional.conv2d(x4g, wref)
            y.backward(dy.view(B, H, H, N).permute(0, 3, 1, 2))
        wref.requires_grad_(True)
        t_wg_m = timeit(miopen_wgrad, iters // 2, 5)
        print(f"{'wgrad':>24} {t_wg_m:9.3f} {t_wg:9.3f} "
              f"{t_wg_m / t_wg:6.2f}   (miopen incl fwd)")

    # fused conv+bn chain vs conv + BN kernels
    print("\nconv+BN train chain (56x56x256->64 class shape):")
    from deeplearning_amd.ops.batchnorm import BatchNorm2d
    from deeplearning_amd.ops.conv1x1 import conv_bn
    B4, C, Hh, N = 256, 256, 56, 64
    x = torch.randn(B4, C, Hh, Hh, device="cuda").to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(C, N, 1, bias=False).cuda()
    bn = BatchNorm2d(N, relu=True).cuda()
    with torch.no_grad():
        t_fused = timeit(lambda: conv_bn(x, conv, bn), iters)
    convm = torch.nn.Conv2d(C, N, 1, bias=False).cuda() \
        .to(memory_format=torch.channels_last).to(torch.bfloat16)
    with torch.no_grad():
        t_sep = timeit(lambda: bn(convm(x)), iters)
    print(f"  fused {t_fused:.3f} ms  vs miopen-conv + HIP BN {t_sep:.3f} ms")

    # CE: new single-launch mean path
    print("\nCE (B=256, C=1000):")
    from deeplearning_amd.ops import cross_entropy
    logits = torch.randn(256, 1000, device="cuda").to(torch.bfloat16)
    logits.requires_grad_(True)
    tgt = torch.randint(0, 1000, (256,), device="cuda")
    def ce_step():
        logits.grad = None
        loss = cross_entropy(logits, tgt)
        loss.backward()
    t_ce = timeit(ce_step, iters)
    def ce_eager():
        logits.grad = None
        loss = torch.nn.functional.cross_entropy(logits.float(), tgt)
        loss.backward()
    t_cee = timeit(ce_eager, iters)
    print(f"  dla {t_ce:.3f} ms  eager {t_cee:.3f} ms  ratio "
          f"{t_cee / t_ce:.2f}")


if __name__ == "__main__":
    main()
