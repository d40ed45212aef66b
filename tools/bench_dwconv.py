#!/usr/bin/env python3
"""Depthwise conv: the HIP kernels of csrc/dwconv.hip against aten (MIOpen)
on the same tensors, bf16 channels_last, batch 64.

Per-shape table (default):
    python tools/bench_dwconv.py [--window-ms T]
  times forward, dgrad and wgrad (+dbias) of the HIP route and forward /
  backward of aten for ConvNeXt-T's four 7x7 shapes and every distinct
  depthwise (H, C, K, stride) of EfficientNet-B0 at 224^2, prints each HIP
  time as a fraction of its byte floor (compulsory reads + writes over the
  8.0 TB/s HBM peak) and the per-(K, stride) family sums the default routing
  table of ops/dwconv.py is decided by.

Whole-step A/B:
    python tools/bench_dwconv.py --model-step convnext_tiny [--rounds 3]
  times a channels_last bf16-autocast train step (batch 64, 224^2, SGD) under
  DLA_DWCONV=0 and =1 in fresh child processes, alternating, each child under
  its own time limit; the first failing child ends the run.

Times are device-event times after warm-up. Needs a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12  # bytes/s, spec
BATCH = 64

CONVNEXT_T = [(56, 96, 7, 1), (28, 192, 7, 1), (14, 384, 7, 1),
              (7, 768, 7, 1)]


def efficientnet_b0_shapes(image=224):
    """Distinct depthwise (H, C, K, stride) of EfficientNet-B0, in order."""
    from deeplearning_amd.models.classification.efficientnet import \
        _B0_STAGES

    shapes, h, cin = [], image // 2, 32
    for expand, k, stride, c, repeats in _B0_STAGES:
        for i in range(repeats):
            s = stride if i == 0 else 1
            shape = (h, cin * expand, k, s)
            if shape not in shapes:
                shapes.append(shape)
            h = (h - 1) // s + 1
            cin = c
    return shapes


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def _iters_for(fn, window_ms, lo, hi):
    """Calls that fill `window_ms`, from a short timed probe after warm-up."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = _events(2)
    t0.record()
    for _ in range(5):
        fn()
    t1.record()
    torch.cuda.synchronize()
    per_call = max(t0.elapsed_time(t1) / 5, 1e-3)
    return int(min(max(window_ms / per_call, lo), hi))


def time_loop(fn, window_ms):
    """ms per call: one event pair around enough back-to-back calls to fill
    `window_ms` (a window of a few ms times the clock ramp, not the kernel)."""
    iters = _iters_for(fn, window_ms, 20, 20000)
    torch.cuda.synchronize()
    t0, t1 = _events(2)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def time_second(setup, fn, window_ms):
    """ms per fn(state) with state = setup() redone, untimed, before each."""
    iters = _iters_for(lambda: fn(setup()), window_ms, 20, 400)
    torch.cuda.synchronize()
    starts, ends = _events(iters), _events(iters)
    for a, b in zip(starts, ends):
        state = setup()
        a.record()
        fn(state)
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in zip(starts, ends)) / iters


def bench_shape(H, C, K, stride, bias, window_ms):
    from deeplearning_amd.ops._ext import ext

    g = torch.Generator(device="cuda").manual_seed(H * 1000 + C + K + stride)
    x = torch.randn(BATCH, C, H, H, device="cuda", generator=g) \
        .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w32 = torch.randn(C, 1, K, K, device="cuda", generator=g) * 0.1
    b32 = torch.randn(C, device="cuda", generator=g) if bias else None
    wa = w32.to(torch.bfloat16).requires_grad_(True)  # what autocast hands aten
    ba = b32.to(torch.bfloat16).requires_grad_(True) if bias else None
    xa = x.clone().requires_grad_(True)
    p = (K - 1) // 2

    y = ext().dwconv_fwd(x, w32, b32, stride)
    dy = torch.randn(y.shape, device="cuda", generator=g).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    ya = F.conv2d(xa, wa, ba, stride, p, 1, C)
    diff = float((y.float() - ya.float()).abs().max() /
                 ya.float().abs().max())

    t = {
        "fwd": time_loop(
            lambda: ext().dwconv_fwd(x, w32, b32, stride), window_ms),
        "dgrad": time_loop(
            lambda: ext().dwconv_dgrad(dy, w32, H, H, stride), window_ms),
        "wgrad": time_loop(
            lambda: ext().dwconv_wgrad(dy, x, K, stride, True), window_ms),
        "aten_fwd": time_loop(
            lambda: F.conv2d(x, wa.detach(), None if ba is None
                             else ba.detach(), stride, p, 1, C), window_ms),
    }
    leaves = [xa, wa] + ([ba] if bias else [])
    t["aten_bwd"] = time_second(
        lambda: F.conv2d(xa, wa, ba, stride, p, 1, C),
        lambda out: torch.autograd.grad(out, leaves, dy), window_ms)
    n_in, n_out = x.numel(), y.numel()
    floor_ms = (n_in + n_out) * 2 / HBM_PEAK * 1e3  # same bytes each way
    t["floor"] = floor_ms
    t["diff"] = diff
    return t


def per_shape(args):
    torch.backends.cudnn.benchmark = True
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
          f"bf16 channels_last, batch {BATCH}, >= {args.window_ms:.0f} ms timed "
          "per figure, ms")
    print("# floor = (elements read + written) * 2 B / 8.0 TB/s; 'of floor' "
          "= floor / time per HIP kernel")
    print(f"{'H':>4} {'C':>5} {'K':>2} {'s':>2} | {'fwd':>7} {'dgrad':>7} "
          f"{'wgrad':>7} {'sum':>7} | {'aten f':>7} {'aten b':>7} "
          f"{'sum':>7} | {'aten/hip':>8} | {'of floor f/d/w':>16} | "
          f"{'max rel diff':>12}")
    fam = {}
    sets = [("ConvNeXt-T", CONVNEXT_T, True),
            ("EfficientNet-B0", efficientnet_b0_shapes(), False)]
    for label, shapes, bias in sets:
        print(f"# {label}")
        for H, C, K, s in shapes:
            t = bench_shape(H, C, K, s, bias, args.window_ms)
            hip = t["fwd"] + t["dgrad"] + t["wgrad"]
            aten = t["aten_fwd"] + t["aten_bwd"]
            fr = "/".join(f"{t['floor'] / t[k]:.2f}"
                          for k in ("fwd", "dgrad", "wgrad"))
            print(f"{H:>4} {C:>5} {K:>2} {s:>2} | {t['fwd']:7.3f} "
                  f"{t['dgrad']:7.3f} {t['wgrad']:7.3f} {hip:7.3f} | "
                  f"{t['aten_fwd']:7.3f} {t['aten_bwd']:7.3f} {aten:7.3f} | "
                  f"{aten / hip:8.2f} | {fr:>16} | {t['diff']:12.2e}",
                  flush=True)
            a = fam.setdefault((K, s), [0.0, 0.0])
            a[0] += hip
            a[1] += aten
    print("# family sums over the shapes above (fwd + dgrad + wgrad), ms")
    for (K, s), (hip, aten) in sorted(fam.items()):
        print(f"family K={K} s={s}: hip {hip:.3f}  aten {aten:.3f}  "
              f"aten/hip {aten / hip:.2f}")


def child_step(args):
    """One process, one setting of DLA_DWCONV: print a JSON line."""
    from deeplearning_amd.models import build_model

    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    model = build_model(args.child, num_classes=1000).cuda() \
        .to(memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.0, momentum=0.9)
    x = torch.randn(BATCH, 3, 224, 224, device="cuda") \
        .contiguous(memory_format=torch.channels_last)
    tgt = torch.randint(0, 1000, (BATCH,), device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(model(x).float(), tgt)
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    t0, t1 = _events(2)
    t0.record()
    for _ in range(args.steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({
        "model": args.child, "DLA_DWCONV": os.environ.get("DLA_DWCONV"),
        "ms_per_step": round(t0.elapsed_time(t1) / args.steps, 3),
        "steps": args.steps, "warmup": args.warmup, "batch": BATCH,
        "loss": round(float(loss), 6)}))


def model_ab(args):
    print(f"# {args.model_step}: channels_last bf16-autocast train step, "
          f"batch {BATCH}, 224^2, {args.steps} steps after {args.warmup} "
          "warm-up; fresh child per line, alternating")
    times = {"0": [], "1": []}
    for r in range(args.rounds):
        for mode in ("0", "1"):
            env = dict(os.environ, DLA_DWCONV=mode)
            cmd = ["timeout", "-k", "10", str(args.child_timeout),
                   sys.executable, str(Path(__file__).resolve()),
                   "--child", args.model_step, "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            out = subprocess.run(cmd, env=env, cwd=ROOT, text=True,
                                 stdout=subprocess.PIPE)
            if out.returncode != 0:
                print(f"# child DLA_DWCONV={mode} round {r + 1} exited "
                      f"{out.returncode}; stopping", flush=True)
                return out.returncode
            line = out.stdout.strip().splitlines()[-1]
            times[mode].append(json.loads(line)["ms_per_step"])
            print(f"DLA_DWCONV={mode} run {r + 1}: {line}", flush=True)
    for mode in ("0", "1"):
        v = times[mode]
        print(f"# DLA_DWCONV={mode}: {min(v):.3f}-{max(v):.3f} ms/step")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window-ms", type=float, default=150.0,
                    help="timed window per figure (per-shape table)")
    ap.add_argument("--model-step", metavar="NAME")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", metavar="NAME", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.model_step:  # the parent never touches the GPU
        return model_ab(args)
    if not torch.cuda.is_available():
        sys.exit("bench_dwconv.py measures on the GPU; none is available")
    if args.child:
        return child_step(args)
    return per_shape(args)


if __name__ == "__main__":
    sys.exit(main())
