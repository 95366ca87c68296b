"""Forward + backward of FCDiscriminator's five 4x4 / stride-2 convolutions: the library path (F.conv2d = MIOpen) against the
project's own kernels (HIAST_DISC_HIP, hiast_disc_conv_*), in ONE process on one GPU.

    python tools/bench_disc_conv.py [--batches 2 8] [--size 512 1024] [--rounds 5] [--iters 10] [--16bit] [--out profiles/NAME.txt]

Paths: `library` and `own` in fp32; with --16bit also `library-fp16` (F.conv2d under torch.autocast(fp16)) and `own-16bit`
(HIAST_DISC_HIP + HIAST_DISC_HIP_16BIT under the same autocast: hiast_disc_conv16_*, fp16 operands, fp32 accumulation, fp32
storage); their loss is scaled by 2^16 as a GradScaler starts out, and the gradients are unscaled before they are compared.
Per batch size: every path is warmed up at the timed shape (code objects, MIOpen's algorithm search), then timed in
alternating rounds (library, own, ..., library, own, ...) with device events around `iters` iterations each; the report gives
the median round, the fastest and slowest round (the spread) and the achieved FLOP/s from the operation count of the shapes
(forward + input gradient + weight gradient = 3 x forward).  It also compares each own path's outputs and gradients with its
library counterpart on the same seeded input.  Needs a GPU: there is no CPU fall-back."""
import argparse
import os
import statistics
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def chain_flops(B, C, H, W):
    """multiply-adds x 2 of the five forward convolutions"""
    chans = [C, 64, 128, 256, 512, 1]
    total = 0
    for i in range(5):
        H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        total += 2 * B * H * W * chans[i + 1] * chans[i] * 16
    return total


# name -> (HIAST_DISC_HIP, HIAST_DISC_HIP_16BIT, autocast type or None, the library path it is compared with)
PATHS = {"library": (False, False, None, None), "own": (True, False, None, "library"),
         "library-fp16": (False, False, torch.float16, None), "own-16bit": (True, True, torch.float16, "library-fp16")}


def select(SW, name):
    hip, bit16, amp, _ = PATHS[name]
    SW.OPT_IN["HIAST_DISC_HIP"] = hip
    SW.OPT_IN["HIAST_DISC_HIP_16BIT"] = bit16
    return amp


LOSS_SCALE = 65536.0      # of the autocast paths: a GradScaler's initial scale (unscaled, fp16 gradients of this loss underflow)


def step(D, x, amp=None):
    x.grad = None
    D.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=amp or torch.float16, enabled=amp is not None):
        out = D(x)
        loss = F.binary_cross_entropy_with_logits(out, torch.zeros_like(out))
    (loss if amp is None else loss * LOSS_SCALE).backward()
    return out, loss


def timed(D, x, iters, amp=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step(D, x, amp)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--size", type=int, nargs=2, default=[512, 1024])
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--16bit", dest="bit16", action="store_true", help="also time F.conv2d and the own 16-bit path under autocast(fp16)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_disc_conv needs the GPU: nothing is measured without one")
    from hiast_amd import switches as SW
    from hiast_amd.sseg.models.modules.discriminator import FCDiscriminator
    torch.backends.cudnn.benchmark = False
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    H, W = args.size
    C = args.classes
    names = ["library", "own"] + (["library-fp16", "own-16bit"] if args.bit16 else [])
    say("# FCDiscriminator forward + backward, %s, %d x %d x %d input; %s; torch %s" % (
        "fp32 and autocast(fp16)" if args.bit16 else "fp32", C, H, W, torch.cuda.get_device_name(0), torch.__version__))
    say("# rounds=%d (alternating %s), iters per round=%d, warm-up iterations per path=%d" % (
        args.rounds, " / ".join(names), args.iters, args.warmup))
    torch.manual_seed(0)
    D = FCDiscriminator(C).cuda()
    for B in args.batches:
        x = torch.softmax(torch.randn(B, C, H, W, device="cuda") * 2.0, 1).requires_grad_(True)
        res, outs = {n: [] for n in names}, {}
        for name in names:
            amp = select(SW, name)
            for _ in range(args.warmup):
                step(D, x, amp)
            out, loss = step(D, x, amp)
            unscale = 1.0 if amp is None else 1.0 / LOSS_SCALE
            outs[name] = (out.detach().float().clone(),) + tuple(
                t.detach().float() * unscale for t in (x.grad, D.conv1.weight.grad, D.conv4.weight.grad))
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name in names:
                res[name].append(timed(D, x, args.iters, select(SW, name)))
        select(SW, "library")
        fl = 3 * chain_flops(B, C, H, W)
        med = {}
        for name in names:
            t = res[name]
            med[name] = statistics.median(t)
            say("B=%d %-12s median %8.3f ms  (min %8.3f  max %8.3f over %d rounds)  %6.1f TFLOP/s of %.1f GFLOP" % (
                B, name, med[name], min(t), max(t), len(t), fl / med[name] / 1e9, fl / 1e9))
        for name in names:
            ref = PATHS[name][3]
            if ref is None:
                continue
            say("B=%d %s / %s = %.2f  (%s is faster)" % (B, name, ref, med[name] / med[ref],
                                                         name if med[name] < med[ref] else ref))
            for what, a, b in zip(("logits", "dx", "dW conv1", "dW conv4"), outs[ref], outs[name]):
                say("B=%d   max |%s - %s| / max |%s|, %-9s %.3e" % (
                    B, name, ref, ref, what + ":", float((a - b).abs().max()) / max(float(a.abs().max()), 1e-30)))
        if args.bit16:
            say("B=%d own-16bit / own = %.2f;  fastest of library-fp16, own-16bit, own: %s" % (
                B, med["own-16bit"] / med["own"], min(("library-fp16", "own-16bit", "own"), key=lambda n: med[n])))
        del x, outs
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
