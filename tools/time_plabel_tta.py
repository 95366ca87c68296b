"""Kernel-level timing of the multi-view pseudo-label pass 1 (hiast_plabel_pass1_tta) at the workload's own size against the two
calls it stands in for: hiast_tta_fused (label only) + hiast_plabel_pass1 (with workspace), same inputs, same process, alternating,
device events, median of the repeats.  Also times the entry's direct form (HIAST_PLTTA_FORM=direct) and checks that both forms
give the same bits.
    python tools/time_plabel_tta.py [B=8] [repeats=15] [launches per window=10]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from hiast_amd import kernels as K  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 15
INNER = int(sys.argv[3]) if len(sys.argv) > 3 else 10
C, H, W = 19, 512, 1024
SIZES = [(384, 768), (512, 1024), (640, 1280)]
assert torch.cuda.is_available(), "this measurement needs the GPU"

zs = [torch.from_numpy(synth.smooth_logits_lr(3300 + i, B, C, s[0] // 8, s[1] // 8)).cuda() for i, s in enumerate(SIZES)]
zfs = [torch.from_numpy(synth.smooth_logits_lr(3310 + i, B, C, s[0] // 8, s[1] // 8)).cuda() for i, s in enumerate(SIZES)]
hist = torch.zeros((C, 15361), dtype=torch.int32, device="cuda")


def form(name):
    if name:
        os.environ["HIAST_PLTTA_FORM"] = name
    else:
        os.environ.pop("HIAST_PLTTA_FORM", None)


def tta_tiled():
    form("")
    return K.plabel_pass1_tta(zs, zfs, SIZES, H, W, hist=hist)


def tta_direct():
    form("direct")
    try:
        return K.plabel_pass1_tta(zs, zfs, SIZES, H, W, hist=hist)
    finally:
        form("")


OPS = [("hiast_tta_fused (label only)", lambda: K.tta_fused(zs, zfs, SIZES, H, W, want_probs=False, want_label=True)),
       ("hiast_plabel_pass1 (workspace)", lambda: K.plabel_pass1(zs[1], H, W, hist=hist)),
       ("hiast_plabel_pass1_tta, tiled form", tta_tiled),
       ("hiast_plabel_pass1_tta, direct form", tta_direct)]

a, b = tta_tiled(), tta_direct()
_, label = OPS[0][1]()
torch.cuda.synchronize()
same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a[:2], b[:2])) and torch.equal(a[1], label)
print("tiled and direct form: same maxprob / argmax bits, argmax == hiast_tta_fused's label: %s" % same, flush=True)
assert same

for _ in range(3):                                   # warm-up of every shape the timed windows use
    for _, f in OPS:
        f()
torch.cuda.synchronize()
times = {n: [] for n, _ in OPS}
for _ in range(REP):                                 # alternating: every repeat times each call once
    for n, f in OPS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            f()
        e1.record()
        e1.synchronize()
        times[n].append(e0.elapsed_time(e1) / INNER)
med = {n: float(np.median(v)) for n, v in times.items()}
print("B = %d, C = %d, %d x %d native, sizes %s + mirror images, smooth logits; per call, median of %d windows of %d launches "
      "(min .. max)" % (B, C, H, W, SIZES, REP, INNER))
for n, _ in OPS:
    print("  %-38s %8.3f ms   (%.3f .. %.3f)" % (n, med[n], min(times[n]), max(times[n])))
parent = med[OPS[0][0]] + med[OPS[1][0]]
print("  tta_fused + plabel_pass1 = %.3f ms; the new entry (default = tiled form) %.3f ms, direct form %.3f ms: the entry takes "
      "%s than the two calls" % (parent, med[OPS[2][0]], med[OPS[3][0]], "no longer" if med[OPS[2][0]] <= parent else "LONGER"))
