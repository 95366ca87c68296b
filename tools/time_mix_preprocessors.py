"""A/B timing of the geometry entry that knows the paste rectangle and of the one-launch copy_paste_mask:

  (a) a batch of CopyPaste records (kind 2, no rectangle) through hiast_aug_geometry_mix_u8 against the same records
      through hiast_aug_geometry_store_u8 (sample_aug.hip, unchanged), the C entries called directly on preallocated
      buffers, interleaved, B = 8, 1024 x 2048 frames -> 512 x 1024;
  (b) device_aug._store_copy_paste_mask (one launch of hiast_aug_paste_mask_u8) against the composition it replaces
      (per frame: torch.where over an int64 index temporary of the whole frame), B = 8 frames of 1024 x 2048.

    python tools/time_mix_preprocessors.py [--reps 30] [--warmup 5]

Each figure is the median over `reps` launches timed one by one with device events; the spread is (p10, p90)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hiast_amd import kernels as K                                   # noqa: E402
from hiast_amd.sseg.datasets import augmentations as A               # noqa: E402
from hiast_amd.sseg.datasets import device_aug as DA                 # noqa: E402
from hiast_amd.sseg.datasets import device_store as DS               # noqa: E402

B, FH, FW, OH, OW = 8, 1024, 2048, 512, 1024


def frame(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (FH, FW, 3), dtype=np.uint8), g.integers(0, 19, (FH, FW), dtype=np.uint8)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def stats(us):
    return "median %8.1f us  (p10 %8.1f, p90 %8.1f)" % (np.median(us), np.percentile(us, 10), np.percentile(us, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    frames = [(i,) + frame(60 + i) for i in range(2 * B)]
    rs = DS.ResidentSet.from_frames(frames, "cuda")
    table = np.zeros(256, np.uint8)
    table[[3, 5, 6, 7, 11, 12, 17, 18]] = 1
    samples = []
    for b in range(B):                       # the 'MS' crop: a window of 700..1000 rows at w = 2 h, flipped every other sample
        ch = 700 + 40 * b
        y1, x1 = 3 * b, 5 * b
        plan = DA.plan_sample(A.resize(OH, OW), (ch, 2 * ch))
        g = plan[0]["ops"][0][1]
        g.src, g.flip = (y1, y1 + ch, x1, x1 + 2 * ch), bool(b % 2)
        samples.append(DA.pack_store_sample(plan, b, rs.frames[b].tolist(), (B + b, rs.frames[B + b].tolist(), table)))
    t = DA.build_batch_tables(samples)
    _, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    K._aug_check_tables(t["blob"].numel(), t["tabs"].numpy(), t["recs"].numpy(), t["ops"].numpy(), oh, ow, max_ch,
                        (rs.buffer.numel(), rs.frames), t["blob"].numpy())
    blob, tabs, recs = t["blob"].cuda(), t["tabs"].cuda(), t["recs"].cuda()
    # the two C entries on the same records and the same preallocated buffers: nothing but the launches between the events
    from hiast_amd import _lib
    lib, ptr, stream = _lib.load(), K._ptr, K._stream
    bufs = [tuple(torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((B, max_ch, ow, 3), (B, oh, ow, 3), (B, oh, ow)))
            for _ in range(2)]

    def old():
        K.check(lib.hiast_aug_geometry_store_u8(ptr(recs), ptr(blob), ptr(rs.buffer), ptr(tabs), *(ptr(x) for x in bufs[0]),
                                                B, max_ch, oh, ow, stream()), "hiast_aug_geometry_store_u8")

    def new():
        K.check(lib.hiast_aug_geometry_mix_u8(ptr(recs), ptr(blob), ptr(rs.buffer), ptr(tabs), *(ptr(x) for x in bufs[1]),
                                              B, max_ch, oh, ow, stream()), "hiast_aug_geometry_mix_u8")
    old()
    new()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0][1], bufs[1][1]) and torch.equal(bufs[0][2], bufs[1][2])
    w_i, w_l = K.aug_geometry_mix_u8(blob, tabs, recs, oh, ow, max_ch, rs.buffer, host=(t["recs"], t["blob"]))
    assert torch.equal(w_i, bufs[0][1]) and torch.equal(w_l, bufs[0][2])
    print("(a) geometry, B = %d, %dx%d -> %dx%d, CopyPaste records of kind 2, interleaved A/B/A/B:" % (B, FH, FW, OH, OW))
    rounds = [timed(f, args.reps, args.warmup) for f in (old, new, old, new)]
    for name, us in zip(("store_u8  (1st)", "mix_u8    (1st)", "store_u8  (2nd)", "mix_u8    (2nd)"), rounds):
        print("    hiast_aug_geometry_%s  %s" % (name, stats(us)))
    m_old, m_new = [np.median(rounds[0]), np.median(rounds[2])], [np.median(rounds[1]), np.median(rounds[3])]
    both = np.array(rounds[0] + rounds[2])
    print("    mix / store = %.4f ; the store entry's own spread: between its two medians %.4f, p10..p90 of its launches %.4f" %
          (np.mean(m_new) / np.mean(m_old), abs(m_old[0] - m_old[1]) / np.mean(m_old),
           (np.percentile(both, 90) - np.percentile(both, 10)) / np.median(both)))

    tt = dict(t)
    tt["cp_masks"] = [None] * B

    def mask_old():
        out = torch.empty((B, FH, FW), dtype=torch.uint8, device="cuda")
        for b in range(B):
            ptab = int(t["recs"][b, DA.R_PTAB])
            src = rs.label(B + b)
            out[b] = torch.where(blob[ptab:ptab + 256][src.long()] != 0, src, torch.full_like(src, 255))
        return out

    mask_new = lambda: DA._store_copy_paste_mask(tt, rs, torch.device("cuda"))                      # noqa: E731
    assert torch.equal(mask_old(), mask_new())
    print("(b) copy_paste_mask, B = %d frames of %dx%d:" % (B, FH, FW))
    rounds = [timed(f, args.reps, args.warmup) for f in (mask_old, mask_new, mask_old, mask_new)]
    for name, us in zip(("torch.where per frame (1st)", "_store_copy_paste_mask (1st)", "torch.where per frame (2nd)",
                         "_store_copy_paste_mask (2nd)"), rounds):
        print("    %-30s %s" % (name, stats(us)))
    print("    old / new = %.2f" % ((np.median(rounds[0]) + np.median(rounds[2])) / (np.median(rounds[1]) + np.median(rounds[3]))))


if __name__ == "__main__":
    main()
