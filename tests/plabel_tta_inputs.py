"""Inputs and the oracle chain of the multi-view pass-1 tests (a plain helper module, no fixtures; numpy + the C oracle only).

view_logits: one base map N(0, 40) at 5 x 9 per image and class, resampled (align_corners, the oracle's resample) to each view's
low-res size, plus N(0, 0.3) noise per view; the mirror view comes from the column-reversed base with its own noise.  A view whose
low-res map is smaller than the base (17 x 33 -> 3 x 5) takes the same resample, which there keeps every second node: all views
of a frame then show the SAME scene.  (Cutting the top-left 3 x 5 nodes out of the base instead makes that view and its mirror
image show other parts of the scene than the rest; no pixel then reaches the top 128 bins at 19 classes — 18 / 82 / 0 % — and
the shares asserted below cannot hold.)  The views agree on most of the frame and disagree near the class borders: the mean
confidence covers everything from below 0.5 to exactly 1.0, so the LDS-counted top bins, the wave-aggregated keys and the
single-lane keys of the kernel all occur.  Shares at 33 x 65, three sizes + flip, seeds as used by the tests (below 0.5 / up to
the top 128 bins / top 128 bins): C = 19: 15 / 71 / 14 %, 16: 11 / 65 / 24 %, 9: 7 / 65 / 28 %, 2: 0 / 59 / 41 %.
"""
import functools

import numpy as np

import synth
from oracle import cref

NBINS = 15361
UPLO = 0x3800                   # fp16(0.5)
TOP = NBINS - 128               # first of the top 128 bins
BASE_SD, NOISE_SD = 40.0, 0.3


def lows(sizes):
    """low-res head map of a view resized to (Hs, Ws): the 1/8 map of the segmentor"""
    return [((Hs - 1) // 8 + 1, (Ws - 1) // 8 + 1) for Hs, Ws in sizes]


def _resampled(base, hs, ws):
    return cref.upsample_bilinear_ac(base, hs, ws)


@functools.lru_cache(maxsize=None)
def view_logits(seed, B, C, sizes, flip, tie=False):
    """-> (zs, zfs or None): lists of fp32 [B,C,hs,ws].  tie: class plane 1 is a copy of plane 0 in every view."""
    g = synth.rng(seed)
    base = (g.standard_normal((B, C, 5, 9)) * BASE_SD).astype(np.float32)
    zs, zfs = [], []
    for hs, ws in lows(sizes):
        zs.append(_resampled(base, hs, ws) + (g.standard_normal((B, C, hs, ws)) * NOISE_SD).astype(np.float32))
        if flip:
            zfs.append(_resampled(np.ascontiguousarray(base[:, :, :, ::-1]), hs, ws)
                       + (g.standard_normal((B, C, hs, ws)) * NOISE_SD).astype(np.float32))
    if tie:
        for z in zs + zfs:
            z[:, 1] = z[:, 0]
    for z in zs + zfs:
        z.setflags(write=False)
    return zs, (zfs if flip else None)


def oracle_chain(zs, zfs, sizes, H, W):
    """the issue's reference chain -> (maxprob f32 [B,H,W], argmax u8 [B,H,W], hist u32 [C,NBINS], probsum f32 [B,C,H,W])"""
    C = zs[0].shape[1]
    n_views = len(zs) * (2 if zfs is not None else 1)
    probs, label = cref.tta(list(zs), list(zfs) if zfs is not None else None, sizes, H, W)
    maxprob = np.minimum(probs.max(1) / np.float32(n_views), np.float32(1)).astype(np.float32)
    return maxprob, label, cref.plabel_hist(maxprob, label, C), probs


@functools.lru_cache(maxsize=None)
def case(seed, B, C, H, W, sizes, flip, tie=False):
    """inputs + oracle outputs of one case, computed once per session and shared (read-only)"""
    zs, zfs = view_logits(seed, B, C, sizes, flip, tie)
    out = oracle_chain(zs, zfs, sizes, H, W)
    for a in out:
        a.setflags(write=False)
    return (zs, zfs) + out


def shares(maxprob):
    """fractions of the pixels below fp16 0.5, from 0.5 to below the top 128 bins, in the top 128 bins"""
    bins = maxprob.astype(np.float16).view(np.uint16).astype(np.int64)
    return float((bins < UPLO).mean()), float(((bins >= UPLO) & (bins < TOP)).mean()), float((bins >= TOP).mean())
