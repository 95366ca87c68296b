"""PREPROCESSOR['CopyPaste'] — HIAST's hard-aware pseudo-label augmentation
(reference: sseg/datasets/preprocessor.py:12-122).

Hard classes = the `selected_num_classes` classes with the lowest mean confidence (from
class_mean_probabilities.npy written by the generator); a class is drawn with probability
∝ (1 - value)^2, one pseudo-labelled image containing it is drawn, and every hard-class pixel of that
image is pasted (image bytes + label) onto the current sample.  Runs on the host inside DataLoader
workers on uint8 arrays (byte copies; nothing for a GPU to win).  The np.random call sequence is the
reference's, so a seeded run reproduces its outputs (tests/golden/copy_paste.npz).

Deviation (documented in DESIGN.md): for SYNTHIA the reference sets the three absent classes'
value to inf, which turns the sampling probabilities into NaN and makes np.random.choice raise
(preprocessor.py:18-19,31-40); here those classes get probability 0 instead.

PREPROCESSOR['ClassMix'] and PREPROCESSOR['CutMix'] — the two other values the reference documents for
cfg.preprocessor.type and does not build (additions).  Both share CopyPaste's surface (run, run_plan,
run_plan_index) and are pure plans: a source index, a class table and, for CutMix, a rectangle, all drawn from
np.random in a documented order that reads no pixel, so the same draws serve the worker path, the bytes path and the
path over device-resident frames.  A paste tuple of theirs may carry a 4th element, rect = (y0, y1, x0, x1) in frame
coordinates, half-open; absent or None = the whole frame (what CopyPaste returns)."""
import math

import numpy as np
from PIL import Image

from hiast_amd.utils.registry.registries import PREPROCESSOR


@PREPROCESSOR.register("CopyPaste")
class CopyPaste:

    def __init__(self, cfg, dataset_copy_from, init_class_value):
        self.cfg = cfg
        self.dataset_copy_from = dataset_copy_from
        self.ignored_classes = [9, 14, 16] if cfg.dataset.source.type == "SYNTHIA" else None
        print("%% Init copy paste with class_value: {}".format(init_class_value))
        self.class_value, self.hard_classes = self.get_hard_classes(np.array(init_class_value, dtype=np.float64))
        self.samples_with_class = self.dataset_copy_from.get_samples_with_class()
        self.class_probs = self.calculate_class_probs()

    def calculate_class_probs(self):
        v = np.asarray(self.class_value, np.float64)
        p = np.where(np.isinf(v), 0.0, (1 - np.where(np.isinf(v), 1.0, v)) ** 2)
        if p.sum() <= 0:                   # every class at confidence 1.0: fall back to uniform over finite classes
            p = np.where(np.isinf(v), 0.0, 1.0)
        return p / p.sum()

    def get_hard_classes(self, class_value):
        if self.ignored_classes is not None:
            for c in self.ignored_classes:
                class_value[c] = np.inf
        hard = np.argsort(class_value)[:self.cfg.preprocessor.copy_paste.selected_num_classes]
        return class_value, hard

    @staticmethod
    def resize(img, lbl, shape):
        h, w = shape[0], shape[1]
        img = np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
        lbl = np.asarray(Image.fromarray(lbl).resize((w, h), Image.NEAREST))
        return img, lbl

    def run(self, img, lbl):
        if self.cfg.preprocessor.copy_paste.mode != "original":
            raise NotImplementedError("copy_paste.mode %r" % self.cfg.preprocessor.copy_paste.mode)
        return self.run_original(img, lbl)

    def run_plan(self, img, lbl):
        """the device_aug form of run(): the same np.random draws and the same source image, but nothing is composited —
        -> ((source image, source label, uint8[256] table: 1 = hard class) or None, copy_paste_mask).  The device takes the
        composite per pixel (table[lbl_src] ? source : own) on the crop window before it resamples; a per-pixel select
        commutes with the crop, so the result is run_original()'s followed by the crop.  The mask stays host-computed at
        native resolution."""
        if self.cfg.preprocessor.copy_paste.mode != "original":
            raise NotImplementedError("copy_paste.mode %r" % self.cfg.preprocessor.copy_paste.mode)
        mask = np.full(lbl.shape, 255, dtype=np.uint8)
        c = self.random_select(self.hard_classes)
        if c is None:
            return None, mask
        name = np.random.choice(self.samples_with_class[c])
        img_, lbl_, _ = self.dataset_copy_from.load_data(self.dataset_copy_from.get_file_to_idx(name))
        if img.shape != img_.shape:
            img_, lbl_ = self.resize(img_, lbl_, lbl.shape)
        table = np.zeros(256, dtype=np.uint8)
        table[np.asarray(self.hard_classes, dtype=np.int64)] = 1
        np.copyto(mask, lbl_, where=table[lbl_] != 0)
        return (img_, lbl_, table), mask

    def run_plan_index(self):
        """run_plan() for device-resident frames (device_store.py): the same np.random draws, but the source stays where it
        is — -> (dataset index of the source image in dataset_copy_from, uint8[256] table) or (None, None).  Nothing is
        decoded: the caller addresses the source in the store, or restores the generators and takes run_plan()."""
        if self.cfg.preprocessor.copy_paste.mode != "original":
            raise NotImplementedError("copy_paste.mode %r" % self.cfg.preprocessor.copy_paste.mode)
        c = self.random_select(self.hard_classes)
        if c is None:
            return None, None
        name = np.random.choice(self.samples_with_class[c])
        table = np.zeros(256, dtype=np.uint8)
        table[np.asarray(self.hard_classes, dtype=np.int64)] = 1
        return self.dataset_copy_from.get_file_to_idx(name), table

    def random_select(self, selected_classes):
        """rejection-sample a hard class (preprocessor.py:70-77).  Deviations: a class that no pseudo-labelled
        image contains is rejected too (the reference would raise in np.random.choice on its empty file list), and
        after 64 rejections the class is drawn directly from the distribution renormalised over the usable classes
        (the reference's loop is unbounded: with nearly all probability mass on unusable classes it spins for
        ~1/P(usable) draws).  With every hard class populated the draw sequence is identical to the reference's."""
        ids = [i for i in range(self.cfg.dataset.num_classes)]
        usable = [c for c in selected_classes if len(self.samples_with_class.get(int(c), [])) > 0]
        if not usable:
            return None
        p_usable = self.class_probs[np.asarray(usable, dtype=int)]
        if float(np.sum(p_usable)) <= 0.0:
            return np.random.choice(usable)     # degenerate: all usable classes have sampling probability 0
        for _ in range(64):
            c = np.random.choice(ids, size=1, replace=False, p=self.class_probs)[0]
            if c in usable:
                return c
        return np.random.choice(usable, p=p_usable / p_usable.sum())

    def run_original(self, img, lbl):
        """Returns (img, lbl, copy_paste_mask).  The reference's retry loop (up to 3 source images)
        always ends after the first paste, because the first pass marks every hard class as
        present (preprocessor.py:104-118); one paste is therefore the whole behaviour."""
        mask = np.full(lbl.shape, 255, dtype=np.uint8)
        c = self.random_select(self.hard_classes)
        if c is None:                      # nothing to paste from
            return img, lbl, mask
        name = np.random.choice(self.samples_with_class[c])
        img_, lbl_, _ = self.dataset_copy_from.load_data(self.dataset_copy_from.get_file_to_idx(name))
        if img.shape != img_.shape:
            img_, lbl_ = self.resize(img_, lbl_, lbl.shape)
        lut = np.zeros(256, dtype=bool)          # one table lookup instead of a compare per hard class
        lut[np.asarray(self.hard_classes, dtype=np.int64)] = True
        sel = lut[lbl_]
        rows = np.flatnonzero(sel.any(axis=1))
        if rows.size:            # img[mask] = img_[mask] as masked copies restricted to the bounding box of the pasted
            r0, r1 = int(rows[0]), int(rows[-1]) + 1         # pixels (labels: np.copyto(where=), a vectorised select; boolean
            cols = np.flatnonzero(sel[r0:r1].any(axis=0))    # fancy indexing measured 3x slower on dense masks)
            c0, c1 = int(cols[0]), int(cols[-1]) + 1
            sub = sel[r0:r1, c0:c1]
            np.copyto(mask[r0:r1, c0:c1], lbl_[r0:r1, c0:c1], where=sub)
            # RGB: byte-wise select with a mask expanded to the three channels, (a & ~m) | (b & m) — three SIMD passes
            # over contiguous bytes instead of numpy's broadcast-mask copy (12 vs 35 ms on a 2048x1024 frame)
            m3 = np.repeat(sub.view(np.uint8) * np.uint8(255), 3, axis=1).reshape(r1 - r0, c1 - c0, 3)
            dst = img[r0:r1, c0:c1]
            keep = np.bitwise_and(dst, ~m3)
            np.bitwise_and(img_[r0:r1, c0:c1], m3, out=m3)
            np.bitwise_or(keep, m3, out=keep)
            dst[...] = keep
            np.copyto(lbl[r0:r1, c0:c1], lbl_[r0:r1, c0:c1], where=sub)
        return img, lbl, mask


class _MixBase:
    """what ClassMix and CutMix share: the source frame comes from dataset_copy_from, the composite is CopyPaste's
    per-pixel select (table[lbl_src] != 0, inside the rectangle: image and label take the source's bytes) and
    copy_paste_mask = the source label where pasted, 255 elsewhere.  draw(shape) is the whole of a sample's randomness."""
    plan_takes_shape = True            # run_plan_index(shape): the destination frame's (H, W), known without a decode

    def __init__(self, cfg, dataset_copy_from, init_class_value=None):
        self.cfg = cfg
        self.dataset_copy_from = dataset_copy_from

    def draw(self, shape):
        """-> (source index | None, uint8[256] table | None, rect | None)"""
        raise NotImplementedError

    def _source(self, j, img, lbl):
        img_, lbl_, _ = self.dataset_copy_from.load_data(j)
        if img.shape != img_.shape:
            img_, lbl_ = CopyPaste.resize(img_, lbl_, lbl.shape)
        return img_, lbl_

    @staticmethod
    def _select(table, lbl_, rect):
        sel = np.asarray(table, np.uint8)[lbl_] != 0
        if rect is not None:
            y0, y1, x0, x1 = rect
            box = np.zeros(sel.shape, bool)
            box[y0:y1, x0:x1] = True
            sel &= box
        return sel

    def run(self, img, lbl):
        """-> (img, lbl, copy_paste_mask); img and lbl are composited in place, as CopyPaste.run does"""
        mask = np.full(lbl.shape, 255, dtype=np.uint8)
        j, table, rect = self.draw(lbl.shape)
        if j is None:
            return img, lbl, mask
        img_, lbl_ = self._source(j, img, lbl)
        sel = self._select(table, lbl_, rect)
        np.copyto(mask, lbl_, where=sel)
        np.copyto(img, img_, where=sel[..., None])
        np.copyto(lbl, lbl_, where=sel)
        return img, lbl, mask

    def run_plan(self, img, lbl):
        """-> ((source image, source label, table[, rect]) | None, copy_paste_mask): run()'s draws, nothing composited"""
        mask = np.full(lbl.shape, 255, dtype=np.uint8)
        j, table, rect = self.draw(lbl.shape)
        if j is None:
            return None, mask
        img_, lbl_ = self._source(j, img, lbl)
        np.copyto(mask, lbl_, where=self._select(table, lbl_, rect))
        return ((img_, lbl_, table) if rect is None else (img_, lbl_, table, rect)), mask

    def run_plan_index(self, shape=None):
        """-> (source index | None, table | None[, rect]): run()'s draws, nothing decoded"""
        j, table, rect = self.draw(shape)
        return (j, table) if rect is None else (j, table, rect)


@PREPROCESSOR.register("ClassMix")
class ClassMix(_MixBase):
    """half of the source frame's classes, as in DACS.  Draws: j = randint(len(dataset_copy_from)); classes(j) = the sorted
    class ids whose samples_with_class list holds frame j's file name (the inversion of get_samples_with_class(), built
    once here: no decode, the same on every path — NOT np.unique of the label, and it inherits the "lowest 10 % per class
    dropped" rule of stat_samples_with_class); none: no paste and no further draw; else
    chosen = choice(classes(j), size=(n + 1) // 2, replace=False)."""

    def __init__(self, cfg, dataset_copy_from, init_class_value=None):
        super().__init__(cfg, dataset_copy_from, init_class_value)
        self.classes_of = [[] for _ in range(len(dataset_copy_from))]
        for c, names in sorted(dataset_copy_from.get_samples_with_class().items()):
            for name in names:
                self.classes_of[dataset_copy_from.get_file_to_idx(name)].append(int(c))
        self.classes_of = [sorted(set(cs)) for cs in self.classes_of]

    def draw(self, shape=None):
        j = int(np.random.randint(len(self.dataset_copy_from)))
        classes = self.classes_of[j]
        if not classes:
            return None, None, None
        chosen = np.random.choice(classes, size=(len(classes) + 1) // 2, replace=False)
        table = np.zeros(256, dtype=np.uint8)
        table[np.asarray(chosen, dtype=np.int64)] = 1
        return j, table, None


@PREPROCESSOR.register("CutMix")
class CutMix(_MixBase):
    """one rectangle of the source frame, label included (a source 255 stays 255).  Draws, with (H, W) the destination
    frame's shape and (lo, hi) = cfg.preprocessor.cut_mix.area_range: j = randint(len(dataset_copy_from));
    p = uniform(lo, hi); fh = exp(uniform(log(p), 0)), fw = p / fh (both in [p, 1]);
    bh = min(H, max(1, int(fh * H + 0.5))), bw likewise; y0 = randint(0, H - bh + 1); x0 = randint(0, W - bw + 1)."""

    def __init__(self, cfg, dataset_copy_from, init_class_value=None):
        super().__init__(cfg, dataset_copy_from, init_class_value)
        lo, hi = (float(v) for v in cfg.preprocessor.cut_mix.area_range)
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError("preprocessor.cut_mix.area_range %r: 0 < lo <= hi <= 1 is required" % ([lo, hi],))
        self.area_range = (lo, hi)

    def draw(self, shape=None):
        if shape is None:
            raise ValueError("CutMix: the destination frame's (H, W) is required")
        H, W = int(shape[0]), int(shape[1])
        j = int(np.random.randint(len(self.dataset_copy_from)))
        p = np.random.uniform(*self.area_range)
        fh = math.exp(np.random.uniform(math.log(p), 0.0))
        fw = p / fh
        bh = min(H, max(1, int(fh * H + 0.5)))
        bw = min(W, max(1, int(fw * W + 0.5)))
        y0 = int(np.random.randint(0, H - bh + 1))
        x0 = int(np.random.randint(0, W - bw + 1))
        return j, np.ones(256, dtype=np.uint8), (y0, y0 + bh, x0, x0 + bw)
