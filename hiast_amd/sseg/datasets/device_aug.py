"""Device-side sample path (cfg.dataset.device_aug / HIAST_DEVICE_AUG=1): a sample is split into a PLAN — every random
decision of augmentations.aug(), drawn on the host in the same order from the same `random` / `np.random.RandomState`
streams, image-independent — and an EXECUTION, a pure function of bytes + plan.  DataLoader workers keep decoding and
drawing; resampling and recolouring run on the device (hiast_amd/csrc/sample_aug.hip), byte-identical to the host code.

    plan_sample(aug_fun, in_shape, index)     -> list of view plans (one per entry of a multi-view aug list)
    execute_plan_host(plan, img, lbl)         -> what augmentations.aug() returns, computed from the plan in numpy: the
                                                 definition the kernels are tested against
    pack_sample / collate                     -> what a worker hands over: ONE uint8 blob, ONE int32 table blob and one
                                                 record row per sample (offsets, not pointers: built without a device)
    assemble_device_batch(batch, device)      -> what utils.to_device_batch returns (normalised float32 CHW views, labels)

With device-resident frames (device_store.py) a sample whose frame — and CopyPaste source frame — is resident carries no
bytes at all: pack_store_sample -> {"plan", "raw": {"store": (index, paste index | -1), ...}}; its record is of
KIND_STORE and addresses the windows in place in the store (assemble_device_batch(batch, device, store)).

A paste (CopyPaste, ClassMix, CutMix: preprocessor.py) is part of the plan: (source, source label, uint8[256] table[, rect]),
rect = (y0, y1, x0, x1) in frame coordinates, half-open, absent / None = the whole frame.  A paste with a rectangle travels
as a record of kind 3 (bytes) or 4 (store): the rectangle follows the table in the blob, in window coordinates.

A view plan is {"ops": [...], "host": bool}; ops are ("geom", Geometry), ("lut", uint8[256]), ("gray",), ("equalize",)
and ("host", name).  At level 1 ColorJitter, GaussianBlur and FDA have no device form (PIL's C HSV conversion, scipy's
float64 correlate, an FFT): a sample whose plan holds one of them is run through augmentations.aug() by the worker as
before and handed over as finished uint8 views (`needs_host`).

plan_sample(level=2) plans ColorJitter and GaussianBlur too; plan_sample(level=3) also FDA, as ("fda", path, border): the
sparse-DFT form `fda_u8` — the view plus the inverse DFT of the at most 25 centre bins whose amplitude the reference
image replaces.  The worker decodes and resizes the reference image (pack_sample); it travels in the uint8 blob.

Resampling restates Pillow's two-pass 8-bit resample in integers (ImagingResample: per-axis coefficient tables in
float64, rounded to 22-bit fixed point, horizontal pass rounded to uint8, then the vertical pass) and its affine
nearest-neighbour scaler (a running float64 sum per axis)."""
import random

import numpy as np
import torch

# the words, kinds and op types of the hand-over tables: defined once, in hiast_amd/aug_records.py
from hiast_amd.aug_records import (  # noqa: F401  (re-exported: callers and tests read them as device_aug.R_KIND, ...)
    FDA_BORDER_SHIFT, FDA_MAX_BORDER, FDA_MIN_SIDE, KIND_FINISHED, KIND_PLAN, KIND_PLAN_RECT, KIND_STORE, KIND_STORE_RECT,
    MAX_KSIZE, MAX_OPS, MIX_TABLE_BYTES, OP_BLUR, OP_CONTRAST, OP_EQUALIZE, OP_FDA, OP_GRAY, OP_HUE, OP_LUT, OP_SAT, OPS_WORDS,
    R_CH, R_CW, R_FLIP, R_HK, R_HLO, R_HN, R_HT, R_IMG, R_KIND, R_LBL, R_NX, R_NY, R_PIMG, R_PLBL, R_PTAB, R_STRIDE, R_VK,
    R_VLO, R_VN, R_VT, REC_WORDS, RECT_BYTES, RECT_KINDS)
from hiast_amd.sseg.datasets import augmentations as A

PRECISION_BITS = 22          # Pillow: 32 - 8 - 2
HOST_ONLY = (A.ColorJitter, A.GaussianBlur, A.FDA)


# ------------------------------------------------------------------------------------------------- tables
def bilinear_table(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle) filter over a whole axis:
    -> (lo int32[n_out], n int32[n_out], k int32[n_out, taps]); taps beyond n are 0.  n_in == n_out has no pass in
    Pillow: the identity table (one tap of weight 2^P) reproduces that exactly."""
    one = 1 << PRECISION_BITS
    if n_in == n_out:
        return (np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32), np.full((n_out, 1), one, np.int32))
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    taps = int(np.ceil(support)) * 2 + 1
    lo = np.zeros(n_out, np.int32)
    n = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, taps), np.int32)
    for i in range(n_out):
        c = (i + 0.5) * scale
        x0 = max(int(c - support + 0.5), 0)
        x1 = min(int(c + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((j + x0 - c + 0.5) * ss)) for j in range(x1 - x0)]
        tot = 0.0
        for v in w:
            tot += v
        lo[i], n[i] = x0, x1 - x0
        for j, v in enumerate(w):
            if tot != 0.0:
                v = v / tot
            k[i, j] = int(0.5 + v * one)
    return lo, n, k


def nearest_table(n_in, n_out):
    """Pillow's ImagingScaleAffine: the source index of every output index, from the running float64 sum"""
    a = n_in / n_out
    x = 0.5 * a
    tab = np.zeros(n_out, np.int32)
    for i in range(n_out):
        tab[i] = min(int(x), n_in - 1)
        x += a
    return tab


class Geometry:
    """flip + crop window + resize (+ a crop of the resized frame) of one source frame as tables over the bytes a worker
    hands over: `src` = (y1, y2, x1, x2), the slice of the UNFLIPPED source frame; with `flip` its columns are read right
    to left.  All table indices are relative to that (flipped) slice."""

    def __init__(self, src, flip, out, hlo, hn, hk, vlo, vn, vk, nx, ny):
        self.src, self.flip, self.out = tuple(int(v) for v in src), bool(flip), (int(out[0]), int(out[1]))
        self.hlo, self.hn, self.hk, self.vlo, self.vn, self.vk, self.nx, self.ny = hlo, hn, hk, vlo, vn, vk, nx, ny


class _GeomState:
    """the geometric transforms met so far on the way down one chain: out = crop_out(resize(crop(flip?(frame))))"""

    def __init__(self, shape):
        self.H, self.W = int(shape[0]), int(shape[1])
        self.flip = False
        self.win = (0, self.H, 0, self.W)        # in the coordinates of the (flipped) frame
        self.resize = None
        self.out_win = None
        self.touched = False

    def shape(self):
        if self.out_win is not None:
            return self.out_win[1] - self.out_win[0], self.out_win[3] - self.out_win[2]
        if self.resize is not None:
            return self.resize
        return self.win[1] - self.win[0], self.win[3] - self.win[2]

    def do_flip(self):
        if self.resize is not None:
            return False
        y1, y2, x1, x2 = self.win                # flip of a window = the mirrored window of the flipped frame
        self.win = (y1, y2, self.W - x2, self.W - x1)
        self.flip = not self.flip
        self.touched = True
        return True

    def do_crop(self, y1, y2, x1, x2):
        self.touched = True
        if self.resize is None:
            oy, ox = self.win[0], self.win[2]
            self.win = (oy + y1, oy + y2, ox + x1, ox + x2)
        else:
            oy, ox = (self.out_win[0], self.out_win[2]) if self.out_win is not None else (0, 0)
            self.out_win = (oy + y1, oy + y2, ox + x1, ox + x2)
        return True

    def do_resize(self, h, w):
        if self.shape() == (h, w):               # Resize.apply / Image.resize to the same size: the bytes unchanged
            return True
        if self.resize is not None:
            return False
        self.resize = (int(h), int(w))
        self.touched = True
        return True

    def build(self):
        y1, y2, x1, x2 = self.win
        ch, cw = y2 - y1, x2 - x1
        rh, rw = self.resize if self.resize is not None else (ch, cw)
        hlo, hn, hk = bilinear_table(cw, rw)
        vlo, vn, vk = bilinear_table(ch, rh)
        nx, ny = nearest_table(cw, rw), nearest_table(ch, rh)
        if self.out_win is not None:
            oy1, oy2, ox1, ox2 = self.out_win
            hlo, hn, hk, nx = hlo[ox1:ox2], hn[ox1:ox2], hk[ox1:ox2], nx[ox1:ox2]
            vlo, vn, vk, ny = vlo[oy1:oy2], vn[oy1:oy2], vk[oy1:oy2], ny[oy1:oy2]
        # hand over only the rows / columns a table reads
        xa = int(min(hlo.min(), nx.min()))
        xb = int(max((hlo + hn).max(), nx.max() + 1))
        ya = int(min(vlo.min(), ny.min()))
        yb = int(max((vlo + vn).max(), ny.max() + 1))
        hlo, nx, vlo, ny = hlo - xa, nx - xa, vlo - ya, ny - ya
        fx1, fx2 = x1 + xa, x1 + xb              # columns of the (flipped) frame
        sx1, sx2 = (self.W - fx2, self.W - fx1) if self.flip else (fx1, fx2)
        c = np.ascontiguousarray
        return Geometry((y1 + ya, y1 + yb, sx1, sx2), self.flip, (len(vlo), len(hlo)),
                        c(hlo, np.int32), c(hn, np.int32), c(hk, np.int32), c(vlo, np.int32), c(vn, np.int32),
                        c(vk, np.int32), c(nx, np.int32), c(ny, np.int32))


# ------------------------------------------------------------------------------------------------- plan
def _lut_of(t, params):
    """the 256-entry table the host transform applies; None = the bytes unchanged"""
    if isinstance(t, A.RandomContrast):
        return A._brightness_contrast_lut(params["alpha"], 0.0)
    if isinstance(t, A.RandomBrightness):
        return A._brightness_contrast_lut(1.0, params["beta"])
    if isinstance(t, A.Posterize):
        bits = params["bits"]
        if bits == 0:
            return np.zeros(256, np.uint8)
        if bits == 8:
            return None
        return np.arange(256, dtype=np.uint8) & np.uint8(~np.uint8(2 ** (8 - bits) - 1))
    if isinstance(t, A.Solarize):
        thr = params["threshold"]
        return np.array([i if i < thr else 255 - i for i in range(256)], np.uint8)
    raise TypeError(type(t).__name__)


class _Walker:
    """one chain of views: the walk of augmentations.aug() with its draws, recording instead of touching pixels"""

    def __init__(self, in_shape, level=1):
        self.level = level
        self.geom = _GeomState(in_shape)
        self.geom_open = True                    # no pixel op recorded yet: geometry may still be folded into view 0's op
        self.ops = []
        self.host = False
        self.stop = False                        # FDA below level 3: its params() read the image — the draws stop here
        self.readers = {}                        # level 3: reference image path -> the read_fn of the FDA that drew it

    def begin_view(self):
        self.ops = []

    def end_view(self):
        self._close_geometry()
        view = {"ops": self.ops, "host": any(o[0] == "host" for o in self.ops)}
        if any(o[0] == "fda" for o in self.ops):
            view["readers"] = {o[1]: self.readers[o[1]] for o in self.ops if o[0] == "fda"}
        return view

    def _close_geometry(self):
        if self.geom_open:
            self.ops.insert(0, ("geom", self.geom.build()))
            self.geom_open = False

    def _pixel_op(self, op):
        self._close_geometry()
        if op[0] == "lut" and self.ops and self.ops[-1][0] == "lut":
            self.ops[-1] = ("lut", op[1][self.ops[-1][1]])          # lut2[lut1]: the same bytes in one pass
        else:
            self.ops.append(op)

    def _geom_op(self, ok):
        if not (self.geom_open and ok):          # geometry after a pixel op, or a second resize: no device form
            self._close_geometry()
            self.ops.append(("host", "geometry"))

    def walk(self, t):
        if self.stop:
            return
        if isinstance(t, A.SomeOf):
            if random.random() < t.p:
                rs = np.random.RandomState(random.randint(0, 2 ** 32 - 1))
                for i in rs.choice(len(t.transforms), size=t.n, replace=t.replace):
                    self.walk(t.transforms[int(i)])
            return
        if isinstance(t, A.Compose):
            if random.random() < t.p:
                for c in t.transforms:
                    self.walk(c)
            return
        if isinstance(t, A.FDA) and self.level < 3:
            self._pixel_op(("host", "FDA"))
            self.stop = True
            return
        if not random.random() < t.p:
            return
        g = self.geom
        if isinstance(t, A.FDA):                 # level 3: the draws of params() without the read
            beta, path = t.draw()
            h, w = g.shape()
            border = int(np.floor(min(h, w) * beta))
            if border > FDA_MAX_BORDER or min(h, w) < FDA_MIN_SIDE:      # (a large beta_limit: the host's FFT)
                self._pixel_op(("host", "FDA"))
            else:
                self.readers[path] = t.read_fn
                self._pixel_op(("fda", path, border))
            return
        params = t.params(None)
        if isinstance(t, A.HorizontalFlip):
            self._geom_op(self.geom_open and g.do_flip())
        elif isinstance(t, A.Resize):
            self._geom_op(self.geom_open and g.do_resize(t.h, t.w))
        elif isinstance(t, A.RandomSizedCrop):
            H, W = g.shape()
            ch, cw = min(params["ch"], H), min(params["cw"], W)
            win = A._crop_coords(H, W, ch, cw, params["h_start"], params["w_start"])
            self._geom_op(self.geom_open and g.do_crop(*win) and g.do_resize(t.h, t.w))
        elif isinstance(t, A.RandomCrop):
            H, W = g.shape()
            if t.h > H or t.w > W:
                raise ValueError("RandomCrop: crop %dx%d is larger than the image %dx%d" % (t.h, t.w, H, W))
            self._geom_op(self.geom_open and g.do_crop(*A._crop_coords(H, W, t.h, t.w, params["h_start"], params["w_start"])))
        elif self.level >= 2 and isinstance(t, A.ColorJitter):
            for i in params["order"]:
                op = _jitter_op(i, params["factors"][i])
                if op is not None:
                    self._pixel_op(op)
        elif self.level >= 2 and isinstance(t, A.GaussianBlur):
            if params["ksize"] > 1:
                k = params["ksize"]
                if k % 2 != 1 or k > MAX_KSIZE or k // 2 >= min(g.shape()):     # (the device reflects a border once)
                    self._pixel_op(("host", "GaussianBlur"))
                else:
                    self._pixel_op(("blur", blur_weights(k, params["sigma"])))
        elif isinstance(t, HOST_ONLY):
            self._pixel_op(("host", type(t).__name__))
        elif isinstance(t, (A.RandomContrast, A.RandomBrightness, A.Posterize, A.Solarize)):
            lut = _lut_of(t, params)
            if lut is not None:
                self._pixel_op(("lut", np.asarray(lut, np.uint8)))
        elif isinstance(t, A.ToGray):
            self._pixel_op(("gray",))
        elif isinstance(t, A.Equalize):
            self._pixel_op(("equalize",))
        else:
            self._pixel_op(("host", type(t).__name__))


def _jitter_op(i, f):
    """step i (0 brightness, 1 contrast, 2 saturation, 3 hue) of A.ColorJitter.apply with its drawn factor as a plan op;
    None = the bytes unchanged (a hue factor of exactly 0)"""
    if i == 0:
        return ("lut", np.clip(np.arange(256, dtype=np.float32) * f, 0, 255).astype(np.uint8))
    if i == 1:
        return ("contrast", float(f))
    if i == 2:
        return ("sat", float(f))
    if f == 0:
        return None
    return ("hue", int(round(256 * f)) % 256)         # also 0: the HSV round trip is not the identity


def blur_weights(ksize, sigma):
    w = A._gaussian_kernel_cv(ksize, sigma)
    assert w.dtype == np.float32 and np.array_equal(w, w[::-1])      # scipy's symmetric-filter loop is the definition
    return w


def plan_sample(aug_fun, in_shape, index=None, level=1):
    """-> list of view plans (one per view; a single aug gives a list of one).  Consumes exactly the draws
    augmentations.aug(aug_fun, img, lbl, index) consumes unless the plan `needs_host` through an FDA, whose parameters read
    the image: the caller restores the state it saved and runs aug() (see BaseDataset).  level 2: ColorJitter and
    GaussianBlur are plan ops too (("contrast", f), ("sat", f), ("hue", shift), ("blur", weights)).  level 3: FDA is the
    plan op ("fda", path, border), drawn as A.FDA.params draws it but without opening the file — the draws are always
    those of aug(); border > 2, or a view with a side below 8, stays ("host", "FDA")."""
    if index is not None:
        random.seed(index)
    w = _Walker(in_shape, level)
    views = []
    for f in (aug_fun if isinstance(aug_fun, (list, tuple)) else [aug_fun]):
        w.begin_view()
        if f is not None:
            w.walk(f)
        views.append(w.end_view())
    for v in views:        # what the device records hold: bounded op lists, at most one Equalize per view
        n_eq = sum(1 for o in v["ops"] if o[0] == "equalize")
        if n_eq > 1 or sum(1 for o in v["ops"] if o[0] != "geom") > MAX_OPS:
            v["host"] = True
    return views


def needs_host(plan):
    return any(v["host"] for v in plan)


def plan_window(plan):
    """(y1, y2, x1, x2) of the source frame the plan reads"""
    return plan[0]["ops"][0][1].src


# ------------------------------------------------------------------------------------------------- host executor
def _resample_axis1(a, lo, n, k):
    """a [R, n_in, C] uint8 -> [R, n_out, C] uint8: one integer pass of Pillow's 8-bit resample along axis 1"""
    acc = np.full((a.shape[0], len(lo), a.shape[2]), 1 << (PRECISION_BITS - 1), np.int32)
    for t in range(k.shape[1]):
        live = n > t
        if not live.any():
            break
        idx = np.minimum(lo + t, a.shape[1] - 1)
        acc += np.where(live, k[:, t], 0).astype(np.int32)[None, :, None] * a[:, idx].astype(np.int32)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def equalize_luts(img):
    """per channel the table augmentations._equalize_cv_channel applies (a constant channel keeps its value)"""
    luts = np.zeros((img.shape[2], 256), np.uint8)
    for c in range(img.shape[2]):
        hist = np.bincount(img[..., c].ravel(), minlength=256)
        first = int(np.nonzero(hist)[0][0])
        total = int(img[..., c].size)
        if hist[first] == total:
            luts[c, :] = first
            continue
        scale = 255.0 / (total - hist[first])
        s = 0
        for i in range(first + 1, 256):
            s += int(hist[i])
            luts[c, i] = min(255, max(0, int(round(s * scale))))
    return luts


def paste_rect(paste):
    """the rectangle (y0, y1, x0, x1; frame coordinates, half-open) of a paste tuple, or None = the whole frame"""
    return None if paste is None or len(paste) < 4 or paste[3] is None else tuple(int(v) for v in paste[3])


def window_rect(rect, src):
    """a frame-coordinate rectangle in the coordinates of the window src = (y1, y2, x1, x2), clipped to it; an empty
    intersection is (0, 0, 0, 0)"""
    y0, y1 = (min(max(int(v) - src[0], 0), src[1] - src[0]) for v in rect[:2])
    x0, x1 = (min(max(int(v) - src[2], 0), src[3] - src[2]) for v in rect[2:])
    return (y0, y1, x0, x1) if y0 < y1 and x0 < x1 else (0, 0, 0, 0)


def execute_geometry_host(g, raw_img, raw_lbl, paste=None):
    """raw_img / raw_lbl: the slices g.src of the frame; paste = (src_img, src_lbl, table uint8[256][, rect]) over the same
    slice: the CopyPaste / ClassMix / CutMix composite, taken per pixel before resampling (and before the flip): where
    table[src_lbl] != 0 and, with a rect (frame coordinates), inside it"""
    if paste is not None:
        p_img, p_lbl, table = paste[:3]
        sel = np.asarray(table, np.uint8)[p_lbl] != 0
        if paste_rect(paste) is not None:
            y0, y1, x0, x1 = window_rect(paste_rect(paste), g.src)
            box = np.zeros(sel.shape, bool)
            box[y0:y1, x0:x1] = True
            sel = sel & box
        raw_img = np.where(sel[..., None], p_img, raw_img)
        raw_lbl = np.where(sel, p_lbl, raw_lbl)
    if g.flip:
        raw_img, raw_lbl = raw_img[:, ::-1], raw_lbl[:, ::-1]
    h8 = _resample_axis1(raw_img, g.hlo, g.hn, g.hk)
    out = _resample_axis1(h8.transpose(1, 0, 2), g.vlo, g.vn, g.vk).transpose(1, 0, 2)
    return np.ascontiguousarray(out), np.ascontiguousarray(raw_lbl[g.ny][:, g.nx])


def _f32div(a, b):
    return (a.astype(np.float32) / b.astype(np.float32)).astype(np.float32)


def rgb_to_hsv_u8(img):
    """Pillow's convert("HSV") (rgb2hsv_row) on uint8 [..., 3], byte for byte: float32 quotients, the hue wrapped in
    float64, H and S truncated"""
    f32, f64 = np.float32, np.float64
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    maxc, minc = img.max(-1), img.min(-1)
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f32)
    s = _f32div(cr, np.maximum(maxc, 1))
    rc, gc, bc = _f32div(maxc - r, cr), _f32div(maxc - g, cr), _f32div(maxc - b, cr)
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                          (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
    hd = h.astype(f64) / 6.0 + 1.0
    h = (hd - np.floor(hd)).astype(f32)                               # fmod(x, 1.0) of a positive x
    H = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(flat, 0, H), np.where(flat, 0, S), maxc], -1).astype(np.uint8)


def hsv_to_rgb_u8(hsv):
    """Pillow's HSV -> RGB (hsv2rgb_row) on uint8 [..., 3], byte for byte: p, q, t in float64 from the float32 fraction and
    saturation, C round() (half away from zero)"""
    f32, f64 = np.float32, np.float64
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    h6 = h.astype(f64) * 6.0 / 255.0
    fl = np.floor(h6)
    f = (h6 - fl).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    vd = v.astype(f64)
    rnd = lambda x: np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)       # noqa: E731  (x >= 0 here)
    p = rnd(vd * (1.0 - fs.astype(f64)))
    q = rnd(vd * (1.0 - fs.astype(f64) * f.astype(f64)))
    t = rnd(vd * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    i = fl.astype(np.int32) % 6
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue_u8(img, shift):
    """A.ColorJitter._hue for a non-zero factor: shift = int(round(256 * f)) mod 256"""
    out = np.empty_like(img)
    flat_i, flat_o = img.reshape(-1, 3), out.reshape(-1, 3)
    for a in range(0, flat_i.shape[0], 1 << 20):                      # (bounded float64 temporaries)
        hsv = rgb_to_hsv_u8(flat_i[a:a + (1 << 20)])
        hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) % 256
        flat_o[a:a + (1 << 20)] = hsv_to_rgb_u8(hsv)
    return out


def contrast_lut(img, f):
    """the table A.ColorJitter._contrast applies to `img`: the gray mean as an exact integer sum / count in float64"""
    mean = np.float64(int(A._gray_cv(img).sum(dtype=np.int64))) / np.float64(img.shape[0] * img.shape[1])
    v = np.arange(256, dtype=np.float32) * np.float32(f) + np.float32(mean * (1.0 - f))
    return np.clip(v, 0, 255).astype(np.uint8)


def saturation_u8(img, f):
    """A.ColorJitter._saturation: c * f32(f) + gray * f32(1 - f), every operation rounded to float32, truncated"""
    g = A._gray_cv(img).astype(np.float32) * np.float32(1 - f)
    out = img.astype(np.float32) * np.float32(f) + g[..., None]
    return np.clip(out, 0, 255).astype(np.uint8)


def blur_pass(x, w, axis):
    """one pass of scipy.ndimage.correlate1d(x float32, w float32 symmetric, mode="mirror") restated: float64,
    o = x[c] * w[s]; o += (x[c - j] + x[c + j]) * w[s - j] for j = s .. 1, rounded to float32 once"""
    x = np.moveaxis(np.asarray(x, np.float32), axis, 0).astype(np.float64)
    w = np.asarray(w, np.float32).astype(np.float64)
    n, s = x.shape[0], len(w) // 2
    if s >= n:
        raise ValueError("blur: half width %d reaches across the axis of %d" % (s, n))
    idx = np.abs(np.arange(-s, n + s))
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    xp = x[idx]
    o = xp[s:s + n] * w[s]
    for j in range(s, 0, -1):
        o = o + (xp[s - j:s - j + n] + xp[s + j:s + j + n]) * w[s - j]
    return np.ascontiguousarray(np.moveaxis(o.astype(np.float32), 0, axis))


def blur_u8(img, w):
    """A._blur_separable: axis 0, then axis 1, rint (half to even), clip"""
    x = blur_pass(blur_pass(img.astype(np.float32), w, 0), w, 1)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def fda_trig(n):
    """cos, sin of 2 pi j / n for j < n (float64): the table every layer reads, indexed by the angle AFTER its integer mod"""
    t = 2.0 * np.pi * np.arange(n, dtype=np.float64) / np.float64(n)
    return np.cos(t), np.sin(t)


def fda_u8(img, target, border):
    """the FDA op: trunc(clip(fda_f64(img, target, border), 0, 255)) on uint8 [H, W, 3] — the definition the executor, the
    kernels and the tests are pinned to.  One deliberate difference from the host FFT: target == img returns img exactly
    (see fda_f64)."""
    return np.clip(fda_f64(img, target, border), 0, 255).astype(np.uint8)


def fda_f64(img, target, border):
    """the values fda_u8 truncates: augmentations.fourier_domain_adaptation(img, target, beta) with
    border = floor(min(H, W) * beta) in its sparse-DFT form, float64: the FFT is linear and every bin outside the centre
    square keeps its value, so per channel c, over the bins (ky, kx) with |ky|, |kx| <= border,
        S = sum_y sum_x img[y, x, c] exp(-2 pi i (((ky y) mod H) / H + ((kx x) mod W) / W)),  T likewise over target,
        D = (|T| - |S|) S / |S|                                  (S == 0: the phase is 1, as np.angle(0) == 0)
        f = img + sum_bins Re(D exp(+2 pi i ...)) / (H W),       out = trunc(clip(f, 0, 255)).
    The input is real: a bin and its conjugate partner are computed once (1, 5 or 13 bins).  With
    e(y) = (1, cos ty, sin ty, cos 2ty, sin 2ty) and r(x) likewise, every bin sum is a signed pair of entries of
    G = e^T img r, and the correction is e C r^T with C built from D / (H W): the form the kernels compute.
    The ONE deliberate difference from the host FFT: with target == img, D is exactly 0 and this form returns img
    exactly; the host's complex64 FFT round trip can move a byte down by one there (and, for any target, wherever f is
    within about 1e-3 of an integer: the host is the noisy party at those knife edges)."""
    img, target = np.asarray(img), np.asarray(target)
    H, W = img.shape[:2]
    nb = int(border)
    if img.dtype != np.uint8 or target.shape != img.shape or img.ndim != 3 or not 0 <= nb <= FDA_MAX_BORDER \
            or min(H, W) < FDA_MIN_SIDE:
        raise ValueError("fda_u8: uint8 [H, W, C] image and target of one shape, border 0..%d, sides >= %d"
                         % (FDA_MAX_BORDER, FDA_MIN_SIDE))
    nc = 1 + 2 * nb

    def basis(n):
        cs, sn = fda_trig(n)
        rows = [np.ones(n)]
        for k in range(1, nb + 1):
            a = (k * np.arange(n)) % n
            rows += [cs[a], sn[a]]
        return np.stack(rows)                                         # [nc, n]
    E, R = basis(H), basis(W)
    f = np.empty(img.shape, np.float64)
    hw = np.float64(H) * np.float64(W)
    for c in range(img.shape[2]):
        v = img[..., c].astype(np.float64)
        gs = E @ (v @ R.T)                                            # rows reduced along x, then the row factors
        gt = E @ (target[..., c].astype(np.float64) @ R.T)
        cf = np.zeros((nc, nc))
        for ky in range(0, nb + 1):
            for kx in range(-nb if ky else 0, nb + 1):
                ax, sg = abs(kx), (-1.0 if kx < 0 else 1.0)
                ci, si, cj, sj = (2 * ky - 1 if ky else 0), 2 * ky, (2 * ax - 1 if ax else 0), 2 * ax

                def bin_of(g):
                    re = g[ci, cj] - (sg * g[si, sj] if ky and ax else 0.0)
                    im = -((g[si, cj] if ky else 0.0) + (sg * g[ci, sj] if ax else 0.0))
                    return re, im
                (sr, sim), (tr, tim) = bin_of(gs), bin_of(gt)
                ms, mt = np.sqrt(sr * sr + sim * sim), np.sqrt(tr * tr + tim * tim)
                pr, pi = (1.0, 0.0) if ms == 0.0 else (sr / ms, sim / ms)
                wgt = 2.0 if (ky or ax) else 1.0                      # the bin and its conjugate partner
                dr, di = wgt * ((mt - ms) * pr / hw), wgt * ((mt - ms) * pi / hw)
                cf[ci, cj] += dr
                if ky and ax:
                    cf[si, sj] -= sg * dr
                if ky:
                    cf[si, cj] -= di
                if ax:
                    cf[ci, sj] -= sg * di
        f[..., c] = v + (E.T @ cf) @ R
    return f


def fda_target(path, shape, read_fn=None):
    """the reference image of an ("fda", path, border) op as the host transform sees it: decoded, resized with Pillow"""
    return np.array(A._resize_img((read_fn or A._read_rgb)(path), int(shape[0]), int(shape[1])), np.uint8, order="C")


def execute_colour_host(ops, img, readers=None):
    """readers: {path: read_fn} of the view's FDA ops (plan_sample(level=3) records them in the view plan)"""
    for op in ops:
        if op[0] == "fda":
            img = fda_u8(img, fda_target(op[1], img.shape, (readers or {}).get(op[1])), op[2])
        elif op[0] == "contrast":
            img = contrast_lut(img, op[1])[img]
        elif op[0] == "sat":
            img = saturation_u8(img, op[1])
        elif op[0] == "hue":
            img = hue_u8(img, op[1])
        elif op[0] == "blur":
            img = blur_u8(img, op[1])
        elif op[0] == "lut":
            img = op[1][img]
        elif op[0] == "gray":
            img = np.repeat(A._gray_cv(img)[..., None], 3, axis=2)
        elif op[0] == "equalize":
            luts = equalize_luts(img)
            img = np.stack([luts[c][img[..., c]] for c in range(img.shape[2])], axis=2)
        else:
            raise ValueError("op %r has no plan form (host fallback)" % (op[0],))
    return img


def execute_plan_host(plan, img, lbl, paste=None, sliced=False):
    """numpy execution of a plan: -> ([image per view], [label per view]), always lists (augmentations.aug() returns a bare
    image / label for a single aug).  img / lbl: the source frame, or with `sliced` the slices plan_window(plan) of it
    (what a worker hands over); paste = (source image, source label, table[, rect]) of a preprocessor's run_plan, its
    arrays sliced likewise (the rect stays in frame coordinates)."""
    g = plan[0]["ops"][0][1]
    if not sliced:
        y1, y2, x1, x2 = g.src
        img, lbl = img[y1:y2, x1:x2], lbl[y1:y2, x1:x2]
        if paste is not None:
            paste = (paste[0][y1:y2, x1:x2], paste[1][y1:y2, x1:x2]) + tuple(paste[2:])
    cur, label = execute_geometry_host(g, img, lbl, paste)
    imgs, lbls = [], []
    for k, v in enumerate(plan):
        cur = execute_colour_host(v["ops"][1:] if k == 0 else v["ops"], cur, v.get("readers"))
        imgs.append(cur)
        lbls.append(label)
    return imgs, lbls


# ------------------------------------------------------------------------------------------------- hand-over
# one int64 record row per sample (offsets into the batch's uint8 blob / int32 table blob) and one op row per (view, sample):
# their words (R_*, REC_WORDS, OPS_WORDS) and kinds (KIND_*) are hiast_amd/aug_records.py's


def paste_table_bytes(table, rect_w=None):
    """what R_PTAB points at: the 256 table bytes, + the window rectangle of a record of kind 3 / 4"""
    table = np.ascontiguousarray(table, np.uint8).reshape(256)
    if rect_w is None:
        return table
    return np.concatenate([table, np.asarray(rect_w, "<i4").reshape(4).view(np.uint8)])


def _align(n, a=16):
    return (n + a - 1) // a * a


class _Blob:
    def __init__(self, dtype):
        self.parts, self.size, self.dtype = [], 0, dtype

    def add(self, a):
        a = np.ascontiguousarray(a, self.dtype).reshape(-1)
        off = self.size
        self.parts.append((off, a))
        self.size = _align(off + a.size, 16)
        return off

    def join(self):
        out = np.zeros(max(self.size, 16), self.dtype)
        for off, a in self.parts:
            out[off:off + a.size] = a
        return out


def pack_sample(plan, raw_img, raw_lbl, paste=None):
    """what a worker returns for a planned sample: {"plan", "raw"} with the slices of plan_window(plan); the reference
    image of every FDA op is decoded and resized to the view here, in the worker (raw["fda"], in op order)"""
    raw = {"img": torch.from_numpy(np.ascontiguousarray(raw_img)), "lbl": torch.from_numpy(np.ascontiguousarray(raw_lbl))}
    _add_fda_views(raw, plan)
    if paste is not None:
        raw["paste_img"] = torch.from_numpy(np.ascontiguousarray(paste[0]))
        raw["paste_lbl"] = torch.from_numpy(np.ascontiguousarray(paste[1]))
        raw["paste_table"] = torch.from_numpy(np.ascontiguousarray(paste[2], np.uint8))
        if paste_rect(paste) is not None:       # (frame coordinates; build_batch_tables translates it into the window's)
            raw["paste_rect"] = torch.tensor(paste_rect(paste), dtype=torch.int64)
    return {"raw": raw, "plan": plan}


def _add_fda_views(raw, plan):
    out_shape = plan[0]["ops"][0][1].out
    fda = [torch.from_numpy(fda_target(op[1], out_shape, v.get("readers", {}).get(op[1])))
           for v in plan for op in v["ops"] if op[0] == "fda"]
    if fda:
        raw["fda"] = fda


def pack_store_sample(plan, index, row, paste=None):
    """what a worker returns for a planned sample whose frame is resident in the device store: no frame bytes.  index /
    row: the frame's dataset index and its row of the residency table (image offset, label offset, H, W);
    paste = (source index, its row, uint8[256] table[, rect]) of a preprocessor's run_plan_index with a resident source of
    the frame's shape.  The FDA target views are decoded and resized here, in the worker, as in pack_sample."""
    rows = torch.full((2, 4), -1, dtype=torch.int64)
    rows[0] = torch.as_tensor(row, dtype=torch.int64)
    raw = {"store": (int(index), -1), "store_rows": rows}
    if paste is not None:
        raw["store"] = (int(index), int(paste[0]))
        rows[1] = torch.as_tensor(paste[1], dtype=torch.int64)
        raw["paste_table"] = torch.from_numpy(np.ascontiguousarray(paste[2], np.uint8))
        if paste_rect(paste) is not None:
            raw["paste_rect"] = torch.tensor(paste_rect(paste), dtype=torch.int64)
    _add_fda_views(raw, plan)
    return {"raw": raw, "plan": plan}


def pack_finished(imgs, lbls):
    """a host-fallback sample: finished uint8 views (lists for multi-view) as utils.transform(raw_u8=True) returns them"""
    multi = isinstance(imgs, (list, tuple))
    return {"raw": {"views": list(imgs) if multi else [imgs], "lbl": lbls[0] if multi else lbls}, "plan": None,
            "multi": multi}


def build_batch_tables(samples):
    """samples: the {"raw", "plan"} parts of a batch -> dict of tensors: blob uint8, tabs int32, recs int64 [B, REC_WORDS],
    ops int64 [V, B, OPS_WORDS], meta int64 [n_views, out_h, out_w, max_ch, multi]"""
    B = len(samples)
    blob, tabs = _Blob(np.uint8), _Blob(np.int32)
    recs = np.full((B, REC_WORDS), -1, np.int64)
    out, n_views, multi = None, None, None
    for s in samples:
        if s["plan"] is None:
            v, shp, m = len(s["raw"]["views"]), tuple(s["raw"]["lbl"].shape), s["multi"]
        else:
            v, shp, m = len(s["plan"]), s["plan"][0]["ops"][0][1].out, len(s["plan"]) > 1
        if out is None:
            out, n_views, multi = shp, v, m
        if (shp, v) != (out, n_views):
            raise ValueError("device_aug batch: samples of different output size / view count (%s x%d vs %s x%d)"
                             % (shp, v, out, n_views))
    ops = np.zeros((n_views, B, OPS_WORDS), np.int64)
    store_idx = np.full((B, 2), -1, np.int64)
    store_rect = np.full((B, 4), -1, np.int64)
    max_ch = 1
    for b, s in enumerate(samples):
        raw, r = s["raw"], recs[b]
        if s["plan"] is None:
            r[R_KIND] = KIND_FINISHED
            r[R_LBL] = blob.add(raw["lbl"].numpy())
            for k, v in enumerate(raw["views"]):
                ops[k, b, 0], ops[k, b, 1] = KIND_FINISHED, blob.add(v.numpy())
            r[R_IMG] = ops[0, b, 1]
            continue
        g = s["plan"][0]["ops"][0][1]
        ch, cw = g.src[1] - g.src[0], g.src[3] - g.src[2]
        rect_w = window_rect(raw["paste_rect"].tolist(), g.src) if "paste_rect" in raw else None
        if "store" in raw:                   # the windows stay where they are: offsets of their first pixels in the store
            (io, lo, fh, fw), (pio, plo, ph, pw) = raw["store_rows"].tolist()
            first = g.src[0] * fw + g.src[2]
            if io < 0 or lo < 0 or g.src[1] > fh or g.src[3] > fw:
                raise ValueError("device_aug: window %s of a resident frame of %dx%d at %d" % (g.src, fh, fw, io))
            r[R_KIND], r[R_CH], r[R_CW], r[R_FLIP], r[R_STRIDE] = KIND_STORE, ch, cw, int(g.flip), fw
            r[R_IMG], r[R_LBL] = io + first * 3, lo + first
            if raw["store"][1] >= 0:
                if pio < 0 or plo < 0 or (ph, pw) != (fh, fw):
                    raise ValueError("device_aug: paste source of %dx%d at %d for a frame of %dx%d" % (ph, pw, pio, fh, fw))
                r[R_PIMG], r[R_PLBL] = pio + first * 3, plo + first
                r[R_PTAB] = blob.add(paste_table_bytes(raw["paste_table"].numpy(), rect_w))
                if rect_w is not None:
                    r[R_KIND], store_rect[b] = KIND_STORE_RECT, raw["paste_rect"].tolist()
            store_idx[b] = raw["store"]
        else:
            if tuple(raw["img"].shape) != (ch, cw, 3) or tuple(raw["lbl"].shape) != (ch, cw):
                raise ValueError("device_aug: raw slices %s do not match the plan's window %s"
                                 % (tuple(raw["img"].shape), g.src))
            r[R_KIND], r[R_CH], r[R_CW], r[R_FLIP] = KIND_PLAN, ch, cw, int(g.flip)
            r[R_IMG], r[R_LBL] = blob.add(raw["img"].numpy()), blob.add(raw["lbl"].numpy())
            if "paste_img" in raw:
                r[R_PIMG], r[R_PLBL] = blob.add(raw["paste_img"].numpy()), blob.add(raw["paste_lbl"].numpy())
                r[R_PTAB] = blob.add(paste_table_bytes(raw["paste_table"].numpy(), rect_w))
                if rect_w is not None:
                    r[R_KIND] = KIND_PLAN_RECT
        r[R_HLO], r[R_HN], r[R_HK], r[R_HT] = tabs.add(g.hlo), tabs.add(g.hn), tabs.add(g.hk), g.hk.shape[1]
        r[R_VLO], r[R_VN], r[R_VK], r[R_VT] = tabs.add(g.vlo), tabs.add(g.vn), tabs.add(g.vk), g.vk.shape[1]
        r[R_NX], r[R_NY] = tabs.add(g.nx), tabs.add(g.ny)
        max_ch = max(max_ch, ch)
        fda = iter(raw.get("fda", ()))
        for k, v in enumerate(s["plan"]):
            row = ops[k, b]
            row[0] = KIND_PLAN
            for op in (v["ops"][1:] if k == 0 else v["ops"]):
                i = int(row[2])
                if op[0] == "lut":
                    row[4 + 2 * i], row[5 + 2 * i] = OP_LUT, blob.add(op[1])
                elif op[0] == "gray":
                    row[4 + 2 * i] = OP_GRAY
                elif op[0] == "equalize":
                    row[4 + 2 * i] = OP_EQUALIZE
                elif op[0] in ("contrast", "sat"):           # the full float64 draw, as its bits
                    row[4 + 2 * i] = OP_CONTRAST if op[0] == "contrast" else OP_SAT
                    row[5 + 2 * i] = np.array([op[1]], np.float64).view(np.int64)[0]
                elif op[0] == "hue":
                    row[4 + 2 * i], row[5 + 2 * i] = OP_HUE, int(op[1])
                elif op[0] == "blur":                        # float32 weights (as bits) in the int32 table blob
                    w = np.ascontiguousarray(op[1], np.float32)
                    row[4 + 2 * i], row[5 + 2 * i] = OP_BLUR, tabs.add(w.view(np.int32)) | (len(w) << 32)
                elif op[0] == "fda":                         # the target view travels as CopyPaste's source frame does
                    t = next(fda).numpy()
                    if tuple(t.shape) != (out[0], out[1], 3) or not 0 <= int(op[2]) <= FDA_MAX_BORDER:
                        raise ValueError("device_aug: FDA target %s for a view of %s, border %r" % (tuple(t.shape), out, op[2]))
                    row[4 + 2 * i], row[5 + 2 * i] = OP_FDA, blob.add(t) | (int(op[2]) << FDA_BORDER_SHIFT)
                else:
                    raise ValueError("op %r has no device form" % (op[0],))
                row[2] = i + 1
    t = {"blob": torch.from_numpy(blob.join()), "tabs": torch.from_numpy(tabs.join()),
         "recs": torch.from_numpy(recs), "ops": torch.from_numpy(ops),
         "meta": torch.tensor([n_views, out[0], out[1], max_ch, int(multi)], dtype=torch.int64)}
    if (store_idx[:, 0] >= 0).any():         # (frame index, paste source index | -1) of the KIND_STORE samples, -1 elsewhere
        t["store_idx"] = torch.from_numpy(store_idx)
        if (store_rect[:, 0] >= 0).any():    # the FRAME rectangle of the KIND_STORE_RECT samples (their copy_paste_mask), -1 elsewhere
            t["store_rect"] = torch.from_numpy(store_rect)
    return t


def collate(samples):
    """DataLoader collate_fn of a device_aug dataset: the sample parts become ONE set of tables per batch (crop windows
    differ in size, nothing is stacked); every other key collates as usual"""
    from torch.utils.data import default_collate
    rest = [{k: v for k, v in s.items() if k not in ("raw", "plan", "multi")} for s in samples]
    # a sample over resident frames has no source label to cut its copy_paste_mask from (None): the masks of such a batch
    # travel one by one and assemble_device_batch builds the missing ones on the device
    masks = [r["copy_paste_mask"] for r in rest] if any(r.get("copy_paste_mask", 0) is None for r in rest) else None
    if masks is not None:
        rest = [{k: v for k, v in r.items() if k != "copy_paste_mask"} for r in rest]
    out = default_collate(rest)
    out["device_aug"] = build_batch_tables(samples)
    if masks is not None:
        out["device_aug"]["cp_masks"] = masks
    return out


def is_device_aug_batch(batch):
    return isinstance(batch, dict) and "device_aug" in batch


def _store_copy_paste_mask(t, store, device):
    """the batch's copy_paste_mask [B, H, W] uint8 ON THE DEVICE, the bytes the worker path delivers: a worker's mask where
    it made one, else where(table[lbl_src] and inside the paste's rectangle, lbl_src, 255) from the resident source label
    (255 everywhere without a source): ONE launch of hiast_aug_paste_mask_u8 for all the frames without a worker's mask"""
    from hiast_amd import kernels as K
    masks, idx = t["cp_masks"], t["store_idx"].tolist()
    shapes = {tuple(m.shape) if m is not None else tuple(int(v) for v in store.frames[idx[b][0], 2:])
              for b, m in enumerate(masks)}
    if len(shapes) != 1:
        raise ValueError("device_aug: copy_paste_mask of frames of different sizes in one batch: %s" % sorted(shapes))
    H, W = shapes.pop()
    out = torch.empty((len(masks), H, W), dtype=torch.uint8, device=device)
    rects = t["store_rect"].tolist() if "store_rect" in t else None
    rows = []                                   # (source label offset | -1, table offset, y0, y1, x0, x1, frame of `out`, 0)
    for b, m in enumerate(masks):
        if m is not None:
            out[b].copy_(m, non_blocking=True)
        elif idx[b][1] < 0:
            rows.append((-1, 0, 0, 0, 0, 0, b, 0))
        else:
            rect = rects[b] if rects is not None and rects[b][0] >= 0 else (0, H, 0, W)
            rows.append((int(store.frames[idx[b][1], 1]), int(t["recs"][b, R_PTAB])) + tuple(rect) + (b, 0))
    if rows:
        K.paste_mask_u8(store.buffer, t["blob"].to(device, non_blocking=True), np.array(rows, np.int64), out)
    return out


def assemble_device_batch(batch, device, store=None):
    """a collated device_aug batch -> what utils.to_device_batch returns for the same samples: normalised float32 CHW
    views (a list for a multi-view dataset) and uint8 labels (a list of the same tensor per view).  store: the
    device_store.ResidentSet of the batch's dataset, needed when the batch holds KIND_STORE samples; their part of
    batch["copy_paste_mask"] is built here, on the device (the tensor then lives there)"""
    from hiast_amd import kernels as K
    from hiast_amd.sseg.datasets.utils import MEAN, STD
    t = batch["device_aug"]
    n_views, oh, ow, max_ch, multi = (int(v) for v in t["meta"])
    if "store_idx" in t:
        if store is None:
            raise ValueError("device_aug: the batch holds samples over device-resident frames but no store was given")
        views, lbl = K.aug_batch_store_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, device, store)
        if "cp_masks" in t:
            batch["copy_paste_mask"] = _store_copy_paste_mask(t, store, device)
    else:
        views, lbl = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, device)
    imgs = [K.normalize_u8(v, MEAN, STD) for v in views]
    if multi:
        return imgs, [lbl for _ in imgs]
    return imgs[0], lbl
