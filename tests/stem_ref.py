"""References and error bounds of the stem, pooling, packing and table kernels (stem.hip, igemm.hip's stem tail / planes / packs,
conv1x1.hip's inference BatchNorm, misc.hip); no GPU needed.  DESIGN.md §2.4 carries the derivations at length.

EXACT entries (bit-equal, no tolerance): split planes (integer round-to-nearest-even of v, then of the fp32 v - hi; inverse hi + lo
in fp32), the packed-weight layout of ig_wp_elem (igemm.hip) for three formats and three modes, max-pool values and window codes,
max-pool backward (fp32 sum over at most 4 windows in ascending (yo, xo) order, rounded once), normalize_u8, ema_update
(numpy float32, unfused), multi_copy (bytes), confusion_hist (the rule in confusion_kernel's comment).

BOUNDED entries, u = 2^-24, u16 = 2^-8 (bf16) | 2^-11 (fp16), every magnitude taken in float64:
  scale / shift   sc = gamma (1 / sqrtf(var + eps)): add, sqrt, divide, multiply — each rounded ONCE: hiast_amd/csrc/Makefile
                  builds with -fno-fast-math and without -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default of
                  correctly rounded fp32 division and square root holds (`assert_flags`).  The add's u is halved by the root:
                  |sc~ - sc| <= 3.5 u |sc|.  sh = fmaf(-mean, sc~, beta): 3.5 u |mean sc| + u |sh|.  t = fmaf(x, sc~, sh~):
                  3.5 u |x sc| + 3.5 u |mean sc| + u |sh| + u |t| <= 4.5 u |x sc| + 5.5 u |mean sc| + 2 u |beta|; the products of
                  (1 + u) factors dropped here are below u^2 x 20: c = C_ELEM = 6 covers them.
                      E_elem = 6 u (|x sc| + |mean sc| + |beta|)                  (the shape of §2.1's y bound)
  bn_act_nhwc_infer   E_elem, + u16 (|want| + E_elem) for bf16 rows.  ReLU never increases an error.
  stem_tail       per activation E_elem, + u16_in (|t| + E_elem) (+ 2^-25 in fp16: a subnormal result) for the rounding to the 16-bit
                  INPUT type behind the ReLU; the error of a window's maximum is at most the largest element error in the window;
                  then the output format: u16_out (|m| + E) (+ 2^-25) for rows, 2^-16 (|m| + E) for hi + lo of split planes.
  stem_eval       float64 convolution on the operands the kernel multiplies (x and w rounded to the format; split planes: the fp32
                  values, + 3 · 2^-16 (1 + 2^-6) S for the dropped lo·lo product and the rounding of both lo, as head_ref has
                  them).  The 16-bit products are exact in fp32; accumulation: seven v_mfma_f32_16x16x32 steps of 32 slots, three
                  per step with split planes: n = 224 | 672 terms in some order: gamma(n) S, S the convolution of the magnitudes.
                  Through the scale: E = |sc| (1 + 3.5 u) E_conv + E_elem(conv value); then the stem_tail chain without the
                  intermediate rounding.  Out-of-map convolution outputs are 0 (behind a ReLU they never win).
"""
import re
import os

import numpy as np
import torch

import synth
from bn_ref import U16, U32, round16
from head_ref import gamma

F = torch.nn.functional
EPS = 1e-5
C_ELEM = 6
SPLIT_REPR = 2.0 ** -16                       # |v - (hi + lo)| <= 2^-16 |v|
SPLIT_OPERANDS = 3 * 2.0 ** -16 * (1 + 2.0 ** -6)
FP16_TINY = 2.0 ** -25
MFMA_K = 32
FMTS = ("bf16", "split", "fp16")
OPERAND_TYPE = {"bf16": "bf16", "fp16": "fp16", "split": "fp32"}


def assert_flags():
    """the flags the scale / shift figure rests on"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "hiast_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.+)$", mk, re.M).group(1).split()
    assert "-fno-fast-math" in flags and "-ffp-contract=off" in flags
    assert not any("correctly-rounded-divide-sqrt" in f and f.startswith("-fno") for f in flags)
    assert not any(f in ("-ffast-math", "-Ofast", "-fapprox-func", "-funsafe-math-optimizations") for f in flags)
    return flags


# ------------------------------------------------------------------------------------------------ bits
def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_bits(a):
    """float32 -> bf16 bits (uint16), round to nearest even in integer arithmetic; a NaN keeps its upper half, made quiet"""
    u = f32_bits(a).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(a, np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_val(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def fp16_bits(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, np.float32).astype(np.float16).view(np.uint16)


def enc16(a, fmt):
    return fp16_bits(a) if fmt == "fp16" else bf16_bits(a)


def dec16(bits, fmt):
    bits = np.asarray(bits, np.uint16)
    return bits.view(np.float16).astype(np.float32) if fmt == "fp16" else bf16_val(bits)


def split_bits(a):
    """-> (hi bits, lo bits): bf16 of v, then bf16 of the FLOAT32 difference v - hi"""
    a = np.ascontiguousarray(a, np.float32)
    hi = bf16_bits(a)
    with np.errstate(invalid="ignore", over="ignore"):
        rem = (a - bf16_val(hi)).astype(np.float32)
    return hi, bf16_bits(rem)


def planes_of(a):
    """fp32 [M][C] -> uint16 [M][2 C]: per 32-channel slab 32 hi then 32 lo (ig_elem<2>)"""
    M, C = a.shape
    hi, lo = split_bits(a)
    return np.stack([hi.reshape(M, C // 32, 32), lo.reshape(M, C // 32, 32)], 2).reshape(M, 2 * C)


def merge_of(p):
    """uint16 [M][2 C] -> fp32 [M][C]: hi + lo in float32"""
    M, C2 = p.shape
    q = p.reshape(M, C2 // 64, 2, 32)
    with np.errstate(invalid="ignore"):
        return (bf16_val(q[:, :, 0]) + bf16_val(q[:, :, 1])).astype(np.float32).reshape(M, C2 // 2)


def planes_value(p):
    """the float64 value hi + lo of split planes [.., 2 C] -> [.., C]"""
    q = p.reshape(p.shape[:-1] + (p.shape[-1] // 64, 2, 32))
    v = bf16_val(q[..., 0, :]).astype(np.float64) + bf16_val(q[..., 1, :]).astype(np.float64)
    return v.reshape(p.shape[:-1] + (p.shape[-1] // 2,))


def out_value(bits, fmt):
    """what an output in operand format fmt (uint16 array, last axis planes * C) holds, float64"""
    return planes_value(bits) if fmt == "split" else dec16(bits, fmt).astype(np.float64)


# ------------------------------------------------------------------------------------------------ packed weights
def pack_elem(n, t, k, taps, KO, PL):
    """ig_wp_elem of igemm.hip: element offset of (row n, tap t, reduction channel k); the lo half of split planes 32 further"""
    row = (n * taps + t) * PL * KO
    return row + (k >> 5) * 64 + (k & 31) if PL == 2 else row + k


def pack_ref(w, fmt, mode):
    """w fp32 [N][K][taps] -> (wp, wpt) uint16, flat, as hiast_pack_conv_weight leaves them: mode 0 (forward, None), 1 (adjoint in
    wp, None), 2 (forward, adjoint).  Forward [N][taps][PL K], adjoint [K][taps flipped][PL N]."""
    N, K, taps = w.shape
    PL = 2 if fmt == "split" else 1
    if fmt == "split":
        hi, lo = split_bits(w)
    else:
        hi, lo = enc16(w, fmt), None
    n, k, t = np.meshgrid(np.arange(N), np.arange(K), np.arange(taps), indexing="ij")

    def form(rows, red, tt, KO, NR):
        out = np.zeros(NR * taps * PL * KO, np.uint16)
        off = pack_elem(rows, tt, red, taps, KO, PL)
        assert off.max() + (32 if PL == 2 else 0) < out.size, "the layout leaves the buffer: a ragged split-plane slab"
        out[off.ravel()] = hi.ravel()
        if PL == 2:
            out[off.ravel() + 32] = lo.ravel()
        return out
    fwd = form(n, k, t, K, N) if mode != 1 else None
    adj = form(k, n, taps - 1 - t, N, K) if mode != 0 else None
    return (adj, None) if mode == 1 else (fwd, adj)


def pack_reach(N, K, taps, PL, mode):
    """the largest element offset (+1) the layout writes per form, against the buffer's element count: (reach, size) forward and
    adjoint — what the refusal of ragged split-plane slabs is about"""
    out = []
    for rows, red in ((N, K), (K, N)):
        reach = pack_elem(rows - 1, taps - 1, red - 1, taps, red, PL) + (33 if PL == 2 else 1)
        out.append((reach, rows * taps * PL * red))
    return out


# ------------------------------------------------------------------------------------------------ max-pool (K18)
def _taps(H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yo, xo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    for k in range(9):
        yy, xx = 2 * yo - 1 + k // 3, 2 * xo - 1 + k % 3
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yield k, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), ok


def maxpool_ref(x):
    """x [B][H][W][C] float32 (the 16-bit values) -> (value [B][Ho][Wo][C] float32, code uint8): the first maximum in row-major
    window order, a later NaN takes over, the code of the first in-image tap where nothing exceeds -inf"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    m = np.full((B, Ho, Wo, C), -np.inf, np.float32)
    code = np.full((B, Ho, Wo, C), 255, np.uint8)
    for k, yy, xx, ok in _taps(H, W):
        v = x[:, yy, xx, :]
        okb = ok[None, :, :, None]
        code = np.where(okb & (code == 255), np.uint8(k), code)
        with np.errstate(invalid="ignore"):
            take = okb & ((v > m) | np.isnan(v))
        m = np.where(take, v, m)
        code = np.where(take, np.uint8(k), code)
    return m, code


def maxpool_bwd_ref(dy, code, H, W, fmt):
    """dy [B][Ho][Wo][C] float32 (16-bit values), code from the forward -> dx bits uint16 [B][H][W][C]: fp32 sum over the windows
    (yo, xo) that hold the pixel, ascending, of dy where code == the pixel's position in the window; rounded once"""
    B, Ho, Wo, C = dy.shape
    yi, xi = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    acc = np.zeros((B, H, W, C), np.float32)
    for a in (0, 1):
        yo = yi // 2 + a
        for c in (0, 1):
            xo = xi // 2 + c
            ok = (a < 1 + (yi & 1)) & (c < 1 + (xi & 1)) & (yo < Ho) & (xo < Wo)
            pos = ((yi - (2 * yo - 1)) * 3 + (xi - (2 * xo - 1))).astype(np.int64)
            yc, xc = np.clip(yo, 0, Ho - 1), np.clip(xo, 0, Wo - 1)
            hit = ok[None, :, :, None] & (code[:, yc, xc, :].astype(np.int64) == pos[None, :, :, None])
            acc = np.where(hit, (acc + dy[:, yc, xc, :]).astype(np.float32), acc)
    return enc16(acc, fmt)


# ------------------------------------------------------------------------------------------------ small exact kernels
def normalize_ref(img, mean, std):
    """uint8 [B][HW][3] -> float32 [B][3][HW]: v = float(u8) / 255; (v - mean) / std, each operation rounded to float32"""
    v = img.astype(np.float32) / np.float32(255.0)
    out = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert out.dtype == np.float32
    return np.ascontiguousarray(np.moveaxis(out, -1, 1))


def ema_ref(ema, p, g, omg):
    g, omg = np.float32(g), np.float32(omg)
    a, b = (ema * g).astype(np.float32), (p * omg).astype(np.float32)      # two roundings, then the add: no fma
    return (a + b).astype(np.float32)


def confusion_ref(pred, target, K):
    """utils/metrics.py as confusion_kernel states it: p = 255 where t == 255 else pred; area_pred counts p in [0, K), area_tgt
    t in [0, K), inter p == t in [0, K) — for K > 255 the value 255 is a class as well as the ignore value"""
    t = np.asarray(target, np.int64)
    p = np.where(t == 255, 255, np.asarray(pred, np.int64))
    inr = lambda a: (a >= 0) & (a < K)
    cnt = lambda a: np.bincount(a, minlength=K).astype(np.int64)
    return cnt(p[inr(p) & (p == t)]), cnt(p[inr(p)]), cnt(t[inr(t)])


# ------------------------------------------------------------------------------------------------ scale / shift, element bound
def bn_vectors(C, seed, with_affine=True):
    g = synth.rng(seed)
    gam = (1.0 + 0.5 * g.standard_normal(C)).astype(np.float32) if with_affine else None
    bet = (0.5 * g.standard_normal(C)).astype(np.float32) if with_affine else None
    return gam, bet, g.standard_normal(C).astype(np.float32), (0.5 + g.random(C)).astype(np.float32)


def scale_shift(gam, bet, mean, var, eps=EPS):
    """float64 from the float32 parameters (eps as the float32 the entry is handed) -> sc, sh, |mean sc|, |beta|"""
    C = len(mean)
    g = np.ones(C) if gam is None else np.asarray(gam, np.float64)
    b = np.zeros(C) if bet is None else np.asarray(bet, np.float64)
    sc = g / np.sqrt(np.asarray(var, np.float64) + float(np.float32(eps)))
    return sc, b - np.asarray(mean, np.float64) * sc, np.abs(np.asarray(mean, np.float64) * sc), np.abs(b)


def scale_shift_f32(gam, bet, mean, var, eps=EPS):
    """the kernels' float32 order: sc = gamma * (1 / sqrtf(var + eps)); sh = fmaf(-mean, sc, beta) (the fma through float64:
    a product of two float32 is exact there, the sum is rounded to double and then to float — double rounding, 2^-29 relative at
    worst, which is why this is a restatement for the bound tests and not an exact reference)"""
    C = len(mean)
    one = np.float32(1.0)
    g = np.ones(C, np.float32) if gam is None else np.asarray(gam, np.float32)
    b = np.zeros(C, np.float32) if bet is None else np.asarray(bet, np.float32)
    inv = (one / np.sqrt((np.asarray(var, np.float32) + np.float32(eps)).astype(np.float32))).astype(np.float32)
    sc = (g * inv).astype(np.float32)
    return sc, fma32(-np.asarray(mean, np.float32), sc, b)


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def elem(x, gam, bet, mean, var, relu=True):
    """x [.., C] (values of its storage type) -> (want float64, E_elem)"""
    sc, sh, ms, ab = scale_shift(gam, bet, mean, var)
    x = np.asarray(x, np.float64)
    t = x * sc + sh
    E = C_ELEM * U32 * (np.abs(x * sc) + ms + ab)
    return (np.maximum(t, 0.0) if relu else t), E


def round_term(want, E, fmt):
    """the error a rounding of the computed value to fmt adds"""
    if fmt == "fp32":
        return 0.0
    return U16[fmt] * (np.abs(want) + E) + (FP16_TINY if fmt == "fp16" else 0.0)


def bn_infer_ref(x, gam, bet, mean, var, relu, dtype):
    want, E = elem(x, gam, bet, mean, var, relu)
    return want, E + round_term(want, E, dtype)


def pool_max(t, E, H, W):
    """t, E [B][H][W][C] -> the 3x3 / stride 2 / padding 1 maximum of t and, per window, the largest E in it"""
    m = e = None
    for k, yy, xx, ok in _taps(H, W):
        okb = ok[None, :, :, None]
        v = np.where(okb, t[:, yy, xx, :], -np.inf)
        ev = np.where(okb, E[:, yy, xx, :], 0.0)
        m = v if m is None else np.maximum(m, v)
        e = ev if e is None else np.maximum(e, ev)
    return m, e


def out_term(m, E, fmt):
    return SPLIT_REPR * (np.abs(m) + E) if fmt == "split" else round_term(m, E, fmt)


def stem_tail_ref(x, in_type, gam, bet, mean, var, fmt):
    """x [B][H][W][C] (values of in_type) -> (want [B][Ho][Wo][C] float64, bound)"""
    B, H, W, C = x.shape
    t, E = elem(x, gam, bet, mean, var)
    E = E + round_term(t, E, in_type)
    m, e = pool_max(t, E, H, W)
    return m, e + out_term(m, e, fmt)


# ------------------------------------------------------------------------------------------------ stem_eval
def stem_operands(x, w, fmt):
    """the values the kernel multiplies: rounded to the 16-bit format, or the fp32 values for split planes"""
    t = OPERAND_TYPE[fmt]
    return round16(x, t).astype(np.float64), round16(w, t).astype(np.float64)


def conv_dims(H, W):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Hc, Wc, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def conv64(x, w):
    """float64 conv 7x7 / stride 2 / padding 3 -> channels-last [B][Hc][Wc][64]"""
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(w)).double(), None, 2, 3)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def stem_terms(fmt):
    return 7 * MFMA_K * (3 if fmt == "split" else 1)


def stem_eval_ref(x, w, gam, bet, mean, var, fmt):
    """x [B][3][H][W], w [64][3][7][7] float32 -> (want [B][Hp][Wp][64] float64, bound)"""
    xo, wo = stem_operands(x, w, fmt)
    a, S = conv64(xo, wo), conv64(np.abs(xo), np.abs(wo))
    Ec = gamma(stem_terms(fmt)) * S + (SPLIT_OPERANDS * S if fmt == "split" else 0.0)
    sc = scale_shift(gam, bet, mean, var)[0]
    t, Ee = elem(a, gam, bet, mean, var)
    E = np.abs(sc) * (1 + 3.5 * U32) * Ec + Ee + C_ELEM * U32 * np.abs(sc) * Ec
    Hc, Wc = a.shape[1:3]
    m, e = pool_max(t, E, Hc, Wc)
    return m, e + out_term(m, e, fmt)


def stem_eval_blocks(ntiles, cus, fmt):
    """the entry's grid: persistent blocks, two per CU in the 16-bit formats, one with split planes (CU reserve 0)"""
    return min(ntiles, (1 if fmt == "split" else 2) * cus)


def stem_tiles(B, H, W):
    _, _, Hp, Wp = conv_dims(H, W)
    return B * (-(-Hp // 4)) * (-(-Wp // 6))


# ------------------------------------------------------------------------------------------------ grids
def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def stem_tail_grid(B, H, W, C, cap=16384):
    """-> (blocks, need, capped) of hiast_stem_tail; None where it refuses"""
    G = C // 8
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nb = -(-B * Ho * Wo * G // 256)
    need = G // gcd(256, G)
    if nb <= cap:
        return nb, need, False
    return (cap - cap % need, need, True) if cap >= need else None


def bn_infer_grid(M, C, dtype):
    """-> (blocks, fixed-channel path?) of hiast_bn_act_nhwc_infer: the kernel takes the fixed-channel path when
    (blocks * 256 * vec) % C == 0"""
    vec = 8 if dtype == "bf16" else 4
    nb = max(1, min(8192, -(-(M * C // vec) // 1024)))
    need = C // gcd(C, 256 * vec)
    if nb >= need:
        nb -= nb % need
    return nb, (nb * 256 * vec) % C == 0


# ------------------------------------------------------------------------------------------------ float32 restatements, mutants
def elem_f32(x, gam, bet, mean, var, relu=True):
    sc, sh = scale_shift_f32(gam, bet, mean, var)
    t = fma32(x, sc, sh)
    return np.maximum(t, np.float32(0)) if relu else t


def store16(m, fmt):
    """float32 -> the value an output of format fmt holds"""
    if fmt == "split":
        hi, lo = split_bits(m)
        return bf16_val(hi).astype(np.float64) + bf16_val(lo).astype(np.float64)
    return dec16(enc16(m, fmt), fmt).astype(np.float64)


def stem_tail_f32(x, in_type, gam, bet, mean, var, fmt, group_shift_after=None):
    """the kernel's order in float32.  group_shift_after = n: MUTANT — flat thread items (pixel, channel group) from index n on
    take the scale / shift of the NEXT channel group (a grid-stride that is no multiple of C / 8, on the second stride)"""
    B, H, W, C = x.shape
    t = elem_f32(x, gam, bet, mean, var)
    if in_type != "fp32":
        t = dec16(enc16(t, in_type), in_type)
    m, _ = pool_max(t.astype(np.float64), np.zeros_like(t, np.float64), H, W)
    if group_shift_after is not None:
        G = C // 8
        roll = lambda v: None if v is None else np.roll(np.asarray(v).reshape(G, 8), -1, 0).reshape(C)
        t2 = elem_f32(x, roll(gam), roll(bet), roll(mean), roll(var))
        if in_type != "fp32":
            t2 = dec16(enc16(t2, in_type), in_type)
        m2, _ = pool_max(t2.astype(np.float64), np.zeros_like(t2, np.float64), H, W)
        flat = np.arange(m.size // 8).reshape(m.shape[:3] + (G,))                   # i = pix * G + cg
        m = np.where(np.repeat(flat >= group_shift_after, 8, -1), m2, m)
    return store16(m.astype(np.float32), fmt)


def _patches(xp, Hc, Wc):
    """xp [B][3][H+pad][W+pad] -> [B][Hc][Wc][3][7][7]"""
    B = xp.shape[0]
    out = np.empty((B, Hc, Wc, 3, 7, 7), xp.dtype)
    for ky in range(7):
        for kx in range(7):
            out[..., ky, kx] = np.moveaxis(xp[:, :, ky:ky + 2 * Hc:2, kx:kx + 2 * Wc:2], 1, -1)
    return out


def stem_eval_f32(x, w, gam, bet, mean, var, fmt, mutant=None):
    """the kernel's arithmetic with a float32 accumulator: per kernel row ky the 21 (with split planes 63) exact products are
    added to the accumulator with one rounding (an MFMA step), then scale / shift, ReLU, zero outside the map, 3x3 maximum, the
    output format.  mutant: "kx6" (tap kx = 6 dropped), "wrap" (padding read from the opposite border), "pool2p" (the window
    starts at 2p instead of 2p - 1), "keep_outside" (out-of-map convolution outputs keep their computed value), "no_lohi"
    (split planes without lo(w) x hi(x))"""
    B, _, H, W = x.shape
    Hc, Wc, Hp, Wp = conv_dims(H, W)
    # the convolution on a grid one output wider on every side: the out-of-map outputs the pooling windows touch
    He, We = Hc + 2, Wc + 2
    pad = ((0, 0), (0, 0), (5, 2 * He + 6), (5, 2 * We + 6))

    def padded(a):
        if mutant == "wrap":
            return np.pad(a, pad, mode="wrap")[:, :, :2 * He + 5, :2 * We + 5]
        return np.pad(a, pad)[:, :, :2 * He + 5, :2 * We + 5]
    if fmt == "split":
        xh, xl = (bf16_val(b) for b in split_bits(x))
        wh, wl = (bf16_val(b) for b in split_bits(w))
        pairs = [(wh, xh), (wl, xh), (wh, xl)]
        if mutant == "no_lohi":
            pairs = [(wh, xh), (wh, xl)]
    else:
        pairs = [(round16(w, fmt), round16(x, fmt))]
    acc = np.zeros((B, He, We, 64), np.float32)
    pts = [(_patches(padded(xv).astype(np.float64), He, We), wv.astype(np.float64)) for wv, xv in pairs]
    for ky in range(7):
        for P, wv in pts:
            wk = wv[:, :, ky, :].copy()
            if mutant == "kx6":
                wk[:, :, 6] = 0.0
            step = np.einsum("bhwck,ock->bhwo", P[..., ky, :], wk)                 # exact products, summed in double
            acc = (acc.astype(np.float64) + step).astype(np.float32)               # one rounding per MFMA step
    t = elem_f32(acc, gam, bet, mean, var)
    inside = np.zeros((He, We), bool)
    inside[1:1 + Hc, 1:1 + Wc] = True
    if mutant != "keep_outside":
        t = np.where(inside[None, :, :, None], t, np.float32(0))
    o = 1 if mutant == "pool2p" else 0                                              # extended index of the window's first tap
    m = None
    for k in range(9):
        ys = 2 * np.arange(Hp) + o + k // 3
        xs = 2 * np.arange(Wp) + o + k % 3
        ok = (ys < He)[:, None] & (xs < We)[None, :]
        v = np.where(ok[None, :, :, None], t[:, np.minimum(ys, He - 1)][:, :, np.minimum(xs, We - 1)], np.float32(0))
        m = v if m is None else np.maximum(m, v)
    return store16(m.astype(np.float32), fmt)


# ------------------------------------------------------------------------------------------------ inputs
def stem_eval_inputs(B, H, W, seed=0, with_affine=True):
    """image-like x (normalised pixels, sigma 1), He-scaled weights, BatchNorm of 64 channels"""
    s = 1000 * seed + 7 * H + W + B
    x = synth.normal_f32(s, (B, 3, H, W), 1.0)
    w = synth.normal_f32(s + 1, (64, 3, 7, 7), 0.12)
    return (x, w) + bn_vectors(64, s + 2, with_affine)


def act_inputs(shape, in_type, seed):
    return round16(synth.normal_f32(seed, shape, 2.0) + np.float32(0.3), in_type)


def pool_input(shape, kind, fmt, seed):
    """max-pool inputs (values of fmt): smooth | ties (a handful of values) | special (15 % -inf, 10 % NaN)"""
    g = synth.rng(seed)
    x = g.standard_normal(shape) * 2.0
    if kind == "ties":
        x = np.round(x)                                                  # a handful of values: most windows hold a tie
    x = dec16(enc16(x.astype(np.float32), fmt), fmt)
    if kind == "special":
        r = g.random(shape)
        x = np.where(r < 0.15, np.float32(-np.inf), x)
        x = np.where((r >= 0.15) & (r < 0.25), np.float32(np.nan), x).astype(np.float32)
    return x


STEM_EVAL_SHAPES = [(1, 1, 1), (1, 2, 3), (2, 9, 14), (1, 16, 24), (1, 17, 25), (1, 13, 21), (2, 67, 101)]
STEM_TAIL_SHAPES = [(1, 1, 1), (1, 3, 3), (2, 5, 4), (2, 37, 53)]
STEM_TAIL_C = [8, 24, 32, 64, 96]
BN_INFER_SHAPES = [(1, 8), (3, 24), (257, 40), (4099, 64), (1025, 2048)]
POOL_SHAPES = [(1, 1, 1, 8), (1, 1, 2, 8), (1, 2, 1, 8), (2, 5, 4, 16), (1, 7, 9, 24), (2, 37, 53, 64)]
