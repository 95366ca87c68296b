"""float64 reference of the BatchNorm (+ residual) (+ ReLU) passes of bn_nhwc.hip / bn_act.hip and error bounds DERIVED from
the arithmetic those files document (a plain helper module: numpy only, no fixtures).

Layouts.  A 2-d activation is channels-last rows [M][C]; anything with more axes is [B][C][...] (NCHW).  Per-channel vectors are
[C].  `x`, `dy`, `res`, `y` hold values already rounded to the storage type; `gamma`, `beta`, `mean`, `invstd` are float32 arrays
taken as given (None = 1 / 0 for gamma / beta).  The elementwise functions use nothing but operators and the methods numpy
arrays and torch tensors share, so a GPU test may hand them float64 device tensors (the 8-million-element shapes would take
seconds per variant on the host); the per-channel functions (`prep` and its bounds) are numpy.

Bounds.  u32 = 2^-24; u16 = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32 storage).
  sums      |S_dev - S_ref| <= (L + k) u32 Σ|term|: a chain of L fp32 additions carries at most L roundings of the running sum,
            each <= u32 Σ|term| to first order; k = 2 for the term's own rounding and the fold's last step (Σx, Σx², Σg), k = 4 for
            Σ g·x̂ (x̂ = (x - mean)·invstd carries two more fp32 roundings).  Everything after the chains is double.
            channels-last: L = ceil(M / (nblk·RPP)) + UNR + RPP (a thread's rows, rounded up to whole chunks of UNR, then the fold
            of the RPP row subsets); NCHW: L = ceil(HW / 256), in whole vectors on the vector path.
  prep      mean, invstd, running statistics: 4 u32 relative against `prep` on the same sums (one rounding double -> float, three
            fp32 operations in the running update); invstd also 2^-40 (Σx²/count) / (var + eps) relative for the cancellation
            in the double var = Σx²/n - mean².
  y         u16 |want| + 4 u32 (|x γ is| + |μ γ is| + |β| + |res|)  (+ 2^-25: half a subnormal step of fp16)
  dx        u16 |want| + 6 u32 |γ is| (|g| + |Σg/n| + |x̂ Σ(g x̂)/n|)   (+ 2^-25 for fp16: the derivation of the relative term
            assumes a normal result; an fp16 result below 2^-14 is rounded to a multiple of 2^-24 — the same half step as in y.
            This is a term ADDED to the formula first written down for dx, which had none; it is not a raised constant)
  exact     dres = dy where open, +0 where closed; dgamma, dbeta = float32(sums); mask bits = (stored y > 0).
"""
import functools

import numpy as np

import synth

U32 = 2.0 ** -24
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}
UNR_PART = 8                 # BNH_UNR_PART
MAXBLK = 512                 # BNH_MAXBLK
MARGIN = 2.0 ** -20


# ------------------------------------------------------------------------------------------------ plumbing
def round16(a, fmt):
    """float32 numpy -> the nearest value of the storage type (round to nearest even), as float32"""
    a = np.ascontiguousarray(a, np.float32)
    if fmt == "fp32":
        return a
    if fmt == "fp16":
        return a.astype(np.float16).astype(np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def _is_t(a):
    return hasattr(a, "new_tensor")


def _f64(a):
    return a.double() if _is_t(a) else np.asarray(a, np.float64)


def _ch(v, x):
    """per-channel vector -> float64, broadcastable against activation x"""
    if _is_t(x) and not _is_t(v):
        v = x.new_tensor(np.asarray(v, np.float64), dtype=x.new_empty(0).double().dtype)
    v = _f64(v)
    return v if x.ndim == 2 else v.reshape((1, -1) + (1,) * (x.ndim - 2))


def _rsum(t, x_ndim, planes=False):
    """Σ over everything but the channel axis -> [C]; planes (NCHW only): per (n, c) plane -> [C][B]"""
    if x_ndim == 2:
        return t.sum(axis=0)
    if planes:
        return t.sum(axis=tuple(range(2, x_ndim))).T
    return t.sum(axis=(0,) + tuple(range(2, x_ndim)))


def _gamma_beta(gamma, beta, like):
    C = len(like)
    g = np.ones(C, np.float32) if gamma is None else np.asarray(gamma)
    b = np.zeros(C, np.float32) if beta is None else np.asarray(beta)
    return g, b


# ------------------------------------------------------------------------------------------------ reference
def sums_fwd(x, planes=False):
    """-> (Σx, Σx²) float64 per channel (per plane [C][B] with planes=True)"""
    x = _f64(x)
    return _rsum(x, x.ndim, planes), _rsum(x * x, x.ndim, planes)


def xhat(x, mean, invstd):
    x = _f64(x)
    return (x - _ch(mean, x)) * _ch(invstd, x)


def sums_bwd(dy, open_, x, mean, invstd, planes=False):
    """-> (Σg, Σ g·x̂) float64, g = dy where open_ (None: everywhere)"""
    g = _f64(dy) if open_ is None else _f64(dy) * _f64(open_)
    return _rsum(g, g.ndim, planes), _rsum(g * xhat(x, mean, invstd), g.ndim, planes)


def prep(sums, count, momentum, eps, run_mean=None, run_var=None, exact=False):
    """the kernels' double formula: -> (mean f32, invstd f32, new running mean f64 | None, new running var f64 | None).
    var is clamped at 0; the running variance is unbiased only when count > 1.  The running values are returned unrounded.
    exact: nothing is rounded to float32 (mean, invstd, eps, momentum stay double) — the mathematical definition, for the
    comparison with float64 autograd."""
    s1, s2 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    count = float(count)
    r32 = (lambda a: a) if exact else (lambda a: np.asarray(a, np.float64).astype(np.float32))
    m = s1 / count
    var = np.maximum(s2 / count - m * m, 0.0)
    mean = r32(m)
    invstd = r32(1.0 / np.sqrt(var + float(r32(eps))))
    if run_mean is None:
        return mean, invstd, None, None
    unb = var * count / (count - 1.0) if count > 1.0 else var
    mom = float(r32(momentum))
    om = 1.0 - momentum if exact else float(np.float32(1.0) - np.float32(momentum))
    new_mean = om * np.asarray(run_mean, np.float64) + mom * np.asarray(mean, np.float64)
    new_var = om * np.asarray(run_var, np.float64) + mom * np.asarray(r32(unb), np.float64)
    return mean, invstd, new_mean, new_var


def pre_activation(x, res, gamma, beta, mean, invstd):
    """-> (x γ is + β - μ γ is (+ res), Σ of the magnitudes of those terms), float64"""
    x = _f64(x)
    g, b = _gamma_beta(gamma, beta, mean)
    sc = _ch(g, x) * _ch(invstd, x)
    a, m, bb = x * sc, _ch(mean, x) * sc, _ch(b, x)
    pre, mag = a + bb - m, abs(a) + abs(m) + abs(bb)
    if res is not None:
        r = _f64(res)
        pre, mag = pre + r, mag + abs(r)
    return pre, mag


def apply(x, res, gamma, beta, mean, invstd, relu):
    """-> (y float64, open set = pre-activation > 0)"""
    pre, _ = pre_activation(x, res, gamma, beta, mean, invstd)
    open_ = pre > 0
    return (pre * open_ if relu else pre), open_


def bwd_apply(dy, open_, x, gamma, mean, invstd, sums, count):
    """-> (dx f64, dres f64, dgamma f32, dbeta f32) from the GIVEN sums (Σg, Σ g·x̂)"""
    g = _f64(dy) if open_ is None else _f64(dy) * _f64(open_)
    gm, _ = _gamma_beta(gamma, None, mean)
    s1, s2 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    k0 = _ch(gm, g) * _ch(invstd, g)
    dx = k0 * (g - _ch(s1 / count, g) - xhat(x, mean, invstd) * _ch(s2 / count, g))
    return dx, g, s2.astype(np.float32), s1.astype(np.float32)


# ------------------------------------------------------------------------------------------------ bounds
def nhwc_nblk(M, C):
    rpp = 256 // (C // 8)
    return int(min(max(-(-M // (16 * rpp)), 1), MAXBLK))


def chain_nhwc(M, C):
    rpp = 256 // (C // 8)
    return -(-M // (nhwc_nblk(M, C) * rpp)) + UNR_PART + rpp


def chain_nchw(HW, vec):
    """vec: elements per vector load on the vector path (8 for 16-bit, 4 for fp32), 1 on the scalar path"""
    return -(-(HW // vec) // 256) * vec if vec > 1 else -(-HW // 256)


def nchw_apply_blocks(HW, vec):
    """blocks per plane of the NCHW elementwise passes (apply_grid of bn_act.hip): one per 1024 vectors (elements on the scalar
    path, vec = 1), at most 64"""
    return int(min(max(-(-(HW // vec) // 1024), 1), 64))


def sums_bound(abs_terms, L, k):
    """(L + k) u32 Σ|term|; abs_terms: the Σ|term| per channel (or plane)"""
    return (L + k) * U32 * abs_terms


def abs_sums_fwd(x, planes=False):
    x = _f64(x)
    return _rsum(abs(x), x.ndim, planes), _rsum(x * x, x.ndim, planes)


def abs_sums_bwd(dy, open_, x, mean, invstd, planes=False):
    g = abs(_f64(dy)) if open_ is None else abs(_f64(dy)) * _f64(open_)
    return _rsum(g, g.ndim, planes), _rsum(g * abs(xhat(x, mean, invstd)), g.ndim, planes)


def prep_bounds(sums, count, momentum, eps, run_mean=None, run_var=None):
    """-> bounds (mean, invstd, running mean, running var) of the values prep returns for the same sums"""
    s1, s2 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    mean, invstd, rm, rv = prep(sums, count, momentum, eps, run_mean, run_var)
    m = s1 / float(count)
    var = np.maximum(s2 / float(count) - m * m, 0.0)
    e = float(np.float32(eps))
    b_mean = 4 * U32 * np.abs(m)
    b_is = (4 * U32 + 2.0 ** -40 * (s2 / float(count)) / (var + e)) * np.abs(invstd.astype(np.float64))
    if run_mean is None:
        return b_mean, b_is, None, None
    return b_mean, b_is, 4 * U32 * np.abs(rm), 4 * U32 * np.abs(rv)


def y_bound(want, mag, fmt):
    """want, mag: what apply / pre_activation return for the device's own save_mean / save_invstd"""
    return U16[fmt] * abs(want) + 4 * U32 * mag + (2.0 ** -25 if fmt == "fp16" else 0.0)


def dx_bound(want, dy, open_, x, gamma, mean, invstd, sums, count, fmt):
    g = _f64(dy) if open_ is None else _f64(dy) * _f64(open_)
    gm, _ = _gamma_beta(gamma, None, mean)
    s1, s2 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    k0 = abs(_ch(gm, g) * _ch(invstd, g))
    mag = abs(g) + abs(_ch(s1 / count, g)) + abs(xhat(x, mean, invstd) * _ch(s2 / count, g))
    return U16[fmt] * abs(want) + 6 * U32 * k0 * mag + (2.0 ** -25 if fmt == "fp16" else 0.0)


# ------------------------------------------------------------------------------------------------ input condition
def near_zero_mask(x, res, gamma, beta, mean, invstd):
    """elements whose pre-activation lies within 2^-20 of the magnitude of its terms of zero: there an fp32 evaluation (gate 2
    recomputes the gate from x) may take the other side than float64"""
    pre, mag = pre_activation(x, res, gamma, beta, mean, invstd)
    return abs(pre) <= MARGIN * mag


def near_zero_count(x, res, gamma, beta, mean, invstd):
    return int(near_zero_mask(x, res, gamma, beta, mean, invstd).sum())


SAFE_X = 0.0


def make_safe(x, res, gamma, beta, momentum_eps_count, fmt):
    """replace the offending elements of x by SAFE_X (a value of every storage type) until the batch statistics of the
    replaced x leave none; -> (x, mean f32, invstd f32, sums).  Raises if three rounds do not get there."""
    eps, count = momentum_eps_count
    x = np.array(x, np.float32)
    for _ in range(3):
        sums = sums_fwd(x)
        mean, invstd, _, _ = prep(sums, count, 0.0, eps)
        bad = near_zero_mask(x, res, gamma, beta, mean, invstd)
        if not bad.any():
            return x, mean, invstd, sums
        x[bad] = SAFE_X
    raise AssertionError("inputs keep a pre-activation inside the 2^-20 margin")


# ------------------------------------------------------------------------------------------------ the kernels' order
def nhwc_sums_f32_order(t1, t2, C):
    """float32 restatement of bnh_partial_kernel + bnh_finalize_kernel for terms t1, t2 [M][C] (float64 arrays holding the exact
    term, e.g. x and x·x): per thread an fp32 chain over its rows in ascending order (every addition rounds once, as s += v and
    fmaf(v, v, s) do), an fp32 fold of the RPP chains of a channel group in ascending order, then double over the blocks."""
    M = t1.shape[0]
    rpp = 256 // (C // 8)
    nblk = nhwc_nblk(M, C)
    chunk = rpp * UNR_PART
    step = nblk * chunk
    b = np.arange(nblk)[:, None]
    j = np.arange(rpp)[None, :]
    cols = t1.shape[1]                  # may be fewer than C (a subset of the channels): the order depends on the row only
    acc = [np.zeros((nblk, rpp, cols), np.float32) for _ in range(2)]
    for p in range(UNR_PART * -(-M // step)):
        r = b * chunk + j + rpp * (p % UNR_PART) + step * (p // UNR_PART)
        ok = (r < M)[:, :, None]
        rc = np.minimum(r, M - 1)
        for a, t in zip(acc, (t1, t2)):
            a[...] = np.where(ok, (a.astype(np.float64) + t[rc]).astype(np.float32), a)
    out = []
    for a in acc:
        fold = np.zeros((nblk, cols), np.float32)
        for q in range(rpp):
            fold = fold + a[:, q, :]
        out.append(fold.astype(np.float64).sum(axis=0))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ shared inputs
NHWC_SHAPES = [(1, 8), (1, 2048), (255, 8), (2049, 8), (37, 16), (100, 32), (513, 64), (300, 128), (1000, 256), (700, 512),
               (3100, 1024), (4099, 2048)]
EPS, MOMENTUM = 1e-5, 0.1


def nhwc_inputs(M, C, fmt, seed=0, mean=0.3, sigma=2.0):
    """one input set of the channels-last tests: x, res, dy (rounded to fmt), gamma, beta, a y for gate 1 and a random bit mask
    for gate 3 that open the SAME set, and the statistics of x after the margin replacement (made without and with res; the
    callers assert near_zero_count == 0 for both before any launch).  Every call returns arrays of its own; only the small
    sets (up to 2^18 elements) are kept between calls, so the 8-million-element ones are freed with the test that drew them."""
    if M * C > 1 << 18:
        return _nhwc_inputs(M, C, fmt, seed, mean, sigma)
    d = _nhwc_inputs_kept(M, C, fmt, seed, mean, sigma)
    return {k: tuple(a.copy() for a in v) if isinstance(v, tuple) else v.copy() if isinstance(v, np.ndarray) else v
            for k, v in d.items()}


def _nhwc_inputs(M, C, fmt, seed, mean, sigma):
    g = synth.rng(100000 * seed + 7 * M + C + (1 if fmt == "fp16" else 0))
    x = round16(g.standard_normal((M, C)) * sigma + mean, fmt)
    res = round16(g.standard_normal((M, C)), fmt)
    dy = round16(g.standard_normal((M, C)), fmt)
    gamma = (1.0 + 0.5 * g.standard_normal(C)).astype(np.float32)
    beta = 0.5 * g.standard_normal(C)
    beta = (np.sign(beta) * (np.abs(beta) + 2.0 ** -6)).astype(np.float32)      # away from 0: with M = 1 the pre-activation IS beta
    bits = g.integers(0, 256, size=(M, C // 8), dtype=np.uint8)
    open3 = np.unpackbits(bits[:, :, None], axis=2, bitorder="little").reshape(M, C).astype(bool)
    ychosen = round16(np.where(open3, np.abs(g.standard_normal((M, C))) + 2.0 ** -10, -np.abs(g.standard_normal((M, C)))), fmt)
    ychosen[~open3 & (g.random((M, C)) < 0.25)] = 0.0          # closed by an exact zero, not only by a negative value
    count = float(M)
    for rs in (None, res):
        x, mu, istd, sums = make_safe(x, rs, gamma, beta, (EPS, count), fmt)
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, bits=bits, open3=open3, ychosen=ychosen, mean=mu, invstd=istd,
                sums=sums, count=count)


_nhwc_inputs_kept = functools.lru_cache(maxsize=8)(_nhwc_inputs)
