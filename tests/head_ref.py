"""float64 references and per-element error bounds of the head kernels (aspp.hip, aspp2.hip, upsample.hip); no GPU needed.

REFERENCE.  ASPP: y = Σ_i conv2d(x, W_i, b_i, dilation = padding = dil_i) as four torch.nn.functional.conv2d calls in float64
on the CPU, autograd for dx, dW_i, db.  For the 16-bit paths the reference takes the operands the kernel multiplies
(`round16` of bn_ref.py on x and dy, `rounded_weights`).  Upsample backward: the adjoint accumulated in double (oracle/cref.py).

BOUNDS.  Every bound is c·u·S per element, S the same convolution on absolute values (`magnitudes`: the Σ|term| of that very
element), u = 2^-24 (fp32 accumulation), c from the number of terms and the reduction tree, written as γ(c) = c u / (1 - c u)
(Higham, Accuracy and Stability of Numerical Algorithms, §3.1: ANY order of summing n terms whose products are rounded once, or
n + 1 terms with fused multiply-adds, errs by at most γ(n) Σ|term|; a tree of partial sums adds the depth of the tree).  None of
the constants comes from a GPU run.

direct form (aspp.hip)
  y     one accumulator per (split, pixel, channel) over 33 taps x Cin / splitK channels, then splitK - 1 additions of the
        partials and 1 of the bias; the centre weight ((w0 + w1) + w2) + w3 and the bias ((b0 + b1) + b2) + b3 are summed in fp32
        first (3 roundings each, on |w_i| resp. |b_i|, which S contains):            c = 33 Cin / splitK + (splitK - 1) + 1 + 3
  dx    one accumulator over 33 taps x Cout channels, the same pre-summed centre weight:                  c = 33 Cout + 3
  dW    per pixel split one accumulator over at most `per` 16-pixel steps (per = ceil(B h ceil(w / 16) / nsplit)), then
        nsplit additions (the reduce starts from 0):                                                   c = 16 per + nsplit
  db    summed in double, rounded once:                                    u |db| + (B h w) 2^-53 Σ|dy|
GEMM + shift-add form (aspp2.hip); a product of two bf16 (8 + 8 bits) or two fp16 (11 + 11 bits) values is exact in fp32
  y     T = Σ over Cin channels in fp32 (any order on the matrix cores), then bias + 33 taps in ascending order; bias pre-summed
        (3 roundings):                                                                                  c = Cin + 33 + 3
        fp16 rows: T is stored as fp16, so each tap product carries 2^-11 |T_tap| (1 + γ(Cin)) + 2^-25 (the smallest fp16 step,
        for a subnormal T); |T_tap| is bounded by the float64 |T_tap| + γ(Cin) S_tap: `tap_magnitudes`.
        fp32 rows / split planes: x = xh + xl + ex with xh = bf16(x), xl = bf16(x - xh), |xl| <= 2^-8 |x| (1 + 2^-8),
        |ex| <= 2^-16 |x|, the same for w.  The kernel adds xh wh + xl wh + xh wl (3 Cin terms): dropped are xl wl
        (<= 2^-16 (1 + 2^-8)^2 |x w|), ex w and x ew (<= 2^-16 |x w| each) and ex ew (2^-32):  3 · 2^-16 (1 + 2^-6) S on top of
        c = 3 Cin + 33 + 3 + 3 (the fp32 centre-weight sum is part of these paths, their reference takes the fp32 weights)
  dx    Σ over 33 Cout gathered values in fp32, then rounded to the 16-bit type: E = γ(33 Cout) S, bound = E + u16 (|ref| + E)
        (+ 2^-25 for a subnormal fp16 result)
  dW    per pixel split at most mps rows (mps = ceil(M / nsplit) rounded up to 32), then nsplit additions:  c = mps + nsplit
upsample backward
  gin   a row of nX = Xb - Xa fused multiply-adds, nY = Yb - Ya rows, the weights wy / wx themselves sums of at most two fp32
        lerp weights (1 rounding each):  c = nX + nY + 2, on S = the same adjoint of |gout|; + u |ref| for the float32 the
        reference is returned in."""
import numpy as np
import torch

import synth
from bn_ref import U16, U32, round16
from head_calls import aspp_splitk, aspp_wgrad_nsplit

F = torch.nn.functional


def gamma(n, u=U32):
    assert n * u < 0.5
    return n * u / (1.0 - n * u)


# ------------------------------------------------------------------------------------------------ inputs, operands
def aspp_inputs(seed, B, Cin, h, w, Cout):
    """x, four weights, four biases, dy (float32 numpy); the scales of tests/test_gpu_kernels.py"""
    x = synth.normal_f32(seed, (B, Cin, h, w), 1.0)
    ws = [synth.normal_f32(seed + 1 + i, (Cout, Cin, 3, 3), 0.05) for i in range(4)]
    bs = [synth.normal_f32(seed + 11 + i, (Cout,), 0.1) for i in range(4)]
    gy = synth.normal_f32(seed + 21, (B, Cout, h, w), 1.0)
    return x, ws, bs, gy


def centre_sum(ws):
    return ((ws[0][:, :, 1, 1] + ws[1][:, :, 1, 1]) + ws[2][:, :, 1, 1]) + ws[3][:, :, 1, 1]           # fp32, ascending


def rounded_weights(ws, fmt):
    """what the 16-bit GEMM multiplies with: every tap rounded to fmt, the four centre taps summed in fp32 (ascending) first;
    expressed as four convolution weights again (the centre in the first, zero in the others)"""
    out = [round16(w, fmt).copy() for w in ws]
    out[0][:, :, 1, 1] = round16(centre_sum(ws), fmt)
    for i in (1, 2, 3):
        out[i][:, :, 1, 1] = 0.0
    return out


def split_hi_lo(a):
    hi = round16(a, "bf16")
    return hi, round16(np.asarray(a, np.float32) - hi, "bf16")


# ------------------------------------------------------------------------------------------------ float64 reference
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _conv_sum(x, ws, bs, dil):
    return sum(F.conv2d(x, ws[i], None if bs is None else bs[i], 1, dil[i], dil[i]) for i in range(4))


def reference(x, ws, bs, dil, gy=None, absolute=False):
    """-> dict(y) and, with gy, dx, dw (list of 4), db; float64 numpy.  absolute=True: the same on |x|, |w|, |b|, |gy| — the
    Σ|term| of every element (db then is Σ|dy|)"""
    f = (lambda a: _t(a).abs()) if absolute else _t
    xt = f(x).requires_grad_(gy is not None)
    wt = [f(v).requires_grad_(gy is not None) for v in ws]
    bt = [f(v).requires_grad_(gy is not None) for v in bs]
    y = _conv_sum(xt, wt, bt, dil)
    out = dict(y=y.detach().numpy())
    if gy is not None:
        y.backward(f(gy))
        out.update(dx=xt.grad.numpy(), dw=[v.grad.numpy() for v in wt], db=bt[0].grad.numpy())
    return out


def magnitudes(x, ws, bs, dil, gy=None):
    return reference(x, ws, bs, dil, gy, absolute=True)


def taps_of(dil):
    """the 33 taps in the kernels' order: the shared centre, then per dilation the 8 ring taps row by row -> [(oy, ox)]"""
    return [(0, 0)] + [((ky - 1) * d, (kx - 1) * d) for d in dil for ky in range(3) for kx in range(3) if (ky, kx) != (1, 1)]


def pack_taps(ws, centre=None):
    """[33][Cout][Cin] in the order of taps_of; the centre pre-summed in fp32 unless given"""
    out = [centre_sum(ws) if centre is None else centre]
    for d in range(4):
        out += [ws[d][:, :, ky, kx] for ky in range(3) for kx in range(3) if (ky, kx) != (1, 1)]
    return np.stack(out)


def shifted(a, oy, ox, wrap=False):
    """b[..., y, x] = a[..., y + oy, x + ox], zero outside the image (wrap=True: read from the opposite side instead)"""
    if wrap:
        return np.roll(a, (-oy, -ox), axis=(-2, -1))
    h, w = a.shape[-2:]
    b = np.zeros_like(a)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[..., y0:y1, x0:x1] = a[..., y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return b


def tap_magnitudes(x, ws, dil):
    """(Σ_tap |T_tap|, Σ_tap Σ_ci |x w|) per output element in float64, T_tap the float64 tap product the shift-add reads:
    what the fp16 rounding of T scales with"""
    Wp = pack_taps([np.asarray(v, np.float64) for v in ws], centre=np.asarray(ws[0][:, :, 1, 1], np.float64))
    x = np.asarray(x, np.float64)
    tsum = np.zeros((x.shape[0], Wp.shape[1]) + x.shape[2:])
    ssum = np.zeros_like(tsum)
    for t, (oy, ox) in enumerate(taps_of(dil)):
        tsum += np.abs(shifted(np.einsum("bchw,oc->bohw", x, Wp[t]), oy, ox))
        ssum += shifted(np.einsum("bchw,oc->bohw", np.abs(x), np.abs(Wp[t])), oy, ox)
    return tsum, ssum


# ------------------------------------------------------------------------------------------------ bounds
def fwd_bound(S, B, Cin, h, w, Cout):
    k = aspp_splitk(B, Cin, h, w, Cout)
    return gamma(33 * Cin // k + (k - 1) + 1 + 3) * S


def bwd_data_bound(S, Cout):
    return gamma(33 * Cout + 3) * S


def bwd_weight_bound(S, B, h, w):
    n = aspp_wgrad_nsplit(B, h, w)
    per = -(-(B * h * ((w + 15) // 16)) // n)
    return gamma(16 * per + n) * S


def db_bound(ref, gy):
    gy = np.asarray(gy, np.float64)
    return U32 * np.abs(ref) + gy[:, 0].size * 2.0 ** -53 * np.abs(gy).sum((0, 2, 3))


SPLIT_TERM = 3 * 2.0 ** -16 * (1 + 2.0 ** -6)


def fwd2_bound(S, Cin, kind, taps=None):
    """kind: "fp32" (fp32 rows and split planes), "bf16", "fp16" (taps = tap_magnitudes(...) of the fp16 operands)"""
    if kind == "fp32":
        return (gamma(3 * Cin + 33 + 3 + 3) + SPLIT_TERM) * S
    b = gamma(Cin + 33 + 3) * S
    if kind == "fp16":
        tsum, ssum = taps
        b = b + U16["fp16"] * (1 + gamma(Cin)) * (tsum + gamma(Cin) * ssum) + 33 * 2.0 ** -25
    return b


def dx2_bound(ref, S, Cout, fmt):
    E = gamma(33 * Cout) * S
    return E + U16[fmt] * (np.abs(ref) + E) + (2.0 ** -25 if fmt == "fp16" else 0.0)


def wgrad2_nsplit(M):
    s = 16
    while s > 1 and M // s < 1024:
        s >>= 1
    return s


def wgrad2_rows(M):
    """rows of one pixel split of the aspp2 weight gradient"""
    return -(-(-(-M // wgrad2_nsplit(M))) // 32) * 32


def dw2_bound(S, M):
    return gamma(wgrad2_rows(M) + wgrad2_nsplit(M)) * S


def upsample_terms(h, w, H, W):
    """an upper limit of the rows / columns of the gather band of one low-res cell: the output rows whose source row floor is
    j - 1 or j, at most 2 ceil((H - 1) / (h - 1)) + 2 of them (all H when h = 1)"""
    nY = H if h == 1 else min(H, 2 * (-(-(H - 1) // (h - 1))) + 2)
    nX = W if w == 1 else min(W, 2 * (-(-(W - 1) // (w - 1))) + 2)
    return nY, nX


def upsample_bwd_bound(ref, S, h, w, H, W):
    nY, nX = upsample_terms(h, w, H, W)
    return gamma(nX + nY + 2) * np.asarray(S, np.float64) + U32 * np.abs(np.asarray(ref, np.float64))


# ------------------------------------------------------------------------------------------------ the kernels' order in float32
# mut = (kind, tap): "drop" leaves the tap out, "flip" negates it, "wrap" reads it from the opposite side of the image instead of
# the zero padding — the deliberate errors the bounds must expose
def _mut(mut, t):
    if mut is None or mut[1] != t:
        return 1.0, False
    return {"drop": 0.0, "flip": -1.0, "wrap": 1.0}[mut[0]], mut[0] == "wrap"


def _bias_sum(bs):
    return ((bs[0] + bs[1]) + bs[2]) + bs[3]


def aspp_fwd_f32(x, ws, bs, dil, splitk, mut=None, chunk=64):
    """aspp_fwd16_kernel / aspp_fwd_kernel: per split one fp32 accumulator, 64-channel chunk outer, tap inner, channels
    ascending; partials added in ascending order, the bias last"""
    f = np.float32
    B, Cin, h, w = x.shape
    Wp = pack_taps(ws)
    cps = Cin // splitk
    parts = []
    for s in range(splitk):
        acc = np.zeros((B, Wp.shape[1], h, w), f)
        for c0 in range(s * cps, (s + 1) * cps, chunk):
            for t, (oy, ox) in enumerate(taps_of(dil)):
                sg, wrap = _mut(mut, t)
                if sg == 0.0:
                    continue
                xs = shifted(x[:, c0:c0 + chunk], oy, ox, wrap)
                for ci in range(chunk):
                    acc = acc + (f(sg) * Wp[t][:, c0 + ci])[None, :, None, None] * xs[:, ci][:, None]
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc + _bias_sum(bs)[None, :, None, None]


def aspp_bwd_data_f32(gy, ws, dil, mut=None):
    """aspp_bwd_data_kernel: tap outer, output channel inner, one fp32 accumulator"""
    f = np.float32
    Wp = pack_taps(ws)
    B, Cout, h, w = gy.shape
    acc = np.zeros((B, Wp.shape[2], h, w), f)
    for t, (oy, ox) in enumerate(taps_of(dil)):
        sg, wrap = _mut(mut, t)
        if sg == 0.0:
            continue
        gs = shifted(gy, -oy, -ox, wrap)
        for co in range(Cout):
            acc = acc + (f(sg) * Wp[t][co])[None, :, None, None] * gs[:, co][:, None]
    return acc


def _unpack_dw(P, Cout, Cin):
    """[33][Cout][Cin] -> four [Cout][Cin][3][3]; every branch's centre is tap 0"""
    dws = [np.zeros((Cout, Cin, 3, 3), P.dtype) for _ in range(4)]
    t = 1
    for d in range(4):
        dws[d][:, :, 1, 1] = P[0]
        for ky in range(3):
            for kx in range(3):
                if (ky, kx) != (1, 1):
                    dws[d][:, :, ky, kx] = P[t]
                    t += 1
    return dws


def _pixel_sum_f32(A, Bm, nsplit, rows):
    """Σ_q A[q][.., None] Bm[q][None, ..] in fp32, q ascending inside each of nsplit ranges of `rows` rows, the partial sums
    added in ascending order starting from 0"""
    f = np.float32
    total = np.zeros(A.shape[1:] + Bm.shape[1:], f)
    for s in range(nsplit):
        acc = np.zeros_like(total)
        for q in range(s * rows, min((s + 1) * rows, A.shape[0])):
            acc = acc + A[q].reshape(A.shape[1:] + (1,) * (Bm.ndim - 1)) * Bm[q]
        total = total + acc
    return total


def aspp_bwd_weight_f32(x, gy, dil, mut=None):
    """aspp_bwd_weight_kernel + aspp_wgrad_reduce_kernel: per tap and pixel split one fp32 accumulator over the pixels in raster
    order (splits of whole 16-pixel steps; a row's last step may be short), partials added from 0 in ascending order"""
    B, Cin, h, w = x.shape
    Cout = gy.shape[1]
    spr = (w + 15) // 16
    nsplit = aspp_wgrad_nsplit(B, h, w)
    per = -(-(B * h * spr) // nsplit)
    # pixels in step order; a step past the row end holds no pixel
    order = [[(n, y, c) for u in range(s * per, min((s + 1) * per, B * h * spr))
              for n, y, st in [(u // (spr * h), (u // spr) % h, u % spr)] for c in range(st * 16, min(st * 16 + 16, w))]
             for s in range(nsplit)]
    xs = []
    for t, (oy, ox) in enumerate(taps_of(dil)):
        sg, wrap = _mut(mut, t)
        xs.append(np.float32(sg) * shifted(x, oy, ox, wrap))
    xs = np.stack(xs)                                                   # [33][B][Cin][h][w]
    total = np.zeros((33, Cout, Cin), np.float32)
    for pix in order:
        acc = np.zeros_like(total)
        for n, y, c in pix:
            acc = acc + gy[n, :, y, c][None, :, None] * xs[:, n, :, y, c][:, None, :]
        total = total + acc
    return _unpack_dw(total, Cout, Cin)


def aspp2_fwd_f32(xops, wops, bs, dil, t16=False, mut=None):
    """hiast_aspp2_fwd: T[q][tap][co] over the channels in fp32 (xops / wops: one [B,Cin,h,w] / [33,Cout,Cin] operand each for
    16-bit rows; (hi, lo) pairs for the split forms: hi hi + lo hi + hi lo per channel), optionally rounded to fp16, then
    bias + the 33 taps in ascending order"""
    f = np.float32
    pairs = [(0, 0)] if len(xops) == 1 else [(0, 0), (1, 0), (0, 1)]
    B, Cin, h, w = xops[0].shape
    Cout = wops[0].shape[1]
    T = np.zeros((33, B, Cout, h, w), f)
    for ci in range(Cin):
        for a, b in pairs:
            T = T + wops[b][:, None, :, ci, None, None] * xops[a][None, :, ci, None]
    if t16:
        T = round16(T, "fp16")
    y = np.broadcast_to(_bias_sum(bs)[None, :, None, None], T.shape[1:]).astype(f)
    for t, (oy, ox) in enumerate(taps_of(dil)):
        sg, wrap = _mut(mut, t)
        if sg != 0.0:
            y = y + f(sg) * shifted(T[t], oy, ox, wrap)
    return y


def aspp2_gather(gy16, dil, mut=None):
    """G[tap][B][Cout][h][w] = dY[q - off(tap)]"""
    out = []
    for t, (oy, ox) in enumerate(taps_of(dil)):
        sg, wrap = _mut(mut, t)
        out.append(np.float32(sg) * shifted(gy16, -oy, -ox, wrap))
    return np.stack(out)


def aspp2_bwd_dx_f32(gy16, w16, dil, fmt, mut=None):
    """dX[q][ci] = Σ_n G[q][n] W[n][ci], n = tap * Cout + co ascending in fp32, rounded to fmt"""
    G = aspp2_gather(gy16, dil, mut)
    Wp = pack_taps(w16, centre=w16[0][:, :, 1, 1])
    B, Cout, h, w = gy16.shape
    acc = np.zeros((B, Wp.shape[2], h, w), np.float32)
    for t in range(33):
        for co in range(Cout):
            acc = acc + Wp[t][co][None, :, None, None] * G[t][:, co][:, None]
    return round16(acc, fmt)


def aspp2_bwd_dw_f32(x16, gy16, dil, mut=None):
    """dWt[n][ci] = Σ_q G[q][n] X[q][ci] over pixel splits (gemm_tn_bf16_kernel + aspp2_wgrad_unpack_kernel)"""
    G = aspp2_gather(gy16, dil, mut)
    B, Cin, h, w = x16.shape
    Cout = gy16.shape[1]
    M = B * h * w
    A = np.ascontiguousarray(G.transpose(1, 3, 4, 0, 2)).reshape(M, 33, Cout)
    X = np.ascontiguousarray(x16.transpose(0, 2, 3, 1)).reshape(M, Cin)
    return _unpack_dw(_pixel_sum_f32(A, X, wgrad2_nsplit(M), wgrad2_rows(M)), Cout, Cin)


# ------------------------------------------------------------------------------------------------ upsample backward
def lerp_matrix(n_in, n_out):
    """[n_out][n_in] float32: the align_corners weights as the kernels form them (src_of of common.h): f = scale · dst in fp32,
    i0 = min(int(f), n_in - 1), l1 = f - i0, l0 = 1 - l1; a cell that is both i0 and i1 gets l0 + l1"""
    f32 = np.float32
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    m = np.zeros((n_out, n_in), f32)
    for d in range(n_out):
        f = f32(scale * f32(d))
        a = min(int(f), n_in - 1)
        l1 = f32(f - f32(a))
        m[d, a] = f32(m[d, a] + f32(f32(1) - l1))
        i1 = a + (1 if a < n_in - 1 else 0)
        m[d, i1] = f32(m[d, i1] + l1)
    return m


def upsample_bwd_f32(gout, h, w, drop_row=None):
    """upsample_bwd_kernel: per low-res cell, rows ascending, inside a row the columns ascending, all in fp32 (terms with a zero
    weight add an exact 0, so the whole row / column range gives the sums of the gather band)"""
    B, C, H, W = gout.shape
    wy, wx = lerp_matrix(h, H), lerp_matrix(w, W)
    acc = np.zeros((B, C, h, w), np.float32)
    for Y in range(H):
        if Y == drop_row:
            continue
        row = np.zeros((B, C, w), np.float32)
        for X in range(W):
            row = row + gout[:, :, Y, X, None] * wx[X][None, None, :]
        acc = acc + row[:, :, None, :] * wy[Y][None, None, :, None]
    return acc


def upsample_bwd_f64(gout, h, w):
    B, C, H, W = gout.shape
    wy, wx = lerp_matrix(h, H).astype(np.float64), lerp_matrix(w, W).astype(np.float64)
    return np.einsum("bcyx,yj,xi->bcji", np.asarray(gout, np.float64), wy, wx)
