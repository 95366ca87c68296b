"""float64 references and per-element error bounds of the fused self-training loss (st_loss.hip) and of the discriminator input
map (dinput.hip); no GPU needed.  TEST INFRASTRUCTURE ONLY.

TRUTH.  The bilinear weights are the float32 ones of src_of (common.h) promoted to float64 (`src_of`, `lerp_matrix64`; the weight
of a clamped cell is l0 + l1 in float64, where head_ref.lerp_matrix rounds that sum to float32 once more); everything after the
weights is float64: the upsampled logits, log-softmax, the four consistency kinds (CE with its [B,B,H,W] broadcast count M, KLDIV
with its double softmax, MSE on the raw logits), the three regions, and the gradient of Σ coef_i s_i / denominator_i with respect
to the low-res logits through the exact adjoint of the same weights.

BOUNDS, first order in u = 2^-24, per element, from the arithmetic as written in the kernels (γ(n) = n u / (1 - n u)):
  z      an upsampled logit: lerp_h then lerp_v, fl(l0 a) + one fmaf each = 4 roundings on the longest path:
         dz = γ(4) · (the same interpolation of |z_lr|)
  exp    e_c = __expf(fl(z_c - max)): relative  ρ_c = u |d_c| + ε_exp(d_c),  ε_exp(x) = (EXP_A |x| + EXP_B) u  (below)
  lse    S = Σ e_c ascending (C - 1 additions), lse = fl(max + __logf(S)):
         arithmetic part  lse_ar = Σ p_c ρ_c + (C - 1) u + LOG_C u + u |lse|;  input part  Σ p_c dz_c
  logp   fl(z_c - lse):  E_logp_c = dz_c + Σ p_k dz_k + lse_ar + u |logp_c|;   p_c = __expf(logp_c):  E_p_c = p_c (E_logp_c + ε_exp(logp_c))
  s0     lse - z_y:            Σ_c |p_c - [c = y]| dz_c + lse_ar + u |t|
  s1     (C lse - Σ z) / C:    Σ_c |p_c - 1/C| dz_c + lse_ar + u |lse| + ((C - 1) u Σ|z_c| + u |C lse - Σ z|) / C + 2 u |t|
  s2     H = -Σ p_c logp_c:    Σ_k p_k |logp_k + H| dz_k + Σ_c p_c |logp_c + 1| (lse_ar + u |logp_c|) + Σ_c p_c |logp_c| ε_exp(logp_c)
                               + (C + 1) u Σ_c p_c |logp_c|
  q1     teacher_prob = fl(__expf(fl(zt_c - mt)) · fl(1 / St)):  E_q1_c = q1_c (ρt_c + Σ q1_k ρt_k + (C - 1) u + 2 u + dt_c + Σ q1_k dt_k)
  s3     SoftCE  -logp_c q1_c:         |logp_c| E_q1_c + q1_c E_logp_c + u |prod|
         CE      M (lse - z_yt):       M (Σ_c |p_c - [c = yt]| dz_c + lse_ar + u |l|) + u |l M|
         KLDIV   q_c ((q1_c - log S2) - logp_c), S2 = Σ __expf(q1_c), q_c = fl(__expf(q1_c) · fl(1 / S2)):
                 ρ2 = Σ q_c (E_q1_c + ε_exp(q1_c)) + (C - 1) u;  ρq_c = E_q1_c + ε_exp(q1_c) + ρ2 + 2 u;
                 E_T_c = E_q1_c + ρ2 + LOG_C u + u |log q_c| + E_logp_c + u |T_c|;   q_c (ρq_c |T_c| + E_T_c) + u |prod|
         MSE     (z_c - q1_c)^2:       2 |d| (dz_c + E_q1_c + u |d|) + u d^2
         each pixel's C products are summed in fp32 first: + γ(C) Σ_c |prod_c|
  fwd    every term is accumulated in fp32 by one thread down its band of n = Y1 - Y0 rows before the switch to double:
         + γ(n) |term|;  the double tree: 2^-49 Σ|term|
  bwd    g_c of a pixel = Σ of the four terms, each A_i · (...) with A_i one float rounding of a double quotient: the element
         errors above through the formulas of the header + 3 u |term| per term + 3 u Σ|term| for the sum (`g_terms` below);
         a low-res cell then is  adjoint(E_g) + γ(rows + cols + 8) · adjoint(Σ|term|):  `rows` the fmaf chain down the longest
         band that feeds the cell's row, `cols` the fold over the columns whose x0 is i - 1 or i, 6 tile terms of the combine,
         1 for fl((1 - w1) + w1) on a clamped column, 1 to spare.  Every cell has its own bound.
dinput: the same z and softmax with expf (EXPF_B, relative) / log2f (LOG2_C, absolute), `dinput_reference`.

INTRINSICS.  hipcc for gfx950 lowers (read from the assembly of the two files, -O3 -ffp-contract=off -fno-fast-math):
  __expf(x)  v_mul_f32 by 0x3fb8aa3b (log2 e rounded, 0.22 u low) + v_exp_f32: no range reduction, no denormal scaling.  The
             product's rounding is u |x log2 e| in the exponent = u |x| relative in the result, the constant 0.22 u |x|, the
             instruction 1 ulp: ε_exp(x) = (a |x| + b) u with a <= 1.22, b <= 2 expected; results below 2^-126 are flushed
             (EXP_TINY, absolute).
  __logf(s)  v_log_f32 (with a v_ldexp_f32 scaling for denormal arguments) and the product with ln 2 in two pieces (v_mul_f32
             0x3f317217, v_fma_f32, v_fmac_f32 0x3377d1cf, v_add_f32): the error is the instruction's 1 ulp of log2 s, up to
             2^-21 ln 2 = 5.5 u for s in [16, 21), plus the last rounding.  Absolute: ε_log = LOG_C u.
  expf(x)    (dinput.hip) the product with log2 e in two pieces, v_rndne_f32, v_exp_f32 of the fraction, v_ldexp_f32: relative EXPF_B u.
  log2f(s)   (dinput.hip) v_log_f32 with the denormal scaling: absolute LOG2_C u max(|log2 s|, 1).
The constants below are TWICE the worst case a probe kernel measured against float64 on the MI355X over dense grids
(tests/test_gpu_loss_extents.py::test_intrinsic_error_constants, which fails when a measurement exceeds half a constant);
measured and chosen values are recorded in DESIGN §2.3."""
import numpy as np


f32, f64 = np.float32, np.float64
U = 2.0 ** -24
IGNORE = 255
SOFTCE, CE, KLDIV, MSE = 0, 1, 2, 3

# ε_exp(x) = (EXP_A |x| + EXP_B) u relative, __expf on [-90, 1]: measured a = 1.295 (max rel / (u |x|) over |x| >= 4), b = 2.124 (max
# rel / u over |x| <= 1).  ε_log = LOG_C u absolute, __logf on [1, 21]: measured 7.530 (the same on [1, 19]).
EXP_A, EXP_B = 2.6, 4.25
LOG_C = 15.1
# expf on [-90, 0], relative: measured 1.389 u; log2f on [1e-30, 1], absolute LOG2_C u max(|log2 s|, 1): measured 1.993
EXPF_B, LOG2_C = 2.8, 4.0
EXP_TINY = 2.0 ** -126
MIN_PROD = 1e-30


def gamma(n):
    """γ(n) = n u / (1 - n u) (Higham §3.1), elementwise"""
    n = np.asarray(n, f64)
    assert (n * U < 0.5).all()
    return n * U / (1.0 - n * U)


def eps_exp(x):
    return (EXP_A * np.abs(x) + EXP_B) * U


# ------------------------------------------------------------------------------------------------ geometry (float32, as the code)
def scale_of(n_in, n_out):
    return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)


def src_of(n_in, n_out):
    """src_of of common.h for every destination index: i0, i1 (int64), l0, l1 (float32)"""
    f = (scale_of(n_in, n_out) * np.arange(n_out, dtype=f32)).astype(f32)
    a = np.minimum(f.astype(np.int64), n_in - 1)
    l1 = (f - a.astype(f32)).astype(f32)
    return a, a + (a < n_in - 1), (f32(1) - l1).astype(f32), l1


def lerp_matrix64(n_in, n_out):
    """[n_out][n_in] float64: the float32 weights of src_of, a clamped cell (i0 == i1) holding l0 + l1 in float64"""
    i0, i1, l0, l1 = src_of(n_in, n_out)
    m = np.zeros((n_out, n_in), f64)
    d = np.arange(n_out)
    np.add.at(m, (d, i0), l0.astype(f64))
    np.add.at(m, (d, i1), l1.astype(f64))
    return m


def band_start(scale, j, n_in, n_out):
    """band_start of common.h, statement by statement"""
    if j <= 0:
        return 0
    if j > n_in - 1:
        return n_out
    if scale <= 0:
        return n_out
    Y = int(f32(j) / scale)
    Y = 0 if Y < 0 else min(Y, n_out)
    while Y > 0 and int(scale * f32(Y - 1)) >= j:
        Y -= 1
    while Y < n_out and int(scale * f32(Y)) < j:
        Y += 1
    return Y


def band_starts(n_in, n_out):
    """band_start for j = 0 .. n_in at once: the first destination index whose UNCLAMPED source index int(scale · dst) is >= j"""
    s = scale_of(n_in, n_out)
    bs = np.full(n_in + 1, n_out, np.int64)
    bs[0] = 0
    if s > 0 and n_in > 1:
        fl = (s * np.arange(n_out, dtype=f32)).astype(f32).astype(np.int64)
        assert (np.diff(fl) >= 0).all()
        bs[1:n_in] = np.searchsorted(fl, np.arange(1, n_in), side="left")
    return bs


def loss_geom(h, w, H, W):
    """loss_check's extent conditions and loss_geom of st_loss.hip in float32 -> dict(sh, sw, TI, nxb), or None when refused"""
    if H < h or W < w:
        return None
    sh, sw = scale_of(h, H), scale_of(w, W)
    TI = int(f32(253) * sw) if sw > 0 else w
    TI = min(max(TI, 1), 253, w)
    ratio = f32(1) / sw if sw > 0 else f32(W)
    if f32(f32(TI) * ratio) + f32(2) > f32(256) and not (sw == 0 and W <= 256):
        return None
    return dict(sh=sh, sw=sw, TI=TI, nxb=(w + TI - 1) // TI)


def workspace_bytes(B, C, h, w, H, W):
    g = loss_geom(h, w, H, W)
    if g is None:
        return 0
    return max(((W + 255) // 256) * h * B * 64, B * C * h * 2 * g["nxb"] * (g["TI"] + 1) * 4) + 256


def tile_blocks(w, W, TI):
    """the column ranges [Xs, Xe) of the backward's tile blocks, and the x0 of every column"""
    bs = band_starts(w, W)
    i0 = np.arange(0, w, TI)
    return bs[i0], bs[np.minimum(i0 + TI, w)], src_of(w, W)[0]


def check_tiling(w, W, TI):
    """what keeps the backward inside its 256-entry LDS arrays: every block has at most 256 columns, the blocks tile [0, W), every
    column's x0 lies in its block's cells -> the largest block"""
    Xs, Xe, x0 = tile_blocks(w, W, TI)
    assert Xs[0] == 0 and Xe[-1] == W and (Xs[1:] == Xe[:-1]).all() and (Xe >= Xs).all(), (w, W, TI)
    assert int((Xe - Xs).max()) <= 256, (w, W, TI, int((Xe - Xs).max()))
    blk = np.searchsorted(Xe, np.arange(W), side="right")
    assert (blk * TI <= x0).all() and (x0 < np.minimum((blk + 1) * TI, w)).all(), (w, W, TI)
    return int((Xe - Xs).max())


# ------------------------------------------------------------------------------------------------ float64 truth and bounds
class Geometry:
    """the weights of one (h, w, H, W) and what the bounds need of them"""

    def __init__(self, h, w, H, W):
        self.dims = (h, w, H, W)
        self.Wy, self.Wx = lerp_matrix64(h, H), lerp_matrix64(w, W)
        i0y, i0x = src_of(h, H)[0], src_of(w, W)[0]
        nby, nbx = np.bincount(i0y, minlength=h), np.bincount(i0x, minlength=w)
        self.band_rows = nby[i0y]                                        # rows of the band of output row Y
        self.empty_bands = int((nby == 0).sum()), int((nbx == 0).sum())
        rows = np.maximum(nby, np.concatenate([[0], nby[:-1]]))
        cols = nbx + np.concatenate([[0], nbx[:-1]])
        self.chain = (rows[:, None] + cols[None, :] + 8).astype(f64)     # [h][w]

    def up(self, x):
        return np.einsum("yj,xi,bcji->bcyx", self.Wy, self.Wx, np.asarray(x, f64), optimize=True)

    def adj(self, g):
        return np.einsum("yj,xi,bcyx->bcji", self.Wy, self.Wx, g, optimize=True)


def _ksum(a):
    return a.sum(1, keepdims=True)


def _softmax_parts(z, dz):
    """per pixel over axis 1: logp, p, lse, its arithmetic error, E_logp"""
    C = z.shape[1]
    m = z.max(1, keepdims=True)
    d = z - m
    lse = m + np.log(_ksum(np.exp(d)))
    logp = z - lse
    p = np.exp(logp)
    rho = U * np.abs(d) + eps_exp(d)
    lse_ar = _ksum(p * rho) + (C - 1) * U + LOG_C * U + U * np.abs(lse)
    E_logp = dz + _ksum(p * dz) + lse_ar + U * np.abs(logp)
    return dict(z=z, dz=dz, logp=logp, p=p, lse=lse, lse_ar=lse_ar, E_logp=E_logp, rho=rho,
                E_p=p * (E_logp + eps_exp(logp)) + EXP_TINY)


def _entropy_parts(s):
    p, logp, C = s["p"], s["logp"], s["z"].shape[1]
    Hent = -_ksum(p * logp)
    E_H = (_ksum(p * np.abs(logp + Hent) * s["dz"]) + _ksum(p * np.abs(logp + 1) * (s["lse_ar"] + U * np.abs(logp)))
           + _ksum(p * np.abs(logp) * eps_exp(logp)) + (C + 1) * U * _ksum(p * np.abs(logp)) + C * EXP_TINY * np.abs(logp).max(1, keepdims=True))
    return Hent, E_H


def _teacher_parts(t):
    """q1 = softmax(zt) as teacher_prob forms it, and its error"""
    C = t["z"].shape[1]
    q1 = t["p"]
    E_q1 = q1 * (t["rho"] + _ksum(q1 * t["rho"]) + (C - 1) * U + 2 * U + t["dz"] + _ksum(q1 * t["dz"])) + EXP_TINY
    return q1, E_q1


def _kldiv_parts(q1, E_q1):
    C = q1.shape[1]
    e2 = np.exp(q1)
    S2 = _ksum(e2)
    q = e2 / S2
    rho2 = _ksum(q * (E_q1 + eps_exp(q1))) + (C - 1) * U
    return q, q * (E_q1 + eps_exp(q1) + rho2 + 2 * U), rho2, np.log(S2)


def _onehot(idx, C):
    return (np.arange(C)[None, :, None, None] == idx[:, None]).astype(f64)


def region_mask(lbl, region):
    ign = lbl == IGNORE
    return ign if region == 0 else (~ign if region == 1 else np.ones_like(ign))


def loss_reference(geo, z_lr, zt_lr, lbl, kind, region, coef=None):
    """-> dict: sums [7] and sum_bound [4] (float64; slots 4-6 exact), min_prod (the smallest |product| slot 6 counts; the caller
    asserts it against MIN_PROD), gap_ok (CE: the arg-max condition of cst_kinds_util); with coef [4]: grad, grad_bound [B,C,h,w]
    for the denominators of this reference.  zt_lr None: no teacher (kind 0 only)."""
    B, C = z_lr.shape[:2]
    h, w, H, W = geo.dims
    lbl = np.asarray(lbl).astype(np.int64)
    assert lbl.shape == (B, H, W) and (zt_lr is not None or kind == SOFTCE)
    g4 = gamma(4)
    s = _softmax_parts(geo.up(z_lr), g4 * geo.up(np.abs(z_lr)))
    z, dz, p, logp, lse, lse_ar, E_logp = (s[k] for k in ("z", "dz", "p", "logp", "lse", "lse_ar", "E_logp"))
    ign = (lbl == IGNORE)[:, None]
    conf = ~ign
    y1h = _onehot(np.where(lbl == IGNORE, 0, lbl), C)
    Hent, E_H = _entropy_parts(s)
    chain = gamma(geo.band_rows.astype(f64))[None, None, :, None]

    t0 = -_ksum(y1h * logp)
    E0 = _ksum(np.abs(p - y1h) * dz) + lse_ar + U * np.abs(t0)
    zsum = _ksum(z)
    t1 = (C * lse - zsum) / C
    E1 = (_ksum(np.abs(p - 1.0 / C) * dz) + lse_ar + U * np.abs(lse)
          + ((C - 1) * U * _ksum(np.abs(z)) + U * np.abs(C * lse - zsum)) / C + 2 * U * np.abs(t1))
    terms = [(conf, t0, E0, np.abs(t0)), (conf, t1, E1, np.abs(t1)), (ign, Hent, E_H, _ksum(p * np.abs(logp)))]

    out = dict(gap_ok=True, min_prod=np.inf)
    n_cst = 0.0
    reg = region_mask(lbl, region)[:, None]
    if zt_lr is not None:
        t = _softmax_parts(geo.up(zt_lr), g4 * geo.up(np.abs(zt_lr)))
        q1, E_q1 = _teacher_parts(t)
        if kind == CE:
            top2 = np.sort(t["z"], axis=1)[:, -2:]
            out["gap_ok"] = bool((top2[:, 1] - top2[:, 0]).min() >= 32.0 * 2.0 ** -23 * np.abs(t["z"]).max())
            yt1h = _onehot(t["z"].argmax(1), C)
            M = reg.sum(0, keepdims=True).astype(f64)                    # [1,1,H,W]
            l = -_ksum(yt1h * logp)
            tc, Ec = l * M, M * (_ksum(np.abs(p - yt1h) * dz) + lse_ar + U * np.abs(l)) + U * np.abs(l * M)
            terms.append((np.ones_like(reg), tc, Ec, np.abs(tc)))
            out["min_prod"] = float(np.abs(l).min())
            n_cst = float((np.broadcast_to(M, l.shape) * (l != 0)).sum())
        else:
            if kind == SOFTCE:
                prod = -logp * q1
                Eprod = np.abs(logp) * E_q1 + q1 * E_logp + U * np.abs(prod)
            elif kind == KLDIV:
                q, E_q, rho2, logS2 = _kldiv_parts(q1, E_q1)
                T = (q1 - logS2) - logp
                E_T = E_q1 + rho2 + LOG_C * U + U * np.abs(q1 - logS2) + E_logp + U * np.abs(T)
                prod = q * T
                Eprod = E_q * np.abs(T) + q * E_T + U * np.abs(prod)
            else:
                d = z - q1
                prod = d * d
                Eprod = 2 * np.abs(d) * (dz + E_q1 + U * np.abs(d)) + U * prod
            mag = _ksum(np.abs(prod))
            terms.append((reg, _ksum(prod), _ksum(Eprod) + gamma(C) * mag, mag))
            if reg.any():
                out["min_prod"] = float(np.abs(prod)[np.broadcast_to(reg, prod.shape)].min())
            n_cst = float(C * reg.sum())
    sums, bound = np.zeros(7), np.zeros(4)
    for k, (msk, val, err, mag) in enumerate(terms):
        sums[k] = (val * msk).sum()
        bound[k] = ((err + chain * mag) * msk).sum() + 2.0 ** -49 * (mag * msk).sum()
    sums[4:7] = float(conf.sum()), float(ign.sum()), n_cst
    out.update(sums=sums, sum_bound=bound)
    if coef is None:
        return out

    # ---- gradient: A_i = coef_i / denominator_i (0 when coef_i == 0), the four terms per full-res element, the exact adjoint
    den = [sums[4], C * sums[4], C * sums[5], sums[6]]
    with np.errstate(divide="ignore", invalid="ignore"):
        A = [0.0 if float(c) == 0.0 else float(f64(c) / f64(d_)) for c, d_ in zip(coef, den)]
    if zt_lr is None:
        A[3] = 0.0
    out["A"] = A
    E_p = s["E_p"]
    g_terms = [(A[0], conf * (p - y1h), conf * (E_p + U * np.abs(p - y1h))),
               (A[1], conf * (p - 1.0 / C), conf * (E_p + U / C + U * np.abs(p - 1.0 / C))),
               (A[2], ign * (-p * (logp + Hent)),
                ign * (E_p * np.abs(logp + Hent) + p * (E_logp + E_H + U * np.abs(logp + Hent)) + U * np.abs(p * (logp + Hent))))]
    if zt_lr is not None:
        if kind == CE:
            g_terms.append((A[3], M * (p - yt1h), M * (E_p + U * np.abs(p - yt1h)) + U * M * np.abs(p - yt1h)))
        elif kind == MSE:
            g_terms.append((A[3], reg * 2 * (z - q1), reg * 2 * (dz + E_q1 + U * np.abs(z - q1))))
        else:
            qq, E_qq = (q1, E_q1) if kind == SOFTCE else (q, E_q)
            Q = _ksum(qq)
            E_Q = _ksum(E_qq) + (C - 1) * U * Q
            g_terms.append((A[3], reg * (p * Q - qq),
                            reg * (E_p * Q + p * E_Q + U * p * Q + E_qq + U * np.abs(p * Q - qq))))
    G, EG, SG = 0.0, 0.0, 0.0
    for a, val, err in g_terms:
        G = G + a * val
        EG = EG + abs(a) * (err + 3 * U * np.abs(val))
        SG = SG + abs(a) * np.abs(val)
    EG = EG + 3 * U * SG
    out["grad"] = geo.adj(G)
    out["grad_bound"] = geo.adj(EG) + gamma(geo.chain)[None, None] * geo.adj(SG)
    return out


# ------------------------------------------------------------------------------------------------ the kernels' order in float32
MUTANTS = ("no_seam", "no_clamped_band", "x1_unclamped", "ent_no_H", "ce_own_mask", "kld_single_softmax")


def fma32(a, b, c):
    """fmaf: the product of two float32 is exact in float64; the sum is rounded to 53 bits and then to 24"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _lerp32(a, b, l0, l1):
    return fma32(l1, b, (l0 * a).astype(f32))


def _exp32(x):
    return np.exp(x.astype(f32)).astype(f32)


def _stats32(zc):
    """max over axis 1 (first maximum), Σ exp ascending -> m, S, arg"""
    m, arg = zc[:, 0].copy(), np.zeros(zc[:, 0].shape, np.int64)
    for c in range(1, zc.shape[1]):
        up = zc[:, c] > m
        m, arg = np.where(up, zc[:, c], m), np.where(up, c, arg)
    S = np.zeros_like(m)
    for c in range(zc.shape[1]):
        S = (S + _exp32(zc[:, c] - m)).astype(f32)
    return m, S, arg


def kernel_order_f32(h, w, H, W, z_lr, zt_lr, lbl, kind, region, coef=None, sums=None, mutant=None):
    """st_loss_fwd_kernel (per-thread fp32 accumulation down a band, then double) and, with coef and sums, st_loss_bwd_kernel +
    st_loss_combine_kernel (the fmaf chain down the band, the fold over the columns of a tile block in ascending order, the tile
    layout [b][c][j][r][xb][TI + 1], the combine with its three (j, r) sources and the seam term) in float32 numpy, numpy's
    float32 exp / log standing in for the intrinsics.  mutant: one of MUTANTS.  -> (sums [7] float64, dlogits float32 or None)"""
    assert mutant is None or mutant in MUTANTS
    B, C = z_lr.shape[:2]
    lbl = np.asarray(lbl).astype(np.int64)
    g = loss_geom(h, w, H, W)
    TI, nxb = g["TI"], g["nxb"]
    teacher = zt_lr is not None
    i0x, i1x, l0x, l1x = src_of(w, W)
    i0y, _, l0y, l1y = src_of(h, H)
    bsy = band_starts(h, H)
    ign_all = lbl == IGNORE
    regm = region_mask(lbl, region)
    Mmap = regm.sum(0).astype(f32)                                       # [H,W]
    one, zero, invC = f32(1), f32(0), f32(1) / f32(C)
    bwd = coef is not None
    if bwd:
        c32 = [f32(c) for c in coef]
        den = [f64(sums[4]), f64(C) * f64(sums[4]), f64(C) * f64(sums[5]), f64(sums[6])]
        with np.errstate(divide="ignore", invalid="ignore"):
            A = [zero if c == 0 else f32(f64(c) / d_) for c, d_ in zip(c32, den)]
        if not teacher:
            A[3] = zero
        tiles = np.zeros((B, C, h, 2, nxb, TI + 1), f32)
    acc64 = np.zeros(7)

    def hband(x, y):
        return _lerp32(x[:, :, y][:, :, i0x], x[:, :, y][:, :, i1x], l0x[None, None], l1x[None, None])

    for j in range(h):
        Y0, Y1 = int(bsy[j]), int(bsy[j + 1])
        if Y0 >= Y1:
            continue
        y1 = j + (1 if j < h - 1 else 0)
        st, sb = hband(z_lr, j), hband(z_lr, y1)                         # [B,C,W]
        if teacher:
            tt, tb = hband(zt_lr, j), hband(zt_lr, y1)
        a = np.zeros((4, B, W), f32)
        n = np.zeros((3, B, W))
        gt, gb = np.zeros((B, C, W), f32), np.zeros((B, C, W), f32)
        for Y in range(Y0, Y1):
            assert i0y[Y] == j
            l0, l1 = l0y[Y], l1y[Y]
            zc = _lerp32(st, sb, l0, l1)
            y = lbl[:, Y]                                                # [B,W]
            ign = ign_all[:, Y]
            ms, Ss, _ = _stats32(zc)
            lse = (ms + np.log(Ss).astype(f32)).astype(f32)
            zy = np.take_along_axis(zc, np.where(ign, 0, y)[:, None], 1)[:, 0]
            zsum = np.zeros_like(ms)
            for c in range(C):
                zsum = (zsum + zc[:, c]).astype(f32)
            logp = (zc - lse[:, None]).astype(f32)
            pexp = _exp32(logp)
            ent = np.zeros_like(ms)
            for c in range(C):
                ent = (ent - (pexp[:, c] * logp[:, c]).astype(f32)).astype(f32)
            a[0] = np.where(ign, a[0], (a[0] + (lse - zy).astype(f32)).astype(f32))
            a[1] = np.where(ign, a[1], (a[1] + (((f32(C) * lse).astype(f32) - zsum).astype(f32) * invC).astype(f32)).astype(f32))
            a[2] = np.where(ign, (a[2] + ent).astype(f32), a[2])
            n[0] += ~ign
            n[1] += ign
            inreg = regm[:, Y] & teacher
            wM = Mmap[Y][None] * np.ones((B, 1), f32)
            if mutant == "ce_own_mask":
                wM = regm[:, Y].astype(f32)
            cs, cn = np.zeros_like(ms), np.zeros(ms.shape)
            if teacher:
                tz = _lerp32(tt, tb, l0, l1)
                mt, St, yt = _stats32(tz)
                invSt = (one / St).astype(f32)
                q1 = (_exp32(tz - mt[:, None]) * invSt[:, None]).astype(f32)
                if kind == CE:
                    zyt = np.take_along_axis(zc, yt[:, None], 1)[:, 0]
                    l = (lse - zyt).astype(f32)
                    cs, cn = (l * wM).astype(f32), np.where(l != 0, wM, 0)
                    on = wM > 0
                else:
                    if kind == KLDIV:
                        S2 = np.zeros_like(ms)
                        for c in range(C):
                            S2 = (S2 + _exp32(q1[:, c])).astype(f32)
                        invS2, logS2 = (one / S2).astype(f32), np.log(S2).astype(f32)
                        qk = (_exp32(q1) * invS2[:, None]).astype(f32)
                        if mutant == "kld_single_softmax":
                            qk, logS2 = q1, np.zeros_like(ms)
                            prods = (qk * ((np.log(np.maximum(q1, f32(1e-37))).astype(f32)) - logp).astype(f32)).astype(f32)
                        else:
                            prods = (qk * ((q1 - logS2[:, None]).astype(f32) - logp).astype(f32)).astype(f32)
                    elif kind == MSE:
                        prods = ((zc - q1).astype(f32) * (zc - q1).astype(f32)).astype(f32)
                    else:
                        prods = ((-logp) * q1).astype(f32)
                    for c in range(C):
                        cs = (cs + prods[:, c]).astype(f32)
                    cn = (prods != 0).sum(1)
                    on = inreg
                a[3] = np.where(on, (a[3] + cs).astype(f32), a[3])
                n[2] += np.where(on, cn, 0)
            if not bwd:
                continue
            Hent = np.where(ign, zero if mutant == "ent_no_H" else ent, zero).astype(f32)
            wconf, wign, wreg = (~ign).astype(f32), ign.astype(f32), inreg.astype(f32)
            Q = np.zeros_like(ms)
            if teacher and kind in (SOFTCE, KLDIV):
                qsrc = q1 if kind == SOFTCE else qk
                for c in range(C):
                    Q = (Q + qsrc[:, c]).astype(f32)
            for c in range(C):
                pc, lp = pexp[:, c], logp[:, c]
                gg = np.where(ign, zero, (A[0] * (pc - (y == c).astype(f32)).astype(f32)).astype(f32))
                gg = (gg + (A[1] * (wconf * (pc - invC).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                gg = (gg + (A[2] * (wign * ((-pc) * (lp + Hent).astype(f32)).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                if teacher:
                    if kind == CE:
                        tcst = (wM * (pc - (yt == c).astype(f32)).astype(f32)).astype(f32)
                    elif kind == MSE:
                        tcst = (wreg * (f32(2) * (zc[:, c] - np.where(inreg, q1[:, c], zero)).astype(f32)).astype(f32)).astype(f32)
                    else:
                        qc = np.where(inreg, qsrc[:, c], zero)
                        tcst = (wreg * ((pc * np.where(inreg, Q, zero)).astype(f32) - qc).astype(f32)).astype(f32)
                    gg = (gg + (A[3] * tcst).astype(f32)).astype(f32)
                gt[:, c] = fma32(l0, gg, gt[:, c])
                gb[:, c] = fma32(l1, gg, gb[:, c])
        for k in range(4):
            acc64[k] += a[k].astype(f64).sum()
        acc64[4:7] += n.sum((1, 2))
        if bwd:
            for X in range(W):
                x0 = int(i0x[X])
                xb = x0 // TI
                ii0 = x0 - xb * TI
                ii1 = ii0 + (1 if (x0 < w - 1 or mutant == "x1_unclamped") else 0)
                w1 = l1x[X]
                for r, gcol in ((0, gt[:, :, X]), (1, gb[:, :, X])):
                    if ii1 == ii0:
                        tiles[:, :, j, r, xb, ii0] = fma32(gcol, f32((one - w1) + w1), tiles[:, :, j, r, xb, ii0])
                    else:
                        tiles[:, :, j, r, xb, ii0] = fma32(gcol, f32(one - w1), tiles[:, :, j, r, xb, ii0])
                        if ii1 <= TI:
                            tiles[:, :, j, r, xb, ii1] = fma32(gcol, w1, tiles[:, :, j, r, xb, ii1])
    if not bwd:
        return acc64, None
    d = np.zeros((B, C, h, w), f32)
    i = np.arange(w)
    xbi, iii = i // TI, i % TI
    seam = (iii == 0) & (xbi > 0) & (mutant != "no_seam")
    for jj in range(h):
        acc = np.zeros((B, C, w), f32)
        srcs = [(jj, 0)] + ([(jj - 1, 1)] if jj > 0 else []) + ([(h - 1, 1)] if jj == h - 1 and mutant != "no_clamped_band" else [])
        for j, r in srcs:
            acc = (acc + tiles[:, :, j, r, xbi, iii]).astype(f32)
            acc = (acc + np.where(seam, tiles[:, :, j, r, np.maximum(xbi - 1, 0), TI], zero)).astype(f32)
        d[:, :, jj] = acc
    return acc64, d


# ------------------------------------------------------------------------------------------------ discriminator input map
def dinput_reference(geo, z_lr, mode, gout=None):
    """softmax (mode 0) or -p log2(p + 1e-30) / log2(C) (mode 1) of the upsampled logits in float64 -> out, out_bound; with gout
    [B,C,H,W]: scratch (the gradient with respect to the upsampled logits), scratch_bound, dlogits, dlogits_bound [B,C,h,w]
    (the adjoint of the scratch bound + the upsample adjoint's own bound of head_ref.py, given by the caller).
      p      m = max, e_c = expf(fl(z_c - m)) (relative u |d_c| + EXPF_B u + the input's dz), S ascending, inv = fl(1 / S),
             p_c = fl(e_c inv):  E_p_c = p_c (ρ_c + Σ p_k ρ_k + (C - 1) u + 2 u + dz_c + Σ p_k dz_k)
      mode 1 L = log2f(fl(p + 1e-30)): LOG2_C u max(|L|, 1) + (u + E_p / (p + 1e-30)) / ln 2 for the argument, invL = fl(1 / log2f(C)):
             v = -(p L) invL: E_v = (E_p |L| + p E_L) / log2 C + (3 + LOG2_C) u |v|
      bwd    t_c = g_c (mode 1: times f_c = -(L_c + fl(p_c / q_c) INV_LN2) invL, 6 roundings + E_L + the p / q part),
             dot = Σ fmaf(p_c, t_c): γ(C) Σ|p t| + Σ (E_p |t| + p E_t);  dz_c = p_c (t_c - dot):
             E_p |t_c - dot| + p_c (E_t_c + E_dot + u |t_c - dot|) + u |dz_c|"""
    C = z_lr.shape[1]
    z = geo.up(z_lr)
    dz = gamma(4) * geo.up(np.abs(z_lr))
    m = z.max(1, keepdims=True)
    d = z - m
    e = np.exp(d)
    p = e / _ksum(e)
    rho = U * np.abs(d) + EXPF_B * U
    E_p = p * (rho + _ksum(p * rho) + (C - 1) * U + 2 * U + dz + _ksum(p * dz)) + EXP_TINY
    out = {}
    L2C = np.log2(float(C))
    if mode == 0:
        out.update(out=p, out_bound=E_p + 0 * p)
    else:
        q = p + 1e-30
        L = np.log2(q)
        E_L = LOG2_C * U * np.maximum(np.abs(L), 1.0) + (U + E_p / q) / np.log(2.0)
        v = -(p * L) / L2C
        out.update(out=v, out_bound=(E_p * np.abs(L) + p * E_L) / L2C + (3 + LOG2_C) * U * np.abs(v))
    if gout is None:
        return out
    g = np.asarray(gout, f64)
    if mode == 0:
        t, E_t = g, 0 * g
    else:
        r = p / q
        f = -(L + r / np.log(2.0)) / L2C
        # d(p / q) = 1e-30 / q^2 dp: E_p 1e-30 / q^2 <= E_p / q; roundings: p + 1e-30, the quotient, the INV_LN2 product and constant,
        # the sum, invL (two: log2f(C) and the reciprocal) and its product
        E_f = (E_L + (E_p * 1e-30 / (q * q) + 3 * U * r) / np.log(2.0) + U * np.abs(L + r / np.log(2.0))) / L2C + (3 + LOG2_C) * U * np.abs(f)
        t = g * f
        E_t = np.abs(g) * E_f + U * np.abs(t)
    dot = _ksum(p * t)
    E_dot = gamma(C) * _ksum(np.abs(p * t)) + _ksum(E_p * np.abs(t) + p * E_t)
    sc = p * (t - dot)
    E_sc = E_p * np.abs(t - dot) + p * (E_t + E_dot + U * np.abs(t - dot)) + U * np.abs(sc)
    out.update(scratch=sc, scratch_bound=E_sc, dlogits=geo.adj(sc), dlogits_scratch_part=geo.adj(E_sc), scratch_abs=geo.adj(np.abs(sc)))
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by both test files
# (h, w, H, W) -> the class counts that run on it; the cases and their reasons head tests/test_gpu_loss_extents.py
GEOMETRIES = {
    (1, 1, 1, 1): (2, 9, 16, 19), (1, 1, 3, 256): (2, 9, 16, 19), (3, 2, 7, 255): (2, 9, 16, 19), (2, 9, 2, 2033): (2, 19),
    (8, 5, 24, 42): (2, 9, 16, 19), (2, 254, 2, 254): (2, 9, 16, 19), (2, 300, 2, 300): (2, 19), (4, 40, 9, 300): (2, 9, 16, 19),
    (5, 9, 33, 65): (2, 9, 16, 19), (2, 512, 2, 711): (2, 19), (512, 2, 711, 3): (2, 19),
}
# the last two: float32 s · (n_out - 1) = 511 + 2^-15 lands ABOVE n_in - 1, so the clamped last column / row carries a weight
# l1 = 2^-15 != 0 (on the first nine the clamp only redirects an exact 0)
CLAMP_GEOMETRIES = ((2, 512, 2, 711), (512, 2, 711, 3))
# the five kernel variants: (name, consistency kind, with teacher, batch: 3 where the CE kind needs its count M)
VARIANTS = (("SoftCE-no-teacher", SOFTCE, False, 1), ("SoftCE", SOFTCE, True, 1), ("CE", CE, True, 3), ("KLDIV", KLDIV, True, 1),
            ("MSE", MSE, True, 1))
COEF = (2.0, 0.3, 0.5, 0.5)


def loss_inputs(seed, B, C, h, w, H, W, p_ignore=0.4):
    """student and teacher logits (sigma 2.5, as tests/test_gpu_kernels.py) and uint8 pseudo-labels with 255 = ignored"""
    import synth
    return (synth.logits_lr(seed, B, C, h, w, 2.5), synth.logits_lr(seed + 1, B, C, h, w, 2.5),
            synth.pseudo_labels(seed + 2, B, H, W, C, p_ignore, np.uint8))


# seeds: the first of 4000 + 16 geometry + class-count index (+ 1000, + 2000, ...) whose inputs keep the CE kind's arg-max gap
# (cst_kinds_util.argmax_gap_ok) and every counted product away from 0 (MIN_PROD) in float64; both are asserted, never skipped
SEED_BUMP = {((3, 2, 7, 255), 16): 1, ((3, 2, 7, 255), 19): 1, ((2, 9, 2, 2033), 19): 1, ((5, 9, 33, 65), 19): 1}


def case_seed(geom, C):
    return 4000 + 16 * list(GEOMETRIES).index(geom) + {2: 0, 9: 1, 16: 2, 19: 3}[C] + 1000 * SEED_BUMP.get((geom, C), 0)


def usable_coef(sums, coef=COEF):
    """coef with a 0 wherever the denominator of its loss is 0: the documented rule under which the gradient stays finite"""
    den = (sums[4], sums[4], sums[5], sums[6])
    return tuple(0.0 if d == 0 else c for c, d in zip(coef, den))
