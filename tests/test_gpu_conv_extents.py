"""Where the convolution kernels touch memory: every entry of the family called through the C ABI on buffers carved out of
0xFF-filled allocations (tests/guard_bands.py).  Inputs sit in NaN poison, outputs / partial-sum buffers / workspaces start
as NaN and are sized by the library's own size functions.  After each launch:
  1. both guard bands of every buffer, inputs included, are untouched (no store left its tensor);
  2. every output payload is entirely finite (each element written, no poison read: tail rows of a partial block, weight
     rows behind N of a ragged column tile and out-of-image taps must come from the buffer range rule as zeros) — the
     workspaces are exempt from "entirely written";
  3. the values match float64 on the rounded operands (tolerances as in the rest of the suite: bf16 2^-8 |want| + 3e-5 max,
     fp16 2^-10 |want| + 3e-5 max, split planes / fp32 output 3e-5 max(1, max), weight gradients 1e-4 max|ref| against the
     float64 CPU gradient; statistics against the sums of the stored output, rtol 1e-5 / atol 1e-3);
  4. the payload is bit-equal to what the ordinary wrapper of hiast_amd.kernels returns for the same operands.
A band holds at least one full block of the kernel under test (256 rows of the tensor; one split range of a workspace).

entry                                   test
hiast_igemm_bn_act (tile kernel)        test_tile_kernel_extents (3 formats x 7 geometries x every epilogue),
                                        test_tile_kernel_ragged_column_tile (N = 640), test_tile_kernel_half_tile_forms
hiast_igemm_bn_act (xconv)              test_xconv_extents (bf16 / fp16 256 -> 1024)
hiast_igemm_bn_act (xconv2)             test_xconv2_extents (split planes 256 -> 1024 | 256)
hiast_igemm_dgrad_bn_stats              test_dgrad_bn_stats_extents
hiast_igemm_dgrad_s2                    test_dgrad_s2_extents
hiast_xconv_dgrad_gated_bn_stats        test_xconv_dgrad_gated_bn_stats_extents
hiast_conv_wgrad_nhwc                   test_conv_wgrad_extents
hiast_conv_wgrad_small_nhwc             test_conv_wgrad_small_extents
hiast_conv_wgrad_group_nhwc             test_conv_wgrad_group_extents
both, on small integers: EXACT dW       test_conv_wgrad_exact_on_small_integers
hiast_stem_train_fwd, hiast_stem_wgrad  test_stem_train_extents
size limits of all of them              test_refused_shapes_write_nothing, test_workspace_one_byte_short_is_refused
"""
import ctypes

import numpy as np
import pytest
import torch

import guard_bands as GB
import synth
from test_gpu_fp16 import _f16r
from test_gpu_kernels import _bf16r, _igemm_ref, _mk_bn, _planes_ref, dev
from test_gpu_round3 import SMALL_WGRAD

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_WS = -1, -2, -3
BF16, SPLIT, FP16 = 1, 2, 3
FMTS = {"bf16": BF16, "fp16": FP16, "split": SPLIT}
BLOCK_ROWS = 256                   # rows of the largest block tile of the family: what a band has to hold


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------------ plumbing
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(fmt):
    return torch.float16 if fmt == FP16 else torch.bfloat16


def _round(fmt, a):
    """fp32 numpy -> the values a kernel of format fmt multiplies"""
    if fmt == SPLIT:
        return sum(_planes_ref(a))
    return _f16r(a) if fmt == FP16 else _bf16r(a)


def _act(K, fmt, a):
    """rounded fp32 numpy [..., C] -> device activation of format fmt ([..., 2C] split planes)"""
    t = dev(a)
    if fmt == SPLIT:
        C = a.shape[-1]
        return K.split_planes(t.view(-1, C)).view(*a.shape[:-1], 2 * C)
    return t.to(_dt(fmt))


def _values(K, fmt, y, C, out_f32=False):
    """device output -> fp32 numpy [..., C]"""
    if out_f32:
        return y.cpu().numpy()
    if fmt == SPLIT:
        return K.merge_planes(y.reshape(-1, 2 * C)).view(*y.shape[:-1], C).cpu().numpy()
    return y.float().cpu().numpy()


def _biteq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _close(fmt, out_f32, got, want, what):
    err = np.abs(got - want)
    if fmt == SPLIT or out_f32:
        tol = 3e-5 * max(1.0, float(np.abs(want).max()))
        assert float(err.max()) <= tol, (what, float(err.max()), tol)
    else:
        u = 2.0 ** -10 if fmt == FP16 else 2.0 ** -8
        bound = u * np.abs(want) + 3e-5 * np.abs(want).max()
        assert bool((err <= bound).all()), (what, float((err - bound).max()))


def _epilogue(conv, bnref, resf, relu):
    """the float64 epilogue of test_gpu_kernels._igemm_ref on a convolution computed once"""
    y = conv
    if bnref is not None:
        g, b, mu, var, eps = bnref
        sc = g / np.sqrt(var + eps)
        y = y * sc + (b - mu * sc)
    if resf is not None:
        y = y + resf.astype(np.float64)
    if relu:
        y = np.maximum(y, 0)
    return y


class Bufs:
    """the carved buffers of one launch"""

    def __init__(self):
        self.handles = []

    def inp(self, name, t, band):
        p, h = GB.carve(tuple(t.shape), t.dtype, t.device, band)
        GB.fill(p, t)
        self.handles.append((name, h))
        return p

    def out(self, name, shape, dtype, band):
        p, h = GB.carve(shape, dtype, "cuda", band)
        self.handles.append((name, h))
        return p

    def check(self, what):
        torch.cuda.synchronize()
        for name, h in self.handles:
            GB.check(h, "%s: %s" % (what, name))

    def untouched(self, what, names):
        torch.cuda.synchronize()
        for name, h in self.handles:
            if name in names:
                GB.check_untouched(h, "%s: %s" % (what, name))
            else:
                GB.check(h, "%s: %s" % (what, name))


def _rows_band(t_or_cols, itemsize=None):
    """BLOCK_ROWS rows of a [.., C] tensor (or of C columns of itemsize bytes)"""
    if itemsize is None:
        return BLOCK_ROWS * t_or_cols.shape[-1] * t_or_cols.element_size()
    return BLOCK_ROWS * t_or_cols * itemsize


def _stats_ok(partial, y2d):
    """per-block sums against the sums of the STORED output"""
    sums = partial.double().sum(0).cpu()
    yd = y2d.double().cpu()
    return (torch.allclose(sums[:, 0], yd.sum(0), rtol=1e-5, atol=1e-3) and
            torch.allclose(sums[:, 1], (yd * yd).sum(0), rtol=1e-5, atol=1e-3))


# ------------------------------------------------------------------------------------------------ hiast_igemm_bn_act
def _igemm_carved(K, fmt, x, wp, geom, bn=None, res=None, relu=False, out_f32=False, want_stats=False, gate=None, what=""):
    """one hiast_igemm_bn_act launch on carved copies of (x, wp, res, gate) into carved (y, partial), marshalled like
    kernels.igemm_bn_act; asserts 1 and 2 -> (y, partial)"""
    B, H, W, Cin, Cout, taps, stride, dil = geom
    PL = 2 if fmt == SPLIT else 1
    lib = K._lib.load()
    Ho, Wo = (H, W) if taps == 1 else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M = B * Ho * Wo
    bufs = Bufs()
    cx = bufs.inp("x", x, _rows_band(x))
    cw = bufs.inp("wp", wp, _rows_band(taps * PL * Cin, 2))
    ycols, ydt = (Cout, torch.float32) if out_f32 else (PL * Cout, x.dtype)
    y = bufs.out("y", (B, Ho, Wo, ycols), ydt, _rows_band(ycols, 4 if out_f32 else 2))
    cres = bufs.inp("res", res, _rows_band(res)) if res is not None else None
    cgate, gate_mask = None, 0
    if gate is not None:
        gate_mask = int(gate.dtype == torch.uint8)
        assert not gate_mask or tuple(gate.shape) == (M, Cout // 8)         # the bit mask: carved at exactly [M][Cout/8]
        cgate = bufs.inp("res_gate", gate, _rows_band(gate))
    partial, rows = None, 0
    if want_stats:
        rows = lib.hiast_igemm_stats_rows(M, Cin, Cout, taps, fmt)
        assert rows > 0
        partial = bufs.out("partial", (rows, Cout, 2), torch.float32, 4 * Cout * 8)
    if bn is not None:
        g, b, mu, var, eps = K._bn_params(bn)
    else:
        g = b = mu = var = ctypes.c_void_p(0)
        eps = 0.0
    rc = lib.hiast_igemm_bn_act(_p(cx), _p(cw), g, b, mu, var, eps, _p(cres), int(bool(relu)), _p(y), B, H, W, Cin, Cout, taps,
                                int(stride), int(dil), fmt, int(bool(out_f32)), _p(partial), rows, _p(cgate), gate_mask, _st())
    assert rc == 0, (what, rc)
    bufs.check(what)
    assert GB.finite(y), what + ": y has unwritten or poisoned elements"
    if partial is not None:
        assert GB.finite(partial), what + ": partial has unwritten or poisoned rows"
    return y, partial


def _igemm_case(K, fmt, geom, seed, epilogues):
    """operands of one geometry, the float64 convolution once, then every epilogue: carved launch, values, wrapper bits"""
    B, H, W, Cin, Cout, taps, stride, dil = geom
    PL = 2 if fmt == SPLIT else 1
    kk = 3 if taps == 9 else 1
    Ho, Wo = (H, W) if taps == 1 else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M = B * Ho * Wo
    xr = _round(fmt, synth.normal_f32(seed, (B, H, W, Cin)))
    w = synth.normal_f32(seed + 1, (Cout, Cin, kk, kk), (2.0 / (Cin * taps)) ** 0.5)
    rr = _round(fmt, synth.normal_f32(seed + 2, (B, Ho, Wo, Cout)))
    gv = _round(BF16 if fmt == SPLIT else fmt, synth.normal_f32(seed + 3, (B, Ho, Wo, Cout)))
    gv[0, 0, :3, :] = 0.0                                                     # exact zeros are closed
    bn, bnref = _mk_bn(seed + 4, Cout)
    x, res = _act(K, fmt, xr), _act(K, fmt, rr)
    wp = K.pack_conv_weight(dev(w), fmt)
    conv = _igemm_ref(xr, _round(fmt, w), None, None, False, stride, dil, taps)
    table = {  # name: (bn, res, relu, out_f32, want_stats, gate kind)
        "plain": (0, 0, 0, 0, 0, None), "bn_relu": (1, 0, 1, 0, 0, None), "bn_res_relu": (1, 1, 1, 0, 0, None),
        "bn_res": (1, 1, 0, 0, 0, None), "bn": (1, 0, 0, 0, 0, None), "res": (0, 1, 0, 0, 0, None),
        "gate_values": (0, 1, 0, 0, 0, "values"), "gate_mask": (0, 1, 0, 0, 0, "mask"), "stats": (0, 0, 0, 0, 1, None),
        "out_f32": (0, 0, 0, 1, 0, None)}
    for name in epilogues:
        has_bn, has_res, relu, out_f32, stats, gk = table[name]
        if PL == 2 and (gk or stats):
            continue                                                          # (one-plane variants)
        what = "%s %s" % (geom, name)
        gate, rref = None, (rr if has_res else None)
        if gk == "values":
            gate = _act(K, fmt, gv)
            rref = rr * (gv > 0)
        elif gk == "mask":
            gate = dev(np.packbits((gv > 0).reshape(M, Cout // 8, 8), axis=-1, bitorder="little").reshape(M, Cout // 8))
            rref = rr * (gv > 0)
        kw = dict(bn=bn if has_bn else None, res=res if has_res else None, relu=bool(relu), out_f32=bool(out_f32),
                  want_stats=bool(stats), gate=gate)
        y, partial = _igemm_carved(K, fmt, x, wp, geom, what=what, **kw)
        want = _epilogue(conv, bnref if has_bn else None, rref, relu)
        _close(fmt, out_f32, _values(K, fmt, y, Cout, out_f32), want, what)
        ref = K.igemm_bn_act(x, wp, PL, kw["bn"], kw["res"], kw["relu"], stride, dil, out_f32=kw["out_f32"],
                             want_stats=kw["want_stats"], res_gate=gate)
        if stats:
            assert _stats_ok(partial, y.view(-1, Cout)), what
            assert _biteq(partial, ref[1]), what + ": partial differs from the wrapper's"
            ref = ref[0]
        assert _biteq(y, ref), what + ": y differs from the wrapper's"


TILE_GEOMS = [  # B, H, W, Cin, Cout, taps, stride, dil
    (1, 9, 17, 64, 64, 1, 1, 1),        # M = 153: one partial block; 64-column tile; one k-step (two in split planes)
    (2, 13, 21, 512, 192, 1, 1, 1),     # M = 546: two blocks + a 34-row tail; three 64-column tiles; a long k loop
    (2, 13, 21, 64, 128, 9, 1, 1),      # 3x3, 128-column tile
    (1, 9, 17, 128, 384, 9, 1, 2),      # 3x3 dilation 2, three 128-column tiles, one partial block
    (2, 13, 21, 128, 256, 1, 1, 1),     # 256-column tile
    (2, 13, 21, 64, 256, 9, 1, 2),      # 3x3 dilation 2, 256-column tile
    (1, 17, 23, 128, 128, 9, 2, 1),     # stride 2 on an odd map (9 x 12 outputs)
]
ALL_EPILOGUES = ["plain", "bn_relu", "bn_res_relu", "bn_res", "gate_values", "gate_mask", "stats", "out_f32"]


@pytest.mark.parametrize("geom", TILE_GEOMS)
@pytest.mark.parametrize("fmt_name", ["bf16", "fp16", "split"])
def test_tile_kernel_extents(K, fmt_name, geom, monkeypatch):
    """the implicit-GEMM tile kernel, every epilogue it has for the format, at partial-block / tail-row geometries of every
    column-tile width"""
    monkeypatch.setenv("HIAST_XCONV", "0")
    monkeypatch.setenv("HIAST_XCONV2", "0")
    _igemm_case(K, FMTS[fmt_name], geom, 9000 + 10 * TILE_GEOMS.index(geom), ALL_EPILOGUES)


@pytest.mark.parametrize("Cin", [64, 256])
@pytest.mark.parametrize("fmt_name", ["bf16", "fp16", "split"])
def test_tile_kernel_ragged_column_tile(K, fmt_name, Cin, monkeypatch):
    """the plain N = 640 GEMM runs on 256-column tiles, the last one hanging 128 columns over N: its weight rows behind N
    must read as zeros (the band behind wp is NaN) and nothing may be stored for them (the band behind y); M = 546"""
    monkeypatch.setenv("HIAST_XCONV", "0")
    monkeypatch.setenv("HIAST_XCONV2", "0")
    _igemm_case(K, FMTS[fmt_name], (2, 13, 21, Cin, 640, 1, 1, 1), 9200 + Cin, ["plain"])


@pytest.mark.parametrize("case", [("bf16", 1, 128, ["plain", "stats", "bn_res_relu"]), ("bf16", 1, 256, ["plain", "stats", "bn_res_relu"]),
                                  ("split", 1, 128, ["bn_relu"]), ("split", 1, 256, ["bn_relu"]), ("split", 9, 128, ["bn_relu"])],
                         ids=lambda c: "%s-taps%d-N%d" % c[:3])
def test_tile_kernel_half_tile_forms(K, case, monkeypatch):
    """the 128 x 128 form (two 4-wave blocks per CU): M = 4160 = 32 full 128-row blocks + a 64-row tail"""
    fmt_name, taps, N, epilogues = case
    monkeypatch.setenv("HIAST_XCONV", "0")
    monkeypatch.setenv("HIAST_XCONV2", "0")
    geom = (1, 64, 65, 128, N, taps, 1, 1)
    with K.force_half_tile(1):
        if taps == 1:         # the form is really taken: one statistics row per 128 rows
            assert K._lib.load().hiast_igemm_stats_rows(4160, 128, N, 1, FMTS[fmt_name]) == 33
        _igemm_case(K, FMTS[fmt_name], geom, 9300 + N + taps, epilogues)


@pytest.mark.parametrize("M_hw", [(1, 64, 65), (2, 50, 77)])
@pytest.mark.parametrize("fmt_name", ["bf16", "fp16"])
def test_xconv_extents(K, fmt_name, M_hw):
    """K9e, the register-resident-weight kernel of the 256 -> 1024 1x1 launches: every epilogue test_xconv_expanding_1x1 /
    test_xconv_fp16 list (bn_res stays on the tile kernel), ragged M with a tail panel"""
    B, H, W = M_hw
    M = B * H * W
    # (the shape leaves the tile kernel: its statistics rows are one per xconv block stream, not one per 256 rows)
    assert M >= 4096 and K._lib.load().hiast_igemm_stats_rows(M, 256, 1024, 1, FMTS[fmt_name]) != (M + 255) // 256
    _igemm_case(K, FMTS[fmt_name], (B, H, W, 256, 1024, 1, 1, 1), 9400 + B,
                ["plain", "bn_relu", "bn_res_relu", "bn_res", "res", "gate_mask", "stats"])


@pytest.mark.parametrize("M_hw", [(1, 64, 65), (2, 50, 77)])
@pytest.mark.parametrize("Cout", [1024, 256])
def test_xconv2_extents(K, M_hw, Cout):
    """K9g, the split-plane 256 -> N form: the epilogues test_xconv2_split_plane_expanding_1x1 lists"""
    B, H, W = M_hw
    _igemm_case(K, SPLIT, (B, H, W, 256, Cout, 1, 1, 1), 9500 + B, ["bn_res_relu", "bn_relu", "bn"])


# ------------------------------------------------------------------------------------------------ data gradients
def _adjoint(w):
    """[Cdy][Ca][k][k] conv weight -> the weight of the adjoint convolution as a forward weight [Ca][Cdy][k][k]"""
    return np.ascontiguousarray(np.flip(w.transpose(1, 0, 2, 3), (2, 3)))


def _bn_bwd_sums(g_stored, gate, bn_x, mean, invstd):
    """float64 (sum g, sum g * xhat) per channel from the stored gradient [M][C]"""
    g = g_stored.double() * gate.double()
    xhat = (bn_x.double() - mean.double()) * invstd.double()
    return torch.stack([g.sum(0), (g * xhat).sum(0)], 1)


@pytest.mark.parametrize("Ca", [64, 256])
@pytest.mark.parametrize("taps,dil", [(1, 1), (9, 2)])
@pytest.mark.parametrize("fmt_name", ["bf16", "fp16"])
def test_dgrad_bn_stats_extents(K, fmt_name, taps, dil, Ca):
    """hiast_igemm_dgrad_bn_stats (STATS = 2 epilogue) at M = 546: dA and the per-block backward sums of the BatchNorm"""
    fmt = FMTS[fmt_name]
    B, H, W, Cdy = 2, 13, 21, 128
    kk = 3 if taps == 9 else 1
    M = B * H * W
    lib = K._lib.load()
    w = synth.normal_f32(9600, (Cdy, Ca, kk, kk), (2.0 / (Ca * taps)) ** 0.5)
    dyr = _round(fmt, synth.normal_f32(9601, (B, H, W, Cdy)))
    bxr = _round(fmt, synth.normal_f32(9602, (B, H, W, Ca), 1.5))
    dy, bx = _act(K, fmt, dyr), _act(K, fmt, bxr)
    wpt = K.pack_conv_weight(dev(w), fmt, transpose=True)
    gamma, beta = dev(synth.normal_f32(9603, (Ca,), 0.5)) + 1.0, dev(synth.normal_f32(9604, (Ca,), 0.3))
    sm = bx.float().mean(dim=(0, 1, 2)).contiguous()
    si = (1.0 / torch.sqrt(bx.float().var(dim=(0, 1, 2), unbiased=False) + 1e-5)).contiguous()
    bufs = Bufs()
    cdy, cw, cbx = bufs.inp("dy", dy, _rows_band(dy)), bufs.inp("wpt", wpt, _rows_band(taps * Cdy, 2)), bufs.inp("bn_x", bx, _rows_band(bx))
    da = bufs.out("da", (B, H, W, Ca), dy.dtype, _rows_band(Ca, 2))
    rows = lib.hiast_igemm_dgrad_bn_stats_rows(M, Cdy, Ca, taps)
    assert rows == (M + 255) // 256
    partial = bufs.out("partial", (rows, Ca, 2), torch.float32, 4 * Ca * 8)
    rc = lib.hiast_igemm_dgrad_bn_stats(_p(cdy), _p(cw), _p(da), B, H, W, Cdy, Ca, taps, dil, _p(cbx), _p(gamma), _p(beta), _p(sm),
                                        _p(si), _p(partial), rows, fmt, _st())
    assert rc == 0
    bufs.check("dgrad_bn_stats")
    assert GB.finite(da) and GB.finite(partial)
    want = _igemm_ref(dyr, _round(fmt, _adjoint(w)), None, None, False, 1, dil, taps)
    _close(fmt, False, da.float().cpu().numpy(), want, "da")
    # the gate of the kernel: fmaf(x, sc, sh) > 0 with sc = gamma * invstd, sh = fmaf(-mean, sc, beta) in fp32 (float64 of fp32
    # products is exact, so the sign below is the sign the kernel sees)
    sc = (gamma * si).double().cpu()
    sh = (beta.double().cpu() - sm.double().cpu() * sc).float().double()
    gate = (bx.view(M, Ca).double().cpu() * sc + sh) > 0
    ref = _bn_bwd_sums(da.view(M, Ca).cpu(), gate, bx.view(M, Ca).cpu(), sm.cpu(), si.cpu())
    assert torch.allclose(partial.double().sum(0).cpu(), ref, rtol=1e-5, atol=1e-3)
    da_w, partial_w = K.igemm_dgrad_bn_stats(dy, wpt, dil, bx, gamma, beta, sm, si)
    assert _biteq(da, da_w) and _biteq(partial, partial_w)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("hw", [(17, 23), (16, 16)])
@pytest.mark.parametrize("fmt_name", ["bf16", "fp16"])
def test_dgrad_s2_extents(K, fmt_name, hw, C):
    """hiast_igemm_dgrad_s2 (the transposed stride-2 form): odd and even maps, one partial block"""
    fmt = FMTS[fmt_name]
    B, (H, W) = 1, hw
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    lib = K._lib.load()
    w = synth.normal_f32(9700, (C, C, 3, 3), (2.0 / (9 * C)) ** 0.5)              # [Cout][Cin][3][3]
    dyr = _round(fmt, synth.normal_f32(9701, (B, Hs, Ws, C)))
    dy = _act(K, fmt, dyr)
    wpt = K.pack_conv_weight(dev(w), fmt, transpose=True)
    bufs = Bufs()
    cdy, cw = bufs.inp("dy", dy, _rows_band(dy)), bufs.inp("wpt", wpt, _rows_band(9 * C, 2))
    dx = bufs.out("dx", (B, H, W, C), dy.dtype, _rows_band(C, 2))
    rc = lib.hiast_igemm_dgrad_s2(_p(cdy), _p(cw), _p(dx), B, H, W, C, C, fmt, _st())
    assert rc == 0
    bufs.check("dgrad_s2")
    assert GB.finite(dx)
    want = torch.nn.grad.conv2d_input((B, C, H, W), torch.from_numpy(_round(fmt, w)).double(),
                                      torch.from_numpy(dyr).double().permute(0, 3, 1, 2), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    _close(fmt, False, dx.float().cpu().numpy(), want, "dx")
    assert _biteq(dx, K.igemm_dgrad_s2(dy, wpt, H, W))


@pytest.mark.parametrize("fmt_name", ["bf16", "fp16"])
def test_xconv_dgrad_gated_bn_stats_extents(K, fmt_name):
    """hiast_xconv_dgrad_gated_bn_stats at (2, 50, 77): M = 7700, ragged, a tail panel"""
    fmt = FMTS[fmt_name]
    B, H, W, Kc, N = 2, 50, 77, 256, 1024
    M = B * H * W
    lib = K._lib.load()
    w = synth.normal_f32(9800, (Kc, N, 1, 1), (2.0 / Kc) ** 0.5)                  # conv1: N -> Kc
    dyr = _round(fmt, synth.normal_f32(9801, (B, H, W, Kc)))
    rr = _round(fmt, synth.normal_f32(9802, (B, H, W, N)))
    bxr = _round(fmt, synth.normal_f32(9803, (B, H, W, N)))
    g = synth.rng(9804)
    gate_b = g.integers(0, 256, size=(M, N // 8), dtype=np.uint8)
    mask_b = g.integers(0, 256, size=(M, N // 8), dtype=np.uint8)
    dy, res, bx = _act(K, fmt, dyr), _act(K, fmt, rr), _act(K, fmt, bxr)
    gate, bmask = dev(gate_b), dev(mask_b)
    wpt = K.pack_conv_weight(dev(w), fmt, transpose=True)
    sm, si = dev(0.1 * synth.normal_f32(9805, (N,))), dev(np.abs(synth.normal_f32(9806, (N,))) + 0.5)
    bufs = Bufs()
    cdy, cw = bufs.inp("dy", dy, _rows_band(dy)), bufs.inp("wpt", wpt, _rows_band(Kc, 2))
    cres, cgate = bufs.inp("res", res, _rows_band(res)), bufs.inp("res_gate", gate, _rows_band(gate))
    cbx, cmask = bufs.inp("bn_x", bx, _rows_band(bx)), bufs.inp("bn_mask", bmask, _rows_band(bmask))
    dx = bufs.out("dx", (B, H, W, N), dy.dtype, _rows_band(N, 2))
    rows = lib.hiast_xconv_dgrad_gated_bn_stats_rows(M, Kc, N)
    assert rows > 0
    partial = bufs.out("partial", (rows, N, 2), torch.float32, 4 * N * 8)
    rc = lib.hiast_xconv_dgrad_gated_bn_stats(_p(cdy), _p(cw), _p(cres), _p(cgate), _p(cbx), _p(cmask), _p(sm), _p(si), _p(dx),
                                              _p(partial), M, Kc, N, fmt, _st())
    assert rc == 0
    bufs.check("xconv_dgrad_gated_bn_stats")
    assert GB.finite(dx) and GB.finite(partial)
    open_ = np.unpackbits(gate_b, axis=-1, bitorder="little").reshape(B, H, W, N)
    want = _igemm_ref(dyr, _round(fmt, _adjoint(w)), None, rr * open_, False, 1, 1, 1)
    _close(fmt, False, dx.float().cpu().numpy(), want, "dx")
    bits = torch.from_numpy(np.unpackbits(mask_b, axis=-1, bitorder="little").reshape(M, N))
    ref = _bn_bwd_sums(dx.view(M, N).cpu(), bits, bx.view(M, N).cpu(), sm.cpu(), si.cpu())
    assert torch.allclose(partial.double().sum(0).cpu(), ref, rtol=1e-5, atol=1e-3)
    dx_w, partial_w = K.xconv_dgrad_gated_bn_stats(dy, wpt, res, gate, bx, bmask, sm, si)
    assert _biteq(dx, dx_w) and _biteq(partial, partial_w)


# ------------------------------------------------------------------------------------------------ weight gradients
def _wgrad_ref(x, dy, k, stride, dil):
    """float64 CPU weight gradient of the 16-bit operands (channels-last device tensors)"""
    Cout, Cin = dy.shape[3], x.shape[3]
    return torch.nn.grad.conv2d_weight(x.cpu().double().permute(0, 3, 1, 2), (Cout, Cin, k, k), dy.cpu().double().permute(0, 3, 1, 2),
                                       stride=stride, padding=dil if k == 3 else 0, dilation=dil if k == 3 else 1)


def _wgrad_close(dw, ref, what):
    err = float((dw.cpu().double() - ref).abs().max())
    assert err <= 1e-4 * float(ref.abs().max()), (what, err, float(ref.abs().max()))


def _wgrad_operands(seed, cfg, dt):
    B, Cin, Cout, H, W, k, dil, stride = cfg
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = dev(synth.normal_f32(seed, (B, H, W, Cin))).to(dt)
    dy = dev(synth.normal_f32(seed + 1, (B, Ho, Wo, Cout))).to(dt)
    return x, dy


@pytest.mark.parametrize("cfg", [(1, 256, 256, 61, 77, 1, 1, 1),      # 1x1, M = 4697: several pixel ranges, a ragged last one
                                 (1, 256, 256, 21, 37, 3, 1, 1),      # 3x3 stride 1, Wo >= 20: the shifted-descriptor form
                                 (3, 256, 256, 9, 12, 3, 1, 2),       # stride 2 on a narrow map (5 x 6 outputs)
                                 (2, 256, 256, 9, 4, 3, 1, 1)])       # Wo = 4: the entry's lower bound
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_conv_wgrad_extents(K, cfg, dt):
    """hiast_conv_wgrad_nhwc: dw and a workspace of exactly hiast_conv_wgrad_workspace_bytes"""
    B, Cin, Cout, H, W, k, dil, stride = cfg
    taps = k * k
    lib = K._lib.load()
    x, dy = _wgrad_operands(9900, cfg, dt)
    need = lib.hiast_conv_wgrad_workspace_bytes(B, dy.shape[1], dy.shape[2], Cin, Cout, taps)
    assert need > 0 and need % (Cout * taps * Cin * 4) == 0
    split_range = Cout * taps * Cin * 4
    bufs = Bufs()
    cdy, cx = bufs.inp("dy", dy, _rows_band(dy)), bufs.inp("x", x, _rows_band(x))
    dw = bufs.out("dw", (Cout, Cin, k, k), torch.float32, split_range)
    ws = bufs.out("workspace", need, torch.uint8, split_range)
    rc = lib.hiast_conv_wgrad_nhwc(_p(cdy), _p(cx), _p(dw), B, H, W, Cin, Cout, taps, stride, dil, K.fmt_of(dy), _p(ws), need, _st())
    assert rc == 0
    bufs.check("conv_wgrad_nhwc")
    assert GB.finite(dw)
    _wgrad_close(dw, _wgrad_ref(x, dy, k, stride, dil), cfg)
    assert _biteq(dw, K.conv_wgrad_nhwc(dy, x, k, stride, dil))


# the rows of test_gpu_round3.SMALL_WGRAD whose pixel count is no multiple of 64 (the rounding of a pixel range: the last
# range is ragged whatever the split), strided ones among them
SMALL_RAGGED = [c for c in SMALL_WGRAD if (c[0] * ((c[3] - 1) // c[7] + 1) * ((c[4] - 1) // c[7] + 1)) % 64 != 0]


def test_small_ragged_rows_cover_the_strided_forms():
    assert (2, 128, 128, 27, 45, 3, 1, 2) in SMALL_RAGGED and (2, 256, 128, 26, 42, 1, 1, 2) in SMALL_RAGGED
    assert any(c[5] == 1 and c[1] == 64 and c[2] >= 128 for c in SMALL_RAGGED)     # the transposed form


@pytest.mark.parametrize("cfg", SMALL_RAGGED)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_conv_wgrad_small_extents(K, cfg, dt):
    """hiast_conv_wgrad_small_nhwc: every tiling form at a ragged last pixel range"""
    B, Cin, Cout, H, W, k, dil, stride = cfg
    taps = k * k
    lib = K._lib.load()
    x, dy = _wgrad_operands(9950, cfg, dt)
    ref = _wgrad_ref(x, dy, k, stride, dil)
    xs, s = x, stride
    if k == 1 and stride != 1:                       # a strided 1x1 is the call on the subsampled input (kernels.py)
        xs, s = x[:, ::stride, ::stride, :].contiguous(), 1
    Hi, Wi = xs.shape[1], xs.shape[2]
    need = lib.hiast_conv_wgrad_small_workspace_bytes(B, dy.shape[1], dy.shape[2], Cin, Cout, taps)
    assert need > 0
    tile = 128 * 128 * 4                             # one partial tile of one block
    bufs = Bufs()
    cdy, cx = bufs.inp("dy", dy, _rows_band(dy)), bufs.inp("x", xs, _rows_band(xs))
    dw = bufs.out("dw", (Cout, Cin, k, k), torch.float32, Cout * taps * Cin * 4)
    ws = bufs.out("workspace", need, torch.uint8, max(tile, Cout * taps * Cin * 4))
    rc = lib.hiast_conv_wgrad_small_nhwc(_p(cdy), _p(cx), _p(dw), B, Hi, Wi, Cin, Cout, taps, s, dil, K.fmt_of(dy), _p(ws), need, _st())
    assert rc == 0
    bufs.check("conv_wgrad_small_nhwc")
    assert GB.finite(dw)
    _wgrad_close(dw, ref, cfg)
    assert _biteq(dw, K.conv_wgrad_small_nhwc(dy, x, k, stride, dil))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_conv_wgrad_group_extents(K, dt):
    """hiast_conv_wgrad_group_nhwc: a 1x1 job (M = 546) and a 3x3 job (M = 777) in one launch, one shared workspace"""
    lib = K._lib.load()
    x1, dy1 = _wgrad_operands(9970, (2, 512, 256, 13, 21, 1, 1, 1), dt)
    x9, dy9 = _wgrad_operands(9980, (1, 256, 256, 21, 37, 3, 2, 1), dt)
    jobs = [(dy1, x1, 1, 1, 1), (dy9, x9, 3, 1, 2)]
    bufs = Bufs()
    arr = (K._lib.WgradJob * 2)()
    dws = []
    for i, (dy, x, k, stride, dil) in enumerate(jobs):
        B, H, W, Cin = x.shape
        Cout = dy.shape[3]
        cdy, cx = bufs.inp("dy%d" % i, dy, _rows_band(dy)), bufs.inp("x%d" % i, x, _rows_band(x))
        dw = bufs.out("dw%d" % i, (Cout, Cin, k, k), torch.float32, Cout * Cin * k * k * 4)
        dws.append(dw)
        arr[i] = K._lib.WgradJob(_p(cdy), _p(cx), _p(dw), B, H, W, Cin, Cout, k * k, stride, dil)
    need = lib.hiast_conv_wgrad_group_workspace_bytes(ctypes.addressof(arr), 2)
    assert need > 0
    ws = bufs.out("workspace", need, torch.uint8, 256 * 9 * 256 * 4)
    rc = lib.hiast_conv_wgrad_group_nhwc(ctypes.addressof(arr), 2, K.fmt_of(dy1), _p(ws), need, _st())
    assert rc == 0
    bufs.check("conv_wgrad_group_nhwc")
    outs = K.conv_wgrad_group(jobs)
    for (dy, x, k, stride, dil), dw, dw_w in zip(jobs, dws, outs):
        assert GB.finite(dw)
        _wgrad_close(dw, _wgrad_ref(x, dy, k, stride, dil), (tuple(x.shape), k))
        assert _biteq(dw, dw_w)


# Exact weight gradients.  dy and x hold integers of {-2 .. 2} (exact in fp16 and bf16): every product and every partial sum
# is an integer of magnitude <= 4 M <= 131072 < 2^24, exact in fp32 whatever the order of summation, so dW must EQUAL the
# float64 gradient — a reduction that skips, repeats or misplaces a pixel range, a tap or a k cannot hide in a tolerance.
# name: ([(B, Cin, Cout, H, W, k, dil, stride), ...], pixel ranges per job on 256 CUs)
EXACT_WGRAD = {
    "1x1, 11 ranges": ([(1, 256, 256, 53, 107, 1, 1, 1)], 11),         # M = 5671: one unrolled round of 8 + a tail of 3, ragged last range
    "3x3 s1, 11 ranges": ([(1, 256, 256, 53, 107, 3, 1, 1)], 11),      # the shifted-descriptor form, tap-strided store
    "1x1, 64 ranges": ([(1, 256, 256, 128, 256, 1, 1, 1)], 64),        # M = 32768, the cap: eight full rounds, empty tail
    "group 1x1 + 3x3": ([(1, 512, 256, 53, 107, 1, 1, 1), (1, 256, 256, 53, 107, 3, 1, 1)], 11),   # the second job's f4_begin
}
_exact_cache = {}


def _exact_wgrad_case(name):
    """-> [(x int8 [B,H,W,Cin], dy int8 [B,Ho,Wo,Cout], float64 dW)] on the CPU, computed once for both operand types"""
    if name not in _exact_cache:
        gen = torch.Generator().manual_seed(9960 + sorted(EXACT_WGRAD).index(name))
        jobs = []
        for B, Cin, Cout, H, W, k, dil, stride in EXACT_WGRAD[name][0]:
            x = torch.randint(-2, 3, (B, H, W, Cin), generator=gen, dtype=torch.int8)
            dy = torch.randint(-2, 3, (B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout), generator=gen, dtype=torch.int8)
            jobs.append((x, dy, _wgrad_ref(x, dy, k, stride, dil)))
        _exact_cache[name] = jobs
    return _exact_cache[name]


@pytest.mark.parametrize("name", list(EXACT_WGRAD))
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_conv_wgrad_exact_on_small_integers(K, name, dt):
    """hiast_conv_wgrad_nhwc / hiast_conv_wgrad_group_nhwc: torch.equal against float64, at the split counts stated above"""
    cfgs, splits = EXACT_WGRAD[name]
    lib = K._lib.load()
    per_split = [Cout * k * k * Cin * 4 for _, Cin, Cout, _, _, k, _, _ in cfgs]
    if len(cfgs) == 1:
        B, Cin, Cout, H, W, k, dil, stride = cfgs[0]
        need = lib.hiast_conv_wgrad_workspace_bytes(B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cin, Cout, k * k)
    else:
        arr = (K._lib.WgradJob * len(cfgs))(*[K._lib.WgradJob(None, None, None, B, H, W, Cin, Cout, k * k, stride, dil)
                                               for B, Cin, Cout, H, W, k, dil, stride in cfgs])
        need = lib.hiast_conv_wgrad_group_workspace_bytes(ctypes.addressof(arr), len(cfgs))
    # (another CU count would split differently and quietly test less)
    assert need % sum(per_split) == 0 and need // sum(per_split) == splits, (need, per_split)
    case = _exact_wgrad_case(name)
    jobs = [(dy.cuda().to(dt), x.cuda().to(dt), c[5], c[7], c[6]) for (x, dy, _), c in zip(case, cfgs)]      # (dy, x, k, stride, dil)
    outs = [K.conv_wgrad_nhwc(*jobs[0])] if len(jobs) == 1 else K.conv_wgrad_group(jobs)
    for dw, (_, _, ref), cfg in zip(outs, case, cfgs):
        assert float(ref.abs().max()) < 2.0 ** 24
        assert torch.equal(dw.cpu().double(), ref), (name, cfg, float((dw.cpu().double() - ref).abs().max()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stem_train_extents(K, dt):
    """hiast_stem_train_fwd + hiast_stem_wgrad at (2, 67, 101): ragged 8 x 16 tiles in both directions"""
    B, H, W = 2, 67, 101
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    fmt = K.FMT_FP16 if dt == torch.float16 else K.FMT_BF16
    lib = K._lib.load()
    x = dev(synth.normal_f32(9990, (B, 3, H, W)))
    w = dev(synth.normal_f32(9991, (64, 3, 7, 7), 0.1))
    bufs = Bufs()
    cx, cw = bufs.inp("x", x, 64 * 1024), bufs.inp("w", w, 64 * 3 * 7 * 7 * 4)
    y = bufs.out("y", (B, Hc, Wc, 64), dt, _rows_band(64, 2))
    nblk = lib.hiast_stem_train_blocks(B, H, W)
    assert nblk > 0
    partial = bufs.out("partial", (nblk, 64, 2), torch.float32, 4 * 64 * 8)
    rc = lib.hiast_stem_train_fwd(_p(cx), _p(cw), _p(y), _p(partial), fmt, B, H, W, _st())
    assert rc == 0
    bufs.check("stem_train_fwd")
    assert GB.finite(y) and GB.finite(partial)
    xr, wr = x.to(dt).double().cpu(), w.to(dt).double().cpu()
    want = torch.nn.functional.conv2d(xr, wr, None, 2, 3).permute(0, 2, 3, 1).numpy()
    _close(fmt, False, y.float().cpu().numpy(), want, "stem y")
    assert _stats_ok(partial, y.view(-1, 64))
    y_w, partial_w = K.stem_train_fwd(x, w, fmt)
    assert _biteq(y, y_w) and _biteq(partial, partial_w)
    # the weight gradient
    dy = dev(synth.normal_f32(9992, (B, Hc, Wc, 64))).to(dt)
    need = lib.hiast_stem_wgrad_workspace_bytes(B, H, W)
    assert need > 0
    bufs = Bufs()
    cx, cdy = bufs.inp("x", x, 64 * 1024), bufs.inp("dy", dy, _rows_band(dy))
    dw = bufs.out("dw", (64, 3, 7, 7), torch.float32, 64 * 3 * 7 * 7 * 4)
    ws = bufs.out("workspace", need, torch.uint8, 64 * 7 * 32 * 4)                # one block's partials
    rc = lib.hiast_stem_wgrad(_p(cx), _p(cdy), _p(dw), fmt, B, H, W, _p(ws), need, _st())
    assert rc == 0
    bufs.check("stem_wgrad")
    assert GB.finite(dw)
    ref = torch.nn.grad.conv2d_weight(xr, (64, 3, 7, 7), dy.double().cpu().permute(0, 3, 1, 2), stride=2, padding=3)
    _wgrad_close(dw, ref, "stem dw")
    assert _biteq(dw, K.stem_wgrad(x, dy))


# ------------------------------------------------------------------------------------------------ size limits
def _tiny(bufs, name, nbytes=4096):
    """a small carved buffer that a refused call must leave at 0xFF"""
    return bufs.out(name, nbytes, torch.uint8, 4096)


def test_refused_shapes_write_nothing(K):
    """a shape just over a limit an entry states is refused on the host, before any launch: the tensors handed over are tiny
    (the batch size alone is over the limit) and stay untouched, bands and payloads"""
    lib = K._lib.load()
    bufs = Bufs()
    a, b, c, d, e, f, g, h, i, j = (_tiny(bufs, n) for n in "abcdefghij")
    names = set("abcdefghij")
    z = ctypes.c_void_p(0)
    # tile kernel: an operand of 2 GiB (2^24 pixels x 64 channels x 2 bytes)
    for fmt in (BF16, FP16, SPLIT):
        rc = lib.hiast_igemm_bn_act(_p(a), _p(b), z, z, z, z, 0.0, z, 0, _p(c), 1 << 18, 8, 8, 64, 64, 1, 1, 1, fmt, 0, z, 0, z, 0, _st())
        assert rc == E_RANGE, fmt
    rc = lib.hiast_igemm_dgrad_bn_stats(_p(a), _p(b), _p(c), 1 << 18, 8, 8, 64, 64, 1, 1, _p(d), z, z, _p(e), _p(f), _p(g),
                                        1 << 16, BF16, _st())
    assert rc == E_RANGE
    rc = lib.hiast_igemm_dgrad_s2(_p(a), _p(b), _p(c), 1 << 18, 8, 8, 256, 256, BF16, _st())
    assert rc == E_RANGE
    # xconv data gradient: dy of 2 GiB, and a map below its 4096-pixel minimum
    for M in (1 << 22, 4095):
        rc = lib.hiast_xconv_dgrad_gated_bn_stats(_p(a), _p(b), _p(c), _p(d), _p(e), _p(f), _p(g), _p(h), _p(i), _p(j), M, 256,
                                                  1024, BF16, _st())
        assert rc == E_RANGE, M
    # weight gradients: M >= 2^24 pixels
    big = (1 << 16, 16, 16)
    rc = lib.hiast_conv_wgrad_nhwc(_p(a), _p(b), _p(c), *big, 256, 256, 1, 1, 1, BF16, _p(d), 4096, _st())
    assert rc == E_RANGE
    rc = lib.hiast_conv_wgrad_small_nhwc(_p(a), _p(b), _p(c), *big, 64, 64, 1, 1, 1, BF16, _p(d), 4096, _st())
    assert rc == E_RANGE
    assert lib.hiast_conv_wgrad_small_workspace_bytes(*big, 64, 64, 1) == 0
    job = (K._lib.WgradJob * 1)(K._lib.WgradJob(_p(a), _p(b), _p(c), *big, 256, 256, 1, 1, 1))
    assert lib.hiast_conv_wgrad_group_workspace_bytes(ctypes.addressof(job), 1) == 0
    assert lib.hiast_conv_wgrad_group_nhwc(ctypes.addressof(job), 1, BF16, _p(d), 4096, _st()) == E_RANGE
    # 3x3 weight gradient on a map with fewer than 4 output columns
    assert lib.hiast_conv_wgrad_nhwc(_p(a), _p(b), _p(c), 1, 8, 3, 256, 256, 9, 1, 1, BF16, _p(d), 4096, _st()) == E_RANGE
    assert lib.hiast_conv_wgrad_nhwc(_p(a), _p(b), _p(c), 1, 8, 6, 256, 256, 9, 2, 1, BF16, _p(d), 4096, _st()) == E_RANGE
    job = (K._lib.WgradJob * 1)(K._lib.WgradJob(_p(a), _p(b), _p(c), 1, 8, 3, 256, 256, 9, 1, 1))
    assert lib.hiast_conv_wgrad_group_nhwc(ctypes.addressof(job), 1, BF16, _p(d), 4096, _st()) == E_RANGE
    # the stem: an image batch of 2^31 elements
    assert lib.hiast_stem_train_blocks(1 << 17, 64, 128) == 0 and lib.hiast_stem_wgrad_workspace_bytes(1 << 17, 64, 128) == 0
    assert lib.hiast_stem_train_fwd(_p(a), _p(b), _p(c), _p(d), BF16, 1 << 17, 64, 128, _st()) == E_RANGE
    assert lib.hiast_stem_wgrad(_p(a), _p(b), _p(c), BF16, 1 << 17, 64, 128, _p(d), 4096, _st()) == E_RANGE
    bufs.untouched("refused", names)


@pytest.mark.parametrize("entry", ["wgrad", "small", "group", "stem"])
def test_workspace_one_byte_short_is_refused(K, entry):
    """HIAST_E_WS for a workspace one byte below the size function's answer; nothing is written"""
    lib = K._lib.load()
    dt = torch.bfloat16
    bufs = Bufs()
    if entry == "stem":
        B, H, W = 2, 67, 101
        x = bufs.inp("x", dev(synth.normal_f32(1, (B, 3, H, W))), 4096)
        dy = bufs.inp("dy", dev(synth.normal_f32(2, (B, 34, 51, 64))).to(dt), 4096)
        dw = bufs.out("dw", (64, 3, 7, 7), torch.float32, 4096)
        need = lib.hiast_stem_wgrad_workspace_bytes(B, H, W)
        ws = bufs.out("workspace", need - 1, torch.uint8, 4096)
        rc = lib.hiast_stem_wgrad(_p(x), _p(dy), _p(dw), BF16, B, H, W, _p(ws), need - 1, _st())
    else:
        C = 64 if entry == "small" else 256
        B, H, W = 1, 21, 37
        x = bufs.inp("x", dev(synth.normal_f32(1, (B, H, W, C))).to(dt), 4096)
        dy = bufs.inp("dy", dev(synth.normal_f32(2, (B, H, W, C))).to(dt), 4096)
        dw = bufs.out("dw", (C, C, 3, 3), torch.float32, 4096)
        if entry == "group":
            job = (K._lib.WgradJob * 1)(K._lib.WgradJob(_p(dy), _p(x), _p(dw), B, H, W, C, C, 9, 1, 1))
            need = lib.hiast_conv_wgrad_group_workspace_bytes(ctypes.addressof(job), 1)
            ws = bufs.out("workspace", need - 1, torch.uint8, 4096)
            rc = lib.hiast_conv_wgrad_group_nhwc(ctypes.addressof(job), 1, BF16, _p(ws), need - 1, _st())
        else:
            size_fn = lib.hiast_conv_wgrad_small_workspace_bytes if entry == "small" else lib.hiast_conv_wgrad_workspace_bytes
            fn = lib.hiast_conv_wgrad_small_nhwc if entry == "small" else lib.hiast_conv_wgrad_nhwc
            need = size_fn(B, H, W, C, C, 9)
            ws = bufs.out("workspace", need - 1, torch.uint8, 4096)
            rc = fn(_p(dy), _p(x), _p(dw), B, H, W, C, C, 9, 1, 1, BF16, _p(ws), need - 1, _st())
    assert need > 1 and rc == E_WS, (entry, need, rc)
    bufs.untouched(entry, {"dw", "workspace"})
