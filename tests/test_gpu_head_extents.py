"""The head and pseudo-label entries (aspp.hip, aspp2.hip, upsample.hip, plabel.hip, plabel2.hip) through the C ABI on buffers
carved out of 0xFF-filled allocations (tests/guard_bands.py), the float outputs of both ASPP forms and of the upsample adjoint
entry by entry against float64 (tests/head_ref.py) with the error bounds derived there.  Inputs sit in NaN poison; outputs and
workspaces start as 0xFF.  After each launch:
  1. both guard bands of every buffer, inputs and workspace included, are untouched;
  2. every output payload is finite and fully written (the workspace is exempt from "fully written"; uint8 outputs are compared
     instead; the accumulating outputs hist / count / sumprob_fx start from values the test chooses and are compared exactly;
     class_total, which the entry overwrites, starts from such a value too);
  3. ASPP outputs (both forms) and the upsample adjoint are inside the bound of head_ref.py at EVERY element; integer and byte
     outputs are bit-equal to numpy / the C oracle, and so are the TTA probability sums; upsample forward and pass 1's maxprob,
     which have their oracle tests through the wrappers, are bit-equal to the wrapper (item 4);
  4. the payload is bit-equal to what the ordinary K.* wrapper returns for the same operands;
  5. a second launch gives the same bits; accumulating outputs double exactly;
  6. workspaces are carved at exactly the size the *_workspace_bytes entry returns.
Bands.  BAND = 64 KiB holds what one block of the NCHW kernels touches in a pass: 256 pixels x 32 channels x 4 bytes (aspp
forward), 64 pixels x 256 channels x 4 (bwd_data), 128 channels x 32 rows x 4 of one tap's partial (bwd_weight), 256 columns of
a band of rows (upsample, pass 1, TTA), 4 x 1024 pixels (pass 2), a 4096-pixel tile (strided_hist).  The row-major buffers of
aspp2.hip (x, T / G / P in the workspace, dx, wt, wd) get 128 rows, the GEMM tile height.

entry                                   test
hiast_aspp_pack_weights, _wpack_bytes   test_direct_aspp (bit-equal to numpy)
hiast_aspp_fwd, _workspace_bytes        test_direct_aspp: Cout 2, 9, 16 (NV = 0), 17 (NV = 1), 18 (NV = 2), 19 (NV = 3), 20 and 32 (the 32-row
                                        kernel); split-K 1 / 2 / 4; XCD remap on (2,256,32,128: 128 blocks) and off (3,64,9,17: 3 blocks)
hiast_aspp_bwd_data                     test_direct_aspp: Cout 9, 16, 19, 20 (Cin 256)
hiast_aspp_bwd_weight                   test_direct_aspp: Cout 9, 16 (NV = 0), 17, 18, 19; 1, 2 (uneven) and 16 pixel splits; w = 3
hiast_aspp2_pack_weights, _np           test_nhwc_forward / test_nhwc_backward (bit-equal to numpy, wd with and without)
hiast_aspp2_fwd, _workspace_bytes       test_nhwc_forward: fp32 rows, split planes, bf16 rows, fp16 rows (fp16 T); workspace exact and - 256
hiast_aspp2_bwd, _workspace_bytes       test_nhwc_backward: bf16, fp16; dx only, weights only, both; workspace exact and - 256
hiast_upsample_bilinear_ac_fwd, _bwd    test_upsample
hiast_plabel_pass1, its workspace size  test_pass1 (workspace: persistent and one-block-per-item form; NULL)
hiast_plabel_pass2                      test_pass2 (vector and scalar path, misaligned pointers), test_pass2_grid_cap
hiast_plabel_strided_hist               test_strided_hist
hiast_tta_fused                         test_tta
argument checks of all of them          test_refused_calls_write_nothing

NOT covered: the grid limits of the other entries.  aspp / aspp2 take B <= 65535 as grid.y (a 65536-image batch); upsample takes
B C <= 65535 and H <= 65535 as grid.z / grid.y; pass 1 takes B <= 65535 and h <= 65535 as grid.z / grid.y and its persistent
form up to 2^30 items; strided_hist's block count passes 2^31 at N = 2^43.
HIAST_ASPP_SPLITK, HIAST_ASPP_WG_NTILE = 2 and HIAST_ASPP_T32 (tuning overrides) are cleared, not exercised.  Images above the
2 GiB the 16-row forward addresses are refused (test_head_host.py) and never launched."""
import numpy as np
import pytest
import torch

import guard_bands as GB
import head_calls as HC
import head_ref as R
import synth
from bn_ref import round16
from oracle import cref
from test_gpu_bn_extents import Bufs, _biteq, _np, _st, twice
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

WORST = {}                           # output class -> worst error / bound seen in this run (test_zz_report_worst_ratios)
BAND = 64 << 10
DILS = [(6, 12, 18, 24), (1, 2, 3, 5)]
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
F32, U8, I32, I64 = torch.float32, torch.uint8, torch.int32, torch.int64
NBINS = 15361


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    from hiast_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for n in ("HIAST_ASPP_SPLITK", "HIAST_ASPP_WG_NTILE", "HIAST_ASPP_T32"):
        monkeypatch.delenv(n, raising=False)


def inside(cls, got, ref, bound):
    """|got - ref| <= bound at every element; records the worst ratio of the class"""
    err = np.abs(_np(got.double() if hasattr(got, "double") else got).astype(np.float64) - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    assert np.isfinite(err).all(), cls
    ratio = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())
    print("head worst-in-case error/bound  %-24s %.4f" % (cls, ratio))
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    over = err > bound
    assert not over.any(), "%s: %d element(s) outside the bound, worst error / bound = %.3f" % (cls, int(over.sum()), ratio)


def rows_band(rowbytes):
    return GB.round_band(128 * rowbytes)


def ok(rc):
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------ direct form (aspp.hip)
# (B, Cin, h, w, Cout, dilation set).  Every Cout of every entry meets a ragged shape and (2,32,128); every shape meets 19 and 16.
DIRECT = [
    (1, 64, 9, 17, 19, 0), (1, 256, 9, 17, 16, 1), (1, 256, 9, 17, 19, 1), (3, 64, 9, 17, 19, 1), (3, 64, 9, 17, 16, 0),
    (2, 128, 5, 70, 19, 0), (2, 256, 5, 70, 16, 1), (1, 256, 7, 3, 19, 0), (1, 256, 7, 3, 16, 1), (1, 128, 20, 70, 19, 1),
    (1, 256, 20, 70, 16, 0), (2, 256, 32, 128, 19, 0), (2, 256, 32, 128, 16, 1),
    (1, 64, 9, 17, 2, 0), (2, 64, 32, 128, 2, 1), (2, 256, 5, 70, 9, 0), (2, 256, 32, 128, 9, 1), (1, 64, 9, 17, 17, 1),
    (2, 64, 32, 128, 17, 0), (1, 128, 20, 70, 18, 0), (2, 64, 32, 128, 18, 1), (1, 256, 9, 17, 20, 0), (2, 256, 32, 128, 20, 1),
    (2, 128, 5, 70, 32, 1), (2, 64, 32, 128, 32, 0),
]


def fwd_path(Cout):
    return "32-row" if Cout > 19 else "NV=%d" % max(0, Cout - 16)


@pytest.mark.parametrize("case", DIRECT, ids=lambda c: "%dx%dx%dx%d-C%d-d%d" % c)
def test_direct_aspp(K, lib, case):
    B, Cin, h, w, Cout, di = case
    dil = DILS[di]
    x, ws, bs, gy = R.aspp_inputs(900 + Cout, B, Cin, h, w, Cout)
    want_b, want_w = Cin % 256 == 0 and Cout <= 20, Cout <= 19
    g = gy if (want_b or want_w) else None
    ref, mag = R.reference(x, ws, bs, dil, g), R.magnitudes(x, ws, bs, dil, g)
    inb = Bufs()
    X, GY = inb.inp("x", dev(x), BAND), inb.inp("dy", dev(gy), BAND)
    Wd = [inb.inp("w%d" % i, dev(ws[i]), BAND) for i in range(4)]
    Bd = [inb.inp("b%d" % i, dev(bs[i]), BAND) for i in range(4)]
    dims = dict(B=B, Cin=Cin, h=h, w=w, Cout=Cout, dil=dil)

    # ---- pack
    nwp = lib.hiast_aspp_wpack_bytes(Cin, Cout)
    assert nwp == (33 * Cin * 32 + 32) * 4

    def pack():
        b = Bufs()
        wp = b.out("wpack", (nwp // 4,), F32, BAND)
        ok(HC.call(lib, "aspp_pack", w0=Wd[0], w1=Wd[1], w2=Wd[2], w3=Wd[3], b0=Bd[0], b1=Bd[1], b2=Bd[2], b3=Bd[3], Cin=Cin,
                   Cout=Cout, wpack=wp, stream=_st()))
        b.check(inb)
        return dict(wpack=wp)
    wp = twice(pack)["wpack"]
    want = np.zeros((33, Cin, 32), np.float32)
    want[:, :, :Cout] = R.pack_taps(ws).transpose(0, 2, 1)
    bias = np.zeros(32, np.float32)
    bias[:Cout] = R._bias_sum(bs)
    assert _biteq(wp, dev(np.concatenate([want.ravel(), bias]))), "wpack is not [33][Cin][32] + the summed bias"
    assert _biteq(wp, K.aspp_pack_weights([dev(t) for t in ws], [dev(t) for t in bs]))
    WP = inb.inp("wpack", wp.clone(), BAND)

    # ---- forward
    nws = lib.hiast_aspp_workspace_bytes(B, Cin, h, w, Cout)
    assert nws % 4 == 0 and nws >= max(HC.used_bytes("splitk", dims), HC.used_bytes("wgrad", dims))

    def fwd():
        b = Bufs()
        y = b.out("y", (B, Cout, h, w), F32, BAND)
        wsb = b.out("workspace", (nws // 4,), F32, BAND, must_fill=False)
        ok(HC.call(lib, "aspp_fwd", x=X, wpack=WP, y=y, ws=wsb, ws_bytes=nws, stream=_st(), **dims))
        b.check(inb)
        return dict(y=y)
    y = twice(fwd)["y"]
    inside("aspp y " + fwd_path(Cout), y, ref["y"], R.fwd_bound(mag["y"], B, Cin, h, w, Cout))
    assert _biteq(y, K.aspp_fwd(dev(x), wp.clone(), Cout, dil))

    # ---- data gradient
    if want_b:
        def bwd_data():
            b = Bufs()
            dx = b.out("dx", (B, Cin, h, w), F32, BAND)
            ok(HC.call(lib, "aspp_bwd_data", dy=GY, wpack=WP, dx=dx, stream=_st(), **dims))
            b.check(inb)
            return dict(dx=dx)
        dx = twice(bwd_data)["dx"]
        inside("aspp dx", dx, ref["dx"], R.bwd_data_bound(mag["dx"], Cout))
        assert _biteq(dx, K.aspp_bwd_data(dev(gy), wp.clone(), Cin, dil))

    # ---- weight gradient
    if want_w:
        def bwd_weight():
            b = Bufs()
            o = {"dw%d" % i: b.out("dw%d" % i, (Cout, Cin, 3, 3), F32, BAND) for i in range(4)}
            o["db"] = b.out("db", (Cout,), F32, BAND)
            wsb = b.out("workspace", (nws // 4,), F32, BAND, must_fill=False)
            ok(HC.call(lib, "aspp_bwd_weight", x=X, dy=GY, ws=wsb, ws_bytes=nws, stream=_st(), **o, **dims))
            b.check(inb)
            return o
        o = twice(bwd_weight)
        for i in range(4):
            inside("aspp dW " + fwd_path(Cout), o["dw%d" % i], ref["dw"][i], R.bwd_weight_bound(mag["dw"][i], B, h, w))
        inside("aspp db", o["db"], ref["db"], R.db_bound(ref["db"], gy))
        dws, db = K.aspp_bwd_weight(dev(x), dev(gy), dil)
        assert all(_biteq(o["dw%d" % i], dws[i]) for i in range(4)) and _biteq(o["db"], db)


# ------------------------------------------------------------------------------------------------ GEMM + shift-add form (aspp2.hip)
NHWC = [(1, 128, 9, 17, 19), (2, 256, 5, 70, 16), (2, 128, 20, 70, 19), (1, 128, 64, 32, 16), (1, 256, 9, 17, 2), (2, 128, 5, 70, 9),
        (2, 128, 5, 70, 32)]
_ids5 = lambda c: "%dx%dx%dx%d-C%d" % c


def nhwc_pack(K, lib, ws, bs, Cin, Cout, inb):
    """hiast_aspp2_pack_weights in carved buffers, with and without wd; -> wt, wd, bias (checked, plain clones)"""
    NP = lib.hiast_aspp2_np(Cout)
    assert NP == -(-33 * Cout // 128) * 128
    Wd = [inb.inp("w%d" % i, dev(ws[i]), BAND) for i in range(4)]
    Bd = [inb.inp("b%d" % i, dev(bs[i]), BAND) for i in range(4)]

    def pack(with_wd):
        b = Bufs()
        o = dict(wt=b.out("wt", (NP, Cin), F32, rows_band(Cin * 4)), bias=b.out("bias", (Cout,), F32, BAND))
        if with_wd:
            o["wd"] = b.out("wd", (Cin, NP), F32, rows_band(NP * 4))
        ok(HC.call(lib, "aspp2_pack", w0=Wd[0], w1=Wd[1], w2=Wd[2], w3=Wd[3], b0=Bd[0], b1=Bd[1], b2=Bd[2], b3=Bd[3], Cin=Cin,
                   Cout=Cout, wt=o["wt"], wd=o.get("wd"), bias=o["bias"], stream=_st()))
        b.check(inb)
        return o
    o = twice(lambda: pack(True))
    assert _biteq(pack(False)["wt"], o["wt"])
    want = np.zeros((NP, Cin), np.float32)
    want[:33 * Cout] = R.pack_taps(ws).reshape(33 * Cout, Cin)
    assert _biteq(o["wt"], dev(want)) and _biteq(o["wd"], dev(want.T)) and _biteq(o["bias"], dev(R._bias_sum(bs)))
    kw = K.aspp2_pack_weights([dev(t) for t in ws], [dev(t) for t in bs], need_dgrad=True)
    assert all(_biteq(a, b) for a, b in zip((o["wt"], o["wd"], o["bias"]), kw))
    return o["wt"].clone(), o["wd"].clone(), o["bias"].clone()


@pytest.mark.parametrize("kind", ["rows32", "planes", "bf16", "fp16"])
@pytest.mark.parametrize("case", NHWC, ids=_ids5)
def test_nhwc_forward(K, lib, case, kind):
    B, Cin, h, w, Cout = case
    dil = DILS[NHWC.index(case) % 2]
    x, ws, bs, _ = R.aspp_inputs(1000 + Cout, B, Cin, h, w, Cout)
    inb = Bufs()
    wt, _, bias = nhwc_pack(K, lib, ws, bs, Cin, Cout, inb)
    NP, M = wt.shape[0], B * h * w
    rows = dev(x).permute(0, 2, 3, 1).contiguous()                      # [B,h,w,Cin] fp32
    if kind == "rows32":
        xd, dt, wsrc, rx, rw, taps = rows, 0, wt, x, ws, None
        wrapper = lambda: K.aspp2_fwd(rows.permute(0, 3, 1, 2), wt, bias, dil)
    elif kind == "planes":
        xd, dt, wsrc, rx, rw, taps = K.split_planes(rows.view(M, Cin)).view(B, h, w, 2 * Cin), 2, K.pack_conv_weight(wt, 2), x, ws, None
        hi, lo = R.split_hi_lo(x)                                      # the planes ARE the split the bound is derived for
        both = np.concatenate([hi, lo], 1).transpose(0, 2, 3, 1).reshape(M, 2 * Cin)        # same values per row, layout opaque
        assert np.array_equal(np.sort(xd.view(M, 2 * Cin).float().cpu().numpy(), axis=1), np.sort(both, axis=1))
        assert np.array_equal(K.merge_planes(xd.view(M, 2 * Cin)).cpu().numpy(), (hi + lo).transpose(0, 2, 3, 1).reshape(M, Cin))
        wrapper = lambda: K.aspp2_fwd(xd.clone(), wt, bias, dil, planes=2)
    else:
        dt = HC.BF16 if kind == "bf16" else HC.FP16
        rx, rw = round16(x, kind), R.rounded_weights(ws, kind)
        xd, wsrc = rows.to(DT[kind]), K.pack_conv_weight(wt, dt)
        assert np.array_equal(xd.float().cpu().numpy(), rx.transpose(0, 2, 3, 1))
        taps = R.tap_magnitudes(rx, rw, dil) if kind == "fp16" else None
        wrapper = lambda: K.aspp2_fwd(xd.permute(0, 3, 1, 2), wt, bias, dil)
    ref, S = R.reference(rx, rw, bs, dil)["y"], R.magnitudes(rx, rw, bs, dil)["y"]
    item = xd.element_size()
    X = inb.inp("x", xd, rows_band(xd.shape[-1] * item))
    WS = inb.inp("wt", wsrc.contiguous().view(-1), rows_band(Cin * 4))
    BI = inb.inp("bias", bias, BAND)
    need = lib.hiast_aspp2_workspace_bytes(B, Cin, h, w, Cout, 0)
    assert need == M * NP * 4 + 256

    def fwd(nbytes):
        b = Bufs()
        y = b.out("y", (B, Cout, h, w), F32, BAND)
        wsb = b.out("workspace", (nbytes // 4,), F32, rows_band(NP * 4), must_fill=False)
        ok(HC.call(lib, "aspp2_fwd", x=X, dtype=dt, wt=WS, bias=BI, y=y, B=B, Cin=Cin, h=h, w=w, Cout=Cout, dil=dil, ws=wsb,
                   ws_bytes=nbytes, stream=_st()))
        b.check(inb)
        return dict(y=y)
    y = twice(lambda: fwd(need))["y"]
    inside("aspp2 y " + kind, y, ref, R.fwd2_bound(S, Cin, {"rows32": "fp32", "planes": "fp32"}.get(kind, kind), taps))
    assert _biteq(y, wrapper()), "the wrapper returns other bits"
    assert _biteq(y, fwd(need - 256)["y"]), "the documented slack of 256 bytes changes the result"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", NHWC, ids=_ids5)
def test_nhwc_backward(K, lib, case, fmt):
    B, Cin, h, w, Cout = case
    dil = DILS[NHWC.index(case) % 2]
    x, ws, bs, gy = R.aspp_inputs(1100 + Cout, B, Cin, h, w, Cout)
    inb = Bufs()
    _, wd, _ = nhwc_pack(K, lib, ws, bs, Cin, Cout, inb)
    NP, M, code = wd.shape[1], B * h * w, HC.BF16 if fmt == "bf16" else HC.FP16
    x16, w16, g16 = round16(x, fmt), R.rounded_weights(ws, fmt), round16(gy, fmt)
    ref, mag = R.reference(x16, w16, bs, dil, g16), R.magnitudes(x16, w16, bs, dil, g16)
    xd = dev(x16).to(DT[fmt]).permute(0, 2, 3, 1).contiguous()
    wdp = K.pack_conv_weight(wd, code)
    X, GY = inb.inp("x", xd, rows_band(Cin * 2)), inb.inp("dy", dev(gy), BAND)
    WD = inb.inp("wd", wdp.contiguous().view(-1), rows_band(NP * 2))
    need = lib.hiast_aspp2_workspace_bytes(B, Cin, h, w, Cout, 1)
    assert need % 4 == 0

    def bwd(want_dx, want_dw, nbytes=need):
        b = Bufs()
        o = {}
        if want_dx:
            o["dx"] = b.out("dx", (B, h, w, Cin), DT[fmt], rows_band(Cin * 2))
        if want_dw:
            o.update({"dw%d" % i: b.out("dw%d" % i, (Cout, Cin, 3, 3), F32, BAND) for i in range(4)})
            o["db"] = b.out("db", (Cout,), F32, BAND)
        wsb = b.out("workspace", (nbytes // 4,), F32, rows_band(NP * 4), must_fill=False)
        kw = dict(dx=None, dw0=None, dw1=None, dw2=None, dw3=None, db=None)
        kw.update(o)
        ok(HC.call(lib, "aspp2_bwd", x=X, dy=GY, wd=WD if want_dx else None, B=B, Cin=Cin, h=h, w=w, Cout=Cout, dil=dil, fmt=code,
                   ws=wsb, ws_bytes=nbytes, stream=_st(), **kw))
        b.check(inb)
        return o
    o = twice(lambda: bwd(True, True))
    inside("aspp2 dx " + fmt, o["dx"].permute(0, 3, 1, 2), ref["dx"], R.dx2_bound(ref["dx"], mag["dx"], Cout, fmt))
    for i in range(4):
        inside("aspp2 dW " + fmt, o["dw%d" % i], ref["dw"][i], R.dw2_bound(mag["dw"][i], M))
    db_ref = gy.astype(np.float64).sum((0, 2, 3))                       # the bias gradient sums the fp32 dy, not the rounded one
    inside("aspp2 db", o["db"], db_ref, R.db_bound(db_ref, gy))
    for name, part in (("dx only", bwd(True, False)), ("weights only", bwd(False, True)), ("256 bytes less", bwd(True, True, need - 256))):
        for n, t in part.items():
            assert _biteq(t, o[n]), "%s changes with %s" % (n, name)
    dxw, dws, db = K.aspp2_bwd(xd.permute(0, 3, 1, 2), dev(gy), wd, dil)
    assert _biteq(o["dx"], dxw.permute(0, 2, 3, 1)) and _biteq(o["db"], db) and all(_biteq(o["dw%d" % i], dws[i]) for i in range(4))


# ------------------------------------------------------------------------------------------------ upsample
UPS = [(1, 19, 5, 7, 5, 7), (1, 2, 3, 4, 100, 301), (2, 3, 9, 17, 65, 129), (1, 1, 4, 4, 1, 3), (1, 1, 1, 1, 8, 8)]


@pytest.mark.parametrize("shape", UPS, ids=lambda s: "x".join(map(str, s)))
def test_upsample(K, lib, shape):
    B, C, h, w, H, W = shape
    x, g = synth.normal_f32(1200, (B, C, h, w), 2.0), synth.normal_f32(1201, (B, C, H, W))
    inb = Bufs()
    X, G = inb.inp("x", dev(x), BAND), inb.inp("gout", dev(g), BAND)
    dims = dict(B=B, C=C, h=h, w=w, H=H, W=W, stream=_st())

    def fwd():
        b = Bufs()
        y = b.out("y", (B, C, H, W), F32, BAND)
        ok(HC.call(lib, "up_fwd", x=X, y=y, **dims))
        b.check(inb)
        return dict(y=y)
    y = twice(fwd)["y"]
    assert _biteq(y, K.upsample_bilinear_ac_fwd(dev(x), H, W)) and _biteq(y, dev(cref.upsample_bilinear_ac(x, H, W)))

    def bwd():
        b = Bufs()
        gin = b.out("gin", (B, C, h, w), F32, BAND)
        ok(HC.call(lib, "up_bwd", gout=G, gin=gin, **dims))
        b.check(inb)
        return dict(gin=gin)
    gin = twice(bwd)["gin"]
    ref = cref.upsample_bilinear_ac_bwd(g, h, w).astype(np.float64)
    S = cref.upsample_bilinear_ac_bwd(np.abs(g), h, w).astype(np.float64)
    inside("upsample gin", gin, ref, R.upsample_bwd_bound(ref, S, h, w, H, W))
    assert _biteq(gin, K.upsample_bilinear_ac_bwd(dev(g), h, w))


# ------------------------------------------------------------------------------------------------ pseudo-label pass 1
def _chosen_counts(seed, shape, dtype):
    """the values an accumulating output starts from"""
    return torch.from_numpy(synth.rng(seed).integers(0, 1000, size=shape)).to(dtype).cuda()


@pytest.mark.parametrize("scattered", [True, False], ids=["workspace", "no-workspace"])
@pytest.mark.parametrize("C", [19, 16, 9, 2])
@pytest.mark.parametrize("geom", [(1, 5, 7, 5, 7), (1, 3, 4, 100, 301), (2, 9, 17, 65, 129), (1, 2, 3, 130, 40)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pass1(K, lib, geom, C, scattered):
    """with a workspace the persistent form counts bands of up to 63 output rows; (1,2,3,130,40) has bands of 129 rows and takes
    the one-block-per-item form with the scattered histogram instead"""
    B, h, w, H, W = geom
    assert (65535 // (1024 * ((H - 1) // (h - 1) + 2)) == 0) == (geom == (1, 2, 3, 130, 40))
    z = synth.logits_lr(1300 + C, B, C, h, w, 3.0)
    if C > 5:
        z[:, 1, : h // 2] = z[:, 0, : h // 2]                           # ties: the lower index must win
    else:
        z[:, 1, : h // 2, ::2] = z[:, 0, : h // 2, ::2]
    mp_o, am_o = cref.plabel_stage_a(z, H, W)
    hist_o = torch.from_numpy(cref.plabel_hist(mp_o, am_o, C).view(np.int32)).cuda()
    assert int(hist_o.sum()) == B * H * W
    h0 = _chosen_counts(1301, (C, NBINS), I32)
    inb = Bufs()
    Z = inb.inp("logits", dev(z), BAND)
    nws = lib.hiast_plabel_pass1_workspace_bytes(C)
    assert nws == 256 * C * 61 * 4
    b = Bufs()
    o = dict(maxprob=b.out("maxprob", (B, H, W), F32, BAND), argmax=b.out("argmax", (B, H, W), U8, BAND))
    hist = b.out("hist", (C, NBINS), I32, BAND, init=h0)
    wsb = b.out("workspace", (nws // 4,), I32, BAND, must_fill=False) if scattered else None
    for launch in (1, 2):
        ok(HC.call(lib, "pass1", logits=Z, B=B, C=C, h=h, w=w, H=H, W=W, hist=hist, ws=wsb, ws_bytes=nws if scattered else 0,
                   stream=_st(), **o))
        b.check(inb)
        assert _biteq(hist, h0 + launch * hist_o), "hist after launch %d" % launch
        assert _biteq(o["argmax"], dev(am_o))
        if launch == 1:
            first = {n: t.clone() for n, t in o.items()}
            o["maxprob"].view(torch.uint8).fill_(GB.FILL)               # the second launch has to write everything again
            o["argmax"].fill_(GB.FILL)
    assert all(_biteq(first[n], o[n]) for n in o), "a second launch gives other bits"
    mp, am, hw_ = K.plabel_pass1(dev(z), H, W, hist=h0.clone())
    assert _biteq(o["maxprob"], mp) and _biteq(o["argmax"], am) and _biteq(hw_, h0 + hist_o)


# ------------------------------------------------------------------------------------------------ pseudo-label pass 2
def _pass2_case(K, lib, B, HW, C, with_thr, shift):
    """shift = 1: maxprob, argmax and plbl each start one element into their payload (the scalar path even at HW % 4 == 0)"""
    p, l = synth.probs_and_labels(1400 + C, B, 1, HW, C)
    l = l.astype(np.uint8)
    thr, thr_up = None, None
    if with_thr:
        thr = np.linspace(0.4, 0.97, C)
        t32 = thr.astype(np.float32)
        thr_up = np.where(t32.astype(np.float64) < thr, np.nextafter(t32, np.float32(np.inf)), t32).astype(np.float32)
    plbl_o, count_o, sfx_o = cref.plabel_select(p, l, thr, C)
    count_o, sfx_o = torch.from_numpy(count_o).cuda(), torch.from_numpy(sfx_o.view(np.int64)).cuda()
    n = B * HW
    inb = Bufs()
    MP = inb.out("maxprob", (n + shift,), F32, BAND, must_fill=False)
    AM = inb.out("argmax", (n + shift,), U8, BAND, must_fill=False)
    MP[shift:].copy_(dev(p).view(-1))
    AM[shift:].copy_(dev(l).view(-1))
    TH = inb.inp("thr", dev(thr_up), BAND) if with_thr else None
    c0, s0 = _chosen_counts(1401, (B, C), I64), _chosen_counts(1402, (C,), I64)
    b = Bufs()
    PL = b.out("plbl", (n + shift,), U8, BAND, must_fill=False)
    CN, SF = b.out("count", (B, C), I64, BAND, init=c0), b.out("sumprob", (C,), I64, BAND, init=s0)
    vec = shift == 0 and HW % 4 == 0
    assert (MP[shift:].data_ptr() % 16 == 0 and AM[shift:].data_ptr() % 4 == 0 and PL[shift:].data_ptr() % 4 == 0) == (shift == 0)
    for launch in (1, 2):
        ok(HC.call(lib, "pass2", maxprob=MP[shift:], argmax=AM[shift:], thr=TH, B=B, C=C, HW=HW, plbl=PL[shift:], count=CN, sumprob=SF,
                   stream=_st()))
        b.check(inb)
        assert torch.equal(PL[shift:].cpu(), torch.from_numpy(plbl_o).view(-1)), "plbl after launch %d" % launch
        assert shift == 0 or int(PL[0]) == GB.FILL, "the byte in front of plbl was written"
        assert _biteq(CN, c0 + launch * count_o) and _biteq(SF, s0 + launch * sfx_o), "count / sumprob_fx after launch %d" % launch
        PL.fill_(GB.FILL)
    wp, wc, wsf = K.plabel_pass2(dev(p), dev(l), TH.clone() if with_thr else None, C, count=c0.clone(), sumprob_fx=s0.clone())
    assert torch.equal(wp.cpu().view(-1), torch.from_numpy(plbl_o).view(-1)) and _biteq(wc, c0 + count_o) and _biteq(wsf, s0 + sfx_o)
    return vec


@pytest.mark.parametrize("with_thr", [True, False], ids=["thr", "no-thr"])
@pytest.mark.parametrize("C", [19, 2])
@pytest.mark.parametrize("HW,shift", [(21, 0), (8385, 0), (8192, 0), (8192, 1)])
def test_pass2(K, lib, HW, shift, C, with_thr):
    assert _pass2_case(K, lib, 3, HW, C, with_thr, shift) == ((HW, shift) == (8192, 0))


@pytest.mark.parametrize("HW,blocks,vec", [(1025 * 1025, 1027, False), (2048 * 2052, 1026, True)], ids=["scalar", "vector"])
def test_pass2_grid_cap(K, lib, HW, blocks, vec):
    """more than 1024 blocks of 4 x 256 (vectors of) pixels per image: the grid is capped and every block strides on"""
    assert -(-(HW // 4 if vec else HW) // 1024) == blocks > 1024
    assert _pass2_case(K, lib, 1, HW, 19, True, 0) == vec


# ------------------------------------------------------------------------------------------------ strided histogram
def strided_ref(p, l, C, interval, offset):
    """pseudo_label_generator.py:142-158 as a list formulation: per class every interval-th pixel in raster order"""
    hist, tot = np.zeros((C, NBINS), np.int64), np.zeros(C, np.int64)
    bins = p.astype(np.float16).view(np.uint16).astype(np.int64)
    for c in range(C):
        idx = np.nonzero(l == c)[0]
        tot[c] = idx.size
        keep = idx[(offset[c] + np.arange(idx.size)) % interval == 0]
        b = bins[keep]
        np.add.at(hist[c], b[b < NBINS], 1)
    return hist, tot


@pytest.mark.parametrize("C", [19, 2])
@pytest.mark.parametrize("N", [1, 4096, 4097, 3 * 4096 + 5])
def test_strided_hist(K, lib, N, C):
    p, l = synth.probs_and_labels(1500 + C, 1, 1, N, C)
    p, l = p.reshape(-1), l.reshape(-1).astype(np.uint8)
    inb = Bufs()
    MP, AM = inb.inp("maxprob", dev(p), BAND), inb.inp("argmax", dev(l), BAND)
    off = synth.rng(1501).integers(0, 10 ** 12, size=C)
    OFF = inb.inp("rank_offset", dev(off), BAND)
    nws = lib.hiast_plabel_strided_hist_workspace_bytes(N, C)
    assert nws == -(-N // 4096) * C * 4
    h0, t0 = _chosen_counts(1502, (C, NBINS), I32), _chosen_counts(1503, (C,), I64)
    for interval in (1, 3, 4):
        for full in (False, True):
            hist_o, tot_o = strided_ref(p, l, C, interval, off if full else np.zeros(C, np.int64))
            hist_o = torch.from_numpy(hist_o).to(I32).cuda()
            b = Bufs()
            hist = b.out("hist", (C, NBINS), I32, BAND, init=h0)
            tot = b.out("class_total", (C,), I64, BAND, init=t0) if full else None
            wsb = b.out("workspace", (nws // 4,), I32, BAND, must_fill=False)
            for launch in (1, 2):
                ok(HC.call(lib, "strided_hist", maxprob=MP, argmax=AM, N=N, C=C, interval=interval, rank_offset=OFF if full else None,
                           class_total=tot, hist=hist, ws=wsb, ws_bytes=nws, stream=_st()))
                b.check(inb)
                assert _biteq(hist, h0 + launch * hist_o), (interval, full, launch)
                assert tot is None or _biteq(tot, dev(tot_o)), "class_total is the batch's counts (overwritten)"
            got = K.plabel_strided_hist(dev(p), dev(l), C, interval, hist=h0.clone(), rank_offset=OFF.clone() if full else None,
                                        want_totals=full)
            assert _biteq(got[0] if full else got, h0 + hist_o) and (not full or _biteq(got[1], dev(tot_o)))


# ------------------------------------------------------------------------------------------------ fused test-time augmentation
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [19, 2])
def test_tta(K, lib, C, n, flip):
    B, H, W = 2, 33, 65
    sizes = [(17, 33), (49, 97), (33, 65)] if n == 3 else [[(17, 33), (49, 97)][int(flip)]]      # below, above, at the native size
    lows = [((Hs - 1) // 8 + 1, (Ws - 1) // 8 + 1) for Hs, Ws in sizes]
    zs = [synth.logits_lr(1600 + 10 * i + C, B, C, hs, ws_, 3.0) for i, (hs, ws_) in enumerate(lows)]
    zfs = [synth.logits_lr(1650 + 10 * i + C, B, C, hs, ws_, 3.0) for i, (hs, ws_) in enumerate(lows)] if flip else None
    probs_o, label_o = cref.tta(zs, zfs, sizes, H, W, want_probs=True)
    inb = Bufs()
    Z = [inb.inp("z%d" % i, dev(z), BAND) for i, z in enumerate(zs)]
    ZF = [inb.inp("zf%d" % i, dev(z), BAND) for i, z in enumerate(zfs)] if flip else None
    wprobs, wlabel = K.tta_fused([dev(z) for z in zs], [dev(z) for z in zfs] if flip else None, sizes, H, W, want_probs=True)
    assert torch.equal(wlabel.cpu(), torch.from_numpy(label_o))
    assert _biteq(wprobs, dev(probs_o)), "probsum is not the oracle's sum bit for bit"
    for want_p, want_l in ((True, False), (False, True), (True, True)):
        def run():
            b = Bufs()
            o = {}
            if want_p:
                o["probsum"] = b.out("probsum", (B, C, H, W), F32, BAND)
            if want_l:
                o["label"] = b.out("label", (B, H, W), U8, BAND)
            ok(HC.call(lib, "tta", z=Z, zf=ZF, hs=[s[0] for s in lows], wss=[s[1] for s in lows], Hs=[s[0] for s in sizes],
                       Ws=[s[1] for s in sizes], n_scales=n, B=B, C=C, H=H, W=W, probsum=o.get("probsum"), label=o.get("label"),
                       stream=_st()))
            b.check(inb)
            return o
        o = twice(run)
        assert not want_p or _biteq(o["probsum"], wprobs)
        assert not want_l or (_biteq(o["label"], wlabel) and torch.equal(o["label"].cpu(), torch.from_numpy(label_o)))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", list(HC.ENTRIES))
def test_refused_calls_write_nothing(lib, entry):
    """the refused calls of the host test on carved buffers: the code is the same and no byte of any buffer changes.  Every
    buffer holds 2 MiB, more than the largest tensor of the valid call the refusals start from."""
    b = Bufs()
    base = HC.placeholders(lib, entry)
    for n in HC.args_of(entry):
        if n in HC.POINTERS and n != "stream":
            base[n] = b.out(n, (2 << 20,), U8, 4096)
    if entry == "tta":
        base.update(z=[b.out("z0", (2 << 20,), U8, 4096)], zf=[b.out("zf0", (2 << 20,), U8, 4096)])
    base["stream"] = _st()
    assert HC.workspace_need(lib, entry, base) <= 2 << 20
    for what, change, code in HC.refused_calls(entry):
        got = HC.call(lib, entry, **HC.apply_change(lib, entry, base, change))
        assert got == code, (entry, what, got, code)
    b.untouched()


def test_zz_report_worst_ratios():
    """prints the worst error / bound per output class of this run; no assertion of its own"""
    for cls in sorted(WORST):
        print("head worst error/bound  %-28s %.4f" % (cls, WORST[cls]))
