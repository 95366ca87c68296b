"""Host side of the head tests (no GPU): the float64 references of tests/head_ref.py against torch float64 in an independent
formulation (33 shifted 1x1 products; F.interpolate autograd for the upsample adjoint), the error bounds against a float32
restatement of each kernel's summation order (inside for the real order; outside once a tap is dropped, its sign flipped, or a
border tap read from the opposite side of the image), and the argument checks of every head / pseudo-label entry (refusals happen
before any launch, so placeholder addresses are never dereferenced)."""
import numpy as np
import pytest
import torch

import head_calls as HC
import head_ref as R
import synth
from bn_ref import round16
from oracle import cref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


SMALL = (1, 64, 9, 17, 19)
DILS = [(1, 2, 3, 5), (6, 12, 18, 24)]
MUTS = [("drop", 1), ("flip", 1), ("wrap", 1), ("drop", 20), ("wrap", 32)]


def _inside(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


def _outside(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert (err > bound).any(), (what, float((err / np.maximum(bound, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("dil", DILS)
def test_conv_reference_equals_33_shifted_products(dil):
    """the tap list, the packed weights and the zero-padded shift every restatement uses give the four float64 convolutions"""
    B, Cin, h, w, Cout = 2, 8, 9, 17, 5
    x, ws, bs, gy = R.aspp_inputs(1, B, Cin, h, w, Cout)
    ref = R.reference(x, ws, bs, dil, gy)
    w64 = [v.astype(np.float64) for v in ws]
    Wp = R.pack_taps(w64, centre=sum(v[:, :, 1, 1] for v in w64))
    x64, g64 = x.astype(np.float64), gy.astype(np.float64)
    y = sum(b.astype(np.float64) for b in bs)[None, :, None, None] + sum(
        R.shifted(np.einsum("bchw,oc->bohw", x64, Wp[t]), oy, ox) for t, (oy, ox) in enumerate(R.taps_of(dil)))
    np.testing.assert_allclose(y, ref["y"], rtol=1e-12, atol=1e-13)
    dx = sum(np.einsum("bohw,oc->bchw", R.shifted(g64, -oy, -ox), Wp[t]) for t, (oy, ox) in enumerate(R.taps_of(dil)))
    np.testing.assert_allclose(dx, ref["dx"], rtol=1e-12, atol=1e-13)
    P = np.stack([np.einsum("bohw,bchw->oc", g64, R.shifted(x64, oy, ox)) for oy, ox in R.taps_of(dil)])
    for got, want in zip(R._unpack_dw(P, Cout, Cin), ref["dw"]):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g64.sum((0, 2, 3)), ref["db"], rtol=1e-13)
    mag = R.magnitudes(x, ws, bs, dil, gy)
    assert all((np.abs(ref[k]) <= mag[k] * (1 + 1e-12)).all() for k in ("y", "dx", "db"))
    assert len(R.taps_of(dil)) == 33 and len(set(R.taps_of(dil))) == 33


def test_rounded_weights_are_values_of_the_type_and_keep_one_centre():
    _, ws, _, _ = R.aspp_inputs(2, 1, 8, 3, 3, 5)
    for fmt, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        r = R.rounded_weights(ws, fmt)
        for v in r:
            assert np.array_equal(torch.from_numpy(v).to(dt).float().numpy(), v)
        assert np.array_equal(r[0][:, :, 1, 1], round16(R.centre_sum(ws), fmt)) and not r[1][:, :, 1, 1].any()
        assert np.array_equal(r[2][:, :, 0, 2], round16(ws[2][:, :, 0, 2], fmt))
    hi, lo = R.split_hi_lo(ws[0])
    assert (np.abs(ws[0].astype(np.float64) - hi - lo) <= 2.0 ** -16 * np.abs(ws[0])).all()
    assert (np.abs(lo) <= 2.0 ** -8 * (1 + 2.0 ** -8) * np.abs(ws[0])).all()


@pytest.mark.parametrize("shape", [(1, 3, 5, 7, 5, 7), (1, 2, 3, 4, 20, 31), (2, 3, 9, 17, 65, 129), (1, 1, 4, 4, 1, 3),
                                   (1, 1, 1, 1, 8, 8)])
def test_upsample_adjoint_reference_and_bound(shape):
    B, C, h, w, H, W = shape
    g = synth.normal_f32(3, (B, C, H, W))
    ref = cref.upsample_bilinear_ac_bwd(g, h, w).astype(np.float64)
    S = cref.upsample_bilinear_ac_bwd(np.abs(g), h, w).astype(np.float64)
    f64 = R.upsample_bwd_f64(g, h, w)
    assert (np.abs(f64 - ref) <= R.U32 * np.abs(ref) + 1e-15 * S).all()            # the reference's float32 output, nothing else
    if H > 1 and W > 1:
        xt = torch.zeros((B, C, h, w), dtype=torch.float64, requires_grad=True)
        torch.nn.functional.interpolate(xt, size=(H, W), mode="bilinear", align_corners=True).backward(torch.from_numpy(g).double())
        assert (np.abs(xt.grad.numpy() - f64) <= 4 * max(H, W) * R.U32 * S + 1e-12).all()    # fp32 lerp weights against float64 ones
    bound = R.upsample_bwd_bound(ref, S, h, w, H, W)
    _inside(R.upsample_bwd_f32(g, h, w), ref, bound, "kernel order")
    if H > 1:
        _outside(R.upsample_bwd_f32(g, h, w, drop_row=H // 2), ref, bound, "a dropped output row")
    # the band limits the bound counts with are upper limits of the kernel's Xb - Xa / Yb - Ya: cells with a non-zero weight
    nY, nX = R.upsample_terms(h, w, H, W)
    assert (R.lerp_matrix(h, H) != 0).sum(0).max() <= nY and (R.lerp_matrix(w, W) != 0).sum(0).max() <= nX


# ------------------------------------------------------------------------------------------------ direct form
def _mutants(run, ref, bound, what):
    for mut in MUTS:
        _outside(run(mut), ref, bound, (what,) + mut)


@pytest.mark.parametrize("case", [(1, 64, 9, 17, 19, 0), (1, 128, 9, 17, 20, 1), (1, 64, 7, 3, 16, 0)])
def test_direct_forward_order_stays_inside_its_bound(case):
    B, Cin, h, w, Cout, di = case
    dil = DILS[di]
    x, ws, bs, _ = R.aspp_inputs(4, B, Cin, h, w, Cout)
    ref, S = R.reference(x, ws, bs, dil)["y"], R.magnitudes(x, ws, bs, dil)["y"]
    k = HC.aspp_splitk(B, Cin, h, w, Cout)
    assert k == (2 if Cin == 128 else 1)
    bound = R.fwd_bound(S, B, Cin, h, w, Cout)
    _inside(R.aspp_fwd_f32(x, ws, bs, dil, k), ref, bound, "kernel order")
    if (h, w) == (9, 17) and di == 0:
        _mutants(lambda m: R.aspp_fwd_f32(x, ws, bs, dil, k, m), ref, bound, "fwd")


def test_direct_bwd_data_order_stays_inside_its_bound():
    B, Cin, h, w, Cout = 1, 256, 9, 17, 19
    dil = DILS[0]
    x, ws, bs, gy = R.aspp_inputs(5, B, Cin, h, w, Cout)
    ref, S = R.reference(x, ws, bs, dil, gy)["dx"], R.magnitudes(x, ws, bs, dil, gy)["dx"]
    bound = R.bwd_data_bound(S, Cout)
    _inside(R.aspp_bwd_data_f32(gy, ws, dil), ref, bound, "kernel order")
    _mutants(lambda m: R.aspp_bwd_data_f32(gy, ws, dil, m), ref, bound, "bwd_data")


@pytest.mark.parametrize("case", [(1, 64, 9, 17, 19, 1), (1, 64, 20, 70, 9, 2)])
def test_direct_bwd_weight_order_stays_inside_its_bound(case):
    B, Cin, h, w, Cout, nsplit = case
    dil = DILS[0]
    assert HC.aspp_wgrad_nsplit(B, h, w) == nsplit
    x, ws, bs, gy = R.aspp_inputs(6, B, Cin, h, w, Cout)
    ref, mag = R.reference(x, ws, bs, dil, gy), R.magnitudes(x, ws, bs, dil, gy)
    bounds = [R.bwd_weight_bound(S, B, h, w) for S in mag["dw"]]
    got = R.aspp_bwd_weight_f32(x, gy, dil)
    for i in range(4):
        _inside(got[i], ref["dw"][i], bounds[i], "dw%d" % i)
    assert (np.abs(np.float32(ref["db"]) - ref["db"]) <= R.db_bound(ref["db"], gy)).all()
    if nsplit == 1:
        for mut in MUTS:                                     # taps 1 and 20 and 32 belong to branches 0, 2 and 3
            bad = R.aspp_bwd_weight_f32(x, gy, dil, mut)
            i = 0 if mut[1] == 0 else (mut[1] - 1) // 8
            _outside(bad[i], ref["dw"][i], bounds[i], ("dw",) + mut)


# ------------------------------------------------------------------------------------------------ GEMM + shift-add form
@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_nhwc_forward_order_stays_inside_its_bound(kind):
    B, Cin, h, w, Cout = 1, 128, 9, 17, 19
    dil = DILS[0]
    x, ws, bs, _ = R.aspp_inputs(7, B, Cin, h, w, Cout)
    if kind == "fp32":
        xo, wo = R.split_hi_lo(x), R.split_hi_lo(R.pack_taps(ws))
        rx, rw, taps = x, ws, None
    else:
        rx, rw = round16(x, kind), R.rounded_weights(ws, kind)
        xo, wo = (rx,), (R.pack_taps(rw, centre=rw[0][:, :, 1, 1]),)
        taps = R.tap_magnitudes(rx, rw, dil) if kind == "fp16" else None
    ref, S = R.reference(rx, rw, bs, dil)["y"], R.magnitudes(rx, rw, bs, dil)["y"]
    bound = R.fwd2_bound(S, Cin, kind, taps)
    run = lambda m=None: R.aspp2_fwd_f32(xo, wo, bs, dil, kind == "fp16", m)
    _inside(run(), ref, bound, "kernel order")
    _mutants(run, ref, bound, "aspp2 fwd " + kind)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_nhwc_backward_order_stays_inside_its_bounds(fmt):
    B, Cin, h, w, Cout = 1, 128, 9, 17, 19
    dil = DILS[0]
    x, ws, bs, gy = R.aspp_inputs(8, B, Cin, h, w, Cout)
    x16, w16, g16 = round16(x, fmt), R.rounded_weights(ws, fmt), round16(gy, fmt)
    ref, mag = R.reference(x16, w16, bs, dil, g16), R.magnitudes(x16, w16, bs, dil, g16)
    bdx = R.dx2_bound(ref["dx"], mag["dx"], Cout, fmt)
    _inside(R.aspp2_bwd_dx_f32(g16, w16, dil, fmt), ref["dx"], bdx, "dx order")
    _mutants(lambda m: R.aspp2_bwd_dx_f32(g16, w16, dil, fmt, m), ref["dx"], bdx, "aspp2 dx " + fmt)
    bdw = [R.dw2_bound(S, B * h * w) for S in mag["dw"]]
    got = R.aspp2_bwd_dw_f32(x16, g16, dil)
    for i in range(4):
        _inside(got[i], ref["dw"][i], bdw[i], "dw%d" % i)
    for mut in MUTS:
        bad = R.aspp2_bwd_dw_f32(x16, g16, dil, mut)
        i = (mut[1] - 1) // 8
        _outside(bad[i], ref["dw"][i], bdw[i], ("aspp2 dw", fmt) + mut)


def test_split_arithmetic():
    assert R.wgrad2_nsplit(2800) == 2 and R.wgrad2_rows(2800) == 1408 and R.wgrad2_nsplit(2048) == 2 and R.wgrad2_rows(2048) == 1024
    assert R.wgrad2_nsplit(153) == 1 and R.wgrad2_rows(153) == 160
    assert HC.aspp_wgrad_nsplit(1, 20, 70) == 2 and HC.aspp_wgrad_nsplit(2, 32, 128) == 16 and HC.aspp_wgrad_nsplit(1, 7, 3) == 1
    assert [HC.aspp_splitk(1, c, 9, 17, 19) for c in (64, 128, 256, 2048)] == [1, 2, 4, 8]
    assert HC.aspp_splitk(1, 4096, 256, 513, 19) == 2


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
@pytest.mark.parametrize("entry", list(HC.ENTRIES))
def test_entries_refuse_bad_arguments_before_any_launch(lib, entry, monkeypatch):
    monkeypatch.delenv("HIAST_ASPP_SPLITK", raising=False)
    monkeypatch.delenv("HIAST_ASPP_WG_NTILE", raising=False)
    base = HC.placeholders(lib, entry)
    calls = HC.refused_calls(entry)
    assert len(calls) >= 4
    for what, change, code in calls:
        got = HC.call(lib, entry, **HC.apply_change(lib, entry, base, change))
        assert got == code, (entry, what, got, code)


def test_image_above_2_gib_is_a_range_error_of_the_narrow_forward_only(lib, monkeypatch):
    """4096 x 256 x 513 fp32 is 2.004 GiB: beyond the 32-bit byte offsets of the 16-row kernel (Cout <= 19), inside what the
    32-row kernel addresses (Cout 20: refused for its missing split-K workspace instead); one pixel row less fits"""
    monkeypatch.delenv("HIAST_ASPP_SPLITK", raising=False)
    base = HC.placeholders(lib, "aspp_fwd")
    big = dict(B=1, Cin=4096, h=256, w=513, ws=None, ws_bytes=0)
    assert HC.call(lib, "aspp_fwd", **dict(base, Cout=19, **big)) == HC.E_RANGE
    assert HC.call(lib, "aspp_fwd", **dict(base, Cout=16, **big)) == HC.E_RANGE
    assert HC.call(lib, "aspp_fwd", **dict(base, Cout=20, **big)) == HC.E_WS
    assert HC.call(lib, "aspp_fwd", **dict(base, Cout=19, **dict(big, h=256, w=512))) == HC.E_WS       # exactly 2 GiB: addressable
    assert 4096 * 256 * 513 * 4 > 2 ** 31 == 4096 * 256 * 512 * 4


def test_workspace_sizes_cover_what_the_entries_use(lib):
    for B, Cin, h, w, Cout in [(1, 64, 9, 17, 19), (3, 64, 9, 17, 2), (2, 256, 32, 128, 32), (1, 128, 20, 70, 17)]:
        need = lib.hiast_aspp_workspace_bytes(B, Cin, h, w, Cout)
        kw = dict(B=B, Cin=Cin, h=h, w=w, Cout=Cout)
        assert need >= HC.used_bytes("splitk", kw) and need >= HC.used_bytes("wgrad", kw)
    for Cout, NP in ((2, 128), (9, 384), (16, 640), (19, 640), (32, 1152)):
        assert lib.hiast_aspp2_np(Cout) == NP
        M = 2 * 20 * 70
        assert lib.hiast_aspp2_workspace_bytes(2, 128, 20, 70, Cout, 0) == M * NP * 4 + 256
        g = -(-M * NP * 2 // 256) * 256
        assert lib.hiast_aspp2_workspace_bytes(2, 128, 20, 70, Cout, 1) == max(M * NP * 4, g + R.wgrad2_nsplit(M) * NP * 128 * 4) + 256
