"""Host side of the stem / pooling / packing / table tests (no GPU): the references of tests/stem_ref.py against torch in float64,
the error bounds against a float32 restatement of each bounded kernel's order (inside for the real order on every device
geometry, outside for named mutants on named geometries), the input conditions the device cases rely on, and the argument checks of
every entry of tests/stem_calls.py (refusals happen before any launch, so placeholder addresses are never dereferenced)."""
import numpy as np
import pytest
import torch

import stem_calls as SC
import stem_ref as R
import synth

F = torch.nn.functional


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ references vs torch float64
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("BHW", [(1, 1, 1), (1, 2, 3), (2, 9, 14), (1, 17, 25)], ids=str)
def test_stem_eval_ref_is_conv_bn_relu_maxpool(BHW, affine):
    x, w, gam, bet, mean, var = R.stem_eval_inputs(*BHW, with_affine=affine)
    for fmt in R.FMTS:
        want, bound = R.stem_eval_ref(x, w, gam, bet, mean, var, fmt)
        xo, wo = R.stem_operands(x, w, fmt)
        y = F.conv2d(_t(xo), _t(wo), None, 2, 3)
        y = F.batch_norm(y, _t(mean), _t(var), None if gam is None else _t(gam), None if bet is None else _t(bet), False, 0.0,
                         float(np.float32(R.EPS)))
        y = _nhwc(F.max_pool2d(torch.relu(y), 3, 2, 1))
        assert y.shape == want.shape == (BHW[0],) + R.conv_dims(*BHW[1:])[2:] + (64,)
        np.testing.assert_allclose(want, y, rtol=1e-12, atol=1e-13)
        assert (bound > 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("BHWC", [(1, 1, 1, 8), (1, 3, 3, 24), (2, 5, 4, 32), (2, 9, 14, 64)], ids=str)
def test_stem_tail_and_bn_infer_refs_are_bn_relu_maxpool(BHWC):
    B, H, W, C = BHWC
    gam, bet, mean, var = R.bn_vectors(C, 5)
    x = R.act_inputs(BHWC, "bf16", 6)
    bn = lambda: F.batch_norm(_nchw(x), _t(mean), _t(var), _t(gam), _t(bet), False, 0.0, float(np.float32(R.EPS)))
    want, _ = R.stem_tail_ref(x, "bf16", gam, bet, mean, var, "bf16")
    np.testing.assert_allclose(want, _nhwc(F.max_pool2d(torch.relu(bn()), 3, 2, 1)), rtol=1e-12, atol=1e-13)
    for relu in (0, 1):
        want, _ = R.bn_infer_ref(x.reshape(-1, C), gam, bet, mean, var, relu, "bf16")
        y = torch.relu(bn()) if relu else bn()
        np.testing.assert_allclose(want, _nhwc(y).reshape(-1, C), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("kind", ["smooth", "ties"])
@pytest.mark.parametrize("BHWC", R.POOL_SHAPES, ids=str)
def test_maxpool_ref_matches_torch(BHWC, kind):
    """values and window codes against F.max_pool2d(return_indices) (the first maximum in row-major order), the backward against
    autograd on gradients whose sums are exact in every type"""
    B, H, W, C = BHWC
    x = R.pool_input(BHWC, kind, "bf16", 3)
    m, code = R.maxpool_ref(x)
    y, ind = F.max_pool2d(_nchw(x), 3, 2, 1, return_indices=True)
    assert np.array_equal(m, _nhwc(y).astype(np.float32))
    Ho, Wo = m.shape[1:3]
    yo, xo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    flat = (2 * yo - 1)[None, :, :, None] * W + (2 * xo - 1)[None, :, :, None] + (code // 3).astype(np.int64) * W + code % 3
    assert np.array_equal(flat, _nhwc(ind))
    if kind == "ties":
        assert (np.diff(np.sort(x.reshape(-1, C), 0), axis=0) == 0).any() or x.size == C
    dy = synth.rng(4).integers(-8, 9, m.shape).astype(np.float32) / 8
    xt = _nchw(x).requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1).backward(_nchw(dy))
    got = R.dec16(R.maxpool_bwd_ref(dy, code, H, W, "bf16"), "bf16")
    assert np.array_equal(got, _nhwc(xt.grad).astype(np.float32))


def test_maxpool_ref_special_values():
    """a window of -inf keeps -inf with the code of its first in-image tap; a NaN takes the maximum and a LATER NaN the code"""
    x = np.full((1, 3, 3, 8), -np.inf, np.float32)
    m, code = R.maxpool_ref(x)
    assert np.isneginf(m).all() and (code[0, 0, 0] == 4).all() and (code[0, 0, 1] == 3).all() and (code[0, 1, 0] == 1).all() \
        and (code[0, 1, 1] == 0).all()
    x[0, 0, 0, 0], x[0, 1, 1, 0], x[0, 1, 0, 1] = np.nan, np.nan, 5.0
    m, code = R.maxpool_ref(x)
    assert np.isnan(m[0, 0, 0, 0]) and code[0, 0, 0, 0] == 8 and code[0, 1, 1, 0] == 0 and np.isnan(m[0, 1, 1, 0])
    assert m[0, 0, 0, 1] == 5.0 and code[0, 0, 0, 1] == 7 and np.isneginf(m[0, 0, 1, 1])


def test_split_and_pack_layouts():
    a = synth.normal_f32(7, (5, 96), 3.0)
    p = R.planes_of(a)
    hi = torch.from_numpy(a).bfloat16().float().numpy()
    lo = torch.from_numpy(a - hi).bfloat16().float().numpy()
    assert np.array_equal(R.bf16_val(p[:, 64:96]), hi[:, 32:64]) and np.array_equal(R.bf16_val(p[:, 96:128]), lo[:, 32:64])
    assert np.array_equal(R.merge_of(p), hi + lo) and np.abs(R.merge_of(p) - a).max() <= 2.0 ** -16 * np.abs(a).max()
    assert np.array_equal(R.fp16_bits(a), torch.from_numpy(a).half().view(torch.int16).numpy().view(np.uint16))
    # the special values of the device test, pinned from the integer arithmetic
    sp = np.array([0x00000000, 0x80000000, 0x00000001, 0x00018000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF], np.uint32).view(np.float32)
    h, l = R.split_bits(sp)
    assert h.tolist() == [0x0000, 0x8000, 0x0000, 0x0002, 0x7F80, 0xFF80, 0x7F7F]      # the largest finite value rounds UP to inf
    assert l.tolist()[:4] == [0x0000, 0x0000, 0x0000, 0x8000] and l.tolist()[4:6] == [0xFF80, 0x7F80] and l[6] == 0x7B00
    # the layout for every format and mode on a shape with a ragged 16-bit row and on a split-plane shape
    for fmt, (N, K, taps) in (("bf16", (5, 7, 4)), ("fp16", (5, 7, 4)), ("split", (32, 64, 3))):
        w = synth.normal_f32(8, (N, K, taps))
        PL = 2 if fmt == "split" else 1
        fwd, adj = R.pack_ref(w, fmt, 2)
        assert np.array_equal(R.pack_ref(w, fmt, 0)[0], fwd) and np.array_equal(R.pack_ref(w, fmt, 1)[0], adj)
        fwd, adj = fwd.reshape(N, taps, PL * K), adj.reshape(K, taps, PL * N)
        val = (lambda b: R.planes_value(b)) if fmt == "split" else (lambda b: R.dec16(b, fmt).astype(np.float64))
        want = R.planes_value(R.planes_of(w.reshape(1, -1))).reshape(w.shape) if fmt == "split" else val(R.enc16(w, fmt))
        assert np.array_equal(val(fwd), np.moveaxis(want, 2, 1))
        assert np.array_equal(val(adj), np.moveaxis(want, 0, 2)[:, ::-1, :].transpose(0, 1, 2))
    # finding 1: at K = 48 the lo halves of channels 32..47 land at 96..111 of a 96-element row
    (reach, size), _ = R.pack_reach(64, 48, 1, 2, 0)
    assert reach - size == 16 and R.pack_elem(0, 0, 47, 1, 48, 2) + 32 == 111
    with pytest.raises(AssertionError):
        R.pack_ref(synth.normal_f32(9, (64, 48, 1)), "split", 0)
    for what, ch in SC.split_pack_refusals():
        f, a = R.pack_reach(ch["N"], ch["K"], ch.get("taps", 9), 2, ch["transpose"])
        over = [r > s for (r, s), used in ((f, ch["transpose"] != 1), (a, ch["transpose"] != 0)) if used]
        assert any(over), what


def test_small_exact_references():
    img = synth.images_u8(1, 2, 3, 5).reshape(2, 15, 3)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    want = ((torch.from_numpy(img).float() / 255.0) - torch.tensor(mean)) / torch.tensor(std)
    assert np.array_equal(R.normalize_ref(img, mean, std), want.permute(0, 2, 1).numpy())
    e, p = synth.normal_f32(2, (1000,)), synth.normal_f32(3, (1000,))
    g = float(np.float32(0.999))
    want = torch.from_numpy(e) * g + torch.from_numpy(p) * float(np.float32(1 - 0.999))
    assert np.array_equal(R.ema_ref(e, p, 0.999, np.float32(1 - 0.999)), want.numpy())
    t = np.array([0, 1, 255, 255, 3, -1, 19, 2 ** 40, 5], np.int64)
    p = np.array([0, 2, 1, 255, 3, 1, 1, 2 ** 40, -1], np.int64)
    inter, ap, at = R.confusion_ref(p, t, 19)
    assert inter.sum() == 2 and inter[0] == 1 and inter[3] == 1 and ap[1] == 2 and ap.sum() == 5 and at.sum() == 4
    inter, ap, at = R.confusion_ref(p, t, 256)                            # 255 is a class here: ignored pixels count for it
    assert inter[255] == 2 and ap[255] == 2 and at[255] == 2 and at[19] == 1


# ------------------------------------------------------------------------------------------------ the bounds are not vacuous
def _ratio(got, want, bound):
    return float((np.abs(got - want) / bound).max())


def test_the_flags_the_bounds_rest_on():
    flags = R.assert_flags()
    assert "-O3" in flags


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("BHW", R.STEM_EVAL_SHAPES, ids=str)
def test_stem_eval_order_in_float32_stays_inside_the_bound(BHW, fmt):
    for affine in ((True, False) if BHW == (2, 9, 14) else (True,)):
        x, w, gam, bet, mean, var = R.stem_eval_inputs(*BHW, with_affine=affine)
        want, bound = R.stem_eval_ref(x, w, gam, bet, mean, var, fmt)
        got = R.stem_eval_f32(x, w, gam, bet, mean, var, fmt)
        assert got.shape == want.shape and _ratio(got, want, bound) <= 1.0, _ratio(got, want, bound)


# mutant -> (geometry, formats): every one lands outside the bound there
STEM_EVAL_MUTANTS = {
    "kx6": ((2, 9, 14), R.FMTS), "wrap": ((2, 9, 14), R.FMTS), "pool2p": ((1, 17, 25), R.FMTS),
    "keep_outside": ((1, 13, 21), R.FMTS), "no_lohi": ((1, 16, 24), ("split",)),
}


@pytest.mark.parametrize("mutant", list(STEM_EVAL_MUTANTS))
def test_stem_eval_mutants_fall_outside_the_bound(mutant):
    BHW, fmts = STEM_EVAL_MUTANTS[mutant]
    x, w, gam, bet, mean, var = R.stem_eval_inputs(*BHW)
    if mutant == "keep_outside":
        bet = bet.copy()
        bet[:16] = 3.0                  # a positive shift: relu(bn(partial window sum)) behind the border is well above 0 ...
        mean = mean.copy()
        mean[:16] = 0.0
    for fmt in fmts:
        want, bound = R.stem_eval_ref(x, w, gam, bet, mean, var, fmt)
        assert _ratio(R.stem_eval_f32(x, w, gam, bet, mean, var, fmt), want, bound) <= 1.0
        bad = R.stem_eval_f32(x, w, gam, bet, mean, var, fmt, mutant=mutant)
        r = np.abs(bad - want) / bound
        assert r.max() > 1.0, (mutant, fmt, float(r.max()))
        if mutant == "keep_outside":    # ... and only windows at a border can differ
            Hc, Wc, Hp, Wp = R.conv_dims(*BHW[1:])
            edge = lambda n, nc: (2 * np.arange(n) - 1 < 0) | (2 * np.arange(n) + 1 >= nc)
            inner = r[:, ~edge(Hp, Hc)][:, :, ~edge(Wp, Wc)]
            assert inner.size > 0 and inner.max() <= 1.0
        if mutant == "no_lohi":
            print("no_lohi worst error / bound %.2f" % r.max())


TAIL_PAIRS = [(i, o) for i in ("fp32", "bf16", "fp16") for o in R.FMTS]


@pytest.mark.parametrize("C", R.STEM_TAIL_C)
@pytest.mark.parametrize("BHW", R.STEM_TAIL_SHAPES, ids=str)
def test_stem_tail_and_bn_infer_order_in_float32_stay_inside_the_bound(BHW, C):
    gam, bet, mean, var = R.bn_vectors(C, 11 + C)
    for in_type, fmt in TAIL_PAIRS:
        if fmt == "split" and C % 32:
            continue
        x = R.act_inputs(BHW + (C,), in_type, 12)
        want, bound = R.stem_tail_ref(x, in_type, gam, bet, mean, var, fmt)
        assert _ratio(R.stem_tail_f32(x, in_type, gam, bet, mean, var, fmt), want, bound) <= 1.0, (in_type, fmt)
    for dtype in ("fp32", "bf16"):
        x = R.act_inputs(BHW + (C,), dtype, 13).reshape(-1, C)
        for relu in (0, 1):
            want, bound = R.bn_infer_ref(x, gam, bet, mean, var, relu, dtype)
            got = R.elem_f32(x, gam, bet, mean, var, relu)
            got = got if dtype == "fp32" else R.dec16(R.enc16(got, dtype), dtype)
            assert _ratio(got.astype(np.float64), want, bound) <= 1.0


@pytest.mark.parametrize("in_type,fmt", [("bf16", "bf16"), ("fp32", "fp16"), ("fp16", "bf16")])
def test_stem_tail_with_a_shifted_channel_group_falls_outside(in_type, fmt):
    """C = 24 (three channel groups) on (2, 5, 4): 36 thread items; from the 19th on — the second stride of a grid whose stride is
    no multiple of the three groups — a thread applies the next group's scale / shift"""
    BHW, C = (2, 5, 4), 24
    gam, bet, mean, var = R.bn_vectors(C, 11 + C)
    x = R.act_inputs(BHW + (C,), in_type, 12)
    want, bound = R.stem_tail_ref(x, in_type, gam, bet, mean, var, fmt)
    bad = R.stem_tail_f32(x, in_type, gam, bet, mean, var, fmt, group_shift_after=18)
    r = (np.abs(bad - want) / bound).reshape(-1, 3, 8)
    assert r[:6].max() <= 1.0 and r[6:].max() > 1.0


def test_bn_infer_mutants_fall_outside():
    M, C = 257, 40
    gam, bet, mean, var = R.bn_vectors(C, 21)
    x = R.act_inputs((M, C), "fp32", 22)
    want, bound = R.bn_infer_ref(x, gam, bet, mean, var, 1, "fp32")
    for name, bad in (("shift without mean", R.elem_f32(x, gam, bet, np.zeros(C, np.float32), var)),
                      ("eps inside the root dropped", R.elem_f32(x, gam, bet, mean, (var - np.float32(R.EPS)).astype(np.float32))),
                      ("channels of the next vector", R.elem_f32(x, np.roll(gam, -4), np.roll(bet, -4), np.roll(mean, -4),
                                                                  np.roll(var, -4)))):
        assert _ratio(bad.astype(np.float64), want, bound) > 1.0, name


def test_grid_rules():
    """the launch rules the device cases name their paths by"""
    assert R.stem_tail_grid(1, 3, 3, 24) == (1, 3, False) and R.stem_tail_grid(2, 37, 53, 96) == (49, 3, False)
    assert R.stem_tail_grid(2, 37, 53, 64)[1] == 1
    # the smallest pooled pixel counts past the cap: 3 groups -> 16384 * 256 / 3 + 1 pixels
    px = 16384 * 256 // 3 + 1
    assert -(-px * 3 // 256) == 16385 and R.stem_tail_grid(1, 2 * px - 1, 1, 24) == (16383, 3, True)
    assert R.stem_tail_grid(1, 2 * (16384 * 32 + 1) - 1, 1, 64) == (16384, 1, True)
    assert R.stem_tail_grid(1, 33, 33, 8 * 16385) is None
    assert R.bn_infer_grid(3, 24, "bf16") == (1, False) and R.bn_infer_grid(3, 24, "fp32") == (1, False)
    assert R.bn_infer_grid(4099, 64, "bf16") == (33, True) and R.bn_infer_grid(1025, 2048, "fp32")[1]
    assert R.stem_tiles(1, 33, 49) == 9 and R.stem_tiles(1, 16, 24) == 1 and R.stem_tiles(1, 17, 25) == 4 \
        and R.stem_tiles(1, 13, 21) == 1 and R.stem_tiles(1, 12, 21) == 1 and R.conv_dims(13, 21) == (7, 11, 4, 6) \
        and R.conv_dims(11, 21)[2] == 3


# ------------------------------------------------------------------------------------------------ input conditions
def test_input_conditions_of_the_device_cases():
    """what the device cases rely on: operands are values of their storage type, every activation is far below the fp16 range,
    variances are positive, the tie inputs hold ties and the special inputs hold -inf and NaN"""
    for BHW in R.STEM_EVAL_SHAPES:
        x, w, gam, bet, mean, var = R.stem_eval_inputs(*BHW)
        assert (var > 0.4).all() and np.isfinite(x).all() and np.isfinite(w).all()
        want, bound = R.stem_eval_ref(x, w, gam, bet, mean, var, "fp16")
        assert want.max() < 1000 and (bound < 0.01 * np.maximum(want, 1.0)).all()
    for C in R.STEM_TAIL_C:
        gam, bet, mean, var = R.bn_vectors(C, 11 + C)
        assert (var > 0.4).all()
        for t in ("fp32", "bf16", "fp16"):
            x = R.act_inputs((2, 37, 53, C), t, 12)
            assert np.array_equal(R.round16(x, t), x) and np.abs(x).max() < 64
            assert R.stem_tail_ref(x, t, gam, bet, mean, var, "fp16")[0].max() < 1000
    for shape in R.POOL_SHAPES:
        for fmt in ("bf16", "fp16"):
            x = R.pool_input(shape, "ties", fmt, 3)
            assert np.array_equal(R.dec16(R.enc16(x, fmt), fmt), x)
            if shape[1] * shape[2] > 2:
                m, code = R.maxpool_ref(x)
                assert len(np.unique(x)) < 20
            s = R.pool_input(shape, "special", fmt, 3)
            if s.size >= 64:
                assert np.isnan(s).any() and np.isneginf(s).any()


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
@pytest.mark.parametrize("entry", list(SC.ENTRIES))
def test_entries_refuse_bad_arguments_before_any_launch(lib, entry):
    base = SC.placeholders(entry)
    calls = SC.refused_calls(entry)
    assert len(calls) >= 3
    for what, change, code in calls:
        got = SC.call(lib, entry, **SC.apply_change(base, change))
        assert got == code, (entry, what, got, code)


def test_pack_conv_weight_refuses_ragged_split_plane_slabs(lib):
    """finding 1 of DESIGN §2.4: every shape whose layout would leave wp / wpt is refused with HIAST_E_RANGE before any launch"""
    base = SC.placeholders("pack")
    for what, ch in SC.split_pack_refusals():
        assert SC.call(lib, "pack", **dict(base, fmt=SC.SPLIT, **ch)) == SC.E_RANGE, what
