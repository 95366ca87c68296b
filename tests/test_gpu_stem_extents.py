"""The stem, pooling, packing and table entries (stem.hip, igemm.hip, conv1x1.hip, misc.hip) through the C ABI (tests/stem_calls.py)
on buffers carved out of 0xFF-filled allocations (tests/guard_bands.py), against the references and bounds of tests/stem_ref.py.
Inputs sit in poison (0xFF.. is a NaN in every float type), outputs start as 0xFF; every per-channel vector, table, chunk array and
idx map is carved too.  After each launch:
  1. both guard bands of every buffer, inputs included, are untouched;
  2. every output payload is fully written, and finite where it is floating point;
  3. the values are bit-equal to the exact reference, or inside the derived bound;
  4. the payload is bit-equal to what the K.* wrapper returns for the same operands;
  5. a second launch gives the same bits (hiast_confusion_hist: counters that start from chosen values are exactly doubled).
A refused call writes nothing.  A band (64 KiB; 256 bytes for vectors and tables) holds more than one block's reach: 256 threads
x 16 bytes of output, a 4 x 6 x 128 pooled tile of hiast_stem_eval, nine input rows of the shapes below.

entry                              test                                            cases
hiast_stem_eval                    test_stem_eval, _null_affine, _persistent_walk,  3 formats x (1,1,1) (1,2,3) (2,9,14) (1,16,24: one
                                   _special_values                                 full 4x6 tile) (1,17,25: one row / column into the next
                                                                                   tile) (1,13,21: smallest image with a 4x6 map) (2,67,101);
                                                                                   B x 33x49 with ntiles > 2 x blocks; NaN / +-inf pixels
hiast_stem_tail                    test_stem_tail, _null_affine, _capped_walk,      3 inputs x 3 formats x C in 8 24 32 64 96 x (1,1,1) (1,3,3)
                                   _special_values                                 (2,5,4) (2,37,53); C = 24 and 64 one block past the cap
hiast_bn_act_nhwc_infer            test_bn_infer, _capped, _special_values          fp32 / bf16 x relu x (1,8) (3,24: fallback path) (257,40)
                                                                                   (4099,64) (1025,2048); C = 24 one block past the cap
hiast_maxpool3x3s2_nhwc_fwd, _bwd  test_maxpool, test_maxpool_capped                bf16 / fp16 x smooth / ties / -inf, NaN x 6 shapes
hiast_split_planes                 test_split_planes, _special_values               both directions, C in 32 96 2048 x M in 1 3 4099, M = 8193
hiast_pack_conv_weight             test_pack_conv_weight, _misaligned_falls_back,   3 tiled + 6 elementwise shapes x 3 formats x 3 modes
                                   _refuses_ragged_split_slabs
hiast_pack_conv_weight_multi       test_pack_conv_weight_multi                     3 formats x modes 0, 2 x (1-tap, 9-tap, mixed) launches
hiast_normalize_u8                 test_normalize_u8                               HW in 1 3 1023 262145 1048579 x B in 1 3, odd img address
hiast_ema_update, hiast_multi_copy test_ema_update, test_multi_copy                 7 sizes, each alignment path, every tensor carved alone
hiast_confusion_hist               test_confusion_hist                             K in 1 19 256 1024 x N in 1 4096 4097 8388609
argument checks of all of them     test_refused_calls_write_nothing

NOT covered: extents past 2^31 elements (the 2^40 limits are host refusals only), a CU reserve other than 0."""
import ctypes
import types

import numpy as np
import pytest
import torch

import guard_bands as GB
import stem_calls as SC
import stem_ref as R
import synth
from test_gpu_bn_extents import Bufs, _biteq, _st
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

WORST = {}                           # entry and format -> worst error / bound seen in this run (test_zz_report_worst_ratios)
BAND, VBAND = 64 << 10, 256
F32, U8, I64 = torch.float32, torch.uint8, torch.int64
T16 = {"bf16": torch.bfloat16, "fp16": torch.float16, "split": torch.bfloat16, "fp32": F32}
EPS32 = float(np.float32(R.EPS))
_REFS = {}


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
def _free_between_cases():
    yield
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ plumbing
def bits(t):
    """a 16-bit device tensor -> numpy uint16"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def as16(a, fmt):
    """float32 numpy holding values of the 16-bit type -> device tensor of that type"""
    return dev(np.ascontiguousarray(a, np.float32)).to(T16[fmt])


def inside(cls, got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(err).all(), cls
    ratio = float((err / bound).max())
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    assert ratio <= 1.0, "%s: %d element(s) outside the bound, worst error / bound = %.3f" % (cls, int((err > bound).sum()), ratio)


def cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


class BN:
    """carved BatchNorm vectors and the module-like object the K.* wrappers take"""

    def __init__(self, bufs, C, seed, affine=True):
        self.np = R.bn_vectors(C, seed, affine)
        gam, bet, mean, var = self.np
        put = lambda n, v: None if v is None else bufs.inp(n, dev(v), VBAND)
        self.gamma, self.beta, self.mean, self.var = put("gamma", gam), put("beta", bet), put("mean", mean), put("var", var)
        self.module = types.SimpleNamespace(weight=self.gamma, bias=self.beta, running_mean=self.mean, running_var=self.var, eps=R.EPS)

    def kw(self):
        return dict(gamma=self.gamma, beta=self.beta, mean=self.mean, var=self.var, eps=EPS32)


def twice(launch, outs, bufs, *more):
    """launch() twice into the same buffers; bands, finiteness, same bits"""
    first = None
    for _ in range(2):
        assert launch() == 0
        bufs.check(*more)
        if first is None:
            first = [o.clone() for o in outs]
    for a, b in zip(first, outs):
        assert _biteq(a, b), "a second launch gives other bits"


def check_special(cls, got_bits, fmt, want, bound):
    """outputs of inputs that hold NaN / inf against the float64 torch result: NaN where it has one, +inf where it has one (a NaN
    in split planes, whose lo half of an infinity is inf - inf), the bound elsewhere"""
    got = R.out_value(got_bits, fmt)
    nan_want = np.isnan(want) | (np.isinf(want) if fmt == "split" else False)
    assert np.array_equal(np.isnan(got), nan_want), "%s: %d NaN where the reference has none, %d missing" % (
        cls, int((np.isnan(got) & ~nan_want).sum()), int((~np.isnan(got) & nan_want).sum()))
    inf = np.isinf(want) & ~nan_want
    assert np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    assert fin.any() and nan_want.any()
    assert (np.abs(got[fin] - want[fin]) <= bound[fin]).all(), cls


# ------------------------------------------------------------------------------------------------ hiast_stem_eval
def _stem_eval_ref(BHW, fmt, affine=True, seed=0):
    def make():
        inp = R.stem_eval_inputs(*BHW, seed=seed, with_affine=affine)
        return inp, R.stem_eval_ref(*inp, fmt)
    return cached(("stem_eval", BHW, fmt, affine, seed), make)


def _run_stem_eval(K, lib, BHW, fmt, affine=True, x=None, special=False):
    B, H, W = BHW
    (x0, w, gam, bet, mean, var), (want, bound) = _stem_eval_ref(BHW, fmt, affine)
    x0 = x0 if x is None else x
    _, _, Hp, Wp = R.conv_dims(H, W)
    PL = 2 if fmt == "split" else 1
    inb = Bufs()
    X, Wt = inb.inp("x", dev(x0), BAND), inb.inp("w", dev(w), BAND)
    bn = BN(inb, 64, 1000 * 0 + 7 * H + W + B + 2, affine)
    assert all(a is b or np.array_equal(a, b) for a, b in zip(bn.np, (gam, bet, mean, var)))
    ob = Bufs()
    out = ob.out("out", (B, Hp, Wp, PL * 64), T16[fmt], BAND, must_fill=not special)
    launch = lambda: SC.call(lib, "stem_eval", x=X, w=Wt, out=out, fmt=SC.FMT[fmt], B=B, H=H, W=W, stream=_st(), **bn.kw())
    twice(launch, [out], ob, inb)
    assert _biteq(out, K.stem_eval(X, Wt, bn.module, SC.FMT[fmt])), "K.stem_eval returns other bits"
    if not special:
        inside("stem_eval " + fmt, R.out_value(bits(out), fmt), want, bound)
    return bits(out), bound


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("BHW", R.STEM_EVAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_eval(K, lib, BHW, fmt):
    _run_stem_eval(K, lib, BHW, fmt)


@pytest.mark.parametrize("fmt", R.FMTS)
def test_stem_eval_null_affine(K, lib, fmt):
    _run_stem_eval(K, lib, (2, 9, 14), fmt, affine=False)


@pytest.mark.parametrize("fmt", R.FMTS)
def test_stem_eval_persistent_walk(K, lib, fmt):
    """B images of 33 x 49 (9 tiles each) with more than twice as many tiles as blocks: a block walks three tiles, so both input
    buffers are reused (it & 1) and the last prefetch reaches past ntiles"""
    cus = lib.hiast_device_cus()
    assert cus >= 8 and lib.hiast_get_reserve_cus() == 0
    cap = (1 if fmt == "split" else 2) * cus
    B = 2 * cap // 9 + 1
    ntiles = R.stem_tiles(B, 33, 49)
    assert ntiles == 9 * B > 2 * cap and R.stem_eval_blocks(ntiles, cus, fmt) == cap
    _run_stem_eval(K, lib, (B, 33, 49), fmt)


@pytest.mark.parametrize("fmt", R.FMTS)
def test_stem_eval_special_values(K, lib, fmt):
    """a few NaN / +-inf pixels, at even and odd columns (the input column right of an output's 7-wide window meets a zero weight
    in the kernel's 8-pixel fragment and must not leak), against conv2d -> batch_norm -> relu -> max_pool2d in float64.  Split
    planes hold an infinity as (inf, NaN): there an infinite pixel counts as a NaN pixel."""
    BHW = (2, 33, 49)
    (x0, w, gam, bet, mean, var), (_, bound) = _stem_eval_ref(BHW, fmt)
    x = x0.copy()
    x[0, 1, 4, 6] = np.nan
    x[0, 0, 20, 31] = np.inf
    x[1, 2, 9, 40] = -np.inf
    x[1, 0, 32, 48] = np.nan
    x[1, 1, 0, 0] = np.inf
    xo, wo = R.stem_operands(np.where(np.isinf(x), np.nan, x) if fmt == "split" else x, w, fmt)
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    y = F.batch_norm(F.conv2d(t(xo), t(wo), None, 2, 3), t(mean), t(var), t(gam), t(bet), False, 0.0, EPS32)
    want = F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    got, _ = _run_stem_eval(K, lib, BHW, fmt, x=x, special=True)
    check_special("stem_eval " + fmt, got, fmt, want, bound)


# ------------------------------------------------------------------------------------------------ hiast_stem_tail
def _tail_launch(lib, X, in_type, bn, out, fmt, B, H, W, C):
    return SC.call(lib, "stem_tail", x=X, dtype=SC.DTYPE[in_type], out=out, fmt=SC.FMT[fmt], B=B, H=H, W=W, C=C, stream=_st(), **bn.kw())


def _run_stem_tail(K, lib, BHW, C, in_type, fmt, affine=True, x=None, special=False):
    B, H, W = BHW
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x0 = R.act_inputs(BHW + (C,), in_type, 12) if x is None else x
    inb = Bufs()
    X = inb.inp("x", as16(x0, in_type), BAND)
    bn = BN(inb, C, 11 + C, affine)
    ob = Bufs()
    out = ob.out("out", (B, Ho, Wo, (2 if fmt == "split" else 1) * C), T16[fmt], BAND, must_fill=not special)
    twice(lambda: _tail_launch(lib, X, in_type, bn, out, fmt, B, H, W, C), [out], ob, inb)
    assert _biteq(out, K.stem_tail(X.permute(0, 3, 1, 2), bn.module, SC.FMT[fmt])), "K.stem_tail returns other bits"
    if not special:
        want, bound = R.stem_tail_ref(x0, in_type, *bn.np, fmt)
        inside("stem_tail %s -> %s" % (in_type, fmt), R.out_value(bits(out), fmt), want, bound)
    return bits(out), bn


@pytest.mark.parametrize("C", R.STEM_TAIL_C)
@pytest.mark.parametrize("BHW", R.STEM_TAIL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_tail(K, lib, BHW, C):
    """every input type x output format; C = 24 and 96 have need = 3: the small ones run in one pass whatever nb is (finding 2)"""
    grid = R.stem_tail_grid(*BHW, C)
    assert grid is not None and not grid[2] and grid[1] == (3 if C in (24, 96) else 1)
    for in_type in ("fp32", "bf16", "fp16"):
        for fmt in R.FMTS:
            if fmt == "split" and C % 32:
                continue
            _run_stem_tail(K, lib, BHW, C, in_type, fmt)


def test_stem_tail_null_affine(K, lib):
    for in_type, fmt in (("fp32", "split"), ("bf16", "bf16"), ("fp16", "fp16")):
        _run_stem_tail(K, lib, (2, 5, 4), 32, in_type, fmt, affine=False)


@pytest.mark.parametrize("in_type,fmt", [("fp32", "bf16"), ("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "split"), ("fp32", "fp16")])
def test_stem_tail_special_values(K, lib, in_type, fmt):
    """NaN and +-inf activations against batch_norm -> relu -> max_pool2d in float64: a NaN passes the ReLU and takes the maximum"""
    BHW, C = (2, 9, 14), 32
    x = R.act_inputs(BHW + (C,), in_type, 12).copy()
    r = synth.rng(77).random(x.shape)
    x[r < 0.02] = np.nan
    x[(r >= 0.02) & (r < 0.03)] = np.inf
    x[(r >= 0.03) & (r < 0.04)] = -np.inf
    got, bn = _run_stem_tail(K, lib, BHW, C, in_type, fmt, x=x, special=True)
    gam, bet, mean, var = bn.np
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    y = torch.relu(F.batch_norm(t(x).permute(0, 3, 1, 2), t(mean), t(var), t(gam), t(bet), False, 0.0, EPS32))
    want = F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    _, bound = R.stem_tail_ref(np.where(np.isfinite(x), x, 0).astype(np.float32), in_type, gam, bet, mean, var, fmt)
    check_special("stem_tail", got, fmt, want, bound)


@pytest.mark.parametrize("C,Ho,Wo", [(24, 233017, 3), (64, 52429, 5)], ids=["C24", "C64"])
def test_stem_tail_capped_walk(lib, C, Ho, Wo):
    """bf16 rows, two images whose B Ho Wo G / 256 is ONE block past the cap of 16384: the grid is capped (C = 24: and rounded to
    16383 = 3 x 5461) and threads stride.  Expected bits: the same entry image by image (each under the cap: the one-pass walk the
    small shapes check against float64); 4096 sampled interior pixels against float64 on top."""
    B, H, W, G = 2, 2 * Ho - 1, 2 * Wo - 1, C // 8
    px = B * Ho * Wo
    # one block past the cap, and one pooled pixel less per image is under it (C = 24: px is the smallest count there is)
    assert -(-px * G // 256) == 16385 and -(-(px - B) * G // 256) <= 16384, "not the smallest extent past the cap"
    assert C != 24 or -(-(px - 1) * G // 256) == 16384
    assert R.stem_tail_grid(B, H, W, C) == (16384 - 16384 % (3 if C == 24 else 1), 3 if C == 24 else 1, True)
    assert not R.stem_tail_grid(1, H, W, C)[2]
    inb = Bufs()
    X, h = GB.carve((B, H, W, C), torch.bfloat16, "cuda", BAND)
    inb.handles.append(("x", h))
    g = torch.Generator(device="cuda").manual_seed(5)
    X.copy_((torch.randn(X.shape, generator=g, device="cuda") * 2 + 0.3).bfloat16())
    bn = BN(inb, C, 11 + C)
    ob = Bufs()
    out = ob.out("out", (B, Ho, Wo, C), torch.bfloat16, BAND)
    twice(lambda: _tail_launch(lib, X, "bf16", bn, out, "bf16", B, H, W, C), [out], ob, inb)
    rb = Bufs()
    ref = rb.out("per image", (B, Ho, Wo, C), torch.bfloat16, BAND)
    for b in range(B):
        assert _tail_launch(lib, X[b], "bf16", bn, ref[b], "bf16", 1, H, W, C) == 0
    rb.check(inb)
    assert _biteq(out, ref), "the capped walk differs from the image-by-image launches"
    gi = synth.rng(6)
    n = 4096
    b, yo, xo = gi.integers(0, B, n), gi.integers(1, Ho - 1, n), gi.integers(1, Wo - 1, n) if Wo > 2 else np.ones(n, np.int64)
    yo[:8] = Ho - 2                                                        # the tail of the walk
    bi, yi, xi = (dev(v) for v in (b, yo, xo))
    patch = torch.stack([X[bi, 2 * yi - 1 + k // 3, 2 * xi - 1 + k % 3] for k in range(9)], 1).float().cpu().numpy()
    t, E = R.elem(patch, *bn.np)
    E = E + R.round_term(t, E, "bf16")
    m, e = t.max(1), E.max(1)
    inside("stem_tail bf16 -> bf16", out[bi, yi, xi].float().cpu().numpy(), m, e + R.out_term(m, e, "bf16"))


# ------------------------------------------------------------------------------------------------ hiast_bn_act_nhwc_infer
def _bn_infer_launch(lib, X, Y, bn, relu, M, C, dtype):
    return SC.call(lib, "bn_infer", x=X, y=Y, relu=relu, M=M, C=C, dtype=SC.DTYPE[dtype], stream=_st(), **bn.kw())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("MC", R.BN_INFER_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bn_infer(K, lib, MC, dtype):
    M, C = MC
    # (3, 24) and (257, 40) want fewer blocks than need = 3 | 5: the stride is no multiple of C, the per-iteration fallback runs
    assert R.bn_infer_grid(M, C, dtype)[1] == (MC not in ((3, 24), (257, 40)))
    x0 = R.act_inputs(MC, dtype, 13)
    for affine in ((True, False) if MC == (257, 40) else (True,)):
        inb = Bufs()
        X = inb.inp("x", as16(x0, dtype), BAND)
        bn = BN(inb, C, 21 + C, affine)
        for relu in (0, 1):
            ob = Bufs()
            Y = ob.out("y", MC, T16[dtype], BAND)
            twice(lambda: _bn_infer_launch(lib, X, Y, bn, relu, M, C, dtype), [Y], ob, inb)
            assert _biteq(Y, K.bn_act_nhwc_infer(X, bn.module, bool(relu)))
            want, bound = R.bn_infer_ref(x0, *bn.np, relu, dtype)
            inside("bn_act_nhwc_infer " + dtype, Y.float().cpu().numpy(), want, bound)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bn_infer_capped(lib, dtype):
    """C = 24, one block past the cap of 8192: the grid is rounded to 8190 (a multiple of need = 3) and every thread keeps its
    channels (the fixed-channel path; test_bn_infer's (3, 24) takes the fallback).  Expected bits: the same entry on the two halves
    of the rows, each under the cap; 4096 sampled rows against float64."""
    C, vec = 24, 8 if dtype == "bf16" else 4
    M = 2 * (8192 * 1024 * vec // C // 2 + 1)
    assert -(-(M * C // vec) // 1024) == 8193 and R.bn_infer_grid(M, C, dtype) == (8190, True)
    half = R.bn_infer_grid(M // 2, C, dtype)
    assert half[0] < 8192 and half[1] and (M // 2 * C * (2 if dtype == "bf16" else 4)) % 16 == 0
    inb = Bufs()
    X, h = GB.carve((M, C), T16[dtype], "cuda", BAND)
    inb.handles.append(("x", h))
    X.copy_((torch.randn(X.shape, generator=torch.Generator(device="cuda").manual_seed(8), device="cuda") * 2 + 0.3).to(X.dtype))
    bn = BN(inb, C, 21 + C)
    ob, rb = Bufs(), Bufs()
    Y, ref = ob.out("y", (M, C), T16[dtype], BAND), rb.out("halves", (M, C), T16[dtype], BAND)
    twice(lambda: _bn_infer_launch(lib, X, Y, bn, 1, M, C, dtype), [Y], ob, inb)
    for s in (0, M // 2):
        assert _bn_infer_launch(lib, X[s:s + M // 2], ref[s:s + M // 2], bn, 1, M // 2, C, dtype) == 0
    rb.check(inb)
    assert _biteq(Y, ref), "the capped launch differs from the two halves"
    rows = dev(np.concatenate([synth.rng(9).integers(0, M, 4088), np.arange(M - 8, M)]))
    want, bound = R.bn_infer_ref(X[rows].float().cpu().numpy(), *bn.np, 1, dtype)
    inside("bn_act_nhwc_infer " + dtype, Y[rows].float().cpu().numpy(), want, bound)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bn_infer_special_values(lib, dtype):
    """relu = 1: NaN -> NaN, -inf -> 0 or NaN by the sign of the scale, +inf likewise, as relu(batch_norm) in float64"""
    M, C = 257, 40
    x = R.act_inputs((M, C), dtype, 13).copy()
    r = synth.rng(78).random(x.shape)
    x[r < 0.02], x[(r >= 0.02) & (r < 0.03)], x[(r >= 0.03) & (r < 0.04)] = np.nan, np.inf, -np.inf
    inb, ob = Bufs(), Bufs()
    X = inb.inp("x", as16(x, dtype), BAND)
    bn = BN(inb, C, 21 + C)
    Y = ob.out("y", (M, C), T16[dtype], BAND, must_fill=False)
    twice(lambda: _bn_infer_launch(lib, X, Y, bn, 1, M, C, dtype), [Y], ob, inb)
    with np.errstate(invalid="ignore"):
        sc, sh, _, _ = R.scale_shift(*bn.np)
        t = x.astype(np.float64) * sc + sh
        want = np.where(np.isnan(t), np.nan, np.maximum(t, 0.0))
    got = Y.float().cpu().numpy().astype(np.float64)
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])


# ------------------------------------------------------------------------------------------------ K18 max-pool
def _pool_launches(lib, X, Y, IDX, DY, DX, dims, fmt):
    f = lambda: SC.call(lib, "pool_fwd", x=X, y=Y, idx=IDX, fmt=SC.FMT[fmt], stream=_st(), **dims)
    b = lambda: SC.call(lib, "pool_bwd", dy=DY, idx=IDX, dx=DX, fmt=SC.FMT[fmt], stream=_st(), **dims)
    return f, b


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["smooth", "ties", "special"])
@pytest.mark.parametrize("BHWC", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool(K, lib, BHWC, kind, fmt):
    B, H, W, C = BHWC
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x0 = R.pool_input(BHWC, kind, fmt, 3)
    dy0 = synth.rng(4).integers(-8, 9, (B, Ho, Wo, C)).astype(np.float32) / 8 if kind != "smooth" else \
        R.dec16(R.enc16(synth.normal_f32(4, (B, Ho, Wo, C)), fmt), fmt)
    m, code = R.maxpool_ref(x0)
    inb, fb, bb = Bufs(), Bufs(), Bufs()
    X, DY = inb.inp("x", as16(x0, fmt), BAND), inb.inp("dy", as16(dy0, fmt), BAND)
    Y = fb.out("y", (B, Ho, Wo, C), T16[fmt], BAND, must_fill=kind != "special")
    IDX = fb.out("idx", (B, Ho, Wo, C), U8, BAND)
    DX = bb.out("dx", BHWC, T16[fmt], BAND)
    f, b = _pool_launches(lib, X, Y, IDX, DY, DX, dict(B=B, H=H, W=W, C=C), fmt)
    twice(f, [Y, IDX], fb, inb)
    assert np.array_equal(IDX.cpu().numpy(), code), "window codes differ"
    gy = Y.float().cpu().numpy()
    assert np.array_equal(np.isnan(gy), np.isnan(m)) and np.array_equal(gy[~np.isnan(m)], m[~np.isnan(m)])
    if kind != "special":
        assert np.array_equal(bits(Y), R.enc16(m, fmt))
    twice(b, [DX], bb, inb, fb)                                            # on the carved idx the forward wrote
    assert np.array_equal(bits(DX), R.maxpool_bwd_ref(dy0, code, H, W, fmt)), "dx bits differ"
    ky, kidx = K.maxpool3x3s2_cl_fwd(X.permute(0, 3, 1, 2))
    assert _biteq(ky.permute(0, 2, 3, 1), Y) and _biteq(kidx, IDX)
    assert _biteq(K.maxpool3x3s2_cl_bwd(DY.permute(0, 3, 1, 2), IDX, H, W).permute(0, 2, 3, 1), DX)


def test_maxpool_capped(lib):
    """C = 8, two images of 1398101 x 5: the forward wants 16385 blocks (cap 16384), the backward 54614 (cap 32768); expected bits
    from image-by-image launches, each under both caps"""
    B, H, W, C, fmt = 2, 1398101, 5, 8, "bf16"
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert -(-B * Ho * Wo // 256) == 16385 and -(-Ho * Wo // 256) <= 16384
    assert -(-B * H * W // 256) > 32768 >= -(-H * W // 256)
    inb, ob, bb, rb = Bufs(), Bufs(), Bufs(), Bufs()
    g = torch.Generator(device="cuda").manual_seed(10)
    X = inb.out("x", (B, H, W, C), torch.bfloat16, BAND, must_fill=False)
    X.copy_(torch.randint(-6, 7, X.shape, generator=g, device="cuda", dtype=torch.int16).bfloat16())   # ties everywhere
    DY = inb.out("dy", (B, Ho, Wo, C), torch.bfloat16, BAND, must_fill=False)
    DY.copy_(torch.randint(-8, 9, DY.shape, generator=g, device="cuda", dtype=torch.int16).bfloat16() / 8)
    Y, IDX, DX = ob.out("y", DY.shape, torch.bfloat16, BAND), ob.out("idx", DY.shape, U8, BAND), bb.out("dx", X.shape, torch.bfloat16, BAND)
    f, b = _pool_launches(lib, X, Y, IDX, DY, DX, dict(B=B, H=H, W=W, C=C), fmt)
    twice(f, [Y, IDX], ob, inb)
    twice(b, [DX], bb, inb, ob)
    RY, RI, RX = rb.out("y", DY.shape, torch.bfloat16, BAND), rb.out("idx", DY.shape, U8, BAND), rb.out("dx", X.shape, torch.bfloat16, BAND)
    for i in range(B):
        f1, b1 = _pool_launches(lib, X[i], RY[i], RI[i], DY[i], RX[i], dict(B=1, H=H, W=W, C=C), fmt)
        assert f1() == 0 and b1() == 0
    rb.check(inb)
    assert _biteq(Y, RY) and _biteq(IDX, RI) and _biteq(DX, RX), "a capped launch differs from the image-by-image launches"
    assert int(IDX.max()) <= 8


# ------------------------------------------------------------------------------------------------ hiast_split_planes
def _split_case(K, lib, a):
    M, C = a.shape
    inb, ob, mb = Bufs(), Bufs(), Bufs()
    X = inb.inp("x", dev(a), BAND)
    P = ob.out("planes", (M, 2 * C), torch.bfloat16, BAND, must_fill=False)
    twice(lambda: SC.call(lib, "split_planes", x=X, planes=P, M=M, C=C, inverse=0, stream=_st()), [P], ob, inb)
    want = R.planes_of(a)
    Y = mb.out("merged", (M, C), F32, BAND, must_fill=False)
    twice(lambda: SC.call(lib, "split_planes", x=Y, planes=P, M=M, C=C, inverse=1, stream=_st()), [Y], mb, inb, ob)
    assert _biteq(P, K.split_planes(X)) and _biteq(Y, K.merge_planes(P))
    return bits(P), want, Y.cpu().numpy(), R.merge_of(want)


@pytest.mark.parametrize("C", [32, 96, 2048])
@pytest.mark.parametrize("M", [1, 3, 4099, 8193])
def test_split_planes(K, lib, M, C):
    """both directions, bit for bit; M = 8193 x C = 2048 is one block past the cap of 8192 blocks"""
    if M == 8193:
        if C != 2048:
            return
        assert -(-(M * C // 8) // 256) == 8193
    got, want, merged, mwant = _split_case(K, lib, synth.normal_f32(M + C, (M, C), 3.0))
    assert np.array_equal(got, want) and np.array_equal(merged.view(np.uint32), mwant.view(np.uint32))


def test_split_planes_special_values(K, lib):
    """+-0, subnormals, the largest finite values (hi rounds UP to inf: lo = -inf and the merge is a NaN), +-inf (lo = inf - inf),
    NaN: hi and every finite lo from the integer arithmetic, bit for bit; a NaN lo only as "a NaN" (its sign is the hardware's)"""
    sp = np.array([0x00000000, 0x80000000, 0x00000001, 0x00018000, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F800000,
                   0xFF800000, 0x7FC00000, 0x3F808000, 0x3F818000], np.uint32).view(np.float32)
    a = np.resize(sp, (13, 32))                                            # 416 = 32 x 13 values, cyclic
    got, want, merged, mwant = _split_case(K, lib, a)
    hi, lo = R.split_bits(a)
    g = got.reshape(-1, 2, 32)
    assert np.array_equal(g[:, 0], hi)
    lo_nan = (lo & 0x7F80 == 0x7F80) & (lo & 0x7F != 0)
    assert lo_nan.any() and np.array_equal((g[:, 1] & 0x7F80 == 0x7F80) & (g[:, 1] & 0x7F != 0), lo_nan)
    assert np.array_equal(g[:, 1][~lo_nan], lo[~lo_nan])
    assert np.array_equal(np.isnan(merged), np.isnan(mwant))
    assert np.array_equal(merged.view(np.uint32)[~np.isnan(mwant)], mwant.view(np.uint32)[~np.isnan(mwant)])
    big = a == np.float32(3.4028234663852886e38)
    assert big.any() and np.isnan(merged[big]).all()


# ------------------------------------------------------------------------------------------------ hiast_pack_conv_weight
TILED = [(64, 64, 1), (128, 64, 9), (64, 192, 9)]
ELEMENTWISE = [(48, 96, 9), (19, 256, 1), (64, 3, 49), (64, 64, 16), (32, 32, 9), (96, 32, 1)]


def _pack_legal(N, K, fmt, mode):
    return fmt != "split" or ((mode == 1 or K % 32 == 0) and (mode == 0 or N % 32 == 0))


def _pack_case(lib, w, fmt, mode, shift=0):
    """-> (rc, wp bits, wpt bits | None, the buffers); shift: wp and wpt start `shift` elements into their payload"""
    N, K, taps = w.shape
    PL = 2 if fmt == "split" else 1
    inb, ob = Bufs(), Bufs()
    Wt = inb.inp("w", dev(w), BAND)
    n_wp = (K * taps * PL * N) if mode == 1 else N * taps * PL * K
    wp = ob.out("wp", (n_wp + shift,), T16[fmt], BAND, must_fill=False)
    wpt = ob.out("wpt", (K * taps * PL * N + shift,), T16[fmt], BAND, must_fill=False) if mode == 2 else None
    kw = dict(w=Wt, N=N, K=K, taps=taps, fmt=SC.FMT[fmt], transpose=mode, wp=wp[shift:], wpt=None if wpt is None else wpt[shift:],
              stream=_st())
    rc = SC.call(lib, "pack", **kw)
    ob.check(inb)
    if rc == 0:
        first = (wp.clone(), None if wpt is None else wpt.clone())
        assert SC.call(lib, "pack", **kw) == 0
        ob.check(inb)
        assert _biteq(first[0], wp) and (wpt is None or _biteq(first[1], wpt)), "a second launch gives other bits"
        assert shift == 0 or (bits(wp[:shift]) == 0xFFFF).all()
    return rc, bits(wp[shift:]), None if wpt is None else bits(wpt[shift:]), ob


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("NKT", TILED + ELEMENTWISE, ids=lambda s: "x".join(map(str, s)))
def test_pack_conv_weight(K, lib, NKT, fmt):
    N, Kc, taps = NKT
    if NKT == (64, 3, 49) and fmt == "split":
        return                                                             # the issue's list: 16-bit formats only (refused: below)
    w = synth.normal_f32(sum(NKT), NKT)
    for mode in (0, 1, 2):
        rc, wp, wpt, ob = _pack_case(lib, w, fmt, mode)
        if not _pack_legal(N, Kc, fmt, mode):
            assert rc == SC.E_RANGE
            ob.untouched()
            continue
        assert rc == 0
        a, b = R.pack_ref(w, fmt, mode)
        assert np.array_equal(wp, a) and (b is None or np.array_equal(wpt, b)), "packed bits differ (mode %d)" % mode
        if int(np.sqrt(taps)) ** 2 == taps:
            k = int(np.sqrt(taps))
            got = K.pack_conv_weight(dev(w).view(N, Kc, k, k), SC.FMT[fmt], transpose=mode == 1, both=mode == 2)
            got = got if mode == 2 else (got,)
            assert np.array_equal(bits(got[0]).ravel(), wp) and (mode != 2 or np.array_equal(bits(got[1]).ravel(), wpt))


@pytest.mark.parametrize("fmt", R.FMTS)
def test_pack_conv_weight_misaligned_falls_back(lib, fmt):
    """a tiled shape with wp and wpt 2 bytes off the 16-byte grid takes the elementwise kernel: the tiled launch's bits, and the
    element in front of each stays 0xFFFF"""
    w = synth.normal_f32(5, (128, 64, 9))
    for mode in (0, 1, 2):
        _, a, at, _ = _pack_case(lib, w, fmt, mode)
        rc, b, bt, _ = _pack_case(lib, w, fmt, mode, shift=1)
        assert rc == 0 and np.array_equal(a, b) and (at is None or np.array_equal(at, bt))


def test_pack_conv_weight_refuses_ragged_split_slabs(lib):
    """finding 1: a split-plane form whose reduction channel count is no multiple of 32 is refused and NOTHING is written — without
    the check the lo halves of the last row's ragged slab land in the 32 bytes behind wp (the trailing band reports them)"""
    for what, ch in SC.split_pack_refusals():
        N, Kc, taps, mode = ch["N"], ch["K"], ch.get("taps", 9), ch["transpose"]
        rc, _, _, ob = _pack_case(lib, synth.normal_f32(3, (N, Kc, taps)), "split", mode)
        ob.untouched()
        assert rc == SC.E_RANGE, what


@pytest.mark.parametrize("fmt", R.FMTS)
def test_pack_conv_weight_multi(lib, fmt):
    """three records per launch: 1-tap records, 9-tap records, and both kinds with max_taps = 9; every wp / wpt carved; the bits of
    the single packs (= pack_ref, which test_pack_conv_weight holds the single entry to)"""
    shapes = [(64, 64), (128, 64), (64, 192)]
    PL = 2 if fmt == "split" else 1
    for mode in (0, 2):
        for taps_of in ((1, 1, 1), (9, 9, 9), (1, 9, 1)):
            inb, ob = Bufs(), Bufs()
            ws = [synth.normal_f32(40 + i, (N, Kc, t)) for i, ((N, Kc), t) in enumerate(zip(shapes, taps_of))]
            wd = [inb.inp("w%d" % i, dev(w), BAND) for i, w in enumerate(ws)]
            wp = [ob.out("wp%d" % i, (w.size * PL,), T16[fmt], BAND, must_fill=False) for i, w in enumerate(ws)]
            wpt = [ob.out("wpt%d" % i, (w.size * PL,), T16[fmt], BAND, must_fill=False) if mode == 2 else None for i, w in enumerate(ws)]
            recs = [(wd[i].data_ptr(), wp[i].data_ptr(), wpt[i].data_ptr() if mode == 2 else 0) + ws[i].shape + (SC.FMT[fmt], mode)
                    for i in range(3)]
            host, ct, cs, mt = SC.pack_tables(recs)
            tab = inb.inp("table", dev(host.view(np.uint8).reshape(-1).copy()), VBAND)
            CT, CS = inb.inp("chunk_tensor", dev(ct), VBAND), inb.inp("chunk_start", dev(cs), VBAND)
            launch = lambda: SC.call(lib, "pack_multi", table=tab, chunk_tensor=CT, chunk_start=CS, n_chunks=len(ct), max_taps=mt, stream=_st())
            twice(launch, wp + [t for t in wpt if t is not None], ob, inb)
            for i, w in enumerate(ws):
                a, b = R.pack_ref(w, fmt, mode)
                assert np.array_equal(bits(wp[i]), a) and (b is None or np.array_equal(bits(wpt[i]), b)), (mode, taps_of, i)


# ------------------------------------------------------------------------------------------------ hiast_normalize_u8
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 3, 1023, 262145, 1048579])
def test_normalize_u8(K, lib, HW, B):
    """img at an odd address, out 4-byte aligned only; HW = 1048579 wants more than the 1024 blocks of the cap"""
    if HW > 2 ** 20:
        assert -(-HW // 1024) > 1024
        if B > 1:
            return
    img = synth.images_u8(HW + B, B, HW, 1).reshape(B, HW, 3)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    inb, ob = Bufs(), Bufs()
    I = inb.out("img", (img.size + 1,), U8, BAND, must_fill=False)
    I[1:].copy_(dev(img.reshape(-1)))
    O = ob.out("out", (B * 3 * HW + 1,), F32, BAND, must_fill=False)
    assert I[1:].data_ptr() % 2 == 1 and O[1:].data_ptr() % 16 == 4
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    twice(lambda: SC.call(lib, "normalize_u8", img=I[1:], out=O[1:], B=B, HW=HW, mean=m, std=s, stream=_st()), [O], ob, inb)
    assert (O[:1].view(U8) == GB.FILL).all(), "the element in front of out was written"
    want = R.normalize_ref(img, mean, std)
    assert np.array_equal(O[1:].cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))
    assert _biteq(K.normalize_u8(dev(img).view(B, HW, 1, 3), mean, std).reshape(-1), O[1:])


# ------------------------------------------------------------------------------------------------ hiast_ema_update, hiast_multi_copy
SIZES = [1, 3, 4, 65535, 65536, 65537, 131077]


def test_ema_update(K, lib):
    """every tensor carved on its own; one with ema 4 bytes off the 16-byte grid, one with p 4 bytes off (the scalar path)"""
    cases = [(n, 0, 0) for n in SIZES] + [(65537, 1, 0), (131077, 0, 1)]
    eb, pb, tb = Bufs(), Bufs(), Bufs()
    e0 = [synth.normal_f32(50 + i, (n,)) for i, (n, _, _) in enumerate(cases)]
    p0 = [synth.normal_f32(70 + i, (n,)) for i, (n, _, _) in enumerate(cases)]
    E = [eb.out("ema%d" % i, (n + se,), F32, BAND, must_fill=False)[se:] for i, (n, se, _) in enumerate(cases)]
    P = [pb.out("p%d" % i, (n + sp,), F32, BAND, must_fill=False)[sp:] for i, (n, _, sp) in enumerate(cases)]
    assert E[-2].data_ptr() % 16 == 4 and P[-1].data_ptr() % 16 == 4
    for t, v in zip(P, p0):
        t.copy_(dev(v))
    recs, ct, cs = SC.ema_tables([(e.data_ptr(), p.data_ptr(), e.numel()) for e, p in zip(E, P)])
    assert len(ct) == sum(-(-n // SC.CHUNK) for n, _, _ in cases)
    tab, CT, CS = tb.inp("table", dev(recs), VBAND), tb.inp("chunk_tensor", dev(ct), VBAND), tb.inp("chunk_start", dev(cs), VBAND)
    g, omg = float(np.float32(0.999)), float(np.float32(1 - 0.999))
    results = []
    for _ in range(2):                                                     # in place: the second launch starts from the same values
        for t, v in zip(E, e0):
            t.copy_(dev(v))
        assert SC.call(lib, "ema", table=tab, chunk_tensor=CT, chunk_start=CS, n_chunks=len(ct), decay=g, one_minus_decay=omg, stream=_st()) == 0
        eb.check(pb, tb)
        results.append([t.clone() for t in E])
    for i, (a, b) in enumerate(zip(*results)):
        assert _biteq(a, b)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), R.ema_ref(e0[i], p0[i], g, omg).view(np.uint32)), cases[i]
        assert np.array_equal(P[i].cpu().numpy(), p0[i])
    plain = [dev(v) for v in e0]
    K.ema_update(K.EmaPlan(plain, [dev(v) for v in p0]), 0.999)
    assert all(_biteq(a, b) for a, b in zip(plain, results[0]))


def test_multi_copy(K, lib):
    """records of 0, 1, 15, 16, 17, 4099 and 8192 bytes, aligned, src-only and dst-only misaligned"""
    cases = [(n, 0, 0) for n in (0, 1, 15, 16, 17, 4099, 8192)] + [(4099, 1, 0), (4099, 0, 1), (8192, 3, 0), (16, 0, 8)]
    sb, db, tb = Bufs(), Bufs(), Bufs()
    src0 = [synth.rng(90 + i).integers(0, 255, max(n, 1), dtype=np.uint8) for i, (n, _, _) in enumerate(cases)]   # never 0xFF
    S = [sb.inp("src%d" % i, dev(np.concatenate([np.zeros(ss, np.uint8), v])), BAND)[ss:] for i, ((n, ss, _), v) in enumerate(zip(cases, src0))]
    D = [db.out("dst%d" % i, (max(n, 1) + sd,), U8, BAND, must_fill=False) for i, (n, _, sd) in enumerate(cases)]
    recs = np.array([(d[sd:].data_ptr(), s.data_ptr(), n) for d, s, (n, _, sd) in zip(D, S, cases)], np.int64)
    tab = tb.inp("table", dev(recs), VBAND)
    for _ in range(2):
        assert SC.call(lib, "multi_copy", table=tab, n_tensors=len(cases), stream=_st()) == 0
        db.check(sb, tb)
        for d, v, (n, _, sd) in zip(D, src0, cases):
            got = d.cpu().numpy()
            assert np.array_equal(got[sd:sd + n], v[:n]) and (got[:sd] == GB.FILL).all() and (got[sd + n:] == GB.FILL).all()
    live = [(v, n) for v, (n, _, _) in zip(src0, cases) if n]
    plain = [torch.zeros(n, dtype=U8, device="cuda") for _, n in live]
    K.multi_copy(K.CopyPlan(plain, [dev(v[:n]) for v, n in live]))
    assert all(np.array_equal(t.cpu().numpy(), v[:n]) for t, (v, n) in zip(plain, live))


# ------------------------------------------------------------------------------------------------ hiast_confusion_hist
@pytest.mark.parametrize("N", [1, 4096, 4097, 2048 * 4096 + 1])
@pytest.mark.parametrize("Kc", [1, 19, 256, 1024])
def test_confusion_hist(K, lib, Kc, N):
    """labels include -1, K, 255 and 2^40; N = 2048 x 4096 + 1 wants one block more than the cap of 2048; the counters start from
    chosen values and the second launch adds the same histogram again"""
    if N > 4097 and Kc not in (19, 256):
        return
    g = synth.rng(N % 1000 + Kc)
    odd = np.array([-1, Kc, 255, 2 ** 40], np.int64)
    draw = lambda: np.where(g.random(N) < 0.2, odd[g.integers(0, 4, N)], g.integers(0, Kc, N))
    pred, tgt = draw(), draw()
    same = g.random(N) < 0.5
    pred = np.where(same, tgt, pred)
    if N >= 4:
        tgt[:4], pred[:4] = odd, odd
    want = R.confusion_ref(pred, tgt, Kc)
    inb, ob = Bufs(), Bufs()
    P, T = inb.inp("pred", dev(pred), BAND), inb.inp("target", dev(tgt), BAND)
    start = [np.arange(Kc, dtype=np.int64) * (i + 2) + 5 for i in range(3)]
    C = [ob.out(n, (Kc,), I64, VBAND, init=dev(s)) for n, s in zip(("inter", "area_pred", "area_tgt"), start)]
    for launch in (1, 2):
        assert SC.call(lib, "confusion", pred=P, target=T, N=N, K=Kc, inter=C[0], area_pred=C[1], area_tgt=C[2], stream=_st()) == 0
        ob.check(inb)
        for c, s, w in zip(C, start, want):
            assert np.array_equal(c.cpu().numpy(), s + launch * w)
    got = K.confusion_hist(P, T, Kc)
    assert all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", list(SC.ENTRIES))
def test_refused_calls_write_nothing(lib, entry):
    """the refused calls of the host test on carved buffers of 1 MiB each: the same code, and no byte of any buffer changes"""
    b = Bufs()
    base = SC.placeholders(entry)
    for n in SC.args_of(entry):
        if n in SC.POINTERS and n != "stream":
            base[n] = b.out(n, (1 << 20,), U8, 4096)
    if entry == "normalize_u8":
        base["mean"], base["std"] = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    base["stream"] = _st()
    n = 0
    for what, change, code in SC.refused_calls(entry):
        assert SC.call(lib, entry, **SC.apply_change(base, change)) == code, (entry, what)
        n += 1
    assert n >= 3
    b.untouched()


def test_zz_report_worst_ratios():
    """prints the worst error / bound per bounded entry and format of this run; no assertion of its own"""
    for cls in sorted(WORST):
        print("stem worst error/bound  %-36s %.4f" % (cls, WORST[cls]))
