"""The loss and discriminator-input entries (st_loss.hip, dinput.hip) through the C ABI (tests/loss_calls.py) on buffers carved out
of 0xFF-filled allocations (tests/guard_bands.py), every sum and EVERY gradient cell against float64 with the per-element bounds
of tests/loss_ref.py.  Logits and teacher logits sit in NaN poison, labels in 0xFF (= HIAST_IGNORE for uint8: a label read one
row too far is counted as "ignored" and only the exact n_ign shows it; -1 for int64: counted as confident), coef, sums (8
doubles), dlogits and the dinput scratch are carved, the workspace is carved at EXACTLY hiast_st_loss_workspace_bytes.  After each
launch:
  1. both guard bands of every buffer, inputs and workspace included, are untouched;
  2. sums and dlogits (dinput: the map, the scratch, dlogits) are finite and fully written, sums[7] == 0.0;
  3. counts (slots 4-6) are exact, sums 0-3 and every gradient cell inside their bounds; slots 0, 1, 2, 4, 5 have the same bits
     for every kind on the same operands; uint8 and int64 labels give the same bits;
  4. the payload is bit-equal to the K.st_loss_* / K.dinput_* wrapper, hiast_st_loss_fwd / _bwd to the _cst_ entries with kind 0;
  5. a second launch into the same buffers gives the same bits.

entry                                        test
hiast_st_loss_fwd, _bwd, _cst_fwd, _cst_bwd  test_loss_entries (below), test_unaligned_pointers, test_zero_denominators
hiast_st_loss_workspace_bytes                every launch (exact size); test_refused_loss_calls_write_nothing (0 for a refused geometry)
hiast_dinput_fwd, _bwd                       test_dinput_entries, test_dinput_underflowed_probability
hiast_upsample_bilinear_ac_bwd               test_dinput_entries (on the scratch dinput_bwd wrote: the bits of its dlogits)
argument checks                              test_refused_loss_calls_write_nothing, test_refused_dinput_calls_write_nothing
__expf, __logf, expf, log2f                  test_intrinsic_error_constants (a probe kernel against float64, NOT the loss kernels)

test_loss_entries, (h, w, H, W):             class counts   why
  (1,1,1,1)                                  2 9 16 19      sh = sw = 0, one pixel (degenerate; one of n_conf / n_ign is 0)
  (1,1,3,256)                                2 9 16 19      w = 1 at the accepted cap: all 256 threads of one block on the sw = 0 path
  (3,2,7,255)                                2 9 16 19      the largest accepted W for w = 2
  (2,9,2,2033)                               2 19           TI = 1, 9 tile blocks of up to 254 columns, fwd grid.x = 8: the largest accepted magnification
  (8,5,24,42)                                2 9 16 19      an empty last band in both directions (float32 sh (H-1) = 6.9999995, sw (W-1) = 3.9999998)
  (2,254,2,254)                              2 9 16 19      identity, TI = 253, the second tile block holds one cell
  (2,300,2,300)                              2 19           identity with W > 256: fwd grid.x = 2, the last block partly live, 2 tile blocks
  (4,40,9,300)                               2 9 16 19      two tile blocks, fwd grid.x = 2: the ordinary multi-block case
  (5,9,33,65)                                2 9 16 19      the ordinary odd shape
  (2,512,2,711)                              2 19           float32 sw (W-1) = 511 + 2^-15: the clamped last column (x1 = x0 = w-1) carries l1 != 0; 3 tile blocks
  (512,2,711,3)                              2 19           the same for the rows: the clamped last band's (j = h-1, r = 1) source carries a weight
On the first nine a clamped column or row only ever has l1 = 0; the last two make the kernels' clamp paths count.
Each runs the five kernel variants (SoftCE without teacher, SoftCE, CE, KLDIV, MSE) x three regions x uint8 / int64 labels: all 40
template configurations of both kernels run on (1,1,1,1) (degenerate) and on (4,40,9,300) (multi-block).  B = 3 for the CE kind
(its count M), 1 elsewhere.  dinput: 2 modes x 4 class counts on (1,1,1,1), (3,4,5,257) (grid.x = 2, one live column in the second
block), (2,3,4,512), (5,7,5,7), (8,5,24,42) and the downsampling (5,7,3,4).

NOT covered: B, h, H above 65535 (the grid limits), label values outside [0, C) + {255} (not detected by the entries)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import guard_bands as GB
import head_ref
import loss_calls as LC
import loss_ref as R
import synth
from test_gpu_bn_extents import Bufs, _biteq, _np, _st
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

WORST = {}                           # quantity -> worst error / bound seen in this run (test_zz_report_worst_ratios)
BAND = 64 << 10                      # more than a block touches: 256 columns x 19 classes x 4 bytes x 2 rows
F32, F64, U8, I64 = torch.float32, torch.float64, torch.uint8, torch.int64
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


def inside(cls, got, ref, bound):
    """|got - ref| <= bound at every element; records the worst ratio of the class"""
    got = _np(got) if torch.is_tensor(got) else np.asarray(got)
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    assert np.isfinite(err).all(), cls
    ratio = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    over = err > bound
    assert not over.any(), "%s: %d element(s) outside the bound, worst error / bound = %.3f" % (cls, int(over.sum()), ratio)


def reference(geom, C, variant, region, inputs=None, tag=None):
    """the float64 sums (and, once the counts are known, the gradient for the usable coefficients), cached per
    (geometry, C, variant, region); asserts the two input conditions (no skipping)"""
    key = (geom, C, variant[0], region, tag)
    if key not in _REFS:
        name, kind, teacher, B = variant
        z, zt, lbl = inputs if inputs is not None else R.loss_inputs(R.case_seed(geom, C), B, C, *geom)
        geo = R.Geometry(*geom)
        ref = R.loss_reference(geo, z, zt if teacher else None, lbl, kind, region)
        assert ref["gap_ok"], "the arg-max gap condition fails for %r" % (key,)
        assert ref["min_prod"] >= R.MIN_PROD, "a counted product is below 1e-30 for %r" % (key,)
        coef = R.usable_coef(ref["sums"])
        ref = R.loss_reference(geo, z, zt if teacher else None, lbl, kind, region, coef)
        ref["coef"] = np.asarray(coef, np.float32)
        _REFS[key] = ref
    return _REFS[key]


class Operands:
    """the carved inputs of one (geometry, C, batch): logits, teacher, labels in both types; shift = 1: each starts one element
    into its payload (logits 4-byte but not 16-byte aligned, uint8 labels at an odd byte)"""

    def __init__(self, z, zt, lbl, shift=0):
        self.bufs = Bufs()
        self.shape = z.shape

        def put(name, t):
            flat = t.reshape(-1)
            p = self.bufs.out(name, (flat.numel() + shift,), t.dtype, BAND, must_fill=False)
            p[shift:].copy_(flat)
            v = p[shift:]
            assert shift == 0 or v.data_ptr() % 16 != 0
            return v
        self.z, self.zt = put("logits", dev(z)), put("teacher", dev(zt))
        self.lbl = {0: put("plbl u8", dev(lbl.astype(np.uint8))), 1: put("plbl i64", dev(lbl.astype(np.int64)))}
        assert shift == 0 or self.lbl[0].data_ptr() % 2 == 1


def launch_pair(lib, ops, geom, C, kind, teacher, region, is_i64, coef, cst_entry, shift=0, ws_short=0):
    """fwd then bwd through the C ABI in carved buffers, each launched twice into the same buffers -> sums, dlogits (payload views)"""
    h, w, H, W = geom
    B = ops.shape[0]
    need = LC.workspace_bytes(lib, B, C, h, w, H, W)
    assert need == R.workspace_bytes(B, C, h, w, H, W) > 0
    kw = dict(logits=ops.z, teacher=ops.zt if teacher else None, plbl=ops.lbl[is_i64], is_i64=is_i64, B=B, C=C, h=h, w=w, H=H, W=W,
              region=region, kind=kind, ws_bytes=need, stream=_st())
    fb = Bufs()
    sums = fb.out("sums", (8,), F64, BAND)
    ws = fb.out("workspace", (need,), U8, BAND, must_fill=False)
    cf = fb.inp("coef", dev(np.asarray(coef, np.float32)), BAND)
    first = None
    for _ in range(2):
        assert LC.loss_call(lib, False, cst_entry, sums=sums, ws=ws, **kw) == 0
        fb.check(ops.bufs)
        assert float(sums[7]) == 0.0
        if first is None:
            first = sums.clone()
    assert _biteq(first, sums), "sums: a second launch gives other bits"
    bb = Bufs()
    n = B * C * h * w
    dl = bb.out("dlogits", (n + shift,), F32, BAND, must_fill=False)
    ws2 = bb.out("workspace", (need,), U8, BAND, must_fill=False)
    first = None
    for _ in range(2):
        assert LC.loss_call(lib, True, cst_entry, sums=sums, coef=cf, dlogits=dl[shift:], ws=ws2, **kw) == 0
        bb.check(ops.bufs, fb)
        assert GB.finite(dl[shift:]), "dlogits: not finite (a cell was not written, or poison was read into it)"
        assert shift == 0 or bool((dl[:shift].view(U8) == GB.FILL).all()), "the element in front of dlogits was written"
        if first is None:
            first = dl.clone()
    assert _biteq(first, dl), "dlogits: a second launch gives other bits"
    return sums, dl[shift:].view(B, C, h, w)


def check_against_reference(name, C, sums, dl, ref):
    got = _np(sums)
    assert np.array_equal(got[4:7], ref["sums"][4:7]), (name, got[4:7], ref["sums"][4:7])
    for k in range(4):
        inside("sum %d %s" % (k, name if k == 3 else ""), got[k], ref["sums"][k], ref["sum_bound"][k])
    inside("gradient " + name, dl, ref["grad"], ref["grad_bound"])


@pytest.mark.parametrize("geom", list(R.GEOMETRIES), ids=lambda g: "x".join(map(str, g)))
def test_loss_entries(K, lib, geom):
    h, w, H, W = geom
    for C in R.GEOMETRIES[geom]:
        ops = {}
        for B in (1, 3):
            ops[B] = Operands(*R.loss_inputs(R.case_seed(geom, C), B, C, h, w, H, W))
        for region in range(3):
            common = {}                                                  # batch -> slots 0, 1, 2, 4, 5 of the first kind seen
            for variant in R.VARIANTS:
                name, kind, teacher, B = variant
                ref = reference(geom, C, variant, region)
                o = ops[B]
                z4, zt4 = o.z.view(o.shape), o.zt.view(o.shape)
                per_type = []
                for is_i64 in (0, 1):
                    sums, dl = launch_pair(lib, o, geom, C, kind, teacher, region, is_i64, ref["coef"], cst_entry=True)
                    check_against_reference(name, C, sums, dl, ref)
                    if kind == 0:
                        s0, d0 = launch_pair(lib, o, geom, C, 0, teacher, region, is_i64, ref["coef"], cst_entry=False)
                        assert _biteq(s0, sums) and _biteq(d0, dl), "hiast_st_loss_fwd / _bwd differ from the _cst_ entries with kind 0"
                    lb = o.lbl[is_i64].view(B, H, W)
                    ks = K.st_loss_fwd(z4, zt4 if teacher else None, lb, H, W, LC.REGIONS[region], cst_kind=kind)
                    kd = K.st_loss_bwd(z4, zt4 if teacher else None, lb, H, W, LC.REGIONS[region], ks, dev(ref["coef"]), cst_kind=kind)
                    assert _biteq(ks, sums) and _biteq(kd, dl), "the K.st_loss_* wrappers return other bits"
                    per_type.append((sums.clone(), dl.clone()))
                assert _biteq(per_type[0][0], per_type[1][0]) and _biteq(per_type[0][1], per_type[1][1]), "uint8 and int64 labels differ"
                slots = per_type[0][0][[0, 1, 2, 4, 5]]
                assert _biteq(common.setdefault(B, slots), slots), "slots 0, 1, 2, 4, 5 depend on the kind (%s)" % name
                if kind == LC.CE:                                        # the CE kind's batch of 3 against SoftCE on the same operands
                    need = LC.workspace_bytes(lib, B, C, h, w, H, W)
                    fb = Bufs()
                    s2 = fb.out("sums", (8,), F64, BAND)
                    wsb = fb.out("workspace", (need,), U8, BAND, must_fill=False)
                    assert LC.call(lib, "cst_fwd", logits=o.z, teacher=o.zt, plbl=o.lbl[0], is_i64=0, B=B, C=C, h=h, w=w, H=H, W=W,
                                   region=region, kind=0, sums=s2, ws=wsb, ws_bytes=need, stream=_st()) == 0
                    fb.check(o.bufs)
                    assert _biteq(s2[[0, 1, 2, 4, 5]], slots), "slots 0, 1, 2, 4, 5 of CE and SoftCE differ at B = 3"


@pytest.mark.parametrize("C", [2, 19])
def test_unaligned_pointers(lib, C):
    """uint8 labels from an odd byte; logits, teacher and dlogits 4-byte but not 16-byte aligned: the bits of the aligned run"""
    geom = (5, 9, 33, 65)
    for variant in (R.VARIANTS[1], R.VARIANTS[2], R.VARIANTS[3]):
        name, kind, teacher, B = variant
        inputs = R.loss_inputs(R.case_seed(geom, C), B, C, *geom)
        ref = reference(geom, C, variant, 2)
        a, u = Operands(*inputs), Operands(*inputs, shift=1)
        for is_i64 in (0, 1):
            sa, da = launch_pair(lib, a, geom, C, kind, teacher, 2, is_i64, ref["coef"], True)
            su, du = launch_pair(lib, u, geom, C, kind, teacher, 2, is_i64, ref["coef"], True, shift=1)
            check_against_reference(name, C, su, du, ref)
            assert _biteq(sa, su) and _biteq(da, du), "unaligned operands change the bits (%s)" % name


@pytest.mark.parametrize("case", ["all ignored", "none ignored", "confident region, all ignored"])
@pytest.mark.parametrize("C", [2, 19])
def test_zero_denominators(lib, C, case):
    """a denominator that is 0 with its coef 0: the gradient is finite and inside its bounds ("0 when coef_i == 0")"""
    geom = (5, 9, 33, 65)
    variant = R.VARIANTS[1]
    z, zt, lbl = R.loss_inputs(R.case_seed(geom, C), 1, C, *geom)
    lbl = np.full_like(lbl, 255) if case != "none ignored" else np.where(lbl == 255, 0, lbl).astype(np.uint8)
    region = 1 if case.startswith("confident") else 2
    ref = reference(geom, C, variant, region, (z, zt, lbl), tag=case)
    want_zero = {"all ignored": (4,), "none ignored": (5,), "confident region, all ignored": (4, 6)}[case]
    assert all(ref["sums"][k] == 0 for k in want_zero) and (ref["sums"][6] == 0) == (6 in want_zero)
    zero_coef = {"all ignored": (0, 1), "none ignored": (2,), "confident region, all ignored": (0, 1, 3)}[case]
    assert [i for i in range(4) if ref["coef"][i] == 0] == list(zero_coef)
    ops = Operands(z, zt, lbl)
    for is_i64 in (0, 1):
        sums, dl = launch_pair(lib, ops, geom, C, 0, True, region, is_i64, ref["coef"], True)
        check_against_reference("SoftCE, " + case, C, sums, dl, ref)
        assert float(dl.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def _carved_arguments(entry, base):
    b = Bufs()
    kw = {n: b.out(n, (2 << 20,), U8, 4096) if n in LC.POINTERS and n != "stream" else 0 for n in LC.args_of(entry)}
    kw.update({k: v for k, v in base.items() if k in kw}, stream=_st())
    return b, kw


@pytest.mark.parametrize("entry", ["fwd", "bwd", "cst_fwd", "cst_bwd"])
def test_refused_loss_calls_write_nothing(lib, entry):
    """the refused calls of the host test on carved buffers of 2 MiB each (sums, dlogits and the workspace among them): the same
    code, and no byte of any buffer changes; a refused geometry has workspace_bytes == 0"""
    b, base = _carved_arguments(entry, LC.LOSS_BASE)
    dims = lambda kw: [kw[n] for n in "B C h w H W".split()]
    base["ws_bytes"] = LC.workspace_bytes(lib, *dims(base))
    assert 0 < base["ws_bytes"] <= 2 << 20
    n = 0
    for what, change, code, zero_ws in LC.loss_refusals():
        if any(k not in base for k in change):
            continue                                         # an argument this entry does not take
        kw = dict(base, **{k: v for k, v in change.items() if k != "ws_bytes"})
        need = LC.workspace_bytes(lib, *dims(kw))
        assert (need == 0) == zero_ws, (what, need)
        if isinstance(change.get("ws_bytes"), tuple):
            kw["ws_bytes"] = need + change["ws_bytes"][1]
        elif 0 < need <= 2 << 20:
            kw["ws_bytes"] = need
        assert LC.call(lib, entry, **kw) == code, (entry, what)
        n += 1
    assert n >= 15
    b.untouched()


@pytest.mark.parametrize("entry", ["dinput_fwd", "dinput_bwd"])
def test_refused_dinput_calls_write_nothing(lib, entry):
    b, base = _carved_arguments(entry, LC.DINPUT_BASE)
    n = 0
    for what, change, code in LC.dinput_refusals():
        if not any(k in base for k in change):
            continue
        assert LC.call(lib, entry, **dict(base, **{k: v for k, v in change.items() if k in base})) == code, (entry, what)
        n += 1
    assert n >= 7
    b.untouched()


# ------------------------------------------------------------------------------------------------ discriminator input map
DINPUT = [(1, 1, 1, 1), (3, 4, 5, 257), (2, 3, 4, 512), (5, 7, 5, 7), (8, 5, 24, 42), (5, 7, 3, 4)]


def _dinput_case(K, lib, geom, C, mode, z, g, tag):
    h, w, H, W = geom
    B = z.shape[0]
    geo = R.Geometry(*geom)
    ref = R.dinput_reference(geo, z, mode, g)
    inb = Bufs()
    Z, G = inb.inp("logits", dev(z), BAND), inb.inp("gout", dev(g), BAND)
    dims = dict(B=B, C=C, h=h, w=w, H=H, W=W, stream=_st())
    fb = Bufs()
    out = fb.out("out", (B, C, H, W), F32, BAND)
    for launch in (1, 2):
        assert LC.call(lib, "dinput_fwd", logits=Z, mode=mode, out=out, **dims) == 0
        fb.check(inb)
        if launch == 1:
            first = out.clone()
    assert _biteq(first, out), "out: a second launch gives other bits"
    inside("dinput map mode %d%s" % (mode, tag), out, ref["out"], ref["out_bound"])
    assert _biteq(out, K.dinput_fwd(dev(z), H, W, bool(mode)))
    bb = Bufs()
    sc, dl = bb.out("scratch", (B, C, H, W), F32, BAND), bb.out("dlogits", (B, C, h, w), F32, BAND)
    for launch in (1, 2):
        assert LC.call(lib, "dinput_bwd", logits=Z, mode=mode, gout=G, scratch=sc, dlogits=dl, **dims) == 0
        bb.check(inb)
        if launch == 1:
            first = (sc.clone(), dl.clone())
    assert _biteq(first[0], sc) and _biteq(first[1], dl), "scratch / dlogits: a second launch gives other bits"
    inside("dinput scratch mode %d%s" % (mode, tag), sc, ref["scratch"], ref["scratch_bound"])
    bound = ref["dlogits_scratch_part"] + head_ref.upsample_bwd_bound(ref["dlogits"], ref["scratch_abs"], h, w, H, W)
    inside("dinput dlogits mode %d%s" % (mode, tag), dl, ref["dlogits"], bound)
    assert _biteq(dl, K.dinput_bwd(dev(z), dev(g), bool(mode)))
    ub = Bufs()                                                          # the adjoint entry on the scratch just written
    gin = ub.out("gin", (B, C, h, w), F32, BAND)
    assert LC.call(lib, "up_bwd", gout=sc, gin=gin, **dims) == 0
    ub.check(inb, bb)
    assert _biteq(gin, dl), "hiast_dinput_bwd's dlogits are not hiast_upsample_bilinear_ac_bwd of its scratch"
    return out, dl


@pytest.mark.parametrize("geom", DINPUT, ids=lambda g: "x".join(map(str, g)))
def test_dinput_entries(K, lib, geom):
    h, w, H, W = geom
    for C in (2, 9, 16, 19):
        z = synth.logits_lr(5000 + C, 2, C, h, w, 3.0)
        g = synth.normal_f32(5001 + C, (2, C, H, W))
        for mode in (0, 1):
            _dinput_case(K, lib, geom, C, mode, z, g, "")


def test_dinput_underflowed_probability(K, lib):
    """the case of test_gpu_warmup.py in guard bands: a class whose probability underflows to 0 — the self-information map and
    its gradient stay finite (the + 1e-30 inside the log) and inside their bounds"""
    B, C, h, w, H, W = 1, 19, 4, 6, 16, 24
    z = synth.logits_lr(33, B, C, h, w, 2.0)
    z[:, 5] = -200.0
    out, dl = _dinput_case(K, lib, (h, w, H, W), C, 1, z, np.ones((B, C, H, W), np.float32), ", underflow")
    assert float(out[:, 5].abs().max()) == 0.0 and bool(torch.isfinite(dl).all())


# ------------------------------------------------------------------------------------------------ the intrinsics' error
PROBE = r"""
#include <hip/hip_runtime.h>
__global__ void probe_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int which)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = which == 0 ? __expf(v) : which == 1 ? __logf(v) : which == 2 ? expf(v) : log2f(v);
}
extern "C" int loss_probe(const float* x, float* y, int n, int which, void* stream)
{
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, n, which);
    return (int)hipGetLastError();
}
"""


def library_build():
    """the compiler and the flags hiast_amd/csrc/Makefile builds the library with: $HIPCC or its `HIPCC ?=` default, its FLAGS
    line with $(ARCH) filled in from $ARCH or its `ARCH ?=` default"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "hiast_amd", "csrc", "Makefile")).read()
    default = lambda name: re.search(r"^%s\s*\?=\s*(\S+)" % name, mk, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", os.environ.get("ARCH") or default("ARCH"))
    assert "$" not in flags, flags
    return os.environ.get("HIPCC") or default("HIPCC"), flags.split()


def test_intrinsic_error_constants(tmp_path):
    """the four math calls of the two files, built with the library's compiler and flags, against float64 over dense grids:
    __expf on [-90, 0] and on [0, 1] (KLDIV's exp(q1)), __logf on [1, 19] and on to 21 (KLDIV's S2 = Σ exp(q1) reaches 18 + e),
    expf on [-90, 0], log2f on [1e-30, 1].  The constants of loss_ref.py are at least twice every measurement; the figures are
    printed."""
    import ctypes
    hipcc, flags = library_build()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags
    src, so = tmp_path / "loss_probe.hip", tmp_path / "libloss_probe.so"
    src.write_text(PROBE)
    subprocess.check_call([hipcc] + flags + ["-shared", str(src), "-o", str(so)])
    fn = ctypes.CDLL(str(so)).loss_probe
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def run(which, x):
        xd = dev(x.astype(np.float32))
        yd = torch.empty_like(xd)
        assert fn(xd.data_ptr(), yd.data_ptr(), xd.numel(), which, _st()) == 0
        torch.cuda.synchronize()
        return xd.cpu().numpy().astype(np.float64), yd.cpu().numpy().astype(np.float64)
    n = 1 << 20
    rnd = synth.rng(6000)
    u = R.U
    # __expf
    x, y = run(0, np.concatenate([np.linspace(-90, 0, n), -90 * rnd.random(n), np.linspace(0, 1, n), rnd.random(n)]))
    t = np.exp(x)
    normal = t >= R.EXP_TINY
    rel = np.abs(y - t)[normal] / t[normal] / u
    ax = np.abs(x[normal])
    a_meas, b_meas = float((rel[ax >= 4] / ax[ax >= 4]).max()), float(rel[ax <= 1].max())
    model = float((rel / (R.EXP_A * ax + R.EXP_B)).max())
    tiny = float(np.abs(y - t)[~normal].max())
    print("probe __expf: a = max rel / (u |x|) over |x| >= 4: %.3f   b = max rel / u over |x| <= 1: %.3f   worst rel / model: %.3f   "
          "flushed results: max abs error %.3g" % (a_meas, b_meas, model, tiny))
    # __logf
    s, y = run(1, np.concatenate([np.linspace(1, 19, n), 1 + 18 * rnd.random(n), np.linspace(19, 21, n // 8)]))
    err = np.abs(y - np.log(s)) / u
    c19, c21 = float(err[s <= 19].max()), float(err.max())
    print("probe __logf: c = max abs error / u on [1, 19]: %.3f, on [1, 21]: %.3f" % (c19, c21))
    # expf, log2f
    x, y = run(2, np.concatenate([np.linspace(-90, 0, n), -90 * rnd.random(n)]))
    t = np.exp(x)
    normal = t >= R.EXP_TINY
    ef = float((np.abs(y - t)[normal] / t[normal]).max() / u)
    ef_tiny = float(np.abs(y - t)[~normal].max())
    p, y = run(3, np.concatenate([np.geomspace(1e-30, 1, n), rnd.random(n)]))
    L = np.log2(p)
    l2 = float((np.abs(y - L) / np.maximum(np.abs(L), 1.0)).max() / u)
    print("probe expf: max rel / u %.3f (flushed: %.3g)   log2f: max abs error / (u max(|log2|, 1)) %.3f" % (ef, ef_tiny, l2))
    WORST.update({"probe __expf a": a_meas, "probe __expf b": b_meas, "probe __logf c": c21, "probe expf": ef, "probe log2f": l2})
    assert 2 * a_meas <= R.EXP_A and 2 * b_meas <= R.EXP_B and model <= 0.5 and tiny <= R.EXP_TINY
    assert 2 * c21 <= R.LOG_C
    assert 2 * ef <= R.EXPF_B and ef_tiny <= R.EXP_TINY and 2 * l2 <= R.LOG2_C


def test_zz_report_worst_ratios():
    """prints the worst error / bound per quantity of this run (and the probe's figures); no assertion of its own"""
    for cls in sorted(WORST):
        print("loss worst error/bound  %-44s %.4f" % (cls, WORST[cls]))
