"""The channels-last BatchNorm entries (bn_nhwc.hip) through the C ABI on buffers carved out of 0xFF-filled allocations
(tests/guard_bands.py), entry by entry against float64 (tests/bn_ref.py) with the error bounds derived there.  Inputs sit in NaN
poison; outputs, the workspace and the per-channel vectors start as 0xFF.  After each launch:
  1. both guard bands of every buffer, inputs included, are untouched;
  2. every output payload is finite and fully written (the workspace is exempt from "fully written");
  3. the values are inside the derived bounds, the exact items (dres, dgamma / dbeta, mask bits) bit-equal;
  4. the payload is bit-equal to what the ordinary K.bn_nhwc_* wrapper returns for the same operands;
  5. a second launch gives the same bits (the kernels promise a fixed summation order).
A band holds what one block touches in a pass (16·RPP rows of the tensor, one partial row of the workspace).

entry                               test
hiast_bn_nhwc_stats                 test_nhwc_entries, test_large_mean_statistics, test_grid_cap_and_streaming_stores
hiast_bn_nhwc_stats_from_partial    test_reduction_trees
hiast_bn_nhwc_apply                 test_nhwc_entries (res x relu x mask, running statistics, gamma / beta NULL), test_grid_cap_...
hiast_bn_nhwc_apply_partial         test_nhwc_entries (the partials of the statistics launch), test_reduction_trees
hiast_bn_nhwc_bwd_stats             test_nhwc_entries (gates 0..3; gate 1: a y the test chooses, gate 3: a random bit mask opening
                                    the same set, gate 2: inputs that keep 2^-20 away from a sign change)
hiast_bn_nhwc_bwd_apply             test_nhwc_entries (gates 0..3 x dres x dparam), test_grid_cap_and_streaming_stores
argument checks of all of them      test_refused_calls_write_nothing

NOT covered: the grid cap of the elementwise passes, BNH_APPLY_MAXBLK = 65535 blocks, needs more than 4 GB of activations
(65535 · 16·RPP rows · C · 2 bytes); the statistics cap BNH_MAXBLK = 512 and the streaming-store branch (64 MiB) are."""
import numpy as np
import pytest
import torch

import bn_calls as BC
import bn_ref as R
import guard_bands as GB
import synth
from bn_calls import apply_change, refused_calls
from test_gpu_fp16 import _f16r
from test_gpu_kernels import _bf16r, dev

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
WORST = {}                           # output class -> worst error / bound seen in this run (test_zz_report_worst_ratios)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    from hiast_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ plumbing
def _st():
    return torch.cuda.current_stream().cuda_stream


def _biteq(a, b):
    return (tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype
            and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def _np(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def inside(cls, err, bound):
    """err <= bound everywhere (numpy arrays or tensors); records the worst ratio of the class"""
    err, bound = (torch.as_tensor(a, dtype=torch.float64) for a in (err, bound))
    assert bool(torch.isfinite(err).all()), cls
    over = err > bound
    ratio = float(torch.where(bound > 0, err / bound, torch.where(err > 0, torch.inf, 0.0).to(err)).max())
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    assert not bool(over.any()), "%s: %d element(s) outside the bound, worst error / bound = %.3f" % (cls, int(over.sum()), ratio)


class Bufs:
    """the carved buffers of one launch (or of one case, for the inputs)"""

    def __init__(self):
        self.handles, self.outs = [], {}

    def inp(self, name, t, band):
        p, h = GB.carve(tuple(t.shape), t.dtype, "cuda", band)
        GB.fill(p, t)
        self.handles.append((name, h))
        return p

    def out(self, name, shape, dtype, band, init=None, must_fill=True):
        p, h = GB.carve(tuple(shape), dtype, "cuda", band)
        if init is not None:
            GB.fill(p, init)
        self.handles.append((name, h))
        if must_fill:
            self.outs[name] = p
        return p

    def check(self, *more):
        torch.cuda.synchronize()
        for b in (self,) + more:
            for name, h in b.handles:
                GB.check(h, name)
        for name, p in self.outs.items():
            if p.dtype == torch.uint8:
                continue                              # a mask byte may be 0xFF; its bits are compared with y instead
            assert GB.finite(p), "%s: not finite (an element was not written, or poison was read into it)" % name

    def untouched(self):
        torch.cuda.synchronize()
        for name, h in self.handles:
            GB.check_untouched(h, name)


def act_band(C):
    return GB.round_band(16 * (256 // (C // 8)) * C * 2)        # 16·RPP rows of a 16-bit activation: what a block touches in a pass


def mask_band(C):
    return GB.round_band(16 * (256 // (C // 8)) * (C // 8))


def vec_band(C, item=4):
    return GB.round_band(C * item)


def cl4(t):
    """[M][C] rows -> the 4-d channels-last tensor the K.bn_nhwc_* wrappers take (same memory)"""
    M, C = t.shape
    return t.view(1, M, 1, C).permute(0, 3, 1, 2)


def rows(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


def twice(launch):
    """launch() -> {name: tensor} (checked); run it twice on fresh buffers, require the same bits; -> the first outputs"""
    first = launch()
    second = launch()
    for name, t in first.items():
        assert _biteq(t, second[name]), name + ": a second launch gives other bits"
    return first


def pack_bits(open_):
    """bool [M][C] -> uint8 [M][C/8], bit k of byte (m, g) = channel 8 g + k"""
    M, C = open_.shape
    w = (2 ** torch.arange(8, device=open_.device)).to(torch.int32)
    return (open_.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_bits(mask, C):
    w = (2 ** torch.arange(8, device=mask.device)).to(torch.int32)
    return ((mask.to(torch.int32)[:, :, None] & w) != 0).view(mask.shape[0], C)


class Case:
    """one input set on the device: carved 16-bit inputs, float64 copies for the reference, host parameters"""

    def __init__(self, d, M, C, fmt):
        self.d, self.M, self.C, self.fmt, self.dt = d, M, C, fmt, DT[fmt]
        self.inb = Bufs()
        ab = act_band(C)
        for n in ("x", "res", "dy", "ychosen"):
            setattr(self, n, self.inb.inp(n, dev(d[n]).to(self.dt), ab))
            assert np.array_equal(_np(getattr(self, n).float()), d[n]), n + " is not a value of the storage type"
        self.bits = self.inb.inp("bits", dev(d["bits"]), mask_band(C))
        for n in ("gamma", "beta", "mean", "invstd"):
            setattr(self, n, self.inb.inp(n, dev(d[n]), vec_band(C)))
        self.x64, self.res64, self.dy64 = self.x.double(), self.res.double(), self.dy.double()
        self.open3 = dev(d["open3"])
        self.count = float(d["count"])
        self.rm0 = (0.5 * d["mean"]).astype(np.float32)                  # same sign as the batch mean: 4 u32 |want| IS the bound
        self.rv0 = (0.5 + synth.rng(C).random(C)).astype(np.float32)

    def sums_dev(self, sums):
        return dev(np.stack([np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)], 1))


def check_sums(cls, got, ref, mag, L):
    got = _np(got)
    for i, k in ((0, 2), (1, 4 if cls.endswith("bwd") else 2)):
        inside("%s[%d]" % (cls, i), np.abs(got[:, i] - _np(ref[i])), R.sums_bound(_np(mag[i]), L, k))


# ------------------------------------------------------------------------------------------------ the launches
def launch_stats(lib, c, x=None, M=None):
    x = c.x if x is None else x
    M = c.M if M is None else M
    b = Bufs()
    sums = b.out("sums", (c.C, 2), torch.float64, vec_band(c.C, 16))
    nws = lib.hiast_bn_nhwc_workspace_bytes(c.C)
    ws = b.out("workspace", (nws // 4,), torch.float32, vec_band(c.C, 8), must_fill=False)
    rc = BC.call(lib, "nhwc_stats", x=x, M=M, C=c.C, sums=sums, ws=ws, ws_bytes=nws, fmt=BC.FMT[c.fmt], stream=_st())
    assert rc == 0, rc
    b.check(c.inb)
    return dict(sums=sums, ws=ws)


def launch_apply(lib, c, res, relu, mask, running, affine, sums=None, partial=None, x=None, M=None, count=None):
    x = c.x if x is None else x
    M = c.M if M is None else M
    b = Bufs()
    o = dict(y=b.out("y", (M, c.C), c.dt, act_band(c.C)), save_mean=b.out("save_mean", (c.C,), torch.float32, vec_band(c.C)),
             save_invstd=b.out("save_invstd", (c.C,), torch.float32, vec_band(c.C)))
    if mask:
        o["mask"] = b.out("mask", (M, c.C // 8), torch.uint8, mask_band(c.C))
    if running:
        o["run_mean"] = b.out("run_mean", (c.C,), torch.float32, vec_band(c.C), init=dev(c.rm0))
        o["run_var"] = b.out("run_var", (c.C,), torch.float32, vec_band(c.C), init=dev(c.rv0))
    kw = dict(x=x, res=res, y=o["y"], gamma=c.gamma if affine else None, beta=c.beta if affine else None,
              run_mean=o.get("run_mean"), run_var=o.get("run_var"), count=c.count if count is None else count,
              momentum=R.MOMENTUM, eps=R.EPS, relu=int(relu), save_mean=o["save_mean"], save_invstd=o["save_invstd"], M=M, C=c.C,
              mask=o.get("mask"), fmt=BC.FMT[c.fmt], stream=_st())
    if partial is None:
        rc = BC.call(lib, "nhwc_apply", sums=b.inp("sums", sums, vec_band(c.C, 16)), **kw)
    else:
        rc = BC.call(lib, "nhwc_apply_partial", partial=b.inp("partial", partial, vec_band(c.C, 8)), nblk=partial.shape[0], **kw)
    assert rc == 0, rc
    b.check(c.inb)
    return o


def launch_bwd_stats(lib, c, gate):
    b = Bufs()
    sums = b.out("sums", (c.C, 2), torch.float64, vec_band(c.C, 16))
    nws = lib.hiast_bn_nhwc_workspace_bytes(c.C)
    ws = b.out("workspace", (nws // 4,), torch.float32, vec_band(c.C, 8), must_fill=False)
    rc = BC.call(lib, "nhwc_bwd_stats", dy=c.dy, y={1: c.ychosen, 3: c.bits}.get(gate), x=c.x, gamma=c.gamma, beta=c.beta,
                 save_mean=c.mean, save_invstd=c.invstd, relu=gate, M=c.M, C=c.C, sums=sums, ws=ws, ws_bytes=nws,
                 fmt=BC.FMT[c.fmt], stream=_st())
    assert rc == 0, rc
    b.check(c.inb)
    return dict(sums=sums)


def launch_bwd_apply(lib, c, gate, sums, dres, dparam, big=None):
    x, dy, y, M, count = (c.x, c.dy, {1: c.ychosen, 3: c.bits}.get(gate), c.M, c.count) if big is None else big
    b = Bufs()
    o = dict(dx=b.out("dx", (M, c.C), c.dt, act_band(c.C)))
    if dres:
        o["dres"] = b.out("dres", (M, c.C), c.dt, act_band(c.C))
    if dparam:
        o["dgamma"] = b.out("dgamma", (c.C,), torch.float32, vec_band(c.C))
        o["dbeta"] = b.out("dbeta", (c.C,), torch.float32, vec_band(c.C))
    rc = BC.call(lib, "nhwc_bwd_apply", dy=dy, y=y, x=x, gamma=c.gamma, beta=c.beta, save_mean=c.mean, save_invstd=c.invstd,
                 sums=b.inp("sums", sums, vec_band(c.C, 16)), count=count, relu=gate, dx=o["dx"], dres=o.get("dres"),
                 dgamma=o.get("dgamma"), dbeta=o.get("dbeta"), M=M, C=c.C, fmt=BC.FMT[c.fmt], stream=_st())
    assert rc == 0, rc
    b.check(c.inb)
    return o


# ------------------------------------------------------------------------------------------------ the checks
def check_prep(c, o, sums, running):
    """save_mean / save_invstd / running statistics against prep on the SAME sums (numpy (Σ1, Σ2))"""
    rm0, rv0 = (c.rm0, c.rv0) if running else (None, None)
    mean, invstd, rm, rv = R.prep(sums, c.count, R.MOMENTUM, R.EPS, rm0, rv0)
    bm, bi, brm, brv = R.prep_bounds(sums, c.count, R.MOMENTUM, R.EPS, rm0, rv0)
    inside("save_mean", np.abs(_np(o["save_mean"]).astype(np.float64) - mean), bm)
    inside("save_invstd", np.abs(_np(o["save_invstd"]).astype(np.float64) - invstd), bi)
    if running:
        inside("running_mean", np.abs(_np(o["run_mean"]).astype(np.float64) - rm), brm)
        inside("running_var", np.abs(_np(o["run_var"]).astype(np.float64) - rv), brv)


def check_y(c, o, res, relu, affine, x64=None):
    """y against float64 on the device's OWN save_mean / save_invstd; mask bits against the stored y"""
    g, b = (c.d["gamma"], c.d["beta"]) if affine else (None, None)
    sm, si = _np(o["save_mean"]), _np(o["save_invstd"])
    x64 = c.x64 if x64 is None else x64
    want, _ = R.apply(x64, res, g, b, sm, si, relu)
    pre, mag = R.pre_activation(x64, res, g, b, sm, si)
    inside("y " + c.fmt, (o["y"].double() - want).abs(), R.y_bound(want, mag, c.fmt))
    if "mask" in o:
        differ = unpack_bits(o["mask"], c.C) != (o["y"] > 0)
        if c.fmt == "fp16":
            # an fp32 result o with 0 < o <= 2^-25 sets the bit and is stored as 0.  o lies within the fp32 term of the y bound,
            # 4 u32 mag, of the float64 pre-activation, so only elements with -4 u32 mag < pre < 2^-24 are excused: a clearly
            # negative pre-activation (the value BEFORE the ReLU, not the 0 it becomes) is not.  pre = 0 exactly is excused:
            # with M = 1 and no beta the fp32 result is the rounding residue of x·s - mean·s.
            differ &= ~((pre > -4 * R.U32 * mag) & (pre < 2.0 ** -24))
        assert not bool(differ.any()), "mask bits differ from y > 0 of the stored y at %d element(s)" % int(differ.sum())


def check_dx(c, o, gate_open, gamma, sums, x64=None, dy64=None, dy=None):
    x64, dy64, dy = (c.x64 if x64 is None else x64), (c.dy64 if dy64 is None else dy64), (c.dy if dy is None else dy)
    args = (dy64, gate_open, x64, gamma, c.d["mean"], c.d["invstd"], sums, c.count)
    want, _, dgamma, dbeta = R.bwd_apply(*args)
    inside("dx " + c.fmt, (o["dx"].double() - want).abs(), R.dx_bound(want, *args, c.fmt))
    if "dres" in o:
        exact = dy if gate_open is None else torch.where(gate_open, dy, torch.zeros_like(dy))       # +0 where closed
        assert _biteq(o["dres"], exact), "dres is not dy where open and +0 where closed, bit for bit"
    if "dgamma" in o:
        assert _biteq(o["dgamma"], dev(dgamma)) and _biteq(o["dbeta"], dev(dbeta)), "dgamma / dbeta != float32(sums)"


# ------------------------------------------------------------------------------------------------ every entry, every shape
def test_rounding_helpers_agree():
    a = synth.normal_f32(3, (4096,), 3.0)
    assert np.array_equal(R.round16(a, "bf16"), _bf16r(a)) and np.array_equal(R.round16(a, "fp16"), _f16r(a))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("MC", R.NHWC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_nhwc_entries(K, lib, MC, fmt):
    M, C = MC
    d = R.nhwc_inputs(M, C, fmt)
    for rs in (None, d["res"]):
        assert R.near_zero_count(d["x"], rs, d["gamma"], d["beta"], d["mean"], d["invstd"]) == 0     # before any launch
    c = Case(d, M, C, fmt)
    L = R.chain_nhwc(M, C)
    x4, res4, dy4 = cl4(c.x.clone()), cl4(c.res.clone()), cl4(c.dy.clone())
    g_t, b_t, mu_t, is_t = (dev(d[n]) for n in ("gamma", "beta", "mean", "invstd"))

    # ---- forward statistics
    s = twice(lambda: launch_stats(lib, c))
    check_sums("sums fwd", s["sums"], d["sums"], R.abs_sums_fwd(c.x64), L)
    assert _biteq(s["sums"], K.bn_nhwc_stats(x4))
    S = c.sums_dev(d["sums"])                                            # the float64 sums: the same input on both sides from here

    # ---- forward apply: res x relu with mask, running statistics and affine parameters; then the variants that must not change y
    for with_res in (False, True):
        res, res64 = (c.res, c.res64) if with_res else (None, None)
        for relu in (False, True):
            o = twice(lambda: launch_apply(lib, c, res, relu, True, True, True, sums=S))
            check_prep(c, o, d["sums"], True)
            check_y(c, o, res64, relu, True)
            rm, rv = dev(c.rm0), dev(c.rv0)
            w = K.bn_nhwc_apply(x4, res4 if with_res else None, g_t, b_t, rm, rv, S, c.count, R.MOMENTUM, R.EPS, relu, want_mask=True)
            for got, want in zip((o["y"], o["save_mean"], o["save_invstd"], o["mask"], o["run_mean"], o["run_var"]),
                                 (rows(w[0]), w[1], w[2], w[3], rm, rv)):
                assert _biteq(got, want), "the wrapper returns other bits"
            plain = launch_apply(lib, c, res, relu, False, False, True, sums=S)
            for n in ("y", "save_mean", "save_invstd"):
                assert _biteq(plain[n], o[n]), n + " changes without mask / running statistics"
    for with_res, relu in ((False, True), (True, False)):                  # gamma / beta NULL
        res, res64 = (c.res, c.res64) if with_res else (None, None)
        o = twice(lambda: launch_apply(lib, c, res, relu, True, False, False, sums=S))
        check_prep(c, o, d["sums"], False)
        check_y(c, o, res64, relu, False)
        w = K.bn_nhwc_apply(x4, res4 if with_res else None, None, None, None, None, S, c.count, R.MOMENTUM, R.EPS, relu, want_mask=True)
        assert _biteq(o["y"], rows(w[0])) and _biteq(o["mask"], w[3])

    # ---- apply_partial on the partial rows the statistics launch left in its workspace
    nblk = R.nhwc_nblk(M, C)
    partial = s["ws"][:nblk * C * 2].clone().view(nblk, C, 2)
    assert bool(torch.isfinite(partial).all())
    sdev = _np(s["sums"])
    o = twice(lambda: launch_apply(lib, c, c.res, True, True, True, True, partial=partial))
    check_prep(c, o, (sdev[:, 0], sdev[:, 1]), True)
    check_y(c, o, c.res64, True, True)
    rm, rv = dev(c.rm0), dev(c.rv0)
    w = K.bn_nhwc_apply_partial(x4, res4, g_t, b_t, rm, rv, partial, c.count, R.MOMENTUM, R.EPS, True, want_mask=True)
    assert _biteq(o["y"], rows(w[0])) and _biteq(o["mask"], w[3]) and _biteq(o["run_var"], rv) and _biteq(o["save_invstd"], w[2])

    # ---- backward: the open sets (gate 1 and gate 3 open the same one)
    open2 = R.apply(c.x64, None, d["gamma"], d["beta"], d["mean"], d["invstd"], True)[1]
    opens = {0: None, 1: c.open3, 2: open2, 3: c.open3}
    assert bool(((c.ychosen > 0) == c.open3).all()) and _biteq(pack_bits(c.open3), c.bits)
    wy = {0: None, 1: cl4(c.ychosen.clone()), 2: None, 3: c.bits.clone()}
    got_sums, got_dx = {}, {}
    for gate in (0, 1, 2, 3):
        ref = R.sums_bwd(c.dy64, opens[gate], c.x64, d["mean"], d["invstd"])
        mag = R.abs_sums_bwd(c.dy64, opens[gate], c.x64, d["mean"], d["invstd"])
        o = twice(lambda: launch_bwd_stats(lib, c, gate))
        check_sums("sums bwd", o["sums"], ref, mag, L)
        assert _biteq(o["sums"], K.bn_nhwc_bwd_stats(dy4, wy[gate], x4, g_t, b_t, mu_t, is_t, gate))
        got_sums[gate] = o["sums"]
        ref_np = (_np(ref[0]), _np(ref[1]))
        Sb = c.sums_dev(ref_np)
        full = twice(lambda: launch_bwd_apply(lib, c, gate, Sb, True, True))
        check_dx(c, full, opens[gate], d["gamma"], ref_np)
        w = K.bn_nhwc_bwd_apply(dy4, wy[gate], x4, g_t, b_t, mu_t, is_t, Sb, c.count, gate, True, True)
        for got, want in zip((full["dx"], full["dres"], full["dgamma"], full["dbeta"]), (rows(w[0]), rows(w[1]), w[2], w[3])):
            assert _biteq(got, want), "the wrapper returns other bits"
        for dres, dparam in ((False, False), (True, False), (False, True)):
            part = launch_bwd_apply(lib, c, gate, Sb, dres, dparam)
            for n, t in part.items():
                assert _biteq(t, full[n]), "%s changes with dres=%s dparam=%s" % (n, dres, dparam)
        got_dx[gate] = full["dx"]
    assert _biteq(got_sums[1], got_sums[3]) and _biteq(got_dx[1], got_dx[3]), "gate 1 and gate 3 differ on the same open set"


def test_large_mean_statistics(lib):
    """mean 16, sigma 1 (bf16 values): Σx² is 257x the variance.  The sums go through the SAME bound; save_invstd of an apply on
    the device's sums is then checked against the error that bound propagates: (δS2 + 2|m| δS1) / count into var, and
    d invstd = invstd/2 · δvar / (var + eps) — no tolerance of its own (plus the rounding of prep itself)"""
    M, C = 1000, 256
    d = R.nhwc_inputs(M, C, "bf16", 1, 16.0, 1.0)
    c = Case(d, M, C, "bf16")
    s = launch_stats(lib, c)
    mag = R.abs_sums_fwd(c.x64)
    L = R.chain_nhwc(M, C)
    check_sums("sums fwd", s["sums"], d["sums"], mag, L)
    o = launch_apply(lib, c, None, True, False, False, True, sums=s["sums"].clone())
    mean, invstd, _, _ = R.prep(d["sums"], c.count, R.MOMENTUM, R.EPS)                     # from the float64 sums
    m = d["sums"][0] / M
    var = d["sums"][1] / M - m * m
    dvar = (R.sums_bound(_np(mag[1]), L, 2) + 2 * np.abs(m) * R.sums_bound(_np(mag[0]), L, 2)) / M
    _, b_is, _, _ = R.prep_bounds(d["sums"], c.count, R.MOMENTUM, R.EPS)
    inside("save_invstd (large mean)", np.abs(_np(o["save_invstd"]).astype(np.float64) - invstd),
           0.5 * invstd.astype(np.float64) * dvar / (var + R.EPS) + b_is)


# ------------------------------------------------------------------------------------------------ the reduction trees
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 63, 64, 65, 192, 193, 240, 241, 256, 257, 1000])
def test_reduction_trees(K, lib, nblk, C):
    """stats_from_partial (16 lanes, 16 rows in flight from nblk = 241 on) and apply_partial's finalize (64 lanes, 4 in flight from
    193 on) on test-made fp32 partials of mixed magnitude inside NaN poison, against the float64 column sums at 2^-49 Σ|p|"""
    g = synth.rng(7000 + 10 * nblk + C)
    p1 = g.standard_normal((nblk, C)) * 10.0 ** g.uniform(-3, 3, (nblk, C))
    p2 = np.abs(g.standard_normal((nblk, C))) * 10.0 ** g.uniform(-3, 3, (nblk, C)) + p1 * p1      # Σp2 >= (Σp1)² / nblk: var >= 0
    part = np.stack([p1, p2], 2).astype(np.float32)
    ref = part.astype(np.float64).sum(0)
    mag = np.abs(part.astype(np.float64)).sum(0)
    count = float(16 * nblk)
    b = Bufs()
    P = b.inp("partial", dev(part), vec_band(C, 8))

    def from_partial():
        o = Bufs()
        sums = o.out("sums", (C, 2), torch.float64, vec_band(C, 16))
        assert BC.call(lib, "nhwc_stats_from_partial", partial=P, nblk=nblk, C=C, sums=sums, stream=_st()) == 0
        o.check(b)
        return dict(sums=sums)
    s = twice(from_partial)
    # 2^-49 Σ|p|, twice the 2^-50 first written down: that allowed for 8 roundings of a running double sum; a lane of the 16-lane
    # tree adds nblk / 16 rows one after the other (63 at nblk = 1000) before the 16 lanes are folded
    inside("tree 16 lanes", np.abs(_np(s["sums"]) - ref), 2.0 ** -49 * mag)
    assert _biteq(s["sums"], K.bn_nhwc_stats_from_partial(dev(part)))

    M = 32
    d = R.nhwc_inputs(M, C, "bf16", 2)
    c = Case(d, M, C, "bf16")
    c.count = count
    o = twice(lambda: launch_apply(lib, c, None, True, True, True, True, partial=P))
    # prep on the float64 column sums; the tree's own 2^-49 Σ|p| is propagated into mean (δS1 / n) and invstd
    sums = (ref[:, 0], ref[:, 1])
    mean, invstd, rm, rv = R.prep(sums, count, R.MOMENTUM, R.EPS, c.rm0, c.rv0)
    bm, bi, _, _ = R.prep_bounds(sums, count, R.MOMENTUM, R.EPS, c.rm0, c.rv0)
    inside("tree 64 lanes: save_mean", np.abs(_np(o["save_mean"]).astype(np.float64) - mean), bm + 2.0 ** -49 * mag[:, 0] / count)
    inside("tree 64 lanes: save_invstd", np.abs(_np(o["save_invstd"]).astype(np.float64) - invstd), bi)
    check_y(c, o, None, True, True)
    w = K.bn_nhwc_apply_partial(cl4(c.x.clone()), None, dev(d["gamma"]), dev(d["beta"]), dev(c.rm0), dev(c.rv0), dev(part), count,
                                R.MOMENTUM, R.EPS, True, want_mask=True)
    assert _biteq(o["y"], rows(w[0])) and _biteq(o["save_mean"], w[1]) and _biteq(o["save_invstd"], w[2])


# ------------------------------------------------------------------------------------------------ grid cap, streaming stores
def test_grid_cap_and_streaming_stores(lib):
    """X_big = 4 copies of X_small (4096 x 2048) stacked along M: 16384 x 2048 bf16 = exactly 64 MiB, the size from which the
    outputs are stored with streaming stores, and nblk = 512 (capped; uncapped it would be 1024).  4·sums and 4·count are exact
    in double and so is 1/(4n): every elementwise output of the big launch must be 4 copies of the small launch's, bit for bit"""
    M, C, fmt = 4096, 2048, "bf16"
    d = R.nhwc_inputs(M, C, fmt, 3)
    c = Case(d, M, C, fmt)
    assert 4 * M * C * 2 == 64 << 20 and R.nhwc_nblk(4 * M, C) == 512 < -(-4 * M // 16)
    big = Bufs()
    X, RES, DY, YC = (big.inp(n, getattr(c, n).repeat(4, 1), act_band(C)) for n in ("x", "res", "dy", "ychosen"))
    c.inb.handles += big.handles
    # statistics with the capped grid
    s = launch_stats(lib, c, x=X, M=4 * M)
    mag = R.abs_sums_fwd(c.x64)
    check_sums("sums fwd", s["sums"], (4 * d["sums"][0], 4 * d["sums"][1]), (4 * mag[0], 4 * mag[1]), R.chain_nhwc(4 * M, C))
    # forward
    S1, S4 = c.sums_dev(d["sums"]), c.sums_dev((4 * d["sums"][0], 4 * d["sums"][1]))
    small = launch_apply(lib, c, c.res, True, True, True, True, sums=S1)
    check_prep(c, small, d["sums"], True)
    check_y(c, small, c.res64, True, True)
    o = launch_apply(lib, c, RES, True, True, False, True, sums=S4, x=X, M=4 * M, count=4 * c.count)
    assert _biteq(o["save_mean"], small["save_mean"]) and _biteq(o["save_invstd"], small["save_invstd"])
    assert _biteq(o["y"], small["y"].repeat(4, 1)) and _biteq(o["mask"], small["mask"].repeat(4, 1))
    del o
    # backward, gate 1 on the chosen y (reads all four activation tensors) with dres and the parameter gradients
    ref = R.sums_bwd(c.dy64, c.open3, c.x64, d["mean"], d["invstd"])
    ref_np = (_np(ref[0]), _np(ref[1]))
    small = launch_bwd_apply(lib, c, 1, c.sums_dev(ref_np), True, True)
    check_dx(c, small, c.open3, d["gamma"], ref_np)
    ref4 = (4 * ref_np[0], 4 * ref_np[1])
    o = launch_bwd_apply(lib, c, 1, c.sums_dev(ref4), True, True, big=(X, DY, YC, 4 * M, 4 * c.count))
    assert _biteq(o["dx"], small["dx"].repeat(4, 1)) and _biteq(o["dres"], small["dres"].repeat(4, 1))
    assert _biteq(o["dgamma"], dev(ref4[1].astype(np.float32))) and _biteq(o["dbeta"], dev(ref4[0].astype(np.float32)))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", list(BC.ENTRIES))
def test_refused_calls_write_nothing(lib, entry):
    """the refused calls of the host test on carved buffers, channels-last and NCHW entries alike: the code is the same and no
    byte of any buffer changes.  Every buffer holds the largest tensor of the valid call (B·C·HW 16-bit elements)."""
    M, C, B, HW = 64, 64, 2, 64
    b = Bufs()
    kw = {}
    for n in BC.args_of(entry):
        if n in BC.POINTERS and n != "stream":
            kw[n] = b.out(n, (B * C * HW * 2 + 64,), torch.uint8, 4096)
    base = BC.placeholders(entry, M=M, C=C, B=B, HW=HW)
    base.update(kw, stream=_st())
    need = R.nhwc_nblk(M, C) * C * 2 * 4
    for what, change, code in refused_calls(entry):
        got = BC.call(lib, entry, **apply_change(base, change, need))
        assert got == code, (entry, what, got, code)
    b.untouched()


def test_zz_report_worst_ratios():
    """prints the worst error / bound per output class of this run (the figures DESIGN §2 quotes); no assertion of its own"""
    for cls in sorted(WORST):
        print("bn nhwc worst error/bound  %-28s %.4f" % (cls, WORST[cls]))
