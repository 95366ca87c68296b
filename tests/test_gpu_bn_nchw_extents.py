"""The NCHW BatchNorm entries (bn_act.hip: hiast_bn_stats, hiast_bn_act_apply in training and inference, hiast_bn_act_bwd_stats,
hiast_bn_act_bwd_apply) through the C ABI on carved buffers, in fp32, bf16 and fp16, with the five checks of
test_gpu_bn_extents.py (bands, finite and fully written, derived bounds of tests/bn_ref.py and exact items, bit-equal to the
K.bn_* wrapper, same bits on a second launch).  Shapes: one element; HW = 7; HW = 63 (scalar path); HW = 128 (vector path);
HW = 2112 (more than one 256-vector sweep of the statistics kernels; still ONE block per plane in the elementwise grid, which
takes ceil(HW / vector / 1024) blocks); HW = 65 x 127 = 8255 (scalar path, 9 blocks per plane) and HW = 64 x 130 = 8320
(vector path: 1040 vectors of 8 -> 2 blocks, 2080 vectors of 4 -> 3 blocks; the last sweep is a tail that only the first
block's first threads take), so that the block-strided loops of bn_apply_kernel and bn_bwd_apply_kernel run with
gridDim.x > 1 (asserted by test_elementwise_grid_has_several_blocks).  The scalar path is also reached
through its other condition, an activation pointer that is not 16-byte aligned (one element into a payload carved one element
larger): the elementwise outputs must then be bit-equal to the aligned launch; the plane sums are summed in another order on
that path (256 chains of single elements instead of vectors), so they are held to the float64 bound of that order instead.
The relu gate of the backward entries reads a y the test chooses."""
import numpy as np
import pytest
import torch

import bn_calls as BC
import bn_ref as R
import guard_bands as GB
import synth
from test_gpu_bn_extents import DT, WORST, Bufs, _biteq, _np, _st, inside, twice
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (3, 10, 7, 9), (2, 5, 8, 16), (2, 4, 33, 64), (1, 2, 65, 127), (1, 2, 64, 130)]
MULTI_BLOCK = [(1, 2, 65, 127), (1, 2, 64, 130)]          # the shapes whose elementwise grid has more than one block per plane
BAND = GB.round_band(256 * 16)             # what a block touches in a pass: 256 threads x 16 bytes
EPS, MOM = R.EPS, R.MOMENTUM


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    from hiast_amd import _lib
    return _lib.load()


def _inputs(shape, fmt):
    B, C, H, W = shape
    g = synth.rng(9000 + B * 1000 + C * 100 + H * W + len(fmt) + (fmt == "fp16"))
    x = R.round16(g.standard_normal(shape) * 2.0 + 0.3, fmt)
    res, dy = R.round16(g.standard_normal(shape), fmt), R.round16(g.standard_normal(shape), fmt)
    open_ = g.random(shape) < 0.5
    ychosen = R.round16(np.where(open_, np.abs(g.standard_normal(shape)) + 2.0 ** -10, -np.abs(g.standard_normal(shape))), fmt)
    ychosen[~open_ & (g.random(shape) < 0.25)] = 0.0
    gamma = (1.0 + 0.5 * g.standard_normal(C)).astype(np.float32)
    beta = (0.5 * g.standard_normal(C)).astype(np.float32)
    rv = (0.5 + g.random(C)).astype(np.float32)
    return dict(x=x, res=res, dy=dy, open=open_, ychosen=ychosen, gamma=gamma, beta=beta, rv=rv)


class Case:
    """carved device inputs; skew = 1: every activation starts one element into a payload carved one element larger"""

    def __init__(self, d, shape, fmt, skew=0):
        self.d, self.shape, self.fmt, self.dt, self.skew = d, shape, fmt, DT[fmt], skew
        self.B, self.C, self.HW = shape[0], shape[1], shape[2] * shape[3]
        self.n = int(np.prod(shape))
        self.inb = Bufs()
        for name in ("x", "res", "dy", "ychosen"):
            flat = torch.full((self.n + skew,), float("nan"), dtype=self.dt, device="cuda")
            flat[skew:] = dev(d[name]).to(self.dt).flatten()
            setattr(self, name, self.inb.inp(name, flat, BAND)[skew:].view(shape))
            assert getattr(self, name).data_ptr() % 16 == (skew * flat.element_size()) % 16
        for name in ("gamma", "beta"):
            setattr(self, name, self.inb.inp(name, dev(d[name]), BAND))
        self.x64, self.res64, self.dy64 = self.x.double(), self.res.double(), self.dy.double()
        self.open = dev(d["open"])
        self.count = float(self.B * self.HW)
        vec = 4 if fmt == "fp32" else 8
        self.L = R.chain_nchw(self.HW, vec if (self.HW % vec == 0 and not skew) else 1)

    def act_out(self, b, name):
        flat = b.out(name, (self.n + self.skew,), self.dt, BAND, must_fill=False)
        view = flat[self.skew:].view(self.shape)
        b.outs[name] = view                                         # with skew the first element stays poison: not part of the tensor
        return view

    def dims(self):
        return dict(B=self.B, C=self.C, HW=self.HW, dtype=BC.DTYPE[self.fmt], stream=_st())


def _part_dev(sums):
    return dev(np.stack([np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)], 2))        # [C][B][2]


def launch_stats(lib, c):
    b = Bufs()
    part = b.out("part", (c.C, c.B, 2), torch.float64, BAND)
    assert BC.call(lib, "stats", x=c.x, part=part, **c.dims()) == 0
    b.check(c.inb)
    return dict(part=part)


def launch_apply(lib, c, res, relu, affine, part=None, running=None):
    """part: training; running = (mean, var) numpy: updated in training, the statistics in inference"""
    b = Bufs()
    o = dict(y=c.act_out(b, "y"))
    if part is not None:
        o["save_mean"] = b.out("save_mean", (c.C,), torch.float32, BAND)
        o["save_invstd"] = b.out("save_invstd", (c.C,), torch.float32, BAND)
    if running is not None:
        o["run_mean"] = b.out("run_mean", (c.C,), torch.float32, BAND, init=dev(running[0]))
        o["run_var"] = b.out("run_var", (c.C,), torch.float32, BAND, init=dev(running[1]))
    rc = BC.call(lib, "apply", x=c.x, res=res, y=o["y"], gamma=c.gamma if affine else None, beta=c.beta if affine else None,
                 run_mean=o.get("run_mean"), run_var=o.get("run_var"), part=None if part is None else b.inp("part", part, BAND),
                 npart=c.B, count=c.count, momentum=MOM, eps=EPS, relu=int(relu), save_mean=o.get("save_mean"),
                 save_invstd=o.get("save_invstd"), **c.dims())
    assert rc == 0, rc
    b.check(c.inb)
    return o


def launch_bwd_stats(lib, c, relu, mean, invstd):
    b = Bufs()
    part = b.out("part", (c.C, c.B, 2), torch.float64, BAND)
    rc = BC.call(lib, "bwd_stats", dy=c.dy, y=c.ychosen if relu else None, x=c.x, save_mean=b.inp("save_mean", mean, BAND),
                 save_invstd=b.inp("save_invstd", invstd, BAND), relu=int(relu), part=part, **c.dims())
    assert rc == 0, rc
    b.check(c.inb)
    return dict(part=part)


def launch_bwd_apply(lib, c, relu, mean, invstd, part, dres, dparam):
    b = Bufs()
    o = dict(dx=c.act_out(b, "dx"))
    if dres:
        o["dres"] = c.act_out(b, "dres")
    if dparam:
        o["dgamma"] = b.out("dgamma", (c.C,), torch.float32, BAND)
        o["dbeta"] = b.out("dbeta", (c.C,), torch.float32, BAND)
    rc = BC.call(lib, "bwd_apply", dy=c.dy, y=c.ychosen if relu else None, x=c.x, gamma=c.gamma,
                 save_mean=b.inp("save_mean", mean, BAND), save_invstd=b.inp("save_invstd", invstd, BAND),
                 part=b.inp("part", part, BAND), npart=c.B, count=c.count, relu=int(relu), dx=o["dx"], dres=o.get("dres"),
                 dgamma=o.get("dgamma"), dbeta=o.get("dbeta"), **c.dims())
    assert rc == 0, rc
    b.check(c.inb)
    return o


def check_part(cls, got, ref, mag, L, k2):
    got = _np(got)
    for i, k in ((0, 2), (1, k2)):
        inside("%s[%d] nchw" % (cls, i), np.abs(got[:, :, i] - _np(ref[i])), R.sums_bound(_np(mag[i]), L, k))


def check_y(c, o, res64, relu, affine, mean, invstd):
    g, b = (c.d["gamma"], c.d["beta"]) if affine else (None, None)
    want, _ = R.apply(c.x64, res64, g, b, mean, invstd, relu)
    _, mag = R.pre_activation(c.x64, res64, g, b, mean, invstd)
    inside("y " + c.fmt + " nchw", (o["y"].double() - want).abs(), R.y_bound(want, mag, c.fmt))


def run_case(K, lib, c, ref_out=None):
    """every entry on one Case; -> the elementwise outputs (for the comparison of the unaligned with the aligned launch).
    ref_out: skip the wrapper comparison (the wrapper cannot be handed an unaligned tensor) and compare with these instead"""
    d, out = c.d, {}
    wrap = ref_out is None
    xs, rs, dys, ys = (t.clone() for t in (c.x, c.res, c.dy, c.ychosen))                  # ordinary tensors for the wrappers
    g_t, b_t = dev(d["gamma"]), dev(d["beta"])

    # ---- forward statistics, per plane
    ref, mag = R.sums_fwd(c.x64, planes=True), R.abs_sums_fwd(c.x64, planes=True)
    s = twice(lambda: launch_stats(lib, c))
    check_part("sums fwd", s["part"], ref, mag, c.L, 2)
    if wrap:
        assert _biteq(s["part"], K.bn_stats(xs))
    ref_np = (_np(ref[0]), _np(ref[1]))
    part = _part_dev(ref_np)                                            # the float64 plane sums: the same input on both sides
    tot = (ref_np[0].sum(1), ref_np[1].sum(1)) if c.B > 1 else (ref_np[0][:, 0], ref_np[1][:, 0])
    mean, invstd, _, _ = R.prep(tot, c.count, MOM, EPS)
    rm0 = (0.5 * mean).astype(np.float32)

    # ---- training forward
    for with_res in (False, True):
        res, res64 = (c.res, c.res64) if with_res else (None, None)
        for relu in (False, True):
            for affine in ((True, False) if relu != with_res else (True,)):
                o = twice(lambda: launch_apply(lib, c, res, relu, affine, part=part, running=(rm0, d["rv"])))
                _, _, rm, rv = R.prep(tot, c.count, MOM, EPS, rm0, d["rv"])
                bm, bi, brm, brv = R.prep_bounds(tot, c.count, MOM, EPS, rm0, d["rv"])
                sm, si = _np(o["save_mean"]), _np(o["save_invstd"])
                inside("save_mean nchw", np.abs(sm.astype(np.float64) - mean), bm)
                inside("save_invstd nchw", np.abs(si.astype(np.float64) - invstd), bi)
                inside("running_mean nchw", np.abs(_np(o["run_mean"]).astype(np.float64) - rm), brm)
                inside("running_var nchw", np.abs(_np(o["run_var"]).astype(np.float64) - rv), brv)
                check_y(c, o, res64, relu, affine, sm, si)
                key = "y train res=%d relu=%d affine=%d" % (with_res, relu, affine)
                out[key] = o["y"]
                out[key + " save_invstd"] = o["save_invstd"]
                if wrap:
                    wrm, wrv = dev(rm0), dev(d["rv"])
                    w = K.bn_act_apply(xs, rs if with_res else None, g_t if affine else None, b_t if affine else None, wrm, wrv,
                                       part, c.count, MOM, EPS, relu)
                    for got, want in zip((o["y"], o["save_mean"], o["save_invstd"], o["run_mean"], o["run_var"]), (*w, wrm, wrv)):
                        assert _biteq(got, want), "the wrapper returns other bits"
                plain = launch_apply(lib, c, res, relu, affine, part=part)              # no running statistics
                assert _biteq(plain["y"], o["y"]) and _biteq(plain["save_mean"], o["save_mean"])

    # ---- inference forward: mean = running_mean, invstd = 1.0f / sqrtf(running_var + eps) in fp32 (restated on the host)
    is32 = (np.float32(1.0) / np.sqrt(d["rv"] + np.float32(EPS))).astype(np.float32)
    for with_res, relu in ((False, True), (True, False), (True, True)):
        res, res64 = (c.res, c.res64) if with_res else (None, None)
        o = twice(lambda: launch_apply(lib, c, res, relu, True, running=(rm0, d["rv"])))
        assert _biteq(o["run_mean"], dev(rm0)) and _biteq(o["run_var"], dev(d["rv"])), "inference changed the running statistics"
        check_y(c, o, res64, relu, True, rm0, is32)
        out["y infer res=%d relu=%d" % (with_res, relu)] = o["y"]
        if wrap:
            w = K.bn_act_apply(xs, rs if with_res else None, g_t, b_t, dev(rm0), dev(d["rv"]), None, c.count, MOM, EPS, relu)
            assert _biteq(o["y"], w[0])

    # ---- backward: relu gate on a y the test chooses
    mu_t, is_t = dev(mean), dev(invstd)
    for relu in (False, True):
        gate = c.open if relu else None
        ref = R.sums_bwd(c.dy64, gate, c.x64, mean, invstd, planes=True)
        mag = R.abs_sums_bwd(c.dy64, gate, c.x64, mean, invstd, planes=True)
        o = twice(lambda: launch_bwd_stats(lib, c, relu, mu_t, is_t))
        check_part("sums bwd", o["part"], ref, mag, c.L, 4)
        if wrap:
            assert _biteq(o["part"], K.bn_act_bwd_stats(dys, ys if relu else None, xs, mu_t, is_t, relu))
        ref_np = (_np(ref[0]), _np(ref[1]))
        bpart = _part_dev(ref_np)
        tot = (ref_np[0].sum(1), ref_np[1].sum(1)) if c.B > 1 else (ref_np[0][:, 0], ref_np[1][:, 0])
        full = twice(lambda: launch_bwd_apply(lib, c, relu, mu_t, is_t, bpart, True, True))
        args = (c.dy64, gate, c.x64, d["gamma"], mean, invstd, tot, c.count)
        want, _, dgamma, dbeta = R.bwd_apply(*args)
        inside("dx " + c.fmt + " nchw", (full["dx"].double() - want).abs(), R.dx_bound(want, *args, c.fmt))
        exact = c.dy if gate is None else torch.where(gate, c.dy, torch.zeros_like(c.dy))
        assert _biteq(full["dres"], exact), "dres is not dy where open and +0 where closed, bit for bit"
        assert _biteq(full["dgamma"], dev(dgamma)) and _biteq(full["dbeta"], dev(dbeta)), "dgamma / dbeta != float32(sums)"
        if wrap:
            w = K.bn_act_bwd_apply(dys, ys if relu else None, xs, g_t, mu_t, is_t, bpart, c.count, relu, True, True)
            for got, wt in zip((full["dx"], full["dres"], full["dgamma"], full["dbeta"]), w):
                assert _biteq(got, wt), "the wrapper returns other bits"
        for dres, dparam in ((False, False), (True, False), (False, True)):
            some = launch_bwd_apply(lib, c, relu, mu_t, is_t, bpart, dres, dparam)
            for n, t in some.items():
                assert _biteq(t, full[n]), "%s changes with dres=%s dparam=%s" % (n, dres, dparam)
        out["dx relu=%d" % relu], out["dres relu=%d" % relu] = full["dx"], full["dres"]
    if not wrap:
        for n, t in out.items():
            assert _biteq(t, ref_out[n]), n + ": the unaligned launch differs from the aligned one"
    return out


@pytest.mark.parametrize("fmt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_entries(K, lib, shape, fmt):
    run_case(K, lib, Case(_inputs(shape, fmt), shape, fmt))


def test_elementwise_grid_has_several_blocks():
    """the launcher's grid (apply_grid of bn_act.hip, restated in bn_ref.nchw_apply_blocks): the MULTI_BLOCK shapes give
    gridDim.x > 1 in every type, on the scalar and on the vector path; every other shape gives 1"""
    for shape in SHAPES:
        HW = shape[2] * shape[3]
        for vec in (4, 8):
            blocks = R.nchw_apply_blocks(HW, vec if HW % vec == 0 else 1)
            assert (blocks > 1) == (shape in MULTI_BLOCK), (shape, vec, blocks)
    assert R.nchw_apply_blocks(65 * 127, 1) == 9 and R.nchw_apply_blocks(64 * 130, 8) == 2 and R.nchw_apply_blocks(64 * 130, 4) == 3
    assert (64 * 130 // 8) % 256 != 0 and (65 * 127) % 256 != 0                # the last sweep is a partial one


@pytest.mark.parametrize("fmt", ["fp32", "bf16", "fp16"])
def test_unaligned_pointers_take_the_scalar_path(K, lib, fmt):
    shape = (2, 5, 8, 16)                    # HW = 128: the vector path when aligned
    d = _inputs(shape, fmt)
    aligned = run_case(K, lib, Case(d, shape, fmt))
    run_case(K, lib, Case(d, shape, fmt, skew=1), ref_out=aligned)


def test_zz_report_worst_ratios():
    """prints the worst error / bound per output class of this run; no assertion of its own"""
    for cls in sorted(WORST):
        if cls.endswith("nchw"):
            print("bn nchw worst error/bound  %-28s %.4f" % (cls, WORST[cls]))
