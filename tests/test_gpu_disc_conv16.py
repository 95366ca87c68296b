"""The discriminator's 4x4 / stride-2 convolutions on the matrix cores (hiast_disc_conv16_fwd / _dgrad / _wgrad,
HF.disc_conv4x4s2(..., fmt), HIAST_DISC_HIP_16BIT=1 under autocast) on the MI355X: operands rounded to fp16 / bf16 as they are
staged, fp32 accumulation, fp32 tensors in memory.

Single layers: the host rounds x, w and dy to the format first (fp16: values below 2^-14 in magnitude are set to 0), so the
device's conversion of them is exact, and the reference is float64 on those same tensors; the backward's operand is
g = round_fmt(float32(dy) * (y > 0 ? 1 : 0.2f)) with the gate of the y handed to the entry point.  The tolerance is the rule of
tests/test_gpu_disc_conv.py, not a new constant: max-abs error over max |ref| at most 8 x that of torch's float32 CPU
computation on the same tensors, never asked below 1e-6 (products of two 16-bit operands are exact in fp32: what is left is fp32
accumulation, the error class of the fp32 kernels).

Largest values measured over the single-layer cases (error of the own kernels | error of the float32 CPU computation at that case):
    fp16   forward 3.78e-07 | 1.59e-06   input gradient 1.94e-07 | 5.21e-07   weight / bias 1.33e-07 | 2.59e-07
    bf16   forward 8.44e-07 | 1.03e-07   input gradient 1.80e-07 | 2.04e-07   weight / bias 1.22e-07 | 8.11e-08
Five-layer chain under autocast(fp16), own | F.conv2d: logits 3.7e-04 | 1.2e-03, input gradient 8.2e-02 | 1.0e-01, parameter
gradients 5.1e-05 ... 7.0e-02 | 1.4e-04 ... 5.1e-02 (an unscaled fp16 backward in both; largest ratio 1.48).
"""
import copy
import ctypes

import pytest
import torch
from torch.nn import functional as F

import guard_bands as GB

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 8.0, 1e-6
SIZES = [(8, 16), (7, 9), (6, 10), (2, 4)]
CHANNELS = [(19, 64), (9, 64), (2, 64), (64, 128), (512, 1)]
FMTS = {"fp16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}
FMT_CODE = {"bf16": 1, "fp16": 3}                     # HIAST_FMT_BF16, HIAST_FMT_FP16
WORST = {}            # (format, operation) -> [own error, float32-CPU error] at the case where the own error was largest


@pytest.fixture(scope="module")
def HF():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import functional
    return functional


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _bound(e32):
    return max(MARGIN * e32, FLOOR)


def _note(key, own, e32):
    if key not in WORST or own > WORST[key][0]:
        WORST[key] = [own, e32]


def _small_to_zero(t, fmt):
    """fp16: no subnormal operand reaches the matrix cores from these tensors"""
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t) if fmt == "fp16" else t


def _round(t, fmt):
    """float32 -> the format (nearest even) -> float32"""
    return t.to(FMTS[fmt][0]).float()


def _case(seed, B, Cin, Cout, H, W, fmt=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / (Cin * 16) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(B, Cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1, generator=g)
    if fmt is not None:
        x, w, dy = (_small_to_zero(_round(t, fmt), fmt) for t in (x, w, dy))
    return x, w, b, dy


def _conv(x, w, b):
    return F.conv2d(x, w, b, stride=2, padding=1)


def _fwd_ref(x, w, b, leaky, dtype):
    y = _conv(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype))
    return F.leaky_relu(y, 0.2) if leaky else y


def _gate(dy, y_dev, leaky, fmt):
    """the backward's 16-bit operand: the float32 product, then rounded"""
    if not leaky:
        return dy
    slope = torch.where(y_dev > 0, torch.ones_like(dy), torch.full_like(dy, 0.2))       # 0.2f, as the kernel has it
    return _round(dy * slope, fmt)


def _bwd_ref(x, w, b, g, dtype):
    """gradients of the (linear) convolution for the output gradient g"""
    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    _conv(x, w, b).backward(g.to(dtype))
    return x.grad, w.grad, b.grad


# ------------------------------------------------------------------------------------------------ 1. one layer vs float64
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("leaky", [True, False])
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_layer_vs_float64(HF, cin, cout, leaky, fmt):
    K = HF.K
    dt = FMTS[fmt][0]
    for B in (1, 2):
        for H, W in SIZES:
            x, w, b, dy = _case(1000 * cin + 10 * H + B, B, cin, cout, H, W, fmt)
            xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
            y = K.disc_conv16_fwd(xd, wd, bd, leaky, dt)
            dx = K.disc_conv16_dgrad(dyd, y, wd, xd.shape, leaky, dt)
            dw, db = K.disc_conv16_wgrad(xd, dyd, y, leaky, dt)
            g = _gate(dy, y.cpu(), leaky, fmt)
            ref = (_fwd_ref(x, w, b, leaky, torch.float64),) + _bwd_ref(x, w, b, g, torch.float64)
            cpu = (_fwd_ref(x, w, b, leaky, torch.float32),) + _bwd_ref(x, w, b, g, torch.float32)
            own = (y, dx, dw, db)
            for op, i in (("fwd", 0), ("dgrad", 1), ("wgrad", 2), ("wgrad", 3)):
                assert own[i].shape == ref[i].shape
                e_own, e32 = _err(own[i], ref[i]), _err(cpu[i], ref[i])
                print("disc_conv16 %s %-5s B=%d %dx%d %d->%d leaky=%d out=%d: own %.3e  fp32-cpu %.3e" % (
                    fmt, op, B, H, W, cin, cout, leaky, i, e_own, e32))
                _note((fmt, op), e_own, e32)
                assert e_own <= _bound(e32), (fmt, op, i, B, H, W, cin, cout, leaky, e_own, e32)


def test_zz_report_worst_errors():
    """prints the figures DESIGN §9 quotes (no assertion of its own beyond 'the cases ran')"""
    for fmt in FMTS:
        for op in ("fwd", "dgrad", "wgrad"):
            if (fmt, op) in WORST:
                print("disc_conv16 worst %s %-5s: own %.3e | fp32-cpu %.3e" % ((fmt, op) + tuple(WORST[(fmt, op)])))


# ------------------------------------------------------------------------------------ 2. the rounding is the format's
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_operands_are_rounded_to_the_format(HF, fmt):
    """unrounded inputs: the result is the convolution of the operands rounded to nearest even (the rule of item 1 against
    float64 on the host-rounded operands), it is NOT the fp32 convolution (it leaves the unrounded float64 result by more than
    that rule allows), and it is no coarser than the format: elementwise within (2u + u^2) S + n 2^-24 S of the unrounded
    float64 result, S = sum_k |a_k| |b_k|, n = Cin * 16 terms (no bias, no activation: the formula has no term for either)"""
    dt, u = FMTS[fmt]
    B, cin, cout, H, W = 2, 19, 64, 8, 16
    x, w, _, _ = _case(4242, B, cin, cout, H, W)
    x, w = _small_to_zero(x, fmt), _small_to_zero(w, fmt)
    y = HF.K.disc_conv16_fwd(x.cuda(), w.cuda(), None, False, dt)
    xr, wr = _round(x, fmt), _round(w, fmt)
    ref_r, cpu_r = _fwd_ref(xr, wr, None, False, torch.float64), _fwd_ref(xr, wr, None, False, torch.float32)
    e_own, e32 = _err(y, ref_r), _err(cpu_r, ref_r)
    ref_u = _fwd_ref(x, w, None, False, torch.float64)
    e_unr = _err(y, ref_u)
    S = _conv(x.double().abs(), w.double().abs(), None)
    lim = (2 * u + u * u) * S + cin * 16 * 2.0 ** -24 * S
    d = (y.double().cpu() - ref_u).abs()
    print("disc_conv16 rounding %s: vs rounded operands own %.3e fp32-cpu %.3e | vs unrounded %.3e | worst |err| / limit %.3f" % (
        fmt, e_own, e32, e_unr, float((d / lim.clamp_min(1e-300)).max())))
    assert e_own <= _bound(e32), (fmt, e_own, e32)
    assert e_unr > _bound(e32), (fmt, e_unr, e32)            # a path that stays fp32 fails here
    assert bool((d <= lim).all()), (fmt, float((d / lim.clamp_min(1e-300)).max()))      # a coarser format fails here


# ------------------------------------------------------------------------------------------------ 3. overflow is visible
def test_fp16_overflow_becomes_inf_and_bf16_stays_finite(HF):
    """a gradient above 65504 (what a GradScaler's scale can produce) is inf as an fp16 operand, not a clamped value: the
    optimisers' found_inf check has to see it.  Ordinary values to the kernel: nothing faults."""
    K = HF.K
    B, cin, cout, H, W = 1, 2, 64, 2, 4
    x, w, b, dy = _case(31, B, cin, cout, H, W, "fp16")
    dy[0, 5, 0, 1] = 1e5
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    y = torch.ones_like(dyd)                                  # gate open everywhere: the operand is dy itself
    for dt, finite in ((torch.float16, False), (torch.bfloat16, True)):
        dx = K.disc_conv16_dgrad(dyd, y, wd, xd.shape, True, dt)
        dw, db = K.disc_conv16_wgrad(xd, dyd, y, True, dt)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx).all()) == finite, (dt, dx)
        assert bool(torch.isfinite(dw).all()) == finite, dt
        assert bool(torch.isfinite(db).all()) == finite, dt


# ------------------------------------------------------------------------------------------------ 4. bit reproducibility
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_wgrad_is_bit_reproducible(HF, fmt):
    K = HF.K
    dt = FMTS[fmt][0]
    for (B, cin, cout, H, W) in ((2, 19, 64, 64, 128), (2, 512, 1, 8, 16), (2, 64, 128, 7, 9)):
        x, w, b, dy = _case(77 + cin, B, cin, cout, H, W)
        xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        y = K.disc_conv16_fwd(xd, wd, bd, True, dt)
        dw1, db1 = K.disc_conv16_wgrad(xd, dyd, y, True, dt)
        junk = torch.randn(1 << 20, device="cuda")                                 # other work in between
        dw2, db2 = K.disc_conv16_wgrad(xd, dyd, y, True, dt)
        assert torch.equal(dw1, dw2) and torch.equal(db1, db2), (fmt, B, cin, cout, H, W)
        del junk


# ------------------------------------------------------------------------------------------------------------ 5. extents
BAND = 4096


def _carved(t):
    p, h = GB.carve(tuple(t.shape), t.dtype, "cuda", BAND)
    GB.fill(p, t)
    return p, h


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("entry", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("cout", [64, 1])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 16)])
def test_extents_in_guarded_poisoned_buffers(HF, entry, cout, H, W, fmt):
    """every input and output carved out of a NaN-filled allocation: guard bands untouched after the launch, every output
    element written, no poison read into an output; a format argument that is neither fp16 nor bf16 is refused before anything
    is launched.  The values are compared coarsely (rtol 2u, atol 1e-5 max |ref|; the tight comparison is
    test_layer_vs_float64) with float32 on the CPU on the operands the kernel multiplies: x, w, dy rounded on the host, the
    gate product rounded to the format — against unrounded operands an output near zero is off by many times 2u of itself."""
    from hiast_amd import _lib
    lib = _lib.load()
    u, code = FMTS[fmt][1], FMT_CODE[fmt]
    B, cin = 2, 19
    x0, w0, b0, dy0 = _case(5 + cout + H, B, cin, cout, H, W, fmt)
    y0 = _fwd_ref(x0, w0, b0, True, torch.float32)
    g0 = _gate(dy0, y0, True, fmt)
    Ho, Wo = y0.shape[2:]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.hiast_disc_conv_workspace_bytes(B, cin, cout, H, W)
    assert need > 0
    handles = {}
    if entry == "fwd":
        (x, handles["x"]), (w, handles["w"]), (b, handles["bias"]) = _carved(x0), _carved(w0), _carved(b0)
        y, handles["y"] = GB.carve((B, cout, Ho, Wo), torch.float32, "cuda", BAND)

        def call(f):
            return lib.hiast_disc_conv16_fwd(_vp(x), _vp(w), _vp(b), _vp(y), B, cin, cout, H, W, 1, f, st)
        outs, want, out_names = [y], [y0], ["y"]
    elif entry == "dgrad":
        (dy, handles["dy"]), (yy, handles["y"]), (w, handles["w"]) = _carved(dy0), _carved(y0), _carved(w0)
        ws, handles["workspace"] = GB.carve(need, torch.uint8, "cuda", BAND)
        dx, handles["dx"] = GB.carve((B, cin, H, W), torch.float32, "cuda", BAND)

        def call(f):
            return lib.hiast_disc_conv16_dgrad(_vp(dy), _vp(yy), _vp(w), _vp(dx), B, cin, cout, H, W, 1, f, _vp(ws), need, st)
        outs, want, out_names = [dx], [_bwd_ref(x0, w0, b0, g0, torch.float32)[0]], ["dx", "workspace"]
    else:
        (x, handles["x"]), (dy, handles["dy"]), (yy, handles["y"]) = _carved(x0), _carved(dy0), _carved(y0)
        ws, handles["workspace"] = GB.carve(need, torch.uint8, "cuda", BAND)
        dw, handles["dw"] = GB.carve((cout, cin, 4, 4), torch.float32, "cuda", BAND)
        db, handles["db"] = GB.carve((cout,), torch.float32, "cuda", BAND)

        def call(f):
            return lib.hiast_disc_conv16_wgrad(_vp(x), _vp(dy), _vp(yy), _vp(dw), _vp(db), B, cin, cout, H, W, 1, f, _vp(ws),
                                               need, st)
        outs, want, out_names = [dw, db], list(_bwd_ref(x0, w0, b0, g0, torch.float32)[1:]), ["dw", "db", "workspace"]
    for bad in (0, 2, 4, -1):                                 # fp32 has its own entries; split-bf16 is no type of this kernel
        assert call(bad) == -1, bad                           # HIAST_E_ARG
    torch.cuda.synchronize()
    for name in out_names:
        GB.check_untouched(handles[name], "%s of %s after a refused call" % (name, entry))
    rc = call(code)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, h in handles.items():
        GB.check(h, "%s of %s" % (name, entry))
    for o, r in zip(outs, want):
        assert GB.finite(o), "an output element was not written, or poison was read into it"
        assert torch.allclose(o.cpu(), r, rtol=max(1e-4, 2 * u), atol=1e-5 * float(r.abs().max()))


# ----------------------------------------------------------------------------------------------------- 6. the five-layer chain
def _disc(C, seed):
    from hiast_amd.sseg.models.modules.discriminator import FCDiscriminator
    torch.manual_seed(seed)
    return FCDiscriminator(C)


def _chain_grads(D, x, dtype, device, params=None, autocast=None):
    D = copy.deepcopy(D).to(dtype).to(device)
    x = x.detach().to(dtype).to(device).requires_grad_(True)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        if params == "frozen":
            out = D(x, {k: v.detach() for k, v in D.named_parameters()})
        else:
            out = D(x)
        loss = F.binary_cross_entropy_with_logits(out, torch.zeros_like(out))
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach()) for k, p in D.named_parameters()}
    return out.detach(), loss.detach(), x.grad.detach(), grads


def _spies(K, monkeypatch):
    calls = {}
    for name in ("disc_conv_fwd", "disc_conv_wgrad", "disc_conv16_fwd", "disc_conv16_wgrad"):
        calls[name] = 0

        def spy(*a, _orig=getattr(K, name), _name=name, **k):
            calls[_name] += 1
            return _orig(*a, **k)

        monkeypatch.setattr(K, name, spy)
    return calls


def test_five_layer_chain_under_autocast(HF, monkeypatch):
    """both switches on, torch.autocast(fp16): every layer and every weight gradient goes through the 16-bit entries; detached
    weights launch no weight gradient and give the same dx, bit for bit.  Accuracy is measured against the default path, not
    against the code under test: error against float64 autograd of the unrounded chain, once for the own 16-bit path and once
    for F.conv2d under the same autocast; own <= 2 x library (both are one draw of the same 2^-11 operand-rounding noise, and
    the own path rounds fewer quantities: it stores activations in fp32)."""
    from hiast_amd import switches as SW
    C = 19
    D = _disc(C, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.softmax(torch.randn(2, C, 64, 128, generator=g) * 2.0, 1)          # what the discriminator is fed: a probability map
    ref = _chain_grads(D, x, torch.float64, "cpu")
    assert SW.on("HIAST_DISC_HIP") is False and SW.on("HIAST_DISC_HIP_16BIT") is False
    lib = _chain_grads(D, x, torch.float32, "cuda", autocast=torch.float16)
    calls = _spies(HF.K, monkeypatch)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", True)
    own = _chain_grads(D, x, torch.float32, "cuda", autocast=torch.float16)
    assert calls == {"disc_conv_fwd": 0, "disc_conv_wgrad": 0, "disc_conv16_fwd": 5, "disc_conv16_wgrad": 5}, calls
    assert tuple(own[0].shape) == (2, 1, 2, 4) and own[0].dtype == torch.float32
    checks = [("logits", own[0], lib[0], ref[0]), ("dx", own[2], lib[2], ref[2])]
    checks += [("d" + k, own[3][k], lib[3][k], ref[3][k]) for k in ref[3]]
    assert len(checks) == 2 + 10
    for name, o, l, r in checks:
        e_own, e_lib = _err(o.float(), r), _err(l.float(), r)
        print("disc_conv16 chain %-18s own %.3e  library-fp16 %.3e" % (name, e_own, e_lib))
        assert e_own <= 2.0 * e_lib, (name, e_own, e_lib)
    for k in calls:
        calls[k] = 0
    frozen = _chain_grads(D, x, torch.float32, "cuda", params="frozen", autocast=torch.float16)
    assert calls == {"disc_conv_fwd": 0, "disc_conv_wgrad": 0, "disc_conv16_fwd": 5, "disc_conv16_wgrad": 0}, calls
    assert all(v is None for v in frozen[3].values())
    assert torch.equal(frozen[0], own[0]) and torch.equal(frozen[2], own[2])


def test_switch_selection(HF, monkeypatch):
    """HIAST_DISC_HIP alone stays fp32 under autocast (and is today's HF.disc_conv4x4s2, bit for bit); both switches without
    autocast stay fp32 too"""
    from hiast_amd import switches as SW
    C = 19
    D = _disc(C, 11).cuda()
    g = torch.Generator().manual_seed(13)
    x = torch.softmax(torch.randn(2, C, 64, 128, generator=g) * 2.0, 1).cuda()
    calls = _spies(HF.K, monkeypatch)
    fp32_only = {"disc_conv_fwd": 5, "disc_conv_wgrad": 0, "disc_conv16_fwd": 0, "disc_conv16_wgrad": 0}
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.float16):
            out = D(x)
        assert calls == fp32_only, calls
        want = x
        for name in ("conv1", "conv2", "conv3", "conv4", "classifier"):
            m = getattr(D, name)
            want = HF.disc_conv4x4s2(want, m.weight, m.bias, name != "classifier")
        assert out.dtype == torch.float32 and torch.equal(out, want)
        for k in calls:
            calls[k] = 0
        monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", True)
        out2 = D(x)                                            # no autocast
        assert calls == fp32_only, calls
        assert torch.equal(out2, want)
