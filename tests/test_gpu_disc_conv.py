"""The discriminator's own 4x4 / stride-2 / padding-1 convolutions (hiast_disc_conv_fwd / _dgrad / _wgrad, HF.disc_conv4x4s2,
HIAST_DISC_HIP=1) on the MI355X.

Reference: F.conv2d + leaky_relu in float64 on the CPU, with autograd, on the same float32 inputs.  The tolerance is not a
constant: every comparison also measures torch's float32 CPU convolution against the same float64 reference (max-abs error over
max |ref|), and the own kernel's error must be at most 8 x that (never asked below 1e-6).

Largest values measured over the single-layer cases below (error of the own kernels | error of the float32 CPU convolution):
    forward          1.04e-06 | 9.23e-07
    input gradient   4.13e-07 | 6.52e-07
    weight / bias    5.24e-05 | 5.24e-05   (a bias gradient that is the difference of two pixels: both fp32 results are the same bits)
Five-layer chain: logits 8.1e-07 | 8.8e-07, input gradient 5.0e-07 | 7.5e-07, parameter gradients at most 3.9e-07 | 1.5e-06.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import guard_bands as GB

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 8.0, 1e-6
SIZES = [(8, 16), (7, 9), (6, 10), (2, 4)]
CHANNELS = [(19, 64), (16, 64), (9, 64), (2, 64), (64, 128), (512, 1)]
WORST = {}            # operation -> [own error, float32-CPU error] at the case where the own error was largest


@pytest.fixture(scope="module")
def HF():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import functional
    return functional


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _bound(e32):
    return max(MARGIN * e32, FLOOR)


def _note(op, own, e32):
    if op not in WORST or own > WORST[op][0]:
        WORST[op] = [own, e32]


def _layer(x, w, b, leaky):
    y = F.conv2d(x, w, b, stride=2, padding=1)
    return F.leaky_relu(y, 0.2) if leaky else y


def _case(seed, B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / (Cin * 16) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(B, Cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1, generator=g)
    return x, w, b, dy


def _grads(x, w, b, dy, leaky, dtype):
    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = _layer(x, w, b, leaky)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("leaky", [True, False])
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_layer_vs_float64(HF, cin, cout, leaky):
    assert HF is not None
    for B in (1, 2):
        for H, W in SIZES:
            x, w, b, dy = _case(1000 * cin + 10 * H + B, B, cin, cout, H, W)
            ref = _grads(x, w, b, dy, leaky, torch.float64)
            cpu = _grads(x, w, b, dy, leaky, torch.float32)
            xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
            assert HF.disc_conv_ok(xd, wd)
            y = HF.disc_conv4x4s2(xd, wd, bd, leaky)
            y.backward(dy.cuda())
            own = (y.detach(), xd.grad, wd.grad, bd.grad)
            for op, i in (("fwd", 0), ("dgrad", 1), ("wgrad", 2), ("wgrad", 3)):
                assert own[i].shape == ref[i].shape
                e_own, e32 = _err(own[i], ref[i]), _err(cpu[i], ref[i])
                print("disc_conv %-5s B=%d %dx%d %d->%d leaky=%d out=%d: own %.3e  fp32-cpu %.3e" % (
                    op, B, H, W, cin, cout, leaky, i, e_own, e32))
                _note(op, e_own, e32)
                assert e_own <= _bound(e32), (op, i, B, H, W, cin, cout, leaky, e_own, e32)


def test_zz_report_worst_errors():
    """prints the figures DESIGN §9 and this module's docstring quote (no assertion of its own beyond 'the cases ran')"""
    for op in ("fwd", "dgrad", "wgrad"):
        if op in WORST:
            print("disc_conv worst %-5s: own %.3e | fp32-cpu %.3e" % (op, WORST[op][0], WORST[op][1]))


# ----------------------------------------------------------------------------------------------------- the five-layer chain
def _disc(C, seed):
    from hiast_amd.sseg.models.modules.discriminator import FCDiscriminator
    torch.manual_seed(seed)
    return FCDiscriminator(C)


def _chain_grads(D, x, dtype, device, params=None):
    D = copy.deepcopy(D).to(dtype).to(device)
    x = x.detach().to(dtype).to(device).requires_grad_(True)
    if params == "frozen":
        out = D(x, {k: v.detach() for k, v in D.named_parameters()})
    else:
        out = D(x)
    loss = F.binary_cross_entropy_with_logits(out, torch.zeros_like(out))
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach()) for k, p in D.named_parameters()}
    return out.detach(), loss.detach(), x.grad.detach(), grads


def test_five_layer_chain_vs_float64(HF, monkeypatch):
    from hiast_amd import switches as SW
    C = 19
    D = _disc(C, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.softmax(torch.randn(2, C, 64, 128, generator=g) * 2.0, 1)          # what the discriminator is fed: a probability map
    ref = _chain_grads(D, x, torch.float64, "cpu")
    cpu = _chain_grads(D, x, torch.float32, "cpu")
    calls = {"fwd": 0, "wgrad": 0}
    K = HF.K
    orig_f, orig_w = K.disc_conv_fwd, K.disc_conv_wgrad

    def spy_f(*a, **k):
        calls["fwd"] += 1
        return orig_f(*a, **k)

    def spy_w(*a, **k):
        calls["wgrad"] += 1
        return orig_w(*a, **k)

    monkeypatch.setattr(K, "disc_conv_fwd", spy_f)
    monkeypatch.setattr(K, "disc_conv_wgrad", spy_w)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    own = _chain_grads(D, x, torch.float32, "cuda")
    assert calls == {"fwd": 5, "wgrad": 5}, calls
    assert tuple(own[0].shape) == (2, 1, 2, 4)
    checks = [("logits", own[0], ref[0], cpu[0]), ("loss", own[1], ref[1], cpu[1]), ("dx", own[2], ref[2], cpu[2])]
    checks += [("d" + k, own[3][k], ref[3][k], cpu[3][k]) for k in ref[3]]
    assert len(checks) == 3 + 10
    for name, o, r, c in checks:
        e_own, e32 = _err(o, r), _err(c, r)
        print("disc_conv chain %-18s own %.3e  fp32-cpu %.3e" % (name, e_own, e32))
        assert e_own <= _bound(e32), (name, e_own, e32)
    # detached weights (`params=`): only dx is formed — no weight-gradient launch — and it is the same dx, bit for bit
    calls["fwd"] = calls["wgrad"] = 0
    frozen = _chain_grads(D, x, torch.float32, "cuda", params="frozen")
    assert calls == {"fwd": 5, "wgrad": 0}, calls
    assert all(v is None for v in frozen[3].values())
    assert torch.equal(frozen[0], own[0]) and torch.equal(frozen[2], own[2])


def test_wgrad_is_bit_reproducible(HF):
    K = HF.K
    for (B, cin, cout, H, W) in ((2, 19, 64, 64, 128), (2, 512, 1, 8, 16), (2, 64, 128, 7, 9)):
        x, w, b, dy = _case(77 + cin, B, cin, cout, H, W)
        xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        y = K.disc_conv_fwd(xd, wd, bd, True)
        dw1, db1 = K.disc_conv_wgrad(xd, dyd, y, True)
        junk = torch.randn(1 << 20, device="cuda")                                 # other work in between
        dw2, db2 = K.disc_conv_wgrad(xd, dyd, y, True)
        assert torch.equal(dw1, dw2) and torch.equal(db1, db2), (B, cin, cout, H, W)
        del junk


# ------------------------------------------------------------------------------------------------------------------ extents
BAND = 4096


def _carved(t):
    p, h = GB.carve(tuple(t.shape), t.dtype, "cuda", BAND)
    GB.fill(p, t)
    return p, h


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("entry", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("cout", [64, 1])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 16)])
def test_extents_in_guarded_poisoned_buffers(HF, entry, cout, H, W):
    """every input and output carved out of a NaN-filled allocation: guard bands untouched after the launch, every output
    element written, no poison read into an output"""
    from hiast_amd import _lib
    lib = _lib.load()
    B, cin = 2, 19
    x0, w0, b0, dy0 = _case(5 + cout + H, B, cin, cout, H, W)
    y0 = _layer(x0, w0, b0, True)
    Ho, Wo = y0.shape[2:]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.hiast_disc_conv_workspace_bytes(B, cin, cout, H, W)
    assert need > 0
    handles = {}
    if entry == "fwd":
        (x, handles["x"]), (w, handles["w"]), (b, handles["bias"]) = _carved(x0), _carved(w0), _carved(b0)
        y, handles["y"] = GB.carve((B, cout, Ho, Wo), torch.float32, "cuda", BAND)
        rc = lib.hiast_disc_conv_fwd(_vp(x), _vp(w), _vp(b), _vp(y), B, cin, cout, H, W, 1, st)
        outs, want = [y], [y0]
    elif entry == "dgrad":
        (dy, handles["dy"]), (yy, handles["y"]), (w, handles["w"]) = _carved(dy0), _carved(y0), _carved(w0)
        ws, handles["workspace"] = GB.carve(need, torch.uint8, "cuda", BAND)
        dx, handles["dx"] = GB.carve((B, cin, H, W), torch.float32, "cuda", BAND)
        rc = lib.hiast_disc_conv_dgrad(_vp(dy), _vp(yy), _vp(w), _vp(dx), B, cin, cout, H, W, 1, _vp(ws), need, st)
        outs, want = [dx], [_grads(x0, w0, b0, dy0, True, torch.float32)[1]]
    else:
        (x, handles["x"]), (dy, handles["dy"]), (yy, handles["y"]) = _carved(x0), _carved(dy0), _carved(y0)
        ws, handles["workspace"] = GB.carve(need, torch.uint8, "cuda", BAND)
        dw, handles["dw"] = GB.carve((cout, cin, 4, 4), torch.float32, "cuda", BAND)
        db, handles["db"] = GB.carve((cout,), torch.float32, "cuda", BAND)
        rc = lib.hiast_disc_conv_wgrad(_vp(x), _vp(dy), _vp(yy), _vp(dw), _vp(db), B, cin, cout, H, W, 1, _vp(ws), need, st)
        outs, want = [dw, db], list(_grads(x0, w0, b0, dy0, True, torch.float32)[2:])
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, h in handles.items():
        GB.check(h, "%s of %s" % (name, entry))
    for o, r in zip(outs, want):
        assert GB.finite(o), "an output element was not written, or poison was read into it"
        assert torch.allclose(o.cpu(), r, rtol=1e-4, atol=1e-5 * float(r.abs().max()))     # the right values, too (coarse: the
        # tight comparison is test_layer_vs_float64)


# ----------------------------------------------------------------------------------- the trainer: no library convolution left
H_IMG, W_IMG, C_CLS = 128, 256, 19


@pytest.fixture(scope="module")
def warmup_trainer(tmp_path_factory):
    """one AdversarialWarmupTrainer on a tiny synthetic dataset, built the way tests/test_gpu_warmup.py builds its own, in
    fp32 (apex_opt O0) so that the library path and the own path of the discriminator run the same arithmetic type"""
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL, TRAINER
    from hiast_amd.tools import synth_data
    from make_golden import seeded_state_dict
    root = str(tmp_path_factory.mktemp("disc_conv"))
    cfg = synth_data.synthetic_cfg(root, n_train=4, n_val=2, h=H_IMG, w=W_IMG)
    cfg.train.apex_opt = "O0"
    cfg.dataset.source.type = "Cityscapes"
    cfg.dataset.source.json_path = cfg.dataset.target.json_path
    cfg.dataset.source.image_dir = cfg.dataset.target.image_dir
    cfg.dataset.source.aug_type = ["PRS-%d-%d" % (H_IMG, W_IMG)]
    cfg.dataset.target.aug_type = ["PRS-%d-%d" % (H_IMG, W_IMG)]
    m = MODEL["SourceOnlySegmentor"](cfg)
    sd = {"seg_model." + k: v for k, v in seeded_state_dict(m.seg_model, 778).items()}
    m.load_state_dict(sd)
    m = m.cuda()
    ds = np.stack([synth_data.make_sample(5 + i, H_IMG, W_IMG)[0].astype(np.float32).transpose(2, 0, 1) for i in range(2)]) / 255.0
    synth_data.calibrate_bn(m, torch.from_numpy((ds - 0.45) / 0.225).cuda())
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    del m
    ck = os.path.join(root, "imagenet_like.pth")
    torch.save(sd, ck)
    cfg.train.resume_from = ck
    cfg.train.gpu_num = 1
    cfg.train.batch_size = 2
    cfg.train.iter_report = 1
    cfg.trainer = "AdversarialWarmupTrainer"
    cfg.model.type = "AdversarialWarmupSegmentor"
    cfg.model.discriminator.is_enabled = True
    cfg.model.discriminator.D_loss.type = "BCEWithLogits"
    cfg.model.predictor.ent_loss.weight = 3.0
    cfg.train.total_iter = 2
    cfg.train.iter_val = 2
    cfg.work_dir = os.path.join(root, "work")
    cfg.freeze()
    torch.manual_seed(21)
    return TRAINER[cfg.trainer](cfg, 0)


def _count_disc_convs(fn):
    """the dispatch-mode counter of tests/test_gpu_fp16.py (every aten op of the step passes it, autograd's backward included),
    narrowed to the discriminator: aten convolution / convolution_backward calls whose weight is [*, *, 4, 4]"""
    from torch.utils._python_dispatch import TorchDispatchMode
    seen = []

    class DiscConvCounter(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "convolution" in str(func):
                if any(isinstance(a, torch.Tensor) and a.dim() == 4 and tuple(a.shape[2:]) == (4, 4) for a in args[:3]):
                    seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with DiscConvCounter():
        out = fn()
    torch.cuda.synchronize()
    return out, seen


def test_warmup_iteration_runs_no_library_convolution_in_the_discriminator(HF, warmup_trainer, monkeypatch):
    from hiast_amd import switches as SW
    from hiast_amd.sseg.datasets import utils as du
    tr = warmup_trainer
    net = tr.model.module
    s_img, s_lbl = du.batch_to_device(tr.next_source_batch(), tr.device)
    t_img, _ = du.batch_to_device(tr.next_target_batch(), tr.device)
    d0 = net.D.conv1.weight.detach().clone()

    def forward_only():
        return {k: float(torch.mean(v.detach().float())) for k, v in tr.train_on(s_img, s_lbl, t_img).items()}

    def iteration():
        losses = tr.train_on(s_img, s_lbl, t_img)
        vals = {k: float(torch.mean(v.detach().float())) for k, v in losses.items()}
        tr.update_model(tr.g_optimizer, tr.d_optimizer, losses)
        return vals

    # the same weights through both paths: the losses agree within the float32 error of this discriminator at this size (CPU
    # float32 against float64 on a probability map of the same shape), scaled by the loss
    assert SW.on("HIAST_DISC_HIP") is False
    off = forward_only()
    with monkeypatch.context() as mp:
        mp.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
        on = forward_only()
    g = torch.Generator().manual_seed(4)
    x = torch.softmax(torch.randn(2, C_CLS, H_IMG, W_IMG, generator=g) * 2.0, 1)
    Dc = copy.deepcopy(net.D).cpu()
    with torch.no_grad():
        y64, y32 = copy.deepcopy(Dc).double()(x.double()), Dc(x)
    e32 = _err(y32, y64)
    assert set(on) == set(off) == {"source_seg_loss", "adv_loss", "D_loss", "target_ent_loss"}
    for k in off:
        print("disc_conv trainer %-16s library %.9g  own %.9g  (fp32-cpu logits error %.3e)" % (k, off[k], on[k], e32))
        assert np.isfinite(on[k]) and abs(on[k] - off[k]) <= _bound(e32) * max(abs(on[k]), abs(off[k])), (k, on[k], off[k], e32)

    # one whole iteration (forward, both backward passes, both optimiser steps) under the counter: library path, then own path
    first, seen_off = _count_disc_convs(iteration)
    assert len(seen_off) >= 15, seen_off                      # 3 passes x 5 layers forward, and their backward
    assert all(abs(first[k] - off[k]) <= _bound(e32) * abs(off[k]) for k in off), (first, off)     # the same forward as above
    d1 = net.D.conv1.weight.detach().clone()
    assert not torch.equal(d0, d1)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    second, seen_on = _count_disc_convs(iteration)
    assert seen_on == [], seen_on                             # the feature: not one aten convolution left in the discriminator
    assert all(np.isfinite(v) for v in second.values()), second
    assert not torch.equal(d1, net.D.conv1.weight.detach()), "discriminator did not move"
    assert all(torch.isfinite(p).all() for p in net.D.parameters())
