"""Round-4 kernels and wiring: the grouped weight-gradient launch (hiast_conv_wgrad_group_nhwc, K9d) and the autograd node
that defers the three weight gradients of a bottleneck to one launch (functional._WGroupFn)."""
import pytest
import torch

from hiast_amd import switches as SW

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ round 4: grouped weight gradients
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cfg", [(2, 24, 40, 512, 256, 2), (1, 33, 47, 1024, 256, 2), (3, 16, 24, 1024, 512, 4),
                                 (8, 64, 128, 1024, 256, 2)])        # the last one: BASELINE configs[2], a layer3 block at B = 8
def test_conv_wgrad_group_vs_single_launches_and_fp32(dt, cfg):
    """hiast_conv_wgrad_group_nhwc (the three weight gradients of a bottleneck in one launch + one reduction) against the
    fp32 weight gradient of the same 16-bit operands and against the one-by-one launches; ragged pixel ranges; repeatable"""
    from hiast_amd import kernels as K
    B, H, W, cin, mid, dl = cfg
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1234)
    mk = lambda c: torch.randn(B, H, W, c, generator=g).to(dt).to(dev)
    x1, d1, x2, d2, x3, d3 = mk(cin), mk(mid), mk(mid), mk(mid), mk(mid), mk(cin)
    jobs = [(d3, x3, 1, 1, 1), (d2, x2, 3, 1, dl), (d1, x1, 1, 1, 1)]
    got = K.conv_wgrad_group(jobs)
    again = K.conv_wgrad_group(jobs)
    for (dy, x, k, _, dil), dw, dw2 in zip(jobs, got, again):
        Cout, Cin = dy.shape[3], x.shape[3]
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, Cin, k, k)
        ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).float(), (Cout, Cin, k, k), dy.permute(0, 3, 1, 2).float(),
                                          stride=1, padding=dil if k == 3 else 0, dilation=dil if k == 3 else 1)
        scale = ref.abs().max().item()
        assert (dw - ref).abs().max().item() <= 1e-4 * scale
        one = K.conv_wgrad_nhwc(dy, x, k, 1, dil)
        assert (dw - one).abs().max().item() <= 2e-5 * scale          # the same products, another summation order
        assert torch.equal(dw, dw2)
    # two jobs (the 1x1 pair of a layer4 block) and the argument checks
    two = K.conv_wgrad_group([jobs[0], jobs[2]])
    assert torch.allclose(two[0], got[0], rtol=0, atol=2e-5 * got[0].abs().max().item())
    with pytest.raises(Exception):
        K.conv_wgrad_group([(mk(64), mk(64), 1, 1, 1), jobs[0]])


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_bottleneck_grouped_weight_gradients_match_the_per_convolution_path(dt, monkeypatch):
    """a layer3-shaped identity bottleneck on the 16-bit training path: the grouped weight-gradient node (_WGroupFn) against
    the per-convolution launches (HIAST_NO_WGROUP=1): same outputs and data gradient bit for bit, weight gradients up to the
    summation order; with and without the side stream; gradient accumulation over two backward passes"""
    from hiast_amd import functional as HF
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    blk = Bottleneck(1024, 256, 1, 2).to(dev).train()
    x0 = torch.randn(2, 1024, 24, 40, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 1024, 24, 40, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
    res = {}
    # (two passes: the second ACCUMULATES into .grad — on the main stream only: with the side stream on, a step must not
    # accumulate, as on the per-convolution path)
    for mode, passes in (("single", 2), ("group", 2), ("single1", 1), ("group_side", 1)):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_NO_WGROUP", mode.startswith("single"))
        HF._wgrad_overlap[0] = mode == "group_side"
        blk.zero_grad()
        for _ in range(passes):
            src = x0.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=dt):
                y = blk(src * 1.0)
            y.backward(gy)
        HF.wgrad_stream_join()
        torch.cuda.synchronize()
        res[mode] = (y.detach().clone(), src.grad.clone(), [c.weight.grad.clone() for c in (blk.conv1, blk.conv2, blk.conv3)])
    HF._wgrad_overlap[0] = False
    for mode, ref in (("group", "single"), ("group_side", "single1")):
        assert torch.equal(res[mode][0], res[ref][0]) and torch.equal(res[mode][1], res[ref][1])
        for a, b in zip(res[mode][2], res[ref][2]):
            assert a.shape == b.shape and (a - b).abs().max().item() <= 2e-5 * b.abs().max().item(), mode


def test_layer4_block_groups_only_its_1x1_pair(monkeypatch):
    """a layer4-shaped block: 68 tiles would fill 204 of 256 CUs, so only conv1 + conv3 share a launch; results as above"""
    from hiast_amd import functional as HF
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    blk = Bottleneck(2048, 512, 1, 4).to(dev).train()
    x0 = torch.randn(1, 2048, 16, 24, device=dev).half().contiguous(memory_format=torch.channels_last)
    gy = torch.randn(1, 2048, 16, 24, device=dev).half().contiguous(memory_format=torch.channels_last)
    wg = HF.wgroup_weights((blk.conv1, blk.conv2, blk.conv3), x0)         # per convolution: (jobs, slot, weight view) or None
    assert wg[1] is None and wg[0][0] is wg[2][0] and [wg[0][1], wg[2][1]] == [0, 1]
    res = {}
    for mode in ("single", "group"):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_NO_WGROUP", mode == "single")
        blk.zero_grad()
        src = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = blk(src * 1.0)
        y.backward(gy)
        torch.cuda.synchronize()
        res[mode] = (src.grad.clone(), [c.weight.grad.clone() for c in (blk.conv1, blk.conv2, blk.conv3)])
    assert torch.equal(res["group"][0], res["single"][0])
    for a, b in zip(res["group"][1], res["single"][1]):
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item()


# ------------------------------------------------------------------------------------------------ the training stem (K9k)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 128), (1, 70, 90), (3, 33, 47), (2, 128, 256), (8, 512, 1024)])
def test_stem_train_fwd_and_wgrad_vs_fp32_on_the_rounded_operands(dt, shape):
    """hiast_stem_train_fwd / hiast_stem_wgrad (conv 7x7 s2 p3, 3 -> 64, of the mixed-precision training forward) against
    torch's fp32 convolution / weight gradient of the SAME 16-bit-rounded operands: outputs within one rounding of the
    16-bit type, the per-block sums equal to the sums of the stored values, dW to fp32 summation order; ragged tiles
    (sizes that are no multiples of the 8 x 16 tile), several images, bitwise repeatable"""
    import torch.nn.functional as F
    from hiast_amd import kernels as K
    B, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(77)
    x = torch.randn(B, 3, H, W, generator=g).to(dev)
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).to(dev)
    fmt = K.FMT_FP16 if dt == torch.float16 else K.FMT_BF16
    y, partial = K.stem_train_fwd(x, w, fmt)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(y.shape) == (B, Hc, Wc, 64) and y.dtype == dt
    xr, wr = x.to(dt).float(), w.to(dt).float()
    ref = F.conv2d(xr, wr, None, 2, 3).permute(0, 2, 3, 1)
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    err = (y.float() - ref).abs()
    assert (err <= eps * ref.abs() + 1e-5 * ref.abs().max()).all(), float(err.max())
    sums = partial.double().sum(0)
    yd = y.double().reshape(-1, 64)
    assert torch.allclose(sums[:, 0], yd.sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(sums[:, 1], (yd * yd).sum(0), rtol=1e-5, atol=1e-3)
    # weight gradient
    dy = torch.randn(B, Hc, Wc, 64, generator=g).to(dt).to(dev)
    dw = K.stem_wgrad(x, dy)
    refw = torch.nn.grad.conv2d_weight(xr, (64, 3, 7, 7), dy.float().permute(0, 3, 1, 2), stride=2, padding=3)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (64, 3, 7, 7)
    assert (dw - refw).abs().max().item() <= (1e-4 if B * H * W < (1 << 21) else 1e-3) * refw.abs().max().item()   # (fp32 sums of 1 M terms)
    assert torch.equal(dw, K.stem_wgrad(x, dy))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_training_forward_with_own_stem_matches_the_library_stem(dt, monkeypatch):
    """ResNet.forward in train mode under 16-bit autocast: the K9k stem (conv + statistics from its epilogue) against the
    library convolution + statistics pass (HIAST_LIB_STEM=1) — trunk output and conv1's weight gradient"""
    from hiast_amd.sseg.models.modules.resnet import ResNet
    torch.manual_seed(3)
    dev = torch.device("cuda:0")
    net = ResNet(layers=(1, 1, 1, 1), strides=(1, 2, 1, 1), dilations=((1, 1), (1, 1), (1, 2), (2, 4))).to(dev).train()
    x = torch.randn(2, 3, 96, 160, device=dev)
    out = {}
    for lib in ("1", "0"):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_LIB_STEM", lib == "1")
        net.zero_grad()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.reset_running_stats()
        with torch.autocast("cuda", dtype=dt):
            y = net(x)
        y.float().square().mean().backward()
        torch.cuda.synchronize()
        out[lib] = (y.detach().float(), net.conv1.weight.grad.clone(), net.bn1.running_mean.clone(), net.bn1.running_var.clone())
    tol = 5e-2 if dt == torch.float16 else 2e-1
    a, b = out["0"], out["1"]
    assert (a[0] - b[0]).abs().max().item() <= tol * b[0].abs().max().item()
    cos = torch.nn.functional.cosine_similarity(a[1].flatten(), b[1].flatten(), dim=0).item()
    # two 16-bit paths whose convolution outputs differ in the last bit: the gates of four blocks and of the pooling decorrelate
    # (the sqrt(e) law of test_gpu_trainstep_oracle.py; measured 0.989 / fp16).  The exact checks of the two kernels are above,
    # and test_training_step_arithmetic_given_the_device_gates bounds conv1's gradient in the assembled step.
    assert cos >= (0.95 if dt == torch.float16 else 0.85), cos
    assert torch.allclose(a[2], b[2], rtol=1e-3, atol=1e-4) and torch.allclose(a[3], b[3], rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------ strided 3x3 data gradient
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cfg", [(2, 32, 48, 128, 128), (1, 33, 47, 128, 128), (3, 16, 18, 64, 128), (1, 40, 24, 256, 256)])
def test_igemm_dgrad_s2_vs_fp32_on_the_rounded_operands(dt, cfg):
    """hiast_igemm_dgrad_s2 (data gradient of a 3x3 / stride-2 / padding-1 convolution: the tile kernel's transposed form)
    against torch's fp32 conv2d_input of the same 16-bit operands: even and odd map sizes, 64 / 128 / 256-column tiles"""
    from hiast_amd import kernels as K
    B, H, W, Cin, Cout = cfg
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(4321)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Hs, Ws, Cout, generator=g).to(dt).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(dev)
    wpt = K.pack_conv_weight(w, K.fmt_of(dy), transpose=True)
    dx = K.igemm_dgrad_s2(dy, wpt, H, W)
    assert tuple(dx.shape) == (B, H, W, Cin) and dx.dtype == dt
    ref = torch.nn.grad.conv2d_input((B, Cin, H, W), w.to(dt).float(), dy.float().permute(0, 3, 1, 2), stride=2,
                                     padding=1).permute(0, 2, 3, 1)
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    err = (dx.float() - ref).abs()
    assert (err <= eps * ref.abs() + 2e-5 * ref.abs().max()).all(), float(err.max())


def test_strided_bottleneck_backward_without_the_library(monkeypatch):
    """a layer2.0-shaped block (3x3 stride 2 + strided downsample) on the 16-bit training path: own transposed data gradient
    against the library's (HIAST_LIB_DGRAD_S2=1)"""
    from hiast_amd import functional as HF
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    import torch.nn as nn
    torch.manual_seed(5)
    dev = torch.device("cuda:0")
    down = nn.Sequential(nn.Conv2d(256, 512, 1, stride=2, bias=False), nn.BatchNorm2d(512))
    blk = Bottleneck(256, 128, 2, 1, down).to(dev).train()
    x0 = torch.randn(2, 256, 32, 48, device=dev).half().contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 512, 16, 24, device=dev).half().contiguous(memory_format=torch.channels_last)
    res = {}
    for own in (False, True):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_LIB_DGRAD_S2", not own)
        blk.zero_grad()
        src = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = blk(src * 1.0)
        y.backward(gy)
        torch.cuda.synchronize()
        res[own] = (y.detach().float(), src.grad.float(), blk.conv1.weight.grad.clone())
    assert torch.equal(res[True][0], res[False][0])
    d = (res[True][1] - res[False][1]).abs()
    assert float(d.max()) <= 2e-2 * float(res[False][1].abs().max())
    assert float(d.mean()) <= 2e-3 * float(res[False][1].abs().mean())
    assert torch.allclose(res[True][2], res[False][2], rtol=0, atol=2e-2 * float(res[False][2].abs().max()))


def test_stage_entry_block_shared_input_gradient_handoff(monkeypatch):
    """a layer3.0-shaped block (stride-1 downsample): conv1's data gradient is added in the epilogue of the downsample
    convolution's data gradient (one rounding, no autograd add kernel) — against the two-gradient form (HIAST_NO_XSUM=1);
    also with a retained graph run twice (the hand-off is consumed once, the second pass falls back to autograd's add)"""
    import torch.nn as nn
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    torch.manual_seed(7)
    dev = torch.device("cuda:0")
    down = nn.Sequential(nn.Conv2d(512, 1024, 1, stride=1, bias=False), nn.BatchNorm2d(1024))
    blk = Bottleneck(512, 256, 1, 1, down).to(dev).train()
    x0 = torch.randn(2, 512, 24, 40, device=dev).half().contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 1024, 24, 40, device=dev).half().contiguous(memory_format=torch.channels_last)
    res = {}
    for off in ("1", "0"):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_NO_XSUM", off == "1")
        blk.zero_grad()
        src = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = blk(src * 1.0)
        y.backward(gy, retain_graph=True)
        g1 = src.grad.clone()
        src.grad = None
        blk.zero_grad()
        y.backward(gy)
        torch.cuda.synchronize()
        res[off] = (y.detach().float(), g1.float(), src.grad.float(), blk.conv1.weight.grad.clone(),
                    blk.downsample[0].weight.grad.clone())
    a, b = res["0"], res["1"]
    assert torch.equal(a[0], b[0])
    for i in (1, 2):        # one fp16 rounding of the sum instead of two
        d = (a[i] - b[i]).abs()
        assert (d <= 2.0 ** -9 * b[i].abs() + 2.0 ** -10 * b[i].abs().max()).all(), float(d.max())
    assert torch.equal(a[2], b[2]) or float((a[2] - b[2]).abs().max()) <= 2.0 ** -9 * float(b[2].abs().max())
    for i in (3, 4):
        assert torch.allclose(a[i], b[i], rtol=0, atol=2e-5 * float(b[i].abs().max()))


# ------------------------------------------------------------------------------------------------ round-3 advisor findings
def test_fused_adam_step_counts_when_a_tensor_sits_out_an_overflow_step():
    """FusedAdam keeps ONE device-side count of skipped (overflow) steps: a parameter that has no gradient during such a step
    must not have it subtracted from its own count.  Sequence: both step; only p0 steps and the step overflows; both step —
    against torch.optim.Adam driven with the unscaled gradients of the steps that were applied to each tensor (round-3 advice:
    t = step - skipped came out one too small, t = 0 gave 1 - beta^0 = 0 and inf parameters)"""
    from hiast_amd.utils.utils import FusedAdam
    torch.manual_seed(11)
    dev = torch.device("cuda:0")
    p_own = [torch.randn(64, 16, device=dev).requires_grad_(True), torch.randn(33, device=dev).requires_grad_(True)]
    p_ref = [p.detach().clone().requires_grad_(True) for p in p_own]
    own = FusedAdam(p_own, lr=1e-2)
    ref = torch.optim.Adam(p_ref, lr=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8, growth_interval=1000)
    scaler.scale(torch.zeros((), device=dev))
    # (who has a gradient, overflow?)
    plan = [((0, 1), False), ((0,), True), ((1,), False), ((0, 1), False), ((1,), True), ((0, 1), False)]
    for who, overflow in plan:
        scale = float(scaler.get_scale())
        gs = {i: torch.randn_like(p_own[i]) for i in who}
        for i, p in enumerate(p_own):
            p.grad = None
            if i in who:
                p.grad = gs[i] * scale
                if overflow:
                    p.grad.view(-1)[0] = float("nan")
        scaler.step(own)
        scaler.update()
        if not overflow:
            for i, p in enumerate(p_ref):
                p.grad = gs[i].clone() if i in who else None
            ref.step()
        for a, b in zip(p_own, p_ref):
            assert torch.isfinite(a).all()
            assert torch.allclose(a.detach(), b.detach(), rtol=2e-6, atol=2e-7), (who, overflow)
    own._fold_steps()
    assert [int(own.state[p]["step"]) for p in p_own] == [int(ref.state[p]["step"]) for p in p_ref] == [3, 4]


def test_small_channel_weight_gradients_on_two_streams_do_not_share_partials(monkeypatch):
    """round-3 advice (high): layer2.0's strided 3x3 has its weight gradient on the MAIN stream (its data gradient used to be
    the library's), the other small-channel weight gradients of the block on the SIDE stream, and all of them shared one
    partial-sum workspace per device — a race.  The workspaces are per (device, stream) now; with the side stream on and kept
    busy, every weight gradient of the block equals the single-stream run bit for bit, repeatedly"""
    import torch.nn as nn
    from hiast_amd import functional as HF
    from hiast_amd import kernels as K
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    torch.manual_seed(13)
    dev = torch.device("cuda:0")
    down = nn.Sequential(nn.Conv2d(256, 512, 1, stride=2, bias=False), nn.BatchNorm2d(512))
    blk = Bottleneck(256, 128, 2, 1, down).to(dev).train()
    x0 = torch.randn(4, 256, 64, 96, device=dev).half().contiguous(memory_format=torch.channels_last)
    gy = torch.randn(4, 512, 32, 48, device=dev).half().contiguous(memory_format=torch.channels_last)
    names = ("conv1", "conv2", "conv3")

    def run(overlap):
        HF._wgrad_overlap[0] = overlap
        blk.zero_grad()
        src = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = blk(src * 1.0)
        y.backward(gy)
        HF.wgrad_stream_join()
        torch.cuda.synchronize()
        return [getattr(blk, n).weight.grad.clone() for n in names] + [blk.downsample[0].weight.grad.clone()]
    try:
        for own_s2 in (True, False):        # (False: the round-3 arrangement — library data gradient, weight gradient on main)
            monkeypatch.setitem(SW.SWITCHES, "HIAST_LIB_DGRAD_S2", not own_s2)
            want = run(False)
            for _ in range(4):
                got = run(True)
                for a, b in zip(got, want):
                    assert torch.equal(a, b)
    finally:
        HF._wgrad_overlap[0] = False
    assert len({k for k in K._wgrad_ws if k[0] == "small"}) >= 2      # one workspace per stream that launched them


# ------------------------------------------------------------------------------------------------ bn3 backward sums from conv1's dgrad
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(8, 64, 128), (2, 50, 77), (1, 64, 65)])
def test_xconv_dgrad_gated_bn_stats_vs_the_two_separate_launches(dt, shape):
    """hiast_xconv_dgrad_gated_bn_stats (conv1's data gradient of an identity bottleneck + the backward sums of the previous
    block's bn3 from its epilogue) against the gated data gradient (hiast_igemm_bn_act) followed by the statistics pass
    (hiast_bn_nhwc_bwd_stats) it replaces: the gradient bit for bit (same products, same order), the sums to fp32 summation
    order; ragged M and a tail panel"""
    from hiast_amd import kernels as K
    B, H, W = shape
    dev = torch.device("cuda:0")
    Kc, N = 256, 1024
    M = B * H * W
    g = torch.Generator(device="cpu").manual_seed(99)
    dy = torch.randn(B, H, W, Kc, generator=g).to(dt).to(dev)
    w = (torch.randn(Kc, N, 1, 1, generator=g) * (2.0 / Kc) ** 0.5).to(dev)        # conv1: N -> Kc
    wpt = K.pack_conv_weight(w, K.fmt_of(dy), transpose=True)
    res = torch.randn(B, H, W, N, generator=g).to(dt).to(dev)
    gate = torch.randint(0, 256, (M, N // 8), generator=g, dtype=torch.uint8).to(dev)
    bx = torch.randn(B, H, W, N, generator=g).to(dt).to(dev)
    bmask = torch.randint(0, 256, (M, N // 8), generator=g, dtype=torch.uint8).to(dev)
    sm = torch.randn(N, generator=g).to(dev) * 0.1
    si = (torch.rand(N, generator=g) + 0.5).to(dev)
    if not K.xconv_dgrad_gated_bn_stats_ok(M, Kc, N):
        pytest.skip("shape below the kernel's minimum")
    dx, partial = K.xconv_dgrad_gated_bn_stats(dy, wpt, res, gate, bx, bmask, sm, si)
    want = K.igemm_bn_act(dy, wpt, 1, None, res, False, 1, 1, res_gate=gate)
    assert torch.equal(dx, want)
    sums = K.bn_nhwc_stats_from_partial(partial)
    to_nchw = lambda t: t.permute(0, 3, 1, 2)
    ref = K.bn_nhwc_bwd_stats(to_nchw(want), bmask, to_nchw(bx), None, None, sm, si, 3)
    scale = ref.abs().max(dim=0).values
    assert ((sums - ref).abs() <= 1e-5 * scale + 1e-3).all(), float((sums - ref).abs().max())


def test_two_identity_bottlenecks_bn3_sums_from_the_next_blocks_conv1(monkeypatch):
    """two layer3-shaped identity blocks in a row on the 16-bit training path: the first block's bn3 takes its backward sums from
    the epilogue of the second block's conv1 data gradient (no statistics pass of its own) — against the unfused form
    (HIAST_NO_BN3_FUSION=1): same outputs, gradients up to the order of the fp32 sums; the fused path really ran"""
    import torch.nn as nn
    from hiast_amd import functional as HF
    from hiast_amd import kernels as K
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    torch.manual_seed(21)
    dev = torch.device("cuda:0")
    net = nn.Sequential(Bottleneck(1024, 256, 1, 2), Bottleneck(1024, 256, 1, 2)).to(dev).train()
    x0 = torch.randn(2, 1024, 48, 64, device=dev).half().contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 1024, 48, 64, device=dev).half().contiguous(memory_format=torch.channels_last)
    calls = {"fused": 0, "stats3": 0}
    real_f, real_s = K.xconv_dgrad_gated_bn_stats, K.bn_nhwc_bwd_stats

    def spy_f(*a, **k):
        calls["fused"] += 1
        return real_f(*a, **k)

    def spy_s(dy, y, x, gamma, beta, sm, si, gate):
        calls["stats3"] += int(gate == 3)
        return real_s(dy, y, x, gamma, beta, sm, si, gate)
    monkeypatch.setattr(K, "xconv_dgrad_gated_bn_stats", spy_f)
    monkeypatch.setattr(K, "bn_nhwc_bwd_stats", spy_s)
    res = {}
    for fuse in (False, True):
        monkeypatch.setitem(SW.SWITCHES, "HIAST_NO_BN3_FUSION", not fuse)
        calls["fused"] = calls["stats3"] = 0
        net.zero_grad()
        src = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = net(src * 1.0)
        y.backward(gy)
        torch.cuda.synchronize()
        res[fuse] = (y.detach().float(), src.grad.float(), [p.grad.clone() for p in net.parameters() if p.grad is not None])
        assert (calls["fused"], calls["stats3"]) == ((1, 1) if fuse else (0, 2)), calls
    a, b = res[True], res[False]
    assert torch.equal(a[0], b[0])
    d = (a[1] - b[1]).abs()
    assert float(d.max()) <= 2e-2 * float(b[1].abs().max()) and float(d.mean()) <= 1e-3 * float(b[1].abs().mean())
    for u, v in zip(a[2], b[2]):
        assert torch.allclose(u, v, rtol=0, atol=5e-3 * float(v.abs().max()))
