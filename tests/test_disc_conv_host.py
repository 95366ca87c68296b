"""Host side of the discriminator's own 4x4 / stride-2 convolutions (hiast_disc_conv_*, HF.disc_conv4x4s2): what needs no
GPU — the predicate, the workspace-size function, the opt-in switch, the argument checks of the entries (refusals happen before
any launch) and the LeakyReLU gate convention the gradient kernels implement."""
import ctypes
import importlib

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def test_disc_conv_ok_refuses_what_the_kernels_do_not_take(lib):
    from hiast_amd import functional as HF
    x = torch.zeros(1, 19, 8, 16)
    w = torch.zeros(64, 19, 4, 4)
    assert not HF.disc_conv_ok(x, w)                                              # CPU tensors
    xm, wm = x.to("meta"), w.to("meta")                                           # (a meta tensor is no device tensor either)
    assert not HF.disc_conv_ok(xm, wm)
    assert not HF.disc_conv_ok(x.half(), w.half())                                # wrong dtype
    assert not HF.disc_conv_ok(x, torch.zeros(64, 19, 3, 3))                      # 3x3 weight
    assert not HF.disc_conv_ok(x, None) and not HF.disc_conv_ok(None, w)


def test_disc_conv_shape_rules(lib):
    from hiast_amd import functional as HF
    ok = HF.disc_conv_shapes_ok
    assert ok((2, 19, 8, 16), (64, 19, 4, 4))
    for cin in (19, 16, 9, 2, 64, 512):
        for cout in (64, 128, 1):
            assert ok((1, cin, 7, 9), (cout, cin, 4, 4)), (cin, cout)
    assert ok((2, 19, 2, 4), (64, 19, 4, 4))
    assert not ok((2, 19, 8, 16), (64, 19, 3, 3))
    assert not ok((2, 19, 8, 16), (64, 19, 4, 3))
    assert not ok((2, 19, 8, 16), (64, 16, 4, 4))                                    # channel mismatch
    assert not ok((2, 19, 1, 16), (64, 19, 4, 4))                                    # no output row
    assert not ok((2, 5000, 8, 16), (64, 5000, 4, 4))
    assert not ok((19, 8, 16), (64, 19, 4, 4))
    assert not ok((64, 19, 4096, 4096), (64, 19, 4, 4))                              # 2^31 elements and more
    assert not ok((0, 19, 8, 16), (64, 19, 4, 4))


def test_workspace_bytes_is_monotone_in_batch_and_extent(lib):
    f = lib.hiast_disc_conv_workspace_bytes
    for cin, cout in ((19, 64), (2, 64), (64, 128), (256, 512), (512, 1)):
        base = f(1, cin, cout, 2, 4)
        assert base > 0 and base % 4 == 0
        assert base >= 16 * cin * cout * 4                                           # the per-class weight repack of dgrad fits
        prev = base
        for b in (1, 2, 3, 4, 8, 16):
            n = f(b, cin, cout, 64, 128)
            assert n >= prev, ("B", cin, cout, b)
            prev = n
        prev = 0
        for h in (2, 3, 6, 7, 8, 16, 33, 64, 127, 128, 256, 512):
            n = f(2, cin, cout, h, 128)
            assert n >= prev > -1, ("H", cin, cout, h)
            prev = n
        prev = 0
        for w in (2, 3, 4, 9, 10, 16, 33, 64, 127, 128, 256, 1024):
            n = f(2, cin, cout, 64, w)
            assert n >= prev, ("W", cin, cout, w)
            prev = n
    assert f(8, 19, 64, 512, 1024) > f(1, 19, 64, 8, 16)                              # the pixel split does grow the partials
    # refused shapes: size 0
    assert f(0, 19, 64, 8, 16) == 0 and f(1, 0, 64, 8, 16) == 0 and f(1, 19, 0, 8, 16) == 0
    assert f(1, 19, 64, 1, 16) == 0 and f(1, 19, 64, 8, 1) == 0
    assert f(1, 5000, 64, 8, 16) == 0 and f(1, 19, 5000, 8, 16) == 0
    assert f(64, 19, 64, 4096, 4096) == 0


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    """null pointers, refused shapes and a short workspace return the project's codes without touching the device"""
    p = ctypes.c_void_p(256)            # never dereferenced: every call below is refused on the host
    nul = ctypes.c_void_p(0)
    assert lib.hiast_disc_conv_fwd(nul, p, p, p, 1, 19, 64, 8, 16, 1, None) == -1
    assert lib.hiast_disc_conv_fwd(p, p, p, nul, 1, 19, 64, 8, 16, 1, None) == -1
    assert lib.hiast_disc_conv_fwd(p, p, p, p, 0, 19, 64, 8, 16, 1, None) == -1
    assert lib.hiast_disc_conv_fwd(p, p, p, p, 1, 19, 64, 1, 16, 1, None) == -2
    assert lib.hiast_disc_conv_fwd(p, p, p, p, 1, 5000, 64, 8, 16, 1, None) == -2
    need = lib.hiast_disc_conv_workspace_bytes(1, 19, 64, 8, 16)
    assert lib.hiast_disc_conv_dgrad(p, p, p, p, 1, 19, 64, 8, 16, 1, p, need - 1, None) == -3
    assert lib.hiast_disc_conv_dgrad(p, nul, p, p, 1, 19, 64, 8, 16, 1, p, need, None) == -1      # leaky needs y
    assert lib.hiast_disc_conv_dgrad(p, p, p, p, 1, 19, 64, 8, 16, 1, nul, need, None) == -1
    assert lib.hiast_disc_conv_dgrad(p, p, p, p, 1, 19, 64, 8, 1, 1, p, need, None) == -2
    assert lib.hiast_disc_conv_wgrad(p, p, p, p, p, 1, 19, 64, 8, 16, 1, p, need - 1, None) == -3
    assert lib.hiast_disc_conv_wgrad(p, p, p, nul, p, 1, 19, 64, 8, 16, 1, p, need, None) == -1
    assert lib.hiast_disc_conv_wgrad(p, p, p, p, p, 1, 19, 64, 1, 16, 1, p, need, None) == -2
    assert lib.hiast_version() == 6


def test_switch_parses_and_is_opt_in(monkeypatch):
    import hiast_amd.switches as SW
    monkeypatch.delenv("HIAST_DISC_HIP", raising=False)
    fresh = importlib.reload(SW)
    try:
        assert fresh.on("HIAST_DISC_HIP") is False                                   # default: the library path
        assert "HIAST_DISC_HIP" not in fresh.SWITCHES and "HIAST_DISC_HIP" in fresh.OPT_IN
        monkeypatch.setenv("HIAST_DISC_HIP", "1")
        assert fresh.on("HIAST_DISC_HIP") is False                                   # read once at import
        assert importlib.reload(SW).on("HIAST_DISC_HIP") is True
        monkeypatch.setenv("HIAST_DISC_HIP", "yes")
        assert importlib.reload(SW).on("HIAST_DISC_HIP") is False                    # only "1" switches it on
        monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)                       # what the tests flip
        assert SW.on("HIAST_DISC_HIP") is True
    finally:
        monkeypatch.undo()
        importlib.reload(SW)
    assert SW.on("HIAST_DISC_HIP") is False


def test_default_discriminator_path_is_untouched_on_the_cpu(monkeypatch):
    """switch off: plain F.conv2d + leaky_relu, bit for bit; switch on with CPU tensors: the predicate fails, same path"""
    from torch.nn import functional as F
    from hiast_amd import switches as SW
    from hiast_amd.sseg.models.modules.discriminator import FCDiscriminator
    torch.manual_seed(3)
    D = FCDiscriminator(9)
    x = torch.rand(1, 9, 32, 64)
    want = x
    for name in ("conv1", "conv2", "conv3", "conv4", "classifier"):
        m = getattr(D, name)
        want = F.conv2d(want, m.weight, m.bias, stride=2, padding=1)
        if name != "classifier":
            want = F.leaky_relu(want, 0.2)
    assert torch.equal(D(x), want)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    assert torch.equal(D(x), want)
    frozen = {k: v.detach() for k, v in D.named_parameters()}
    assert torch.equal(D(x, frozen), want)


def test_leaky_gate_from_the_saved_output_matches_torch():
    """the gradient kernels gate dy with (y > 0 ? 1 : 0.2) on the layer's OUTPUT y: with slope 0.2 sign(y) is the sign of the
    pre-activation, and y == 0 takes 0.2 — what F.leaky_relu's backward does (checked on the CPU, exact zeros included)"""
    from torch.nn import functional as F
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(4096, generator=g)
    pre[::7] = 0.0
    pre[1::7] = -0.0
    pre[2::7] = torch.finfo(torch.float32).tiny * 0.5            # subnormal: 0.2 * it is still > 0
    dy = torch.randn(4096, generator=g)
    for inplace in (False, True):
        a = pre.clone().requires_grad_(True)
        y = F.leaky_relu(a * 1.0, 0.2, inplace=inplace)
        y.backward(dy)
        gate = torch.where(y.detach() > 0, dy, 0.2 * dy)
        assert torch.equal(a.grad, gate), inplace
