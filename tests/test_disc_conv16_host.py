"""Host side of the 16-bit form of the discriminator's own convolutions (hiast_disc_conv16_*, HIAST_DISC_HIP_16BIT): what needs
no GPU — the switch and its default, the path FCDiscriminator.forward picks for every combination of the two switches and
autocast, and the refusals of the new entries (they happen before any launch)."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def test_switch_is_opt_in_and_off_by_default(monkeypatch):
    import importlib
    from hiast_amd import switches as SW
    assert "HIAST_DISC_HIP_16BIT" in SW.OPT_IN and "HIAST_DISC_HIP_16BIT" not in SW.SWITCHES
    monkeypatch.delenv("HIAST_DISC_HIP_16BIT", raising=False)
    fresh = importlib.reload(importlib.import_module("hiast_amd.switches"))
    try:
        assert fresh.OPT_IN["HIAST_DISC_HIP_16BIT"] is False and fresh.on("HIAST_DISC_HIP_16BIT") is False
    finally:
        importlib.reload(fresh)


class _Autocast:
    """device autocast state without a device: the flags FCDiscriminator.forward reads (torch.autocast("cuda") itself
    disables autocast when there is no GPU); CPU tensors are not touched by it"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = (torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda"))
        if self.dtype is not None:
            torch.set_autocast_enabled("cuda", True)
            torch.set_autocast_dtype("cuda", self.dtype)

    def __exit__(self, *exc):
        torch.set_autocast_enabled("cuda", self.prev[0])
        torch.set_autocast_dtype("cuda", self.prev[1])


@pytest.mark.parametrize("autocast", [None, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("bit16", [False, True])
@pytest.mark.parametrize("hip", [False, True])
def test_forward_path_table(monkeypatch, hip, bit16, autocast):
    """the two switches x autocast off / on (both 16-bit types): F.conv2d without HIAST_DISC_HIP whatever else is set; the fp32
    kernels (fmt None) with HIAST_DISC_HIP alone or without autocast; the 16-bit kernels in the autocast type only with both
    switches under autocast"""
    from hiast_amd import functional as HF, switches as SW
    from hiast_amd.sseg.models.modules import discriminator as DM
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", hip)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", bit16)
    seen, lib_calls = [], []

    def stub(x, weight, bias, leaky, fmt=None):
        seen.append((bool(leaky), fmt))
        return torch.zeros(x.shape[0], weight.shape[0], x.shape[2] // 2, x.shape[3] // 2)

    real_conv2d = DM.F.conv2d

    def conv2d(*a, **k):
        lib_calls.append(1)
        return real_conv2d(*a, **k)

    monkeypatch.setattr(HF, "disc_conv_ok", lambda x, w: True)
    monkeypatch.setattr(HF, "disc_conv4x4s2", stub)
    monkeypatch.setattr(DM.F, "conv2d", conv2d)
    torch.manual_seed(0)
    D = DM.FCDiscriminator(3, ndf=4)
    x = torch.rand(1, 3, 32, 64)
    with torch.no_grad(), _Autocast(autocast):
        out = D(x)
    assert tuple(out.shape) == (1, 1, 1, 2)
    if not hip:
        assert seen == [] and len(lib_calls) == 5
        return
    want = autocast if (bit16 and autocast is not None) else None
    assert lib_calls == []
    assert seen == [(True, want)] * 4 + [(False, want)], seen


def test_autocast_in_another_type_stays_fp32(monkeypatch):
    """autocast types the kernels do not have (float32 'autocast', a CPU-only autocast) leave the fp32 kernels in place"""
    from hiast_amd import switches as SW
    from hiast_amd.sseg.models.modules import discriminator as DM
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", True)
    with _Autocast(torch.float32):
        assert DM._own_fmt() is None
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert DM._own_fmt() is None
    with _Autocast(torch.float16):
        assert DM._own_fmt() is torch.float16
        monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", False)
        assert DM._own_fmt() is None


def test_python_wrappers_refuse_a_wrong_format():
    from hiast_amd import functional as HF, kernels as K
    x, w = torch.zeros(1, 19, 8, 16), torch.zeros(64, 19, 4, 4)
    with pytest.raises(TypeError):
        HF.disc_conv4x4s2(x, w, None, True, torch.float32)
    for bad in (None, 0, K.FMT_SPLIT_BF16, torch.float64):
        with pytest.raises((TypeError, ValueError)):
            K._disc_fmt(bad)
    assert K._disc_fmt(torch.float16) == K.FMT_FP16 == 3 and K._disc_fmt(torch.bfloat16) == K.FMT_BF16 == 1
    assert K._disc_fmt(K.FMT_FP16) == 3


def test_entries_refuse_before_any_launch(lib):
    """the checks of the fp32 entries, plus the format: anything but HIAST_FMT_FP16 / HIAST_FMT_BF16 is HIAST_E_ARG"""
    buf = ctypes.create_string_buffer(64)
    p, nul = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    need = lib.hiast_disc_conv_workspace_bytes(1, 19, 64, 8, 16)
    for fmt in (0, 2, 4, -1, 16):
        assert lib.hiast_disc_conv16_fwd(p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, None) == -1
        assert lib.hiast_disc_conv16_dgrad(p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, p, need, None) == -1
        assert lib.hiast_disc_conv16_wgrad(p, p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, p, need, None) == -1
    for fmt in (1, 3):
        assert lib.hiast_disc_conv16_fwd(nul, p, p, p, 1, 19, 64, 8, 16, 1, fmt, None) == -1
        assert lib.hiast_disc_conv16_fwd(p, p, p, p, 0, 19, 64, 8, 16, 1, fmt, None) == -1
        assert lib.hiast_disc_conv16_fwd(p, p, p, p, 1, 19, 64, 1, 16, 1, fmt, None) == -2
        assert lib.hiast_disc_conv16_fwd(p, p, p, p, 1, 5000, 64, 8, 16, 1, fmt, None) == -2
        assert lib.hiast_disc_conv16_dgrad(p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, p, need - 1, None) == -3
        assert lib.hiast_disc_conv16_dgrad(p, nul, p, p, 1, 19, 64, 8, 16, 1, fmt, p, need, None) == -1      # leaky needs y
        assert lib.hiast_disc_conv16_dgrad(p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, nul, need, None) == -1
        assert lib.hiast_disc_conv16_dgrad(p, p, p, p, 1, 19, 64, 8, 1, 1, fmt, p, need, None) == -2
        assert lib.hiast_disc_conv16_wgrad(p, p, p, p, p, 1, 19, 64, 8, 16, 1, fmt, p, need - 1, None) == -3
        assert lib.hiast_disc_conv16_wgrad(p, p, p, nul, p, 1, 19, 64, 8, 16, 1, fmt, p, need, None) == -1
        assert lib.hiast_disc_conv16_wgrad(p, p, p, p, p, 1, 19, 64, 1, 16, 1, fmt, p, need, None) == -2
