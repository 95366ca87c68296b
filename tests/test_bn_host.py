"""Host side of the BatchNorm tests (no GPU): the float64 reference of tests/bn_ref.py against torch autograd, the error bounds
against a float32 restatement of the kernels' summation order (inside for the real order, outside once a term is dropped or
its sign flipped), the input-condition checker the gate-2 cases rely on, and the argument checks of every hiast_bn_nhwc_* /
hiast_bn_* entry (refusals happen before any launch, so placeholder addresses are never dereferenced)."""
import numpy as np
import pytest
import torch

import bn_calls as BC
import bn_ref as R
import synth
from bn_calls import E_ARG, E_RANGE, E_WS


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ bn_ref vs autograd
AUTOGRAD_SHAPES = [(3, 5, 2, 3), (2, 8, 7, 9), (4, 16, 1, 1)]
RTOL = 1e-12


def _close(got, want, what):
    """rtol 1e-12; an element that is the difference of O(max) terms (y next to 0, dx) cannot be relatively accurate in ANY float64
    evaluation, so a few double roundings of the largest element (1e-15 max|want|) are granted as an absolute term"""
    want = want.detach().numpy()
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=RTOL, atol=1e-15 * np.abs(want).max(), err_msg=what)


def _draw(shape, seed):
    g = synth.rng(seed)
    C = shape[1]
    x = g.standard_normal(shape) * 2.0 + 0.3
    res, dy = g.standard_normal(shape), g.standard_normal(shape)
    gamma, beta = 1.0 + 0.5 * g.standard_normal(C), 0.5 * g.standard_normal(C)
    rm, rv = g.standard_normal(C), 0.5 + g.random(C)
    return x, res, dy, gamma, beta, rm, rv


def _cl(a):
    """NCHW -> channels-last rows [M][C]"""
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, a.shape[1])


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES)
def test_ref_matches_float64_autograd(shape, with_res, relu, layout):
    x, res, dy, gamma, beta, rm, rv = _draw(shape, 11)
    C, count = shape[1], x.size // shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
    xt = torch.from_numpy(x).requires_grad_(True)
    rt = torch.from_numpy(res).requires_grad_(True)
    yt = bn(xt) + rt if with_res else bn(xt)
    yt = torch.relu(yt) if relu else yt
    yt.backward(torch.from_numpy(dy))

    f = _cl if layout == "nhwc" else (lambda a: a)
    xa, ra, da = f(x), (f(res) if with_res else None), f(dy)
    sums = R.sums_fwd(xa)
    mean, invstd, nrm, nrv = R.prep(sums, count, R.MOMENTUM, R.EPS, rm, rv, exact=True)
    y, open_ = R.apply(xa, ra, gamma, beta, mean, invstd, relu)
    _close(y, f(yt) if layout == "nchw" else torch.from_numpy(_cl(yt.detach().numpy())), "y")
    _close(nrm, bn.running_mean, "running_mean")
    _close(nrv, bn.running_var, "running_var")
    gate = open_ if relu else None
    bs = R.sums_bwd(da, gate, xa, mean, invstd)
    dx, dres, dgamma, dbeta = R.bwd_apply(da, gate, xa, gamma, mean, invstd, bs, count)
    t = (lambda a: torch.from_numpy(_cl(a.detach().numpy()))) if layout == "nhwc" else (lambda a: a)
    _close(dx, t(xt.grad), "dx")
    if with_res:
        _close(dres, t(rt.grad), "dres")
    np.testing.assert_allclose(bs[1], bn.weight.grad.numpy(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(bs[0], bn.bias.grad.numpy(), rtol=RTOL, atol=0)
    assert dgamma.dtype == np.float32 and np.array_equal(dgamma, bs[1].astype(np.float32))
    assert dbeta.dtype == np.float32 and np.array_equal(dbeta, bs[0].astype(np.float32))


def test_per_plane_sums_add_up():
    x, _, dy, _, _, _, _ = _draw((3, 5, 4, 6), 12)
    s, sp = R.sums_fwd(x), R.sums_fwd(x, planes=True)
    assert sp[0].shape == (5, 3)
    np.testing.assert_allclose(sp[0].sum(1), s[0], rtol=1e-13)
    np.testing.assert_allclose(sp[1].sum(1), s[1], rtol=1e-13)


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES)
def test_bwd_with_an_arbitrary_open_set(shape):
    """(bn(x) + res) * open for a random 0/1 tensor: what gates 1 and 3 of the channels-last backward are handed"""
    x, res, dy, gamma, beta, rm, rv = _draw(shape, 13)
    C, count = shape[1], x.size // shape[1]
    open_ = synth.rng(14).random(shape) < 0.5
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
    xt = torch.from_numpy(x).requires_grad_(True)
    rt = torch.from_numpy(res).requires_grad_(True)
    ((bn(xt) + rt) * torch.from_numpy(open_)).backward(torch.from_numpy(dy))
    mean, invstd, _, _ = R.prep(R.sums_fwd(x), count, R.MOMENTUM, R.EPS, exact=True)
    bs = R.sums_bwd(dy, open_, x, mean, invstd)
    dx, dres, _, _ = R.bwd_apply(dy, open_, x, gamma, mean, invstd, bs, count)
    _close(dx, xt.grad, "dx")
    _close(dres, rt.grad, "dres")
    np.testing.assert_allclose(bs[1], bn.weight.grad.numpy(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(bs[0], bn.bias.grad.numpy(), rtol=RTOL, atol=0)
    assert np.array_equal(np.asarray(dres)[~open_], np.zeros((~open_).sum()))


def test_prep_clamps_and_uses_the_biased_variance_for_one_element():
    s = (np.array([3.0, 2.0]), np.array([9.0, 3.9]))          # count 1: var = 0;  a negative var (3.9 - 4): clamped
    mean, invstd, nrm, nrv = R.prep(s, 1, 0.1, 1e-5, np.zeros(2), np.ones(2))
    assert np.array_equal(mean, np.float32([3, 2]))
    want = np.float32(1.0 / np.sqrt(float(np.float32(1e-5))))
    assert np.array_equal(invstd, np.float32([want, want]))
    np.testing.assert_allclose(nrv, [float(np.float32(1) - np.float32(0.1))] * 2, rtol=1e-15)   # + momentum * 0, no count/(count-1)
    _, _, _, nrv2 = R.prep((np.array([0.0]), np.array([8.0])), 2, 0.1, 1e-5, np.zeros(1), np.zeros(1))
    np.testing.assert_allclose(nrv2, [float(np.float32(0.1)) * 8.0], rtol=1e-7)                 # var 4, unbiased 8


def test_round16_is_round_to_nearest_even():
    a = synth.normal_f32(15, (4096,), 3.0)
    assert np.array_equal(R.round16(a, "bf16"), torch.from_numpy(a).bfloat16().float().numpy())
    assert np.array_equal(R.round16(a, "fp16"), torch.from_numpy(a).half().float().numpy())
    ties = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])          # halfway between two bf16 values
    assert np.array_equal(R.round16(ties, "bf16"), np.float32([1.0, 1.0 + 2.0 ** -6]))


# ------------------------------------------------------------------------------------------------ the bounds are not vacuous
def _outside(got, ref, bound):
    return np.abs(got - ref) > bound


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("MC", R.NHWC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_order_in_float32_stays_inside_the_sums_bound(MC, fmt):
    """the restatement of the kernels' order (fp32 chain per thread, fp32 fold of RPP chains, double over the blocks) is inside
    (L + k) u32 Σ|term| for every input set of the device tests; with ONE term dropped, or its sign flipped, it is outside"""
    M, C = MC
    d = R.nhwc_inputs(M, C, fmt)
    assert R.near_zero_count(d["x"], None, d["gamma"], d["beta"], d["mean"], d["invstd"]) == 0
    assert R.near_zero_count(d["x"], d["res"], d["gamma"], d["beta"], d["mean"], d["invstd"]) == 0
    L = R.chain_nhwc(M, C)
    x = d["x"].astype(np.float64)
    g = d["dy"].astype(np.float64) * d["open3"]
    xh = ((d["x"] - d["mean"]).astype(np.float32) * d["invstd"]).astype(np.float32).astype(np.float64)   # two fp32 roundings
    cases = [("fwd", x, x * x, R.sums_fwd(d["x"]), R.abs_sums_fwd(d["x"]), (2, 2)),
             ("bwd", g, g * xh, R.sums_bwd(d["dy"], d["open3"], d["x"], d["mean"], d["invstd"]),
              R.abs_sums_bwd(d["dy"], d["open3"], d["x"], d["mean"], d["invstd"]), (2, 4))]
    for name, t1, t2, ref, mag, ks in cases:
        got = R.nhwc_sums_f32_order(t1, t2, C)
        for i in (0, 1):
            bound = R.sums_bound(mag[i], L, ks[i])
            assert not _outside(got[i], ref[i], bound).any(), (name, i, float((np.abs(got[i] - ref[i]) / bound).max()))
        # one term of one channel: the largest there is (a term of ordinary size, not a rounding-sized one).  With M = 1 every
        # g·x̂ is 0 (x̂ = 0): dropping that term changes nothing and is not asked to
        r, c = np.unravel_index(int(np.argmax(np.abs(t1))), t1.shape)
        assert t1[r, c] != 0
        for kind in ("dropped", "flipped"):
            m1, m2 = t1[:, c:c + 1].copy(), t2[:, c:c + 1].copy()
            m1[r, 0], m2[r, 0] = (0.0, 0.0) if kind == "dropped" else (-m1[r, 0], -m2[r, 0])
            bad = R.nhwc_sums_f32_order(m1, m2, C)
            for i in ((0, 1) if t2[r, c] != 0 else (0,)):
                bound = R.sums_bound(mag[i][c], L, ks[i])
                assert abs(bad[i][0] - ref[i][c]) > bound, (name, kind, i, abs(bad[i][0] - ref[i][c]), bound)


def test_large_mean_inputs_stay_inside_the_same_bound():
    """mean 16, sigma 1: Σx² is 257x the variance; the order restatement is still inside the (unchanged) sums bound"""
    M, C = 1000, 256
    d = R.nhwc_inputs(M, C, "bf16", 1, 16.0, 1.0)
    x = d["x"].astype(np.float64)
    got, ref, mag = R.nhwc_sums_f32_order(x, x * x, C), R.sums_fwd(d["x"]), R.abs_sums_fwd(d["x"])
    for i in (0, 1):
        assert not _outside(got[i], ref[i], R.sums_bound(mag[i], R.chain_nhwc(M, C), 2)).any()
    assert abs(float(x.mean()) - 16.0) < 0.1 and np.array_equal(R.round16(d["x"], "bf16"), d["x"])


def test_chain_lengths():
    assert R.nhwc_nblk(1, 8) == 1 and R.nhwc_nblk(4099, 2048) == 257 and R.nhwc_nblk(3100, 1024) == 97
    assert R.nhwc_nblk(16384, 2048) == 512 and R.nhwc_nblk(2049, 8) == 1
    assert R.chain_nhwc(4099, 2048) == 16 + 8 + 1 and R.chain_nhwc(255, 8) == 1 + 8 + 256
    assert R.chain_nchw(2112, 8) == 16 and R.chain_nchw(2112, 4) == 12 and R.chain_nchw(63, 1) == 1 and R.chain_nchw(128, 8) == 8


# ------------------------------------------------------------------------------------------------ input condition
def test_near_zero_count_sees_what_fp32_could_flip():
    one = np.float32([1.0])
    mean, invstd, gamma, beta = np.float32([0.5]), np.float32([2.0]), np.float32([1.0]), np.float32([-1.0])
    # pre = 2 x - 1 - 1 = 2 x - 2: zero at x = 1
    x = np.float32([[1.0], [1.0 + 2.0 ** -20], [1.0 + 2.0 ** -17], [3.0]])
    m = R.near_zero_mask(x, None, gamma, beta, mean, invstd)
    assert m[:, 0].tolist() == [True, True, False, False]            # |pre| = 0, 2^-19, 2^-16 against 2^-20 * ~4
    assert R.near_zero_count(x, None, gamma, beta, mean, invstd) == 2
    res = np.float32([[0.0], [0.0], [0.0], [-4.0]])                                    # the residual moves the last one onto 0
    assert R.near_zero_mask(x, res, gamma, beta, mean, invstd)[:, 0].tolist() == [True, True, False, True]
    assert R.near_zero_count(one[None], None, None, None, np.float32([1.0]), one) == 1   # gamma / beta absent: x - mean = 0


def test_make_safe_replaces_until_nothing_is_left():
    g = synth.rng(16)
    x = R.round16(g.standard_normal((64, 8)) * 2.0, "bf16")
    gamma, beta = np.ones(8, np.float32), np.full(8, 0.25, np.float32)
    # plant elements whose pre-activation is (nearly) zero for the statistics of the planted x: x = mean - beta / invstd, as a
    # fixed point (an element moves its channel's mean by 1/64 of its own change)
    for _ in range(10):
        mean, invstd, _, _ = R.prep(R.sums_fwd(x), 64, 0.0, R.EPS)
        x[5, 3] = mean[3] - 0.25 / invstd[3]
        x[9, 0] = mean[0] - 0.25 / invstd[0]
    mean, invstd, _, _ = R.prep(R.sums_fwd(x), 64, 0.0, R.EPS)
    assert R.near_zero_count(x, None, gamma, beta, mean, invstd) >= 2
    xs, mu, istd, sums = R.make_safe(x, None, gamma, beta, (R.EPS, 64.0), "bf16")
    assert xs[5, 3] == R.SAFE_X and xs[9, 0] == R.SAFE_X and (xs != x).sum() == 2
    assert R.near_zero_count(xs, None, gamma, beta, mu, istd) == 0
    assert np.array_equal(sums[0], R.sums_fwd(xs)[0])


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
@pytest.mark.parametrize("entry", list(BC.ENTRIES))
def test_entries_refuse_bad_arguments_before_any_launch(lib, entry):
    M, C = 64, 64
    base = BC.placeholders(entry, M=M, C=C)
    need = R.nhwc_nblk(M, C) * C * 2 * 4
    assert lib.hiast_bn_nhwc_workspace_bytes(C) == R.MAXBLK * C * 2 * 4 >= need
    for what, change, code in BC.refused_calls(entry):
        got = BC.call(lib, entry, **BC.apply_change(base, change, need))
        assert got == code, (entry, what, got, code)
