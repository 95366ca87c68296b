"""hiast_plabel_pass1_tta (plabel_tta.hip) on the MI355X, through the C ABI on buffers carved out of 0xFF-filled allocations
(tests/guard_bands.py) and through the K.plabel_pass1_tta wrapper, against the oracle chain of tests/plabel_tta_inputs.py:
    probs, label = cref.tta(zs, zfs, sizes, H, W);  argmax_o = label
    maxprob_o = min(probs.max(1) / float32(n_views), float32(1));  hist_o = cref.plabel_hist(maxprob_o, argmax_o, C)
argmax, maxprob (as bits) and hist are BIT-EQUAL to that chain: no tolerance, no excluded pixel.  Inputs sit in NaN poison; after
each launch both guard bands of every buffer are untouched and every output is fully written; a second launch rewrites everything
with the same bits; hist starts from counts the test chooses and grows by hist_o per launch; with and without the workspace; in
the tiled form (the LDS patch) and in the direct form (HIAST_PLTTA_FORM=direct, and by itself where a view is 3x the frame)."""
import ctypes

import numpy as np
import pytest
import torch

import guard_bands as GB
import plabel_tta_inputs as P
from test_gpu_bn_extents import Bufs, _biteq, _st

pytestmark = pytest.mark.gpu

BAND = 64 << 10                  # more than a block touches of any buffer in a pass: 256 pixels x 19 classes x 4 bytes
F32, U8, I32 = torch.float32, torch.uint8, torch.int32
S3 = ((17, 33), (49, 97), (33, 65))                       # below, above and at the native size
# (B, H, W, sizes, flip, C)
CASES = [(2, 33, 65, S3, True, 19), (2, 33, 65, S3, False, 19), (2, 33, 65, S3, True, 2), (2, 33, 65, S3, False, 2),
         (2, 33, 65, ((49, 97),), True, 16), (2, 33, 65, ((49, 97),), True, 9),
         (1, 40, 301, ((56, 421),), True, 19),            # W no multiple of 256 / of the tile; Ws odd, the mirror column crosses tile edges
         (1, 33, 65, ((97, 193),), True, 19)]             # a view 3x the frame: its footprint exceeds the LDS patch (direct form)
_id = lambda c: "%dx%dx%d-%s-%s-C%d" % (c[0], c[1], c[2], "+".join("%dx%d" % s for s in c[3]), "flip" if c[4] else "plain", c[5])


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    from hiast_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # (a copy: the shared case arrays are read-only)


def call(lib, Z, ZF, sizes, B, C, H, W, maxprob, argmax, hist, ws, nbytes):
    n = len(Z)
    vp = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    iv = lambda vs: (ctypes.c_int * n)(*[int(v) for v in vs])
    return lib.hiast_plabel_pass1_tta(vp(Z), vp(ZF) if ZF is not None else None, iv([z.shape[2] for z in Z]),
                                      iv([z.shape[3] for z in Z]), iv([s[0] for s in sizes]), iv([s[1] for s in sizes]), n, B, C,
                                      H, W, maxprob.data_ptr(), argmax.data_ptr(), hist.data_ptr(),
                                      ws.data_ptr() if ws is not None else None, nbytes, _st())


def run_case(K, lib, seed, case, scattered, tie=False):
    B, H, W, sizes, flip, C = case
    zs, zfs, mp_o, am_o, hist_o, probs_o = P.case(seed, B, C, H, W, sizes, flip, tie)
    assert int(hist_o.sum()) == B * H * W and float(mp_o.max()) <= 1.0
    hist_o = torch.from_numpy(np.array(hist_o).view(np.int32)).cuda()
    h0 = torch.from_numpy(P.synth.rng(seed + 1).integers(0, 1000, size=(C, P.NBINS))).to(I32).cuda()
    inb = Bufs()
    Z = [inb.inp("z%d" % i, dev(z), BAND) for i, z in enumerate(zs)]
    ZF = [inb.inp("zf%d" % i, dev(z), BAND) for i, z in enumerate(zfs)] if flip else None
    nws = lib.hiast_plabel_pass1_tta_workspace_bytes(C)
    assert nws == 256 * C * 61 * 4
    b = Bufs()
    o = dict(maxprob=b.out("maxprob", (B, H, W), F32, BAND), argmax=b.out("argmax", (B, H, W), U8, BAND))
    hist = b.out("hist", (C, P.NBINS), I32, BAND, init=h0)
    wsb = b.out("workspace", (nws // 4,), I32, BAND, must_fill=False) if scattered else None
    for launch in (1, 2):
        rc = call(lib, Z, ZF, sizes, B, C, H, W, o["maxprob"], o["argmax"], hist, wsb, nws if scattered else 0)
        assert rc == 0, rc
        b.check(inb)
        assert _biteq(o["argmax"], dev(am_o)), "argmax differs from the oracle on %d pixels (launch %d)" % (
            int((o["argmax"] != dev(am_o)).sum()), launch)
        assert _biteq(o["maxprob"], dev(mp_o)), "maxprob differs from the oracle in its bits on %d pixels (launch %d)" % (
            int((o["maxprob"].view(I32) != dev(mp_o).view(I32)).sum()), launch)
        assert _biteq(hist, h0 + launch * hist_o), "hist after launch %d" % launch
        if launch == 1:
            o["maxprob"].view(U8).fill_(GB.FILL)               # the second launch has to write everything again
            o["argmax"].fill_(GB.FILL)
    mp, am, hw_ = K.plabel_pass1_tta([dev(z) for z in zs], [dev(z) for z in zfs] if flip else None, sizes, H, W, hist=h0.clone())
    assert _biteq(o["maxprob"], mp) and _biteq(o["argmax"], am) and _biteq(hw_, h0 + hist_o), "the wrapper returns other bits"
    return mp_o, am_o, probs_o


@pytest.mark.parametrize("form", ["auto", "direct"])
@pytest.mark.parametrize("scattered", [True, False], ids=["workspace", "no-workspace"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pass1_tta_equals_the_oracle_chain(K, lib, case, scattered, form, monkeypatch):
    if form == "direct":
        monkeypatch.setenv("HIAST_PLTTA_FORM", "direct")
    else:
        monkeypatch.delenv("HIAST_PLTTA_FORM", raising=False)
    B, H, W, sizes, flip, C = case
    mp_o, _, _ = run_case(K, lib, 4000 + C, case, scattered)
    lo, mid, top = P.shares(mp_o)
    print("shares of the oracle's maxprob  %s  below 0.5: %.3f  0.5 .. top 128 bins: %.3f  top 128 bins: %.3f  max %.9g"
          % (_id(case), lo, mid, top, float(mp_o.max())))
    if sizes == S3 and flip:                               # every counting path is exercised
        assert mid >= 0.05 and top >= 0.05 and (lo >= 0.05 or C == 2), (lo, mid, top)


@pytest.mark.parametrize("form", ["auto", "direct"])
def test_exact_ties_name_the_first_class(K, lib, form, monkeypatch):
    """class plane 1 is a copy of plane 0 in every view: wherever those two lead, their sums are equal to the bit"""
    monkeypatch.setenv("HIAST_PLTTA_FORM", form)
    case = (2, 33, 65, S3, True, 19)
    _, am_o, probs_o = run_case(K, lib, 4100, case, True, tie=True)
    assert np.array_equal(probs_o[:, 0].view(np.uint32), probs_o[:, 1].view(np.uint32))
    tied = probs_o.max(1) == probs_o[:, 0]
    assert int(tied.sum()) >= 50, int(tied.sum())
    assert (am_o[tied] == 0).all() and not (am_o == 1).any()          # (the kernel's argmax was compared with am_o above)


@pytest.mark.parametrize("C", [19, 2])
def test_one_native_view_is_pass_1(K, lib, C):
    """one view at the native size without flip: the mean over one view of softmax(up(z)) — maxprob is pass 1's to the bit, argmax
    wherever the two largest probabilities differ (where they are equal, pass 1 names the larger LOGIT)"""
    B, H, W = 2, 33, 65
    case = (B, H, W, ((H, W),), False, C)
    zs, _, mp_o, am_o, hist_o, probs_o = P.case(4200 + C, B, C, H, W, ((H, W),), False)
    mp, am, hist = K.plabel_pass1_tta([dev(zs[0])], None, [(H, W)], H, W)
    mp1, am1, hist1 = K.plabel_pass1(dev(zs[0]), H, W)
    assert _biteq(mp, dev(mp_o)) and _biteq(am, dev(am_o)) and _biteq(hist, torch.from_numpy(np.array(hist_o).view(np.int32)).cuda())
    assert _biteq(mp, mp1), "maxprob of one native view differs from pass 1 on %d pixels" % int((mp.view(I32) != mp1.view(I32)).sum())
    top2 = np.sort(probs_o, axis=1)[:, -2:]
    clear = torch.from_numpy(top2[:, 1] > top2[:, 0]).cuda()
    assert torch.equal(am[clear], am1[clear]) and float(clear.float().mean()) > 0.9
    if bool(clear.all()):
        assert _biteq(hist, hist1)
    run_case(K, lib, 4200 + C, case, True)


def test_empty_batch_launches_nothing(K):
    z = torch.zeros((0, 19, 5, 9), dtype=F32, device="cuda")
    h0 = torch.full((19, P.NBINS), 7, dtype=I32, device="cuda")
    mp, am, hist = K.plabel_pass1_tta([z], [z], [(33, 65)], 33, 65, hist=h0)
    assert tuple(mp.shape) == (0, 33, 65) and tuple(am.shape) == (0, 33, 65) and hist is h0 and bool((hist == 7).all())
