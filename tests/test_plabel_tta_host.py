"""Host side of the multi-view pseudo-label pass 1 (hiast_plabel_pass1_tta; no GPU): the workspace size, every refusal of the
entry (made before any launch, so placeholder addresses are never dereferenced) with the refusals of the view arguments repeated on
hiast_tta_fused, which checks them with the same function, the config key and the view-list logic of HipPlabelEngine."""
import ctypes

import pytest
import torch

E_ARG, E_RANGE, E_WS = -1, -2, -3
FAKE = 0x10000                                    # a non-null address that no refused call may touch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def call(lib, fused=False, **over):
    """hiast_plabel_pass1_tta (fused: hiast_tta_fused, which takes the same view arguments) on placeholder addresses; `over`
    replaces arguments (z / zf: lists of addresses or None; hs, ws, Hs, Ws: lists)"""
    a = dict(z=[FAKE, FAKE], zf=[FAKE, FAKE], hs=[5, 7], ws=[9, 13], Hs=[33, 49], Ws=[65, 97], n_scales=2, B=2, C=19, H=33, W=65,
             maxprob=FAKE, argmax=FAKE, hist=FAKE, workspace=None, workspace_bytes=0, probsum=FAKE, label=FAKE, stream=None)
    a.update(over)
    vp = lambda v: None if v is None else (ctypes.c_void_p * len(v))(*v)
    iv = lambda v: None if v is None else (ctypes.c_int * len(v))(*v)
    views = (vp(a["z"]), vp(a["zf"]), iv(a["hs"]), iv(a["ws"]), iv(a["Hs"]), iv(a["Ws"]), a["n_scales"], a["B"], a["C"], a["H"], a["W"])
    if fused:
        return lib.hiast_tta_fused(*views, a["probsum"], a["label"], a["stream"])
    return lib.hiast_plabel_pass1_tta(*views, a["maxprob"], a["argmax"], a["hist"], a["workspace"], a["workspace_bytes"], a["stream"])


def test_workspace_bytes(lib):
    for C in (19, 16, 9, 2):
        assert lib.hiast_plabel_pass1_tta_workspace_bytes(C) == 256 * C * 61 * 4 == lib.hiast_plabel_pass1_workspace_bytes(C)
    for C in (0, -1, 1, 3, 17, 18, 20, 32, 33):
        assert lib.hiast_plabel_pass1_tta_workspace_bytes(C) == 0


VIEWS_REFUSED = [                                 # the view arguments: one check for both entries
    ("z null", dict(z=None), E_ARG), ("hs null", dict(hs=None), E_ARG), ("ws null", dict(ws=None), E_ARG),
    ("Hs null", dict(Hs=None), E_ARG), ("Ws null", dict(Ws=None), E_ARG),
    ("no scales", dict(n_scales=0), E_ARG), ("B = 0", dict(B=0), E_ARG), ("C = 0", dict(C=0), E_ARG), ("H = 0", dict(H=0), E_ARG),
    ("W = -1", dict(W=-1), E_ARG), ("a null view", dict(z=[FAKE, None]), E_ARG),
    ("zf with a null entry", dict(zf=[FAKE, None]), E_ARG), ("zf with its first entry null", dict(zf=[None, FAKE]), E_ARG),
    ("hs = 0", dict(hs=[0, 7]), E_ARG), ("ws = 0", dict(ws=[9, 0]), E_ARG),
    ("Hs < hs", dict(Hs=[4, 49]), E_ARG), ("Ws < ws", dict(Ws=[65, 12]), E_ARG),
    ("9 scales", dict(n_scales=9, z=[FAKE] * 9, zf=None, hs=[5] * 9, ws=[9] * 9, Hs=[33] * 9, Ws=[65] * 9), E_RANGE),
    ("B = 65536", dict(B=65536), E_RANGE), ("H = 65536", dict(H=65536), E_RANGE),
]
REFUSED = VIEWS_REFUSED + [
    ("maxprob null", dict(maxprob=None), E_ARG), ("argmax null", dict(argmax=None), E_ARG), ("hist null", dict(hist=None), E_ARG),
    ("C = 5", dict(C=5), E_RANGE), ("C = 20", dict(C=20), E_RANGE), ("C = 18", dict(C=18), E_RANGE),
    ("workspace one byte short", dict(workspace=FAKE, workspace_bytes=256 * 19 * 61 * 4 - 1), E_WS),
    ("workspace of another class count", dict(workspace=FAKE, workspace_bytes=256 * 16 * 61 * 4), E_WS),
    ("workspace not 4-byte aligned", dict(workspace=FAKE + 2, workspace_bytes=256 * 19 * 61 * 4), E_WS),
]
FUSED_REFUSED = VIEWS_REFUSED + [("both outputs null", dict(probsum=None, label=None), E_ARG), ("C = 5", dict(C=5), E_RANGE)]


@pytest.mark.parametrize("what,change,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_before_any_launch(lib, what, change, code):
    assert call(lib, **change) == code, what
    if "zf" not in change:
        assert call(lib, zf=None, **change) == code, what + " (no mirror views)"


@pytest.mark.parametrize("what,change,code", FUSED_REFUSED, ids=[r[0] for r in FUSED_REFUSED])
def test_tta_fused_refuses_the_same_views(lib, what, change, code):
    """hiast_tta_fused on the same placeholder addresses: the same codes, with either output alone as well"""
    assert call(lib, fused=True, **change) == code, what
    if "zf" not in change:
        assert call(lib, fused=True, zf=None, **change) == code, what + " (no mirror views)"
    if "label" not in change:
        assert call(lib, fused=True, label=None, **change) == code, what + " (probsum only)"
        assert call(lib, fused=True, probsum=None, **change) == code, what + " (label only)"


def test_wrapper_names_what_is_supported():
    from hiast_amd import kernels as K
    assert all(K.plabel_pass1_tta_supported(C, n) for C in (19, 16, 9, 2) for n in (1, 8))
    assert not any(K.plabel_pass1_tta_supported(C, 1) for C in (1, 3, 17, 20))
    assert not K.plabel_pass1_tta_supported(19, 0) and not K.plabel_pass1_tta_supported(19, 9)
    with pytest.raises(Exception, match="CUDA"):                               # no CPU path
        K.plabel_pass1_tta([torch.zeros(1, 19, 5, 9)], None, [(33, 65)], 33, 65)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
S3 = ((17, 33), (49, 97), (33, 65))


@pytest.mark.parametrize("C", [19, 16, 9, 2])
def test_inputs_reach_every_counting_path(C):
    import plabel_tta_inputs as P
    """the recipe at 33 x 65, three sizes + flip, on the oracle's output: at least 5 % of the pixels below fp16 0.5 (never at two
    classes), from 0.5 to the top 128 bins, and in the top 128 bins"""
    lo, mid, top = P.shares(P.case(4000 + C, 2, C, 33, 65, S3, True)[2])
    assert mid >= 0.05 and top >= 0.05 and (lo >= 0.05 if C > 2 else lo == 0.0), (lo, mid, top)


# ------------------------------------------------------------------------------------------------ config and view list
def test_config_defaults_are_off():
    from hiast_amd.utils.default_config import get_default_cfg
    from hiast_amd.workflows.pseudo_label_generator import tta_views
    c = get_default_cfg()
    assert c.pseudo_policy.tta.resize_sizes == [] and c.pseudo_policy.tta.is_flip is False
    assert tta_views(c.pseudo_policy) == ([], False)
    c.pseudo_policy.tta.resize_sizes = [[17, 33], [49, 97]]
    c.pseudo_policy.tta.is_flip = True
    assert tta_views(c.pseudo_policy) == ([[17, 33], [49, 97]], True)


class _Double:
    """an engine double with the two-call interface; records what the generator tells it about views"""

    def __init__(self):
        self.told = []

    def set_views(self, sizes, flip):
        self.told.append((sizes, flip))


def test_generator_construction_stays_on_the_old_path_by_default(tmp_path):
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import PSEUDO_POLICY
    from hiast_amd.tools import synth_data
    c = synth_data.synthetic_cfg(str(tmp_path), n_train=3, n_val=1, h=32, w=64)
    c.dataset.num_workers = 0
    eng = _Double()
    gen = PSEUDO_POLICY["CT"](c, engine=eng)
    assert gen.engine is eng and eng.told == []                                # defaults: the engine is never told of views
    c.pseudo_policy.save_dir = str(tmp_path / "second" / "pseudo_labels")
    c.pseudo_policy.tta.is_flip = True
    PSEUDO_POLICY["CT"](c, engine=eng)
    assert eng.told == [([], True)]
    c.pseudo_policy.save_dir = str(tmp_path / "third" / "pseudo_labels")
    c.pseudo_policy.tta.resize_sizes = [[24, 48], [40, 80]]
    PSEUDO_POLICY["CT"](c, engine=eng)
    assert eng.told[-1] == ([[24, 48], [40, 80]], True)


def test_view_list_logic():
    from hiast_amd._lib import HiastLibraryError
    from hiast_amd.workflows.pseudo_label_generator import HipPlabelEngine
    dev = torch.device("cuda", 0)                                              # (a device object only: nothing is launched)
    off = HipPlabelEngine(None, dev, 19)
    assert not off.views and off.view_sizes(512, 1024) == [(512, 1024)]
    assert off.group(2, (512, 1024)) == 2 and off.group(2, (33, 65)) == 1      # today's grouping
    flip_only = HipPlabelEngine(None, dev, 19, sizes=[], flip=True)
    assert flip_only.views and flip_only.flip and flip_only.view_sizes(512, 1024) == [(512, 1024)]
    assert flip_only.group(2, (512, 1024)) == 1
    multi = HipPlabelEngine(None, dev, 19, sizes=[[384, 768], [640, 1280]], flip=False)
    assert multi.views and not multi.flip and multi.view_sizes(512, 1024) == [(384, 768), (640, 1280)]
    assert multi.group(2, (512, 1024)) == 1 and multi.group(1, (1024, 2048)) == 1
    HipPlabelEngine(None, dev, 2, sizes=[[8 * i, 16 * i] for i in range(1, 9)], flip=True)          # 8 sizes are the most
    with pytest.raises(HiastLibraryError, match="at most 8"):
        HipPlabelEngine(None, dev, 19, sizes=[[8 * i, 16 * i] for i in range(1, 10)], flip=True)
    with pytest.raises(HiastLibraryError, match="classes"):
        HipPlabelEngine(None, dev, 7, sizes=[], flip=True)
    HipPlabelEngine(None, dev, 7)                                              # without views any class count goes on as before
    multi.set_views(None, False)
    assert not multi.views and multi.group(2, (512, 1024)) == 2
    with pytest.raises(RuntimeError, match="HIP device only"):
        HipPlabelEngine(None, torch.device("cpu"), 19, sizes=[], flip=True)
