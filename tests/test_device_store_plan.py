"""cfg.dataset.device_store_gb, host side (hiast_amd/sseg/datasets/device_store.py and what it touches; no GPU): a sample
over resident frames is the bytes sample's plan with the generators left in the same state, the fallbacks take today's
path, the budget rule (the first k frames, never more than the budget), the host check of records of kind 2, and the two
new entries of the C ABI.  Everything here is an equality or a refusal."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import device_store_world as W
from hiast_amd.sseg.datasets import device_aug as DA
from hiast_amd.sseg.datasets import device_store as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 128)] * 5 + [(37, 91)] * 3            # target frames 0..4 and 5..7


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return W.make_world(str(tmp_path_factory.mktemp("device_store_plan")), SHAPES)


def _place(ds, budget=1 << 30):
    store = DS.DeviceStore("cpu", budget)
    return store, store.place(ds, 2)


def _both(ds, table, index, seed):
    """the item of `index` read as bytes and with the residency table attached, from the same seeds
    -> (bytes item, store-path item, generator states equal)"""
    ds.__dict__.pop("store_table", None)
    W.seed_all(seed)
    plain = ds[index]
    states = (random.getstate(), np.random.get_state())
    ds.store_table = table
    W.seed_all(seed)
    item = ds[index]
    after = (random.getstate(), np.random.get_state())
    return plain, item, W.same(states, after)


# ------------------------------------------------------------------------------------------------- plan-only item
@pytest.mark.parametrize("aug_type,copy_paste,level", [(["MS", "CCA"], True, 1), (["MS", "CCA"], True, 2),
                                                       (["MS", "FDA-Target"], False, 3)],
                         ids=["level1", "level2", "level3-fda"])
def test_store_item_is_the_plan_of_the_bytes_item(world, aug_type, copy_paste, level):
    c = world.clone()
    if level == 3:
        c.dataset.source.type = "Oxford"             # (what 'FDA-Target' on a Cityscapes set is defined for)
    ds = W.target_dataset(c, aug_type, copy_paste, level)
    store, rs = _place(ds)
    assert rs.all_resident() and torch.equal(ds.store_table, rs.table) and rs.table.is_shared()
    n_store = n_paste = n_fda = 0
    for k in range(20):
        index, seed = k % len(SHAPES), 100 + k
        plain, item, states_equal = _both(ds, rs.table, index, seed)
        assert states_equal, "random / np.random differ after index %d (seed %d)" % (index, seed)
        assert item["image_paths"] == plain["image_paths"]
        if "store" not in item["raw"]:               # a fallback: today's sample, whole
            assert W.same(item, plain), (index, seed)
            continue
        n_store += 1
        assert plain["plan"] is not None and W.same(item["plan"], plain["plan"]), (index, seed)
        assert item["raw"]["store"][0] == index
        big = [(p, n) for p, n in W.arrays_of(item["raw"]) if n > 256 and p[0] != "fda"]
        assert not big, "a store sample carries %s" % big
        assert not {"img", "lbl", "paste_img", "paste_lbl"} & set(item["raw"])
        if "fda" in plain["raw"]:
            n_fda += 1
            assert W.same(item["raw"]["fda"], plain["raw"]["fda"])
        if copy_paste:
            assert item["copy_paste_mask"] is None and "copy_paste_mask" in plain
            if "paste_img" in plain["raw"]:
                n_paste += 1
                p_index = item["raw"]["store"][1]
                assert p_index >= 0 and torch.equal(item["raw"]["paste_table"], plain["raw"]["paste_table"])
                y1, y2, x1, x2 = DA.plan_window(item["plan"])      # the source the bytes path cut its window from
                assert np.array_equal(plain["raw"]["paste_lbl"].numpy(), rs.label(p_index).numpy()[y1:y2, x1:x2])
                assert np.array_equal(plain["raw"]["paste_img"].numpy(), rs.image(p_index).numpy()[y1:y2, x1:x2])
            else:
                assert item["raw"]["store"][1] == -1
        y1, y2, x1, x2 = DA.plan_window(item["plan"])
        assert np.array_equal(plain["raw"]["img"].numpy(), rs.image(index).numpy()[y1:y2, x1:x2])
        assert np.array_equal(plain["raw"]["lbl"].numpy(), rs.label(index).numpy()[y1:y2, x1:x2])
    assert n_store >= 5, "only %d of 20 samples took the store path" % n_store
    assert n_paste >= 1 if copy_paste else n_fda >= 5


# ------------------------------------------------------------------------------------------------- fallbacks
def _find(ds, table, want):
    """the first (index, seed) whose pair (bytes item, item with `table` attached) satisfies `want`"""
    for seed in range(200, 300):
        for index in range(len(SHAPES)):
            plain, item, eq = _both(ds, table, index, seed)
            assert eq
            if want(plain, item):
                return index, seed
    raise AssertionError("no seed gives the wanted sample")


def _source_index(ds, index, seed):
    """the CopyPaste source that the draws of (index, seed) choose"""
    W.seed_all(seed)
    DA.plan_sample(ds.aug_fun, ds.frame_shape(index), level=ds.device_aug_level)
    return ds.preprocessor.run_plan_index()[0]


def test_fallbacks_take_todays_path(world):
    ds = W.target_dataset(world, ["MS", "CCA"], True, 1)
    store, rs = _place(ds)
    # a frame that is not resident
    index, seed = _find(ds, rs.table, lambda plain, item: "store" in item["raw"])
    table = rs.table.clone()
    table[index, :2] = -1
    plain, item, eq = _both(ds, table, index, seed)
    assert eq and plain["plan"] is not None and "store" not in item["raw"] and W.same(item, plain)
    # a paste source that is not resident
    index, seed = _find(ds, rs.table, lambda plain, item: "store" in item["raw"] and item["raw"]["store"][1] >= 0)
    src = _both(ds, rs.table, index, seed)[1]["raw"]["store"][1]
    assert src == _source_index(ds, index, seed)
    table = rs.table.clone()
    table[src, :2] = -1
    plain, item, eq = _both(ds, table, index, seed)
    assert eq and "paste_img" in plain["raw"] and "store" not in item["raw"] and W.same(item, plain)
    # a paste source of another shape (it would need CopyPaste.resize): all frames resident, and still the bytes path
    index, seed = _find(ds, rs.table, lambda plain, item: plain["plan"] is not None and "store" not in item["raw"])
    plain, item, eq = _both(ds, rs.table, index, seed)
    assert ds.frame_shape(_source_index(ds, index, seed)) != ds.frame_shape(index)
    assert eq and "paste_img" in plain["raw"] and W.same(item, plain)
    # a plan that needs the host: finished views, as today
    index, seed = _find(ds, rs.table, lambda plain, item: plain["plan"] is None)
    plain, item, eq = _both(ds, rs.table, index, seed)
    assert eq and item["plan"] is None and "views" in item["raw"] and W.same(item, plain)


# ------------------------------------------------------------------------------------------------- budget
class _Frames:
    """a dataset double: n frames of given shapes, some of which fail to load"""

    def __init__(self, shapes, failing=()):
        self.shapes, self.failing, self.loaded = list(shapes), set(failing), []

    def __len__(self):
        return len(self.shapes)

    def frame_shape(self, i):
        return self.shapes[i]

    def load_data(self, i):
        self.loaded.append(i)
        if i in self.failing:
            raise OSError("frame %d cannot be read" % i)
        return W.frame(i, *self.shapes[i]) + ("frame_%d.png" % i,)


def test_budget_places_the_first_k_frames():
    shapes = [(37, 91), (64, 128), (37, 91), (64, 128), (37, 91), (64, 128)]
    need = [DS.frame_bytes(h, w) for h, w in shapes]
    assert need[0] == 10112 + 3376 and need[0] % 16 == 0           # 37 * 91 * 3 = 10101 and 3367, each padded to 16
    for k in range(len(shapes) + 1):
        for short, want in ((0, k), (1, max(k - 1, 0))):
            budget = sum(need[:k]) - short
            if budget < 0:
                continue
            ds = _Frames(shapes)
            store = DS.DeviceStore("cpu", budget)
            rs = store.place(ds, 3)
            resident = [i for i in range(len(shapes)) if rs.resident(i)]
            assert resident == list(range(want)), (k, short, resident)
            assert store.bytes_held() <= budget and store.bytes_held() == sum(need[:want])
            assert sorted(ds.loaded) == resident                   # nothing past the budget is decoded
            assert ds.store_table is rs.table and rs.table.is_shared() and rs.all_resident() == (want == len(shapes))
            for i in resident:
                img, lbl = W.frame(i, *shapes[i])
                assert np.array_equal(rs.image(i).numpy(), img) and np.array_equal(rs.label(i).numpy(), lbl)
                assert int(rs.frames[i, 0]) % 16 == 0 and int(rs.frames[i, 1]) % 16 == 0


def test_one_budget_per_process_in_the_order_of_the_calls():
    a, b = _Frames([(64, 128)] * 2), _Frames([(64, 128)] * 3)
    one = DS.frame_bytes(64, 128)
    store = DS.DeviceStore("cpu", 4 * one + 5)
    ra, rb = store.place(a, 1), store.place(b, 16)
    assert ra.all_resident() and [rb.resident(i) for i in range(3)] == [True, True, False]
    assert store.bytes_held() == 4 * one and store.place(a, 1) is ra and store.of(b) is rb


def test_a_frame_whose_load_raises_is_left_out():
    shapes = [(37, 91), (64, 128), (37, 91), (64, 128)]
    ds = _Frames(shapes, failing=(1,))
    store = DS.DeviceStore("cpu", 1 << 20)
    rs = store.place(ds, 2)
    assert [rs.resident(i) for i in range(4)] == [True, False, True, True] and not rs.all_resident()
    assert store.bytes_held() <= 1 << 20
    for i in (0, 2, 3):
        img, lbl = W.frame(i, *shapes[i])
        assert np.array_equal(rs.image(i).numpy(), img) and np.array_equal(rs.label(i).numpy(), lbl)


# ------------------------------------------------------------------------------------------------- table check
def _records(frames, window, index, paste_index=None, out=(16, 32)):
    """one hand-built batch of one KIND_STORE record over `frames` = [(index, img, lbl)]: `window` = (y1, y2, x1, x2) of
    frame `index` resampled to `out`; -> (ResidentSet, tables)"""
    from hiast_amd.sseg.datasets import augmentations as A
    rs = DS.ResidentSet.from_frames(frames, "cpu")
    y1, y2, x1, x2 = window
    plan = DA.plan_sample(A.resize(*out), (y2 - y1, x2 - x1))
    g = plan[0]["ops"][0][1]
    g.src = (y1, y2, x1, x2)
    paste = None
    if paste_index is not None:
        table = np.zeros(256, np.uint8)
        table[[3, 7]] = 1
        paste = (paste_index, rs.frames[paste_index].tolist(), table)
    t = DA.build_batch_tables([DA.pack_store_sample(plan, index, rs.frames[index].tolist(), paste)])
    return rs, t


def _check(t, rs, recs=None, store=True, out=(16, 32)):
    from hiast_amd import kernels as K
    K._aug_check_tables(t["blob"].numel(), t["tabs"].numpy(), t["recs"].numpy() if recs is None else recs, t["ops"].numpy(),
                        out[0], out[1], int(t["meta"][3]), (rs.buffer.numel(), rs.frames) if store else None)


def test_host_check_of_store_records():
    frames = [(0, *W.frame(1, 37, 91)), (1, *W.frame(2, 64, 128)), (2, *W.frame(3, 37, 91))]
    rs, t = _records(frames, (5, 30, 7, 80), 0, paste_index=2)
    r = t["recs"].numpy()
    assert int(r[0, DA.R_KIND]) == DA.KIND_STORE and int(r[0, DA.R_STRIDE]) == 91 and int(r[0, DA.R_CW]) == 73
    assert int(r[0, DA.R_IMG]) == int(rs.frames[0, 0]) + (5 * 91 + 7) * 3 and int(r[0, DA.R_LBL]) == int(rs.frames[0, 1]) + 5 * 91 + 7
    assert int(r[0, DA.R_PIMG]) == int(rs.frames[2, 0]) + (5 * 91 + 7) * 3
    _check(t, rs)

    def bad(**words):
        b = r.copy()
        for k, v in words.items():
            b[0, getattr(DA, k)] = v
        return b
    cases = {
        "stride below cw": bad(R_STRIDE=72),
        "one pixel past the frame's last row": bad(R_IMG=r[0, DA.R_IMG] + 8 * 91 * 3, R_LBL=r[0, DA.R_LBL] + 8 * 91),
        "one pixel past the frame's last column": bad(R_IMG=r[0, DA.R_IMG] + 12 * 3, R_LBL=r[0, DA.R_LBL] + 12),
        "the label alone past its frame": bad(R_LBL=r[0, DA.R_LBL] + 8 * 91),
        "a paste window past the store's end": bad(R_PLBL=r[0, DA.R_PLBL] + 8 * 91),
        "a negative offset": bad(R_IMG=-3),
        "a negative paste offset": bad(R_PIMG=-1),
        "a stride that is not the frame's width": bad(R_STRIDE=92),
    }
    assert r[0, DA.R_CH] == 25 and 5 + 25 + 7 == 37 and 7 + 73 + 11 == 91      # (7 rows and 11 columns of room, no more)
    assert int(r[0, DA.R_PLBL]) + 8 * 91 + 24 * 91 + 73 > rs.buffer.numel()     # (the paste source is the store's last frame)
    _check(t, rs, bad(R_IMG=r[0, DA.R_IMG] + (7 * 91 + 11) * 3, R_LBL=r[0, DA.R_LBL] + 7 * 91 + 11))     # flush in the corner
    for what, recs in cases.items():
        print(what)
        with pytest.raises(ValueError):
            _check(t, rs, recs)
    with pytest.raises(ValueError, match="no store"):
        _check(t, rs, store=False)
    # the window that ends exactly on the last pixel of the last frame is accepted; so is one on another frame's last pixel
    rs, t = _records(frames, (12, 37, 18, 91), 2, paste_index=0)
    _check(t, rs)
    last = int(t["recs"][0, DA.R_LBL]) + 24 * 91 + 73
    assert last == int(rs.frames[2, 1]) + 37 * 91 and last <= rs.buffer.numel() < last + 16
    rs, t = _records(frames, (40, 64, 100, 128), 1)
    _check(t, rs)
    from hiast_amd import kernels as K
    with pytest.raises(ValueError):                                             # and the wrapper asks for a store at all
        K.aug_batch_store_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 16, 32, int(t["meta"][3]), "cuda", None)
    with pytest.raises(ValueError, match="no store"):                           # kind 2 through the entry without a store
        K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 16, 32, int(t["meta"][3]), "cuda")


def test_switch_and_config_default_to_off(monkeypatch):
    from hiast_amd import switches
    from hiast_amd.utils.default_config import get_default_cfg
    c = get_default_cfg()
    assert c.dataset.device_store_gb == 0.0 and switches.device_store_bytes(c) == 0
    c.dataset.device_store_gb = 1.5
    assert switches.device_store_bytes(c) == 3 << 29
    monkeypatch.setitem(switches.SIZES, "HIAST_DEVICE_STORE_GB", 0.25)
    assert switches.device_store_bytes(c) == 1 << 28


# ------------------------------------------------------------------------------------------------- ABI
E_ARG, E_RANGE = -1, -2
FAKE = 0x10000                                    # a non-null address that no refused call may touch
NEW = {"hiast_aug_geometry_store_u8": 12, "hiast_normalize_gather_u8": 8}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def test_new_entries_in_header_exports_and_ctypes(lib):
    from hiast_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiast_hip.h")).read(), flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, txt, flags=re.S)
        assert m and m.group(1).count(",") + 1 == arity, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == arity
    assert lib.hiast_version() == 6


def _geometry(lib, **over):
    a = dict(recs=FAKE, blob=FAKE, store=FAKE, tabs=FAKE, tmp=FAKE, img_out=FAKE, lbl_out=FAKE, B=2, max_ch=64, oh=16, ow=32)
    a.update(over)
    return lib.hiast_aug_geometry_store_u8(a["recs"], a["blob"], a["store"], a["tabs"], a["tmp"], a["img_out"], a["lbl_out"],
                                           a["B"], a["max_ch"], a["oh"], a["ow"], None)


def _gather(lib, **over):
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    a = dict(store=FAKE, offsets=FAKE, out=FAKE, B=2, HW=64 * 128, mean=f3, std=f3)
    a.update(over)
    return lib.hiast_normalize_gather_u8(a["store"], a["offsets"], a["out"], a["B"], a["HW"], a["mean"], a["std"], None)


GEOMETRY_REFUSED = ([("%s null" % p, {p: None}, E_ARG) for p in ("recs", "blob", "store", "tabs", "tmp", "img_out", "lbl_out")]
                    + [("B = 0", dict(B=0), E_ARG), ("max_ch = 0", dict(max_ch=0), E_ARG), ("oh = -1", dict(oh=-1), E_ARG),
                       ("ow = 0", dict(ow=0), E_ARG), ("B = 65536", dict(B=65536), E_RANGE),
                       ("max_ch = 65536", dict(max_ch=65536), E_RANGE), ("oh = 65536", dict(oh=65536), E_RANGE),
                       ("ow = 2^20 + 1", dict(ow=(1 << 20) + 1), E_RANGE)])
GATHER_REFUSED = ([("%s null" % p, {p: None}, E_ARG) for p in ("store", "offsets", "out", "mean", "std")]
                  + [("B = 0", dict(B=0), E_ARG), ("HW = 0", dict(HW=0), E_ARG), ("B = 65536", dict(B=65536), E_RANGE)])


@pytest.mark.parametrize("what,change,code", GEOMETRY_REFUSED, ids=[r[0] for r in GEOMETRY_REFUSED])
def test_geometry_store_refusals_before_any_launch(lib, what, change, code):
    assert _geometry(lib, **change) == code, what
    if "store" not in change:                        # the existing entry refuses the same extents with the same codes
        a = dict(recs=FAKE, blob=FAKE, tabs=FAKE, tmp=FAKE, img_out=FAKE, lbl_out=FAKE, B=2, max_ch=64, oh=16, ow=32)
        a.update(change)
        assert lib.hiast_aug_geometry_u8(a["recs"], a["blob"], a["tabs"], a["tmp"], a["img_out"], a["lbl_out"], a["B"],
                                         a["max_ch"], a["oh"], a["ow"], None) == code


@pytest.mark.parametrize("what,change,code", GATHER_REFUSED, ids=[r[0] for r in GATHER_REFUSED])
def test_normalize_gather_refusals_before_any_launch(lib, what, change, code):
    assert _gather(lib, **change) == code, what
    if not {"store", "offsets"} & set(change):       # hiast_normalize_u8 refuses the same extents with the same codes
        f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        a = dict(store=FAKE, out=FAKE, B=2, HW=64 * 128, mean=f3, std=f3)
        a.update(change)
        assert lib.hiast_normalize_u8(a["store"], a["out"], a["B"], a["HW"], a["mean"], a["std"], None) == code


def test_wrappers_have_no_cpu_path():
    from hiast_amd import kernels as K
    with pytest.raises(Exception, match="CUDA"):
        K.normalize_gather_u8(torch.zeros(64, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), 2, 2, (0.5,) * 3, (0.5,) * 3)
