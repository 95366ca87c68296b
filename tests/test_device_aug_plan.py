"""cfg.dataset.device_aug, host side (hiast_amd/sseg/datasets/device_aug.py): the resample tables against Pillow, the plan
against augmentations.aug() (bytes and the state of `random`), the share of samples that fall back to the host, and the
CopyPaste select against CopyPaste.run_original.  Everything here is equality: the device path is byte-identical to the
worker path or it is wrong."""
import random

import numpy as np
import pytest
import torch

import synth
from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA

# (in_h, in_w, out_h, out_w): full frame, upscale, odd sizes, twelve 'MS' crop heights, one axis unchanged, 'OMS', tiny
_MS_HEIGHTS = [358, 377, 402, 455, 512, 519, 600, 683, 701, 850, 941, 999]
SHAPES = ([(1024, 2048, 512, 1024), (341, 682, 512, 1024), (1000, 2000, 512, 1024), (777, 1554, 512, 1024)]
          + [(h, 2 * h, 512, 1024) for h in _MS_HEIGHTS]
          + [(600, 1024, 512, 1024), (512, 900, 512, 1024), (1024, 2048, 768, 1024), (37, 91, 64, 128),
             (720, 1280, 512, 1024), (640, 1365, 768, 1024), (341, 683, 512, 1024)])


def _frame(seed, h, w):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 20, (h, w), dtype=np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_tables_reproduce_pillow(shape):
    h, w, oh, ow = shape
    assert len(SHAPES) == 23
    img, lbl = _frame(h * 7 + w, h, w)
    plan = DA.plan_sample(A.resize(oh, ow), (h, w))
    assert not DA.needs_host(plan) and len(plan) == 1
    imgs, lbls = DA.execute_plan_host(plan, img, lbl)
    want_i, want_l = A._resize_img(img, oh, ow), A._resize_mask(lbl, oh, ow)
    assert int((imgs[0] != want_i).sum()) == 0 and int((lbls[0] != want_l).sum()) == 0


def _dataset(tmp_path, aug_type, n_frames=8, n=200, h=400, w=800):
    """a Cityscapes dataset object of n indices over n_frames synthetic frames"""
    from hiast_amd.tools import synth_data
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    c = synth_data.synthetic_cfg(str(tmp_path), n_train=n_frames, n_val=1, h=h, w=w, upscale=4)

    class Wrapped(CityscapesDataset):
        def load_data(self, index):
            return super().load_data(index % n_frames)

    ds = Wrapped(c, c.dataset.target.json_path, c.dataset.target.image_dir, aug_type=aug_type)
    ds.img_path_list = ds.img_path_list * (n // n_frames)
    ds.lbl_path_list = ds.lbl_path_list * (n // n_frames)
    return ds


AUGS = [["MS", "CCA"], ["MS"], ["OMS"], ["DACS"], ["PRS-256-512"], ["PRS-64-128", "CCA"]]


@pytest.mark.parametrize("aug_type", AUGS, ids=lambda a: "+".join(a))
def test_plan_reproduces_aug(tmp_path, aug_type):
    """indices 0..199: every unflagged sample's plan, executed in numpy, equals aug() in every view and label and leaves
    `random` in the same state; a flagged sample leaves the dataset as the finished views the plain dataset returns"""
    ds = _dataset(tmp_path, aug_type)
    multi = isinstance(ds.aug_fun, list)
    flagged = 0
    for i in range(200):
        img, lbl, _ = ds.load_data(i)
        want_i, want_l = A.aug(ds.aug_fun, img.copy(), lbl.copy(), i)
        state = random.getstate()
        ds.device_transform = True
        ds.device_aug = False
        plain = ds[i]
        ds.device_aug = True
        item = ds[i]
        assert item["image_paths"] == plain["image_paths"]
        plan = DA.plan_sample(ds.aug_fun, img.shape[:2], i)
        if DA.needs_host(plan):
            flagged += 1
            assert item["plan"] is None
            pi, pl = (plain["images"], plain["labels"]) if multi else ([plain["images"]], [plain["labels"]])
            assert len(item["raw"]["views"]) == len(pi)
            assert all(torch.equal(a, b) for a, b in zip(item["raw"]["views"], pi))
            assert torch.equal(item["raw"]["lbl"], pl[0])
            continue
        assert random.getstate() == state
        got_i, got_l = DA.execute_plan_host(plan, img, lbl)
        wi, wl = (want_i, want_l) if multi else ([want_i], [want_l])
        assert len(got_i) == len(wi)
        for a, b in zip(got_i, wi):
            assert a.shape == b.shape and int((a != b).sum()) == 0, (i, aug_type)
        for a, b in zip(got_l, wl):
            assert int((a != b).sum()) == 0, (i, aug_type)
        # what the worker hands over is the window the plan reads, and executes to the same bytes
        y1, y2, x1, x2 = DA.plan_window(item["plan"])
        assert np.array_equal(item["raw"]["img"].numpy(), img[y1:y2, x1:x2])
        if i % 8 == 0:
            s_i, s_l = DA.execute_plan_host(item["plan"], item["raw"]["img"].numpy(), item["raw"]["lbl"].numpy(), sliced=True)
            assert all(np.array_equal(a, b) for a, b in zip(s_i + s_l, wi + wl))
    if "CCA" not in aug_type:
        assert flagged == 0


def test_collated_tables_round_trip(tmp_path):
    """collate(): one blob, one table blob, one record row per sample, planned and finished samples in one batch"""
    ds = _dataset(tmp_path, ["MS", "CCA"], n=16)
    ds.device_transform = ds.device_aug = True
    items = [ds[i] for i in range(16)]
    assert any(it["plan"] is None for it in items) and any(it["plan"] is not None for it in items)
    batch = DA.collate(items)
    t = batch["device_aug"]
    assert DA.is_device_aug_batch(batch) and len(batch["image_paths"]) == 16
    assert t["recs"].shape == (16, DA.REC_WORDS) and t["ops"].shape == (2, 16, DA.OPS_WORDS)
    assert [int(v) for v in t["meta"]][:3] == [2, 512, 1024] and int(t["meta"][4]) == 1
    blob = t["blob"].numpy()
    for b, it in enumerate(items):
        r = t["recs"][b]
        if it["plan"] is None:
            assert int(r[DA.R_KIND]) == DA.KIND_FINISHED
            off = int(t["ops"][1, b, 1])
            assert np.array_equal(blob[off:off + 512 * 1024 * 3], it["raw"]["views"][1].numpy().ravel())
        else:
            n = it["raw"]["img"].numel()
            assert np.array_equal(blob[int(r[DA.R_IMG]):int(r[DA.R_IMG]) + n], it["raw"]["img"].numpy().ravel())
    from hiast_amd import kernels as K
    K._aug_check_tables(blob.size, t["tabs"].numpy(), t["recs"].numpy(), t["ops"].numpy(), 512, 1024, int(t["meta"][3]))
    bad = t["recs"].numpy().copy()
    b0 = next(b for b, it in enumerate(items) if it["plan"] is not None)
    bad[b0, DA.R_IMG] = blob.size - 16          # a window that ends outside the bytes handed over
    with pytest.raises(ValueError):
        K._aug_check_tables(blob.size, t["tabs"].numpy(), bad, t["ops"].numpy(), 512, 1024, int(t["meta"][3]))
    bad = t["recs"].numpy().copy()
    bad[b0, DA.R_CW] -= 1                       # a table that reads one column past the window
    with pytest.raises(ValueError):
        K._aug_check_tables(blob.size, t["tabs"].numpy(), bad, t["ops"].numpy(), 512, 1024, int(t["meta"][3]))


def _flagged_share(aug_fun, shape, n=2000):
    k = 0
    for s in range(n):
        k += DA.needs_host(DA.plan_sample(aug_fun, shape, s))
    return k / n


def test_fallback_share_is_what_the_pool_implies():
    """ColorJitter or GaussianBlur among the 3 of 8 picked and applied: 0.348 expected (standard deviation 0.011 at
    n = 2000); the flag is not a hiding place for anything else"""
    ms = A.flip_crop_resize(512, 1024, (341, 1000), 2)
    share = _flagged_share([ms, A.complex_color_aug()], (1024, 2048))
    print("flagged share of ['MS', 'CCA'] over seeds 0..1999: %.4f" % share)
    assert 0.30 <= share <= 0.42
    assert _flagged_share(ms, (1024, 2048)) == 0
    assert _flagged_share(A.flip_crop_resize(768, 1024, (341, 1000), 1280 / 960), (1024, 2048)) == 0
    assert _flagged_share(A.resize_crop(512, 1024, 512, 512), (1024, 2048)) == 0
    assert _flagged_share(A.resize(256, 512), (1024, 2048), 200) == 0
    assert _flagged_share([A.resize(64, 128), A.simple_color_aug()], (1024, 2048)) > 0.6      # 'SCA': 3 in 4, expected


def test_copy_paste_select_then_crop_equals_run_original_then_crop(golden):
    """the inputs of tests/golden/copy_paste.npz: run_plan() draws what run_original() draws; the select on the crop window
    (host executor) equals run_original() followed by the same crop + resize"""
    from hiast_amd.utils.default_config import get_default_cfg
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import PREPROCESSOR
    g = golden("copy_paste")
    N, H, W, C = [int(v) for v in g["shape"]]
    imgs = synth.images_u8(1100, N, H, W)
    lbls = np.stack([synth.pseudo_labels(1110 + i, 1, H, W, C, 0.3)[0] for i in range(N)])
    names = ["img_%d.png" % i for i in range(N)]
    swc = {c: [names[i] for i in range(N) if (lbls[i] == c).any()] for c in range(C)}

    class DS:
        def get_samples_with_class(self):
            return swc

        def get_file_to_idx(self, f):
            return names.index(f)

        def load_data(self, i):
            return imgs[i].copy(), lbls[i].copy(), names[i]

    c = get_default_cfg()
    c.dataset.source.type = "GTAV"
    cp = PREPROCESSOR["CopyPaste"](c, DS(), g["class_value"].copy())
    aug = A.flip_crop_resize(H // 2, W // 2 + 3, (H // 3, H), 2)
    np.random.seed(888)
    want = [cp.run_original(imgs[i].copy(), lbls[i].copy()) for i in range(N)]
    state = np.random.get_state()
    np.random.seed(888)
    pasted = 0
    for i in range(N):
        assert np.array_equal(want[i][0], g["img"][i])
        paste, mask = cp.run_plan(imgs[i].copy(), lbls[i].copy())
        assert np.array_equal(mask, want[i][2])
        plan = DA.plan_sample(aug, (H, W), i)
        w_i, w_l = A.aug(aug, want[i][0], want[i][1], i)
        got_i, got_l = DA.execute_plan_host(plan, imgs[i], lbls[i], paste=paste)
        assert np.array_equal(got_i[0], w_i) and np.array_equal(got_l[0], w_l)
        pasted += paste is not None and bool((paste[2][paste[1]] != 0).any())
    assert pasted > 0
    s2 = np.random.get_state()
    assert state[0] == s2[0] and np.array_equal(state[1], s2[1]) and state[2:] == s2[2:]


def test_op_constants_are_the_same_in_the_planner_the_wrappers_and_the_header():
    """the op types and limits of a view's op row are written three times (device_aug.py for the planner, kernels.py for
    the host checks and the launch rounds, include/hiast_hip.h for the kernels): they must be one set of numbers"""
    import os
    import re
    from hiast_amd import kernels as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "hiast_hip.h")).read()
    hdr = {m.group(1): eval(m.group(2).replace("HIAST_AUG_MAX_OPS", "8"), {})
           for m in re.finditer(r"^#define HIAST_AUG_(\w+) (.+)$", txt, flags=re.M)}
    names = ("OP_LUT", "OP_GRAY", "OP_EQUALIZE", "OP_CONTRAST", "OP_SAT", "OP_HUE", "OP_BLUR", "OP_FDA", "MAX_OPS", "MAX_KSIZE",
             "OPS_WORDS", "REC_WORDS", "FDA_MAX_BORDER", "FDA_BORDER_SHIFT")
    assert sorted(hdr) == sorted(names)
    for n in names:
        assert getattr(K, "AUG_" + n) == getattr(DA, n) == hdr[n], n
    assert K.AUG_FDA_MIN_SIDE == DA.FDA_MIN_SIDE
    assert sorted(hdr[n] for n in names if n.startswith("OP_")) == list(range(1, 9))
    assert K.AUG_LEVEL1_OPS == (DA.OP_LUT, DA.OP_GRAY, DA.OP_EQUALIZE)
    assert K.AUG_TABLE_OPS == (DA.OP_EQUALIZE, DA.OP_CONTRAST) and K.AUG_CLOSING_OPS == (DA.OP_BLUR, DA.OP_FDA)
