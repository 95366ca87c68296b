"""cfg.dataset.device_aug on the device (hiast_amd/csrc/sample_aug.hip, the colour ops in sample_aug2.hip): the kernels against the numpy executor of the same
plan (device_aug.execute_plan_host, itself pinned to augmentations.aug() and Pillow in tests/test_device_aug_plan.py), and
the whole path — dataset, collate, assemble_device_batch, one training iteration — against the worker path.  Equality
everywhere: bytes for uint8, bits for float32."""
import json
import os
import random

import numpy as np
import pytest
import torch

from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def _frame(seed, h, w):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 20, (h, w), dtype=np.uint8)


def _paste_for(seed, h, w):
    img, lbl = _frame(seed, h, w)
    table = np.zeros(256, np.uint8)
    table[[3, 7, 12, 18]] = 1
    return img, lbl, table


def _plan_with_flip(aug, shape, flip):
    for seed in range(64):
        plan = DA.plan_sample(aug, shape, seed)
        if plan[0]["ops"][0][1].flip == flip:
            return plan
    raise AssertionError("no seed gives flip=%s" % flip)


def _pack(plan, img, lbl, paste=None):
    y1, y2, x1, x2 = DA.plan_window(plan)
    if paste is not None:
        paste = (paste[0][y1:y2, x1:x2], paste[1][y1:y2, x1:x2], paste[2])
    return DA.pack_sample(plan, img[y1:y2, x1:x2], lbl[y1:y2, x1:x2], paste)


def _run(K, samples):
    t = DA.build_batch_tables(samples)
    n_views, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    views, lbl = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, "cuda")
    torch.cuda.synchronize()
    assert len(views) == n_views
    return [v.cpu().numpy() for v in views], lbl.cpu().numpy()


def _compare(K, cases):
    """cases: (plan, img, lbl, paste or None); every sample of the batch against the numpy executor"""
    views, lbl = _run(K, [_pack(*c) for c in cases])
    for b, (plan, img, lbl_h, paste) in enumerate(cases):
        want_i, want_l = DA.execute_plan_host(plan, img, lbl_h, paste=paste)
        for k, w in enumerate(want_i):
            d = int((views[k][b] != w).sum())
            assert d == 0, "sample %d view %d: %d differing bytes" % (b, k, d)
        assert int((lbl[b] != want_l[0]).sum()) == 0, "sample %d: label" % b


def test_geometry_full_size_batch_of_eight(K):
    """8 samples, 8 windows, all to 512 x 1024: an 'MS' crop at full size (1000 x 2000), an upscale (341 x 682), one axis
    unchanged (512 x 900), further 'MS' heights; with and without flip, with and without the CopyPaste select"""
    ms = lambda h: A.flip_crop_resize(512, 1024, (h, h), 2)       # noqa: E731
    big, big_l = _frame(1, 1024, 2048)
    mid, mid_l = _frame(2, 640, 1280)
    flat, flat_l = _frame(3, 512, 900)
    cases = [
        (_plan_with_flip(ms(1000), (1024, 2048), True), big, big_l, _paste_for(11, 1024, 2048)),
        (_plan_with_flip(ms(341), (1024, 2048), False), big, big_l, None),
        (_plan_with_flip(A.resize(512, 1024), (512, 900), False), flat, flat_l, _paste_for(12, 512, 900)),
        (_plan_with_flip(ms(341), (640, 1280), True), mid, mid_l, _paste_for(13, 640, 1280)),
        (_plan_with_flip(ms(455), (640, 1280), False), mid, mid_l, _paste_for(14, 640, 1280)),
        (_plan_with_flip(ms(519), (640, 1280), True), mid, mid_l, None),
        (_plan_with_flip(ms(600), (640, 1280), False), mid, mid_l, None),
        (_plan_with_flip(ms(640), (640, 1280), True), mid, mid_l, None),
    ]
    assert len({DA.plan_window(c[0]) for c in cases}) == 8
    g0 = cases[0][0][0]["ops"][0][1]
    assert (g0.src[1] - g0.src[0], g0.src[3] - g0.src[2]) == (1000, 2000) and g0.hk.shape[1] == 5
    _compare(K, cases)


def test_geometry_small_odd_sizes_and_crop_after_resize(K):
    """output rows that are no multiple of 4 bytes (the scalar paths), a 33-tap downscale, 'DACS' (resize, then crop)"""
    img, lbl = _frame(4, 37, 91)
    odd = lambda s, flip: _plan_with_flip(A.Compose([A.HorizontalFlip(0.5), A.RandomSizedCrop((20, 37), 63, 125, 2)]),  # noqa: E731
                                          (37, 91), flip)
    _compare(K, [(odd(0, True), img, lbl, _paste_for(15, 37, 91)), (odd(1, False), img, lbl, None)])
    big, big_l = _frame(5, 512, 1024)
    _compare(K, [(DA.plan_sample(A.resize(32, 64), (512, 1024)), big, big_l, None),
                 (DA.plan_sample(A.resize(32, 64), (512, 1024)), big[::-1].copy(), big_l[::-1].copy(), _paste_for(16, 512, 1024))])
    mid, mid_l = _frame(6, 300, 500)
    _compare(K, [(DA.plan_sample(A.resize_crop(128, 256, 96, 96), (300, 500), s), mid, mid_l, None) for s in range(3)])


def _colour_plan(shape, *view_ops):
    plan = DA.plan_sample(None, shape)
    plan[0]["ops"] += list(view_ops[0])
    return plan + [{"ops": list(o), "host": False} for o in view_ops[1:]]


@pytest.mark.parametrize("shape", [(96, 160), (63, 125)], ids=["words", "bytes"])
def test_colour_ops_alone_and_composed(K, shape):
    h, w = shape
    g = np.random.Generator(np.random.PCG64(21))
    img, lbl = _frame(22, h, w)
    narrow = (img // 3 + 40).astype(np.uint8)                      # a histogram that equalisation stretches
    const = img.copy()
    const[..., 1] = 77                                              # Equalize: a constant channel stays as it is
    spike = img.copy()
    spike[..., 2] = 10                                              # the lowest bin holds all but one pixel
    spike[h // 2, w // 3, 2] = 200
    lut1 = g.integers(0, 256, 256).astype(np.uint8)
    lut2 = A._brightness_contrast_lut(1.7, 0.0)
    sol = np.array([i if i < 128 else 255 - i for i in range(256)], np.uint8)
    L, G, E = (lambda t: ("lut", t)), ("gray",), ("equalize",)
    cases = [
        (_colour_plan(shape, [L(lut1)]), img, lbl, None),
        (_colour_plan(shape, [G]), img, lbl, None),
        (_colour_plan(shape, [E]), narrow, lbl, None),
        (_colour_plan(shape, [E]), const, lbl, None),
        (_colour_plan(shape, [E]), spike, lbl, None),
        (_colour_plan(shape, [L(lut2), E, G]), narrow, lbl, None),
        (_colour_plan(shape, [G, L(sol), E]), img, lbl, None),
        (_colour_plan(shape, []), img, lbl, None),
    ]
    _compare(K, cases)
    # the serial multi-view rule: view 1 = its ops on view 0's bytes
    two = [(_colour_plan(shape, [L(lut2)], [E, L(sol)]), narrow, lbl, None),
           (_colour_plan(shape, [], [G]), img, lbl, None),
           (_colour_plan(shape, [E], []), spike, lbl, None)]
    _compare(K, two)
    want = DA.execute_plan_host(cases[4][0], spike, lbl)[0][0]
    assert set(np.unique(want[..., 2])) == {0, 255}                 # (the spike case is the one it claims to be)


def test_level1_batches_issue_the_level1_launches(K, monkeypatch):
    """rows of level-1 ops go through the segment kernels in ONE round: geometry, the table launches only when a row
    equalises, one colour pass; a batch without ops and without finished samples is the geometry alone"""
    img, lbl = _frame(23, 48, 96)
    lut = A._brightness_contrast_lut(1.3, 0.0)

    def plan(*ops):
        p = DA.plan_sample(A.resize(32, 64), (48, 96))
        p[0]["ops"] += list(ops)
        return p
    L, E = ("lut", lut), ("equalize",)
    geometry, table, colour = "hiast_aug_geometry_u8", "hiast_aug2_table_u8", "hiast_aug2_colour_u8"
    seen = []
    check = K.check
    monkeypatch.setattr(K, "check", lambda rc, what: (seen.append(what), check(rc, what))[1])
    for rows, want in (([[L], [L]], [geometry, colour]),
                       ([[L], [L, E]], [geometry, table, colour]),
                       ([[], []], [geometry])):
        del seen[:]
        _compare(K, [(plan(*ops), img, lbl, None) for ops in rows])
        assert seen == want, (rows, seen)


def test_bad_tables_are_refused_on_the_host(K):
    img, lbl = _frame(7, 64, 128)
    t = DA.build_batch_tables([_pack(DA.plan_sample(A.resize(32, 64), (64, 128)), img, lbl)])
    recs = t["recs"].clone()
    recs[0, DA.R_CW] = 64
    with pytest.raises(ValueError):
        K.aug_batch_u8(t["blob"], t["tabs"], recs, t["ops"], 32, 64, 64, "cuda")
    with pytest.raises(Exception):
        K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 32, 64, 64, "cpu")


# ------------------------------------------------------------------------------------------------- end to end
H, W, N = 400, 800, 8


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a target set with hand-written generator artefacts: pseudo-labels = the labels, every class 'hard' in turn"""
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    from hiast_amd.tools import synth_data
    root = str(tmp_path_factory.mktemp("device_aug"))
    cfg = synth_data.synthetic_cfg(root, n_train=N, n_val=1, h=H, w=W, upscale=4)
    pdir = cfg.pseudo_policy.save_dir
    os.makedirs(pdir, exist_ok=True)
    swc = {c: [] for c in range(19)}
    for e in json.load(open(cfg.dataset.target.json_path)):
        lbl = np.array(Image.open(os.path.join(cfg.dataset.target.image_dir, e["mask_name"])))
        stem = os.path.splitext(os.path.basename(e["image_name"]))[0]
        Image.fromarray(lbl).save(os.path.join(pdir, stem + "_pseudo_label.png"))
        for c in range(19):
            if (lbl == c).any():
                swc[c].append([os.path.basename(e["image_name"]), int((lbl == c).sum())])
    with open(os.path.join(pdir, "..", "samples_with_class.json"), "w") as f:
        json.dump(swc, f)
    np.save(os.path.join(pdir, "..", "class_mean_probabilities.npy"), np.linspace(0.55, 0.95, 19))
    torch.manual_seed(31)
    ck = os.path.join(root, "init.pth")
    torch.save(MODEL["SelfTrainingSegmentor"](cfg).state_dict(), ck)
    cfg.train.resume_from = ck
    cfg.train.amp_dtype = "bf16"
    cfg.trainer = "ConsistencySelfTrainingTrainer"
    cfg.dataset.target.pseudo_dir = pdir
    cfg.dataset.target.aug_type = ["MS", "CCA"]
    cfg.cst_training.is_enabled = True
    cfg.cst_training.cst_loss.weight = 0.5
    cfg.preprocessor.type = "CopyPaste"
    cfg.train.gpu_num, cfg.train.batch_size, cfg.train.total_iter = 1, 4, 1
    cfg.train.iter_report = cfg.train.iter_val = 10 ** 6
    cfg.train.lr = 3e-6
    cfg.work_dir = os.path.join(root, "work")
    return cfg


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_dataset_to_device_batch_is_bit_equal(K, world):
    """the same seeded samples (['MS', 'CCA'], CopyPaste on) read by the worker path and as plans: planned and host-fallback
    samples in one batch; assemble_device_batch vs to_device_batch"""
    from torch.utils.data import default_collate
    from hiast_amd.sseg.datasets import utils as du
    from hiast_amd.sseg.datasets.preprocessor import CopyPaste
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    t = world.dataset.target
    ds = CityscapesDataset(world, t.json_path, t.image_dir, pseudo_dir=t.pseudo_dir, aug_type=t.aug_type)
    ds.set_preprocessor(CopyPaste(world, ds, np.load(os.path.join(t.pseudo_dir, "..", "class_mean_probabilities.npy"))))
    ds.device_transform = True
    ds.device_aug = False
    _seed(5)
    plain = default_collate([ds[i] for i in range(N)])
    ds.device_aug = True
    _seed(5)
    items = [ds[i] for i in range(N)]
    n_host = sum(it["plan"] is None for it in items)
    assert 0 < n_host < N, "the batch must hold planned and host-fallback samples (%d of %d fell back)" % (n_host, N)
    assert any("paste_img" in it["raw"] for it in items)
    batch = DA.collate(items)
    assert torch.equal(batch["copy_paste_mask"], plain["copy_paste_mask"]) and batch["image_paths"] == plain["image_paths"]
    want_i, want_l = du.to_device_batch(plain["images"], plain["labels"], torch.device("cuda"))
    got_i, got_l = du.assemble_device_batch(batch, torch.device("cuda"))
    torch.cuda.synchronize()
    assert len(got_i) == len(want_i) == 2
    for a, b in zip(got_i, want_i):
        assert a.dtype == torch.float32 and a.shape == b.shape == (N, 3, 512, 1024)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(got_l, want_l):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_one_training_iteration_is_bit_equal(K, world):
    from hiast_amd.utils.registry.registries import TRAINER
    losses = []
    for on in (False, True):
        c = world.clone()
        c.dataset.device_aug = on
        c.freeze()
        _seed(9)
        tr = TRAINER[c.trainer](c, 0)
        assert bool(tr.t_dataset.device_aug) is on
        _seed(9)
        out = tr.train()
        torch.cuda.synchronize()
        losses.append({k: v.detach().float().cpu().clone() for k, v in out.items()})
        tr.t_iter = tr.t_loader = None
        del tr
    assert set(losses[0]) == set(losses[1]) and len(losses[0]) >= 3
    for k in losses[0]:
        print(k, float(losses[0][k]), float(losses[1][k]))
        assert torch.isfinite(losses[0][k]).all()
        assert torch.equal(losses[0][k].view(torch.int32), losses[1][k].view(torch.int32)), k
