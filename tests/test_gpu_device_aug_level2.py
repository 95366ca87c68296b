"""cfg.dataset.device_aug_level = 2 on the device (hiast_amd/csrc/sample_aug2.hip), everything through the C ABI: hue over all
2^24 colours against Pillow, saturation and contrast against augmentations.ColorJitter, the blur against
augmentations._blur_separable, chains against the numpy executor (device_aug.execute_plan_host, pinned to the host
transforms in tests/test_device_aug_level2_plan.py), and the whole path — dataset, collate, assemble_device_batch, one
training iteration — against the worker path.  Equality everywhere: bytes for uint8, bits for float32."""
import itertools
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


def _smooth(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([127.5 + 127.5 * np.sin(x / 37.0 + y / 91.0), 255.0 * x / max(w - 1, 1), 255.0 * (y / max(h - 1, 1)) ** 2], -1)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _plan(shape, *view_ops):
    """an identity geometry + the given op lists, one per view"""
    plan = DA.plan_sample(None, shape)
    plan[0]["ops"] += list(view_ops[0])
    return plan + [{"ops": list(o), "host": False} for o in view_ops[1:]]


def _run(K, samples):
    t = DA.build_batch_tables(samples)
    n_views, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    views, lbl = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, "cuda")
    torch.cuda.synchronize()
    assert len(views) == n_views
    return [v.cpu().numpy() for v in views], lbl.cpu().numpy()


def _device(K, plans_and_images):
    """[(plan, img)] of one output size -> per sample the list of its views"""
    lbl = np.zeros(plans_and_images[0][1].shape[:2], np.uint8)
    views, _ = _run(K, [DA.pack_sample(p, img, lbl) for p, img in plans_and_images])
    return [[v[b] for v in views] for b in range(len(plans_and_images))]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    d = int((got != want).sum())
    assert d == 0, "%s: %d differing bytes" % (what, d)


@pytest.fixture(scope="module")
def colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("shift", [0, 1, 51, 128, 205, 255])
def test_hue_on_all_colours_equals_pillow(K, colours, shift):
    """item 7: one 4096 x 4096 sample that holds every colour; shift 0 comes from a non-zero factor"""
    f = 0.001 if shift == 0 else shift / 256.0
    assert f != 0 and int(round(256 * f)) % 256 == shift
    op = DA._jitter_op(3, f)
    assert op == ("hue", shift)
    got = _device(K, [(_plan((4096, 4096), [op]), colours)])[0][0]
    _same(got, A.ColorJitter._hue(colours, f), "hue shift %d" % shift)


def test_saturation_and_contrast_on_all_colours_equal_the_host(K, colours):
    """item 7: the same frame; the contrast table is built on the device from the frame's gray mean (no integer)"""
    m = float(A._gray_cv(colours).mean())
    assert m != round(m)
    rs = random.Random(7)
    for f in (0.8, 1.2, rs.uniform(0.8, 1.2)):
        got = _device(K, [(_plan((4096, 4096), [("sat", f)], [("contrast", f)]), colours)])[0]
        sat = A.ColorJitter._saturation(colours, f)
        _same(got[0], sat, "saturation %r" % f)
        _same(got[1], A.ColorJitter._contrast(sat, f), "contrast %r (on the saturated frame)" % f)


def test_blur_batches_equal_blur_separable(K):
    """item 8: 512 x 1024: eight ksizes (3 and 41 among them) + one sample without a blur in one batch; 63 x 125 (rows of
    375 bytes: the byte path); noise and smooth frames"""
    big = [_frame(81, 512, 1024)[0], _smooth(512, 1024)]
    ks = [3, 5, 9, 15, 21, 31, 37, 41]
    cases = [(_plan((512, 1024), [("blur", DA.blur_weights(k, 0))]), big[n % 2]) for n, k in enumerate(ks)]
    cases.append((_plan((512, 1024), []), big[0]))
    got = _device(K, cases)
    for (plan, img), g, k in zip(cases, got, ks + [None]):
        want = img if k is None else A._blur_separable(img, A._gaussian_kernel_cv(k, 0))
        _same(g[0], want, "512x1024 ksize %s" % k)
    small = [_frame(82, 63, 125)[0], _smooth(63, 125)]
    ks = [3, 7, 13, 27, 41, 41]
    cases = [(_plan((63, 125), [("blur", DA.blur_weights(k, 0))]), small[n % 2]) for n, k in enumerate(ks)]
    for (plan, img), g, k in zip(cases, _device(K, cases), ks):
        _same(g[0], A._blur_separable(img, A._gaussian_kernel_cv(k, 0)), "63x125 ksize %d" % k)


def _compare_with_executor(K, cases, what):
    got = _device(K, cases)
    for b, (plan, img) in enumerate(cases):
        want, _ = DA.execute_plan_host(plan, img, np.zeros(img.shape[:2], np.uint8))
        assert len(want) == len(got[b])
        for k, w in enumerate(want):
            _same(got[b][k], w, "%s: sample %d view %d" % (what, b, k))


@pytest.mark.parametrize("shape", [(96, 160), (63, 125)], ids=["words", "bytes"])
def test_chains_equal_the_numpy_executor(K, shape):
    """item 9: ColorJitter in all 24 orders; ColorJitter + Equalize + GaussianBlur in the 6 orders; a second view that
    blurs the first view's bytes"""
    img = _frame(91, *shape)[0]
    narrow = (img // 3 + 40).astype(np.uint8)
    cj = lambda order, fs: [op for op in (DA._jitter_op(i, fs[i]) for i in order) if op is not None]      # noqa: E731
    orders = list(itertools.permutations(range(4)))
    assert len(orders) == 24
    cases = []
    for n, order in enumerate(orders):
        fs = (0.83 + 0.01 * n, 1.17 - 0.01 * n, 0.9 + 0.005 * n, (0.001, 0.17, -0.137, 0.2, -0.05, 0.0)[n % 6])
        ops = cj(order, fs)
        assert len(ops) == (3 if fs[3] == 0.0 else 4)
        # the plan of the host transform itself is what runs
        want = A.ColorJitter().apply(img, [], factors=fs, order=list(order))[0]
        assert np.array_equal(DA.execute_colour_host(ops, img), want)
        cases.append((_plan(shape, ops), img if n % 2 else narrow))
    for a in range(0, 24, 8):
        _compare_with_executor(K, cases[a:a + 8], "ColorJitter orders %d.." % a)
    fs = (1.1, 0.85, 1.15, -0.09)
    parts = {"cj": cj((2, 0, 3, 1), fs), "eq": [("equalize",)], "blur": [("blur", DA.blur_weights(11, 0))]}
    cases = [(_plan(shape, sum((parts[p] for p in perm), [])), narrow) for perm in itertools.permutations(parts)]
    assert len(cases) == 6 and all(len(c[0][0]["ops"]) == 7 for c in cases)
    _compare_with_executor(K, cases, "ColorJitter + Equalize + GaussianBlur")
    lut = A._brightness_contrast_lut(1.3, 0.0)
    two = [(_plan(shape, [("lut", lut), ("contrast", 0.9)], [("blur", DA.blur_weights(5, 0))]), img),
           (_plan(shape, [], [("blur", DA.blur_weights(21, 0)), ("hue", 40), ("blur", DA.blur_weights(3, 0))]), narrow),
           (_plan(shape, [("equalize",), ("contrast", 1.2), ("equalize",)], []), narrow),
           (_plan(shape, [("gray",)], [("sat", 1.1)]), img)]
    _compare_with_executor(K, two, "two views")


def test_bad_level2_rows_never_reach_the_device(K):
    img, lbl = _frame(7, 64, 128)
    plan = _plan((64, 128), [("blur", DA.blur_weights(9, 0))])
    t = DA.build_batch_tables([DA.pack_sample(plan, img, lbl)])
    ops = t["ops"].clone()
    ops[0, 0, 5] = (int(ops[0, 0, 5]) & 0xFFFFFFFF) | (8 << 32)
    with pytest.raises(ValueError):
        K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], ops, 64, 128, 64, "cuda")
    ops = t["ops"].clone()
    ops[0, 0, 4] = 9
    with pytest.raises(ValueError):
        K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], ops, 64, 128, 64, "cuda")


# ------------------------------------------------------------------------------------------------- end to end
H, W, N = 400, 800, 8
BATCH_SEED = 5


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a target set with hand-written generator artefacts: pseudo-labels = the labels, every class 'hard' in turn"""
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    from hiast_amd.tools import synth_data
    root = str(tmp_path_factory.mktemp("device_aug2"))
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


def test_dataset_to_device_batch_is_bit_equal_at_level_2(K, world):
    """item 10: the same seeded samples (['MS', 'CCA'], CopyPaste on) read by the worker path and as level-2 plans: no
    finished sample, ColorJitter and GaussianBlur samples among them; assemble_device_batch vs to_device_batch"""
    from torch.utils.data import default_collate
    from hiast_amd.sseg.datasets import utils as du
    from hiast_amd.sseg.datasets.preprocessor import CopyPaste
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    t = world.dataset.target
    ds = CityscapesDataset(world, t.json_path, t.image_dir, pseudo_dir=t.pseudo_dir, aug_type=t.aug_type)
    ds.set_preprocessor(CopyPaste(world, ds, np.load(os.path.join(t.pseudo_dir, "..", "class_mean_probabilities.npy"))))
    ds.device_transform = True
    ds.device_aug = False
    _seed(BATCH_SEED)
    plain = default_collate([ds[i] for i in range(N)])
    ds.device_aug = True
    ds.device_aug_level = 2
    _seed(BATCH_SEED)
    items = [ds[i] for i in range(N)]
    assert sum(it["plan"] is None for it in items) == 0, "a sample fell back to the worker path at level 2"
    names = [[op[0] for v in it["plan"] for op in v["ops"]] for it in items]
    assert any("contrast" in n and "sat" in n for n in names), "no ColorJitter sample in the batch"
    assert any("blur" in n for n in names), "no GaussianBlur sample in the batch"
    assert any("paste_img" in it["raw"] for it in items)
    batch = DA.collate(items)
    assert torch.equal(batch["copy_paste_mask"], plain["copy_paste_mask"]) and batch["image_paths"] == plain["image_paths"]
    assert int((batch["device_aug"]["recs"][:, DA.R_KIND] != DA.KIND_PLAN).sum()) == 0
    want_i, want_l = du.to_device_batch(plain["images"], plain["labels"], torch.device("cuda"))
    got_i, got_l = du.assemble_device_batch(batch, torch.device("cuda"))
    torch.cuda.synchronize()
    assert len(got_i) == len(want_i) == 2
    for a, b in zip(got_i, want_i):
        assert a.dtype == torch.float32 and a.shape == b.shape == (N, 3, 512, 1024)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(got_l, want_l):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_one_training_iteration_is_bit_equal_at_level_2(K, world):
    """item 11: device_aug off against device_aug at level 2"""
    from hiast_amd.utils.registry.registries import TRAINER
    losses = []
    for on in (False, True):
        c = world.clone()
        c.dataset.device_aug = on
        c.dataset.device_aug_level = 2 if on else 1
        c.freeze()
        _seed(9)
        tr = TRAINER[c.trainer](c, 0)
        assert bool(tr.t_dataset.device_aug) is on
        assert tr.t_dataset.device_aug_level == (2 if on else 1)
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
