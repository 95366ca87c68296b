"""cfg.dataset.device_aug_level = 3 on the device (hiast_amd/csrc/sample_aug3.hip), through the C ABI: FDA in its
sparse-DFT form.

Comparison B — the device against device_aug.fda_u8 (the same formula, float64 on both sides, another summation order):
bytes are equal except where the float64 value before truncation (device_aug.fda_f64) is within 1e-6 of an integer; there
they differ by at most 1; at most 1e-4 of the bytes lie in that band (asserted first).  Comparison A (against the host
FFT, tests/test_device_aug_level3_plan.py) is used where the worker path is the other side."""
import json
import os
import random

import numpy as np
import pytest
import torch

import guard_bands as gb
from fda_compare import band_b, comparison_a, comparison_b, smooth_noise

from hiast_amd.sseg.datasets import device_aug as DA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def _plan(shape, ops, targets=()):
    """an identity geometry + the ops of ONE view; targets: the frames its ("fda", key, border) ops name"""
    plan = DA.plan_sample(None, shape)
    plan[0]["ops"] += list(ops)
    frames = {"target/%d" % i: t for i, t in enumerate(targets)}
    plan[0]["readers"] = {k: frames.__getitem__ for k in frames}
    return plan


def _device(K, cases):
    """[(plan, img)] of one shape -> the view of every sample"""
    lbl = np.zeros(cases[0][1].shape[:2], np.uint8)
    t = DA.build_batch_tables([DA.pack_sample(p, img, lbl) for p, img in cases])
    n_views, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    views, _ = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, "cuda")
    torch.cuda.synchronize()
    assert n_views == len(views) == 1
    return views[0].cpu().numpy()


@pytest.fixture(scope="module")
def frames():
    """per shape: four images, three targets of another mean (computed once, never written).  In a frame of under
    10 000 bytes ONE byte within 1e-6 of an integer is already above comparison B's cap of 1e-4, which every test asserts
    on the oracle first: the seeds are such that the cap holds (it is a property of the input, not of the device)"""
    out = {}
    for h, w in ((33, 47), (61, 83), (72, 40), (130, 258)):
        out[(h, w)] = ([smooth_noise(7 * h + w + 10 * i, h, w, 90.0 + 5 * i) for i in range(4)],
                       [smooth_noise(7 * w + h + 10 * i, h, w, 150.0 + 7 * i) for i in range(3)])
    return out


@pytest.mark.parametrize("shape", [(33, 47), (61, 83), (72, 40), (130, 258)], ids=lambda s: "%dx%d" % s)
def test_fda_batches_against_fda_u8(K, frames, shape):
    """borders 0, 1 and 2 in one batch + a sample without an FDA op (bit-equal to its input); rows of W * 3 bytes that
    are no multiple of 4 (the byte path), odd heights, 130 rows = 5 row-band partials per sample; the same call twice"""
    imgs, tgts = frames[shape]
    cases = [(_plan(shape, [("fda", "target/0", b)], [tgts[b]]), imgs[b]) for b in (0, 1, 2)]
    cases.append((_plan(shape, []), imgs[3]))
    got = _device(K, cases)
    for b in (0, 1, 2):
        f = DA.fda_f64(imgs[b], tgts[b], b)
        want = DA.fda_u8(imgs[b], tgts[b], b)
        assert int((want != imgs[b]).sum()) > want.size // 2
        comparison_b(got[b], want, band_b(f, "%s border %d" % (shape, b)), "%s border %d" % (shape, b))
    assert np.array_equal(got[3], imgs[3]), "the sample without an FDA op was touched"
    assert np.array_equal(_device(K, cases), got), "the same call returned other bytes"


def test_target_equal_to_the_image_returns_the_image(K, frames):
    for shape in ((33, 47), (130, 258)):
        imgs, _ = frames[shape]
        cases = [(_plan(shape, [("fda", "target/0", b)], [imgs[b].copy()]), imgs[b]) for b in (0, 1, 2)]
        got = _device(K, cases)
        for b in (0, 1, 2):
            assert np.array_equal(got[b], imgs[b]), (shape, b)


def test_two_fda_ops_in_one_row(K, frames):
    """each closes a segment of its own; the second meets the bytes the first wrote"""
    shape = (61, 83)
    imgs, tgts = frames[shape]
    plan = _plan(shape, [("fda", "target/0", 1), ("fda", "target/1", 2)], tgts[:2])
    got = _device(K, [(plan, imgs[0]), (_plan(shape, [("fda", "target/0", 0)], [tgts[2]]), imgs[1])])
    first = band_b(DA.fda_f64(imgs[0], tgts[0], 1), "first FDA op")
    assert not first.any(), "a byte of the first op sits in the band: the second op would see another image (bad input)"
    mid = DA.fda_u8(imgs[0], tgts[0], 1)
    comparison_b(got[0], DA.fda_u8(mid, tgts[1], 2), band_b(DA.fda_f64(mid, tgts[1], 2), "second FDA op"), "two FDA ops")
    comparison_b(got[1], DA.fda_u8(imgs[1], tgts[2], 0), band_b(DA.fda_f64(imgs[1], tgts[2], 0), "one"), "one FDA op")


@pytest.mark.parametrize("shape", [(33, 47), (40, 72)], ids=lambda s: "%dx%d" % s)
def test_guarded_buffers(K, frames, shape):
    """image, workspace and trig table carved out of poisoned allocations: nothing outside them is written (the
    workspace size function is sufficient as stated) and no poison is read into the result"""
    from hiast_amd import _lib
    lib = _lib.load()
    H, W = shape
    imgs = [smooth_noise(300 + i, H, W, 100.0) for i in range(3)]
    tgts = [smooth_noise(400 + i, H, W, 160.0) for i in range(2)]
    borders = (2, 1)
    B = 3
    blob = DA._Blob(np.uint8)
    rows = np.zeros((B, DA.OPS_WORDS), np.int64)
    for b, bd in enumerate(borders):
        rows[b, 2], rows[b, 4], rows[b, 5] = 1, DA.OP_FDA, blob.add(tgts[b]) | (bd << DA.FDA_BORDER_SHIFT)
    seg = K._aug_segments(rows)
    assert seg.shape == (1, B, 4) and seg[0].tolist() == [[0, 0, -1, 0], [0, 0, -1, 0], [0, 0, -1, -1]]
    dev = "cuda"
    ops_d, seg_d, blob_d = torch.from_numpy(rows).to(dev), torch.from_numpy(seg[0]).to(dev), torch.from_numpy(blob.join()).to(dev)
    ws_bytes = lib.hiast_aug3_fda_workspace_bytes(B, H, W)
    assert ws_bytes == B * (2 * ((H + 31) // 32) + 1) * 75 * 8
    assert lib.hiast_aug3_fda_workspace_bytes(0, H, W) == 0
    img, h_img = gb.carve((B, H, W, 3), torch.uint8, dev, 4096)
    gb.fill(img, torch.from_numpy(np.stack(imgs)))
    ws, h_ws = gb.carve(ws_bytes, torch.float64, dev, 4096)
    trig, h_trig = gb.carve((2 * H + 2 * W,), torch.float64, dev, 4096)
    gb.fill(trig, torch.from_numpy(np.concatenate(DA.fda_trig(H) + DA.fda_trig(W))))
    rc = lib.hiast_aug3_fda_u8(ops_d.data_ptr(), seg_d.data_ptr(), blob_d.data_ptr(), trig.data_ptr(), img.data_ptr(),
                               ws.data_ptr(), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0
    for h, nm in ((h_img, "img"), (h_ws, "ws"), (h_trig, "trig")):
        gb.check(h, nm)
    got = img.cpu().numpy()
    for b, bd in enumerate(borders):
        what = "%s guarded, border %d" % (shape, bd)
        comparison_b(got[b], DA.fda_u8(imgs[b], tgts[b], bd), band_b(DA.fda_f64(imgs[b], tgts[b], bd), what), what)
    assert np.array_equal(got[2], imgs[2])
    # refused calls write nothing
    out, h_out = gb.carve((B, H, W, 3), torch.uint8, dev, 4096)
    assert lib.hiast_aug3_fda_u8(ops_d.data_ptr(), seg_d.data_ptr(), blob_d.data_ptr(), trig.data_ptr(), out.data_ptr(),
                                 None, B, H, W, None) == -1
    assert lib.hiast_aug3_fda_u8(ops_d.data_ptr(), seg_d.data_ptr(), blob_d.data_ptr(), trig.data_ptr(), out.data_ptr(),
                                 ws.data_ptr(), B, 7, W, None) == -2
    torch.cuda.synchronize()
    gb.check_untouched(h_out, "img of a refused call")


def _dilate(mask, r):
    """mask [H, W, C] grown by r pixels along both image axes"""
    out = mask.copy()
    for axis in (0, 1):
        acc = out.copy()
        for s in range(1, r + 1):
            acc |= np.roll(out, s, axis) | np.roll(out, -s, axis)
        out = acc
    return out.any(-1, keepdims=True) | out


def test_fda_between_level2_ops_against_the_numpy_executor(K, frames):
    """ColorJitter's steps before the FDA, a GaussianBlur after it: equal bytes, except within the blur's reach of a byte
    of the FDA step that sits in comparison B's band"""
    shape = (61, 83)
    imgs, tgts = frames[shape]
    jitter = [DA._jitter_op(0, 1.1), DA._jitter_op(1, 0.9), DA._jitter_op(2, 1.15), DA._jitter_op(3, -0.09)]
    cases, wants, bands = [], [], []
    for b, k in ((0, 5), (1, 9), (2, 3)):
        plan = _plan(shape, jitter + [("fda", "target/0", b), ("blur", DA.blur_weights(k, 0))], [tgts[b]])
        cases.append((plan, imgs[b]))
        pre = DA.execute_colour_host(jitter, imgs[b])
        band = band_b(DA.fda_f64(pre, tgts[b], b), "chain %d" % b)
        bands.append(_dilate(band, k // 2))
        wants.append(DA.execute_plan_host(plan, imgs[b], np.zeros(shape, np.uint8))[0][0])
        assert np.array_equal(wants[-1], DA.blur_u8(DA.fda_u8(pre, tgts[b], b), DA.blur_weights(k, 0)))
    got = _device(K, cases)
    for b in range(3):
        comparison_b(got[b], wants[b], bands[b], "ColorJitter + FDA + GaussianBlur, border %d" % b)


# ------------------------------------------------------------------------------------------------- end to end
H, W, N = 400, 800, 4


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a synthetic Cityscapes target set with hand-written generator artefacts; its val split is the GTAV source set, so
    an FDA never draws the frame it is applied to as its reference (target == img is tested on its own above)"""
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    from hiast_amd.tools import synth_data
    root = str(tmp_path_factory.mktemp("device_aug3"))
    cfg = synth_data.synthetic_cfg(root, n_train=N, n_val=N, h=H, w=W, upscale=4)
    cfg.dataset.source.type = "GTAV"
    cfg.dataset.source.json_path, cfg.dataset.source.image_dir = cfg.dataset.val.json_path, cfg.dataset.val.image_dir
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
    cfg.dataset.target.aug_type = ["MS", "FDA-Source"]
    cfg.cst_training.is_enabled = True
    cfg.cst_training.cst_loss.weight = 0.5
    cfg.preprocessor.type = "CopyPaste"
    cfg.train.gpu_num, cfg.train.batch_size, cfg.train.total_iter = 1, 2, 1
    cfg.train.iter_report = cfg.train.iter_val = 10 ** 6
    cfg.train.lr = 3e-6
    cfg.work_dir = os.path.join(root, "work")
    return cfg


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_dataset_to_device_batch_at_level_3(K, world):
    """['MS', 'FDA-Target'] on the source dataset, read by the worker path and as level-3 plans: no finished sample;
    assemble_device_batch against to_device_batch: labels and the MS view bit-equal, the FDA view under comparison A"""
    from torch.utils.data import default_collate
    from hiast_amd.sseg.datasets import utils as du
    from hiast_amd.sseg.datasets.loader.gtav_dataset import GTAVDataset
    s = world.dataset.source
    ds = GTAVDataset(world, s.json_path, s.image_dir, aug_type=["MS", "FDA-Target"])
    ds.device_transform = True
    ds.device_aug = False
    _seed(5)
    plain_items = [ds[i] for i in range(N)]
    plain = default_collate(plain_items)
    ds.device_aug = True
    ds.device_aug_level = 3
    _seed(5)
    items = [ds[i] for i in range(N)]
    assert sum(it["plan"] is None for it in items) == 0, "a sample fell back to the worker path at level 3"
    batch = DA.collate(items)
    assert int((batch["device_aug"]["recs"][:, DA.R_KIND] != DA.KIND_PLAN).sum()) == 0
    assert batch["image_paths"] == plain["image_paths"]
    dev = torch.device("cuda")
    want_i, want_l = du.to_device_batch(plain["images"], plain["labels"], dev)
    got_i, got_l = du.assemble_device_batch(batch, dev)
    torch.cuda.synchronize()
    assert len(got_i) == len(want_i) == 2 and got_i[1].shape == want_i[1].shape == (N, 3, 512, 1024)
    for a, b in zip(got_l, want_l):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(got_i[0].view(torch.int32), want_i[0].view(torch.int32))
    t = batch["device_aug"]
    views, _ = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 512, 1024, int(t["meta"][3]), "cuda")
    assert torch.equal(K.normalize_u8(views[1], du.MEAN, du.STD).view(torch.int32), got_i[1].view(torch.int32))
    got_u8 = views[1].cpu().numpy()
    for b, it in enumerate(items):
        op = it["plan"][1]["ops"][0]
        assert op[0] == "fda"
        ms_view = plain["images"][0][b].numpy()
        f = DA.fda_f64(ms_view, it["raw"]["fda"][0].numpy(), op[2])
        comparison_a(got_u8[b], plain["images"][1][b].numpy(), f, "sample %d" % b)
        comparison_b(got_u8[b], np.clip(f, 0, 255).astype(np.uint8), band_b(f, "sample %d" % b), "sample %d" % b)


def test_one_training_iteration_at_level_3(K, world):
    """a ['MS', 'FDA-Source'] target set (CopyPaste on) through the trainer's own loader at level 3: plans, finite losses"""
    from hiast_amd.utils.registry.registries import TRAINER
    c = world.clone()
    c.dataset.device_aug = True
    c.dataset.device_aug_level = 3
    c.freeze()
    _seed(9)
    tr = TRAINER[c.trainer](c, 0)
    assert tr.t_dataset.device_aug is True and tr.t_dataset.device_aug_level == 3
    seen = []
    fetch = tr.next_target_batch

    def watched():
        b = fetch()
        seen.append(b)
        return b
    tr.next_target_batch = watched
    out = tr.train()
    torch.cuda.synchronize()
    assert len(seen) == 1 and "device_aug" in seen[0]
    recs, ops = seen[0]["device_aug"]["recs"], seen[0]["device_aug"]["ops"]
    assert int((recs[:, DA.R_KIND] != DA.KIND_PLAN).sum()) == 0 and bool((ops[1, :, 4] == DA.OP_FDA).all())
    assert len(out) >= 3
    for k, v in out.items():
        print(k, float(v))
        assert torch.isfinite(v.detach().float()).all(), k
    tr.t_iter = tr.t_loader = None
    del tr
