"""cfg.dataset.device_store_gb on the device (hiast_aug_geometry_store_u8, hiast_normalize_gather_u8 and the path above them):
records of kind 2 read their windows in place from the store of decoded frames.  Every comparison is an equality — bytes for
uint8, bits for float32, integers for the validation counts — against the bytes path, and for the geometry also against
the numpy executor on the full frames.  Neighbouring frames of the store hold different seeded bytes, so a read across a
frame boundary (a wrong stride, a wrong offset) changes the result."""
import os

import numpy as np
import pytest
import torch

import device_store_world as W
from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA
from hiast_amd.sseg.datasets import device_store as DS

pytestmark = pytest.mark.gpu

# the store of the kernel tests: 37 x 91 (row bytes 273, no multiple of 4) and 64 x 128, each twice (a CopyPaste source needs
# the frame's shape), and one frame large enough for a 33-tap downscale to 16 x 32 and 11 x 33; the last frame is a small one
FRAME_SHAPES = [(37, 91), (64, 128), (180, 520), (37, 91), (64, 128)]


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import kernels
    assert torch.cuda.is_available()
    return kernels


@pytest.fixture(scope="module")
def frames():
    return [(i,) + W.frame(40 + i, h, w) for i, (h, w) in enumerate(FRAME_SHAPES)]


@pytest.fixture(scope="module")
def store(K, frames):
    rs = DS.ResidentSet.from_frames(frames, "cuda")
    for i, img, lbl in frames:                                         # (what lies in the store is what was put there)
        assert np.array_equal(rs.image(i).cpu().numpy(), img) and np.array_equal(rs.label(i).cpu().numpy(), lbl)
    return rs


TABLE = np.zeros(256, np.uint8)
TABLE[[3, 7, 12, 18]] = 1


def _plan(window, out, flip=False):
    """the plan that reads `window` = (y1, y2, x1, x2) of its frame (flipped: columns right to left) and resamples it to `out`"""
    y1, y2, x1, x2 = window
    plan = DA.plan_sample(A.resize(*out), (y2 - y1, x2 - x1))
    g = plan[0]["ops"][0][1]
    assert g.src == (0, y2 - y1, 0, x2 - x1) and g.out == tuple(out)
    g.src, g.flip = (y1, y2, x1, x2), flip
    return plan


def _store_sample(store, plan, index, paste_index=None):
    paste = None if paste_index is None else (paste_index, store.frames[paste_index].tolist(), TABLE)
    return DA.pack_store_sample(plan, index, store.frames[index].tolist(), paste)


def _bytes_sample(frames, plan, index, paste_index=None):
    y1, y2, x1, x2 = DA.plan_window(plan)
    paste = None if paste_index is None else (frames[paste_index][1][y1:y2, x1:x2], frames[paste_index][2][y1:y2, x1:x2], TABLE)
    return DA.pack_sample(plan, frames[index][1][y1:y2, x1:x2], frames[index][2][y1:y2, x1:x2], paste)


def _run(K, samples, store=None):
    t = DA.build_batch_tables(samples)
    n_views, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    if store is None:
        views, lbl = K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, "cuda")
    else:
        views, lbl = K.aug_batch_store_u8(t["blob"], t["tabs"], t["recs"], t["ops"], oh, ow, max_ch, "cuda", store)
    torch.cuda.synchronize()
    assert len(views) == n_views
    return [v.cpu().numpy() for v in views], lbl.cpu().numpy(), t


def _cases(out):
    """(what, window, frame, paste source | None, flip)"""
    oh, ow = out
    return [
        ("strictly inside its frame", (5, 30, 7, 80), 0, None, False),
        ("ends on the frame's last row and column", (9, 37, 20, 91), 0, None, False),
        ("the last frame of the store, to its last pixel", (30, 64, 50, 128), 4, None, False),
        ("flipped", (3, 60, 11, 120), 1, None, True),
        ("with a paste source and table", (2, 35, 4, 88), 3, 0, False),
        ("flipped, pasted, in the last frame", (10, 64, 1, 127), 4, 1, True),
        ("an upscale", (20, 20 + oh // 2, 40, 40 + ow // 2), 1, None, False),
        ("a 33-tap downscale", (2, 178, 5, 517), 2, None, False),
    ]


@pytest.mark.parametrize("out", [(16, 32), (11, 33)], ids=["words", "bytes"])
def test_geometry_from_the_store(K, frames, store, out):
    """one batch of store records -> the numpy executor on the full frames and aug_batch_u8 on the windows as bytes"""
    cases = _cases(out)
    plans = [_plan(win, out, flip) for _, win, _, _, flip in cases]
    assert plans[-1][0]["ops"][0][1].hk.shape[1] == 33 and plans[-2][0]["ops"][0][1].hk.shape[1] == 3
    assert (out[1] * 3) % 4 == (0 if out == (16, 32) else 3)
    got_v, got_l, t = _run(K, [_store_sample(store, p, i, pi) for p, (_, _, i, pi, _) in zip(plans, cases)], store)
    recs = t["recs"].numpy()
    assert (recs[:, DA.R_KIND] == DA.KIND_STORE).all() and (recs[:, DA.R_STRIDE] > recs[:, DA.R_CW]).all()
    assert t["blob"].numel() == 2 * 256                                   # nothing but the two paste tables travels
    ref_v, ref_l, _ = _run(K, [_bytes_sample(frames, p, i, pi) for p, (_, _, i, pi, _) in zip(plans, cases)])
    for b, (what, _, i, pi, _) in enumerate(cases):
        paste = None if pi is None else (frames[pi][1], frames[pi][2], TABLE)
        want_i, want_l = DA.execute_plan_host(plans[b], frames[i][1], frames[i][2], paste=paste)
        for name, ref_img, ref_lbl in (("numpy executor", want_i[0], want_l[0]), ("bytes path", ref_v[0][b], ref_l[b])):
            d = int((got_v[0][b] != ref_img).sum())
            assert d == 0, "%s vs %s: %d differing image bytes" % (what, name, d)
            assert int((got_l[b] != ref_lbl).sum()) == 0, "%s vs %s: label" % (what, name)
    # (the inputs do what they claim: pasting and flipping change bytes)
    plain = DA.execute_plan_host(plans[4], frames[3][1], frames[3][2])[0][0]
    assert int((plain != got_v[0][4]).sum()) > 0


def test_kinds_0_1_2_in_one_batch(K, frames, store):
    out = (16, 32)
    p2, p0, p1 = _plan((5, 30, 7, 80), out), _plan((3, 60, 11, 120), out, True), _plan((9, 37, 20, 91), out)
    fin_i, fin_l = DA.execute_plan_host(p1, frames[3][1], frames[3][2])
    samples = [_store_sample(store, p2, 0, 3), _bytes_sample(frames, p0, 1, 4),
               DA.pack_finished(torch.from_numpy(fin_i[0]), torch.from_numpy(fin_l[0])), _store_sample(store, p0, 4)]
    got_v, got_l, t = _run(K, samples, store)
    assert t["recs"][:, DA.R_KIND].tolist() == [2, 0, 1, 2]
    for b, s in enumerate(samples):
        alone_v, alone_l, _ = _run(K, [s], store if "store" in s["raw"] else None)
        assert np.array_equal(got_v[0][b], alone_v[0][0]) and np.array_equal(got_l[b], alone_l[0]), b
    assert np.array_equal(got_v[0][2], fin_i[0]) and np.array_equal(got_l[2], fin_l[0])


def test_the_entry_without_a_store_refuses_kind_2(K, frames, store):
    t = DA.build_batch_tables([_store_sample(store, _plan((5, 30, 7, 80), (16, 32)), 0)])
    with pytest.raises(ValueError, match="no store"):
        K.aug_batch_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 16, 32, int(t["meta"][3]), "cuda")
    bad = t["recs"].clone()
    bad[0, DA.R_STRIDE] = 72
    with pytest.raises(ValueError):
        K.aug_batch_store_u8(t["blob"], t["tabs"], bad, t["ops"], 16, 32, int(t["meta"][3]), "cuda", store)


@pytest.mark.parametrize("shape", [(37, 91), (64, 128)], ids=lambda s: "%dx%d" % s)
def test_normalize_gather_is_normalize_of_the_stacked_frames(K, shape):
    """three frames at non-adjacent offsets (other frames, of other bytes, between them)"""
    from hiast_amd.sseg.datasets.utils import MEAN, STD
    h, w = shape
    other = (64, 128) if shape == (37, 91) else (37, 91)
    shapes = [shape, other, shape, other, other, shape]
    fr = [(i,) + W.frame(70 + i, *s) for i, s in enumerate(shapes)]
    rs = DS.ResidentSet.from_frames(fr, "cuda")
    pick = [5, 0, 2]
    offs = torch.from_numpy(rs.frames[pick, 0].copy())
    assert int(np.diff(np.sort(offs.numpy())).min()) > DS.frame_bytes(h, w) and offs.tolist() != sorted(offs.tolist())
    want = K.normalize_u8(torch.from_numpy(np.stack([fr[i][1] for i in pick])).cuda(), MEAN, STD)
    for o in (offs, offs.cuda()):
        got = K.normalize_gather_u8(rs.buffer, o, h, w, MEAN, STD)
        torch.cuda.synchronize()
        assert got.shape == want.shape == (3, 3, h, w) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    for bad in (torch.tensor([-1]), torch.tensor([rs.buffer.numel() - h * w * 3 + 1])):
        with pytest.raises(ValueError):
            K.normalize_gather_u8(rs.buffer, bad, h, w, MEAN, STD)


# ------------------------------------------------------------------------------------------------- dataset to batch
N, N_VAL = 8, 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """8 target frames and 3 validation frames of 64 x 128 (one size: a batch's copy_paste_mask is one tensor)"""
    from hiast_amd.utils.registry.registries import MODEL
    root = str(tmp_path_factory.mktemp("device_store"))
    cfg = W.make_world(root, [(64, 128)] * N, [(64, 128)] * N_VAL)
    torch.manual_seed(31)
    ck = os.path.join(root, "init.pth")
    torch.save(MODEL["SelfTrainingSegmentor"](cfg).state_dict(), ck)
    cfg.train.resume_from = ck
    cfg.train.amp_dtype = "bf16"
    cfg.trainer = "ConsistencySelfTrainingTrainer"
    cfg.dataset.target.aug_type = ["MS", "CCA"]
    cfg.cst_training.is_enabled = True
    cfg.cst_training.cst_loss.weight = 0.5
    cfg.train.gpu_num, cfg.train.batch_size, cfg.train.total_iter = 1, 2, 1
    cfg.train.iter_report = cfg.train.iter_val = 10 ** 6
    cfg.train.lr = 3e-6
    cfg.dataset.device_aug = True
    cfg.dataset.device_aug_level = 2            # (no 'CCA' sample falls back: every sample of the trainer's batch is a plan)
    cfg.work_dir = os.path.join(root, "work")
    return cfg


def _items(ds, table, seed):
    ds.__dict__.pop("store_table", None)
    if table is not None:
        ds.store_table = table
    W.seed_all(seed)
    return [ds[i] for i in range(len(ds))]


def _assemble(items, rs):
    from hiast_amd.sseg.datasets import utils as du
    batch = DA.collate(items)
    imgs, lbls = du.assemble_device_batch(batch, torch.device("cuda"), rs)
    torch.cuda.synchronize()
    return batch, (imgs if isinstance(imgs, list) else [imgs]), (lbls if isinstance(lbls, list) else [lbls])


def _same_batches(a, b):
    (batch_a, imgs_a, lbls_a), (batch_b, imgs_b, lbls_b) = a, b
    assert len(imgs_a) == len(imgs_b) and batch_a["image_paths"] == batch_b["image_paths"]
    for x, y in zip(imgs_a, imgs_b):
        assert x.dtype == torch.float32 and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(lbls_a, lbls_b):
        assert x.dtype == y.dtype == torch.uint8 and torch.equal(x, y)


@pytest.mark.parametrize("resident", [N, 5], ids=["all-resident", "some-resident"])
def test_dataset_to_device_batch_with_and_without_the_store(K, world, resident):
    """['MS', 'CCA'] + CopyPaste, level 1: store samples, bytes samples (a frame or a source that is not resident) and
    finished samples in one batch; every view, the label and copy_paste_mask against the same call without the store"""
    ds = W.target_dataset(world, ["MS", "CCA"], True, 1)
    dstore = DS.DeviceStore("cuda", resident * DS.frame_bytes(64, 128) + 100)
    rs = dstore.place(ds, 2)
    assert [rs.resident(i) for i in range(N)] == [i < resident for i in range(N)] and dstore.bytes_held() <= dstore.budget
    for seed in (5, 6):
        plain = _assemble(_items(ds, None, seed), None)
        items = _items(ds, rs.table, seed)
        kinds = ["store" if "store" in it["raw"] else "finished" if it["plan"] is None else "bytes" for it in items]
        got = _assemble(items, rs)
        _same_batches(got, plain)
        mask = got[0]["copy_paste_mask"]
        assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), plain[0]["copy_paste_mask"]), kinds
        assert bool((plain[0]["copy_paste_mask"] != 255).any())
        assert kinds.count("store") >= 2 and any(it["raw"].get("store", (0, -1))[1] >= 0 for it in items), kinds
        if resident < N:
            assert "bytes" in kinds, kinds
    with pytest.raises(ValueError, match="no store"):
        _assemble(items, None)


@pytest.mark.parametrize("level,aug_type,copy_paste", [(2, ["MS", "CCA"], True), (3, ["MS", "FDA-Target"], False)],
                         ids=["level2", "level3-fda"])
def test_colour_levels_start_from_store_records(K, world, level, aug_type, copy_paste):
    """the colour kernels are unchanged; this pins the hand-over from the geometry pass over store records to them"""
    c = world.clone()
    if level == 3:
        c.dataset.source.type = "Oxford"
    ds = W.target_dataset(c, aug_type, copy_paste, level)
    rs = DS.DeviceStore("cuda", 1 << 24).place(ds, 2)
    assert rs.all_resident()
    plain = _assemble(_items(ds, None, 7), None)
    items = _items(ds, rs.table, 7)
    got = _assemble(items, rs)
    _same_batches(got, plain)
    t = got[0]["device_aug"]
    assert int((t["recs"][:, DA.R_KIND] == DA.KIND_STORE).sum()) >= N // 2
    types = t["ops"][1, :, 4::2][t["recs"][:, DA.R_KIND] == DA.KIND_STORE]
    if level == 3:
        assert bool((types[:, 0] == DA.OP_FDA).any())
    else:
        assert bool(((types >= DA.OP_CONTRAST) & (types <= DA.OP_BLUR)).any())


def _trainer(world, gb):
    from hiast_amd.utils.registry.registries import TRAINER
    c = world.clone()
    c.dataset.device_store_gb = gb
    c.freeze()
    W.seed_all(9)
    return TRAINER[c.trainer](c, 0)


def test_one_training_iteration_is_bit_equal(K, world):
    runs = []
    for gb in (0.0, 0.01):
        tr = _trainer(world, gb)
        assert (tr.device_store is not None) == (gb > 0) and tr.t_dataset.device_aug
        seen, fetch = [], tr.next_target_batch
        tr.next_target_batch = lambda: (seen.append(fetch()), seen[-1])[1]
        W.seed_all(9)
        out = tr.train()
        if not getattr(out, "backward_done", False):
            sum(torch.mean(v) for v in out.values()).backward()
        torch.cuda.synchronize()
        kinds = seen[0]["device_aug"]["recs"][:, DA.R_KIND].tolist()
        if gb > 0:
            assert tr.store_of("t_dataset").all_resident() and tr.store_of("_v_dataset").all_resident()
            assert hasattr(tr.t_dataset, "store_table") and kinds == [DA.KIND_STORE] * 2, kinds
        else:
            assert not hasattr(tr.t_dataset, "store_table") and DA.KIND_STORE not in kinds
        named = [(n, p.grad) for n, p in tr.model.module.named_parameters() if p.grad is not None]
        assert len(named) > 50
        runs.append(({k: v.detach().float().cpu().clone() for k, v in out.items()},
                     {n: g.detach().float().cpu().clone() for n, g in named[::max(1, len(named) // 12)]}))
        tr.t_iter = tr.t_loader = None
        del tr
    (l0, g0), (l1, g1) = runs
    assert set(l0) == set(l1) and len(l0) >= 3 and sorted(g0) == sorted(g1)
    for k in l0:
        print(k, float(l0[k]), float(l1[k]))
        assert torch.isfinite(l0[k]).all() and torch.equal(l0[k].view(torch.int32), l1[k].view(torch.int32)), k
    for n in g0:
        assert float(g0[n].abs().max()) > 0 and torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), n


class _Raises:
    def __iter__(self):
        raise AssertionError("validation iterated over the loader")


def _counts(tr, model):
    """the intersection / union integers of get_validate_result (it returns their quotient): read where they are summed"""
    from hiast_amd.utils import metrics
    got, orig = [], metrics.intersection_union_counts

    def spy(pred, lbl, C):
        i, u = orig(pred, lbl, C)
        got.append((i.clone(), u.clone()))
        return i, u
    metrics.intersection_union_counts = spy
    try:
        iou, miou = tr.get_validate_result(model)
    finally:
        metrics.intersection_union_counts = orig
    torch.cuda.synchronize()
    return torch.stack([i for i, _ in got]).sum(0).cpu(), torch.stack([u for _, u in got]).sum(0).cpu(), len(got), iou, miou


def test_validation_reads_the_store(K, world, tmp_path):
    tr = _trainer(world, 0.01)
    rs = tr.store_of("_v_dataset")
    assert rs is not None and rs.all_resident() and tr.v_resident is not None
    assert [idx for idx, _, _ in tr.v_resident[1]] == [[0, 1], [2]]                 # the loader's order, ragged last batch
    loader = tr.v_loader
    results = {}
    for model, name in ((tr.model, "student"), (tr.ema_model, "ema")):
        tr.v_loader = _Raises()
        inter, union, n, iou, miou = _counts(tr, model)                             # the store: the loader is not touched
        resident, tr.v_resident, tr.v_loader = tr.v_resident, None, loader
        inter_l, union_l, n_l, iou_l, miou_l = _counts(tr, model)                   # the loader, as without a store
        tr.v_resident = resident
        assert n == n_l == 2 and inter.dtype == torch.int64 and int(union.sum()) > 0
        assert torch.equal(inter, inter_l) and torch.equal(union, union_l), name
        assert np.array_equal(iou, iou_l) and miou == miou_l
        results[name] = (inter, union)
    # one frame of another size in a batch: the set is read through the loader as a whole
    c = W.make_world(str(tmp_path), [(64, 128)], [(64, 128), (37, 91), (64, 128)])
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    tr._v_dataset = CityscapesDataset(tr.cfg, c.dataset.val.json_path, c.dataset.val.image_dir, num_classes=19)
    tr.build_val_data_reader()
    assert tr.store_of("_v_dataset").all_resident() and tr.v_resident is None and tr.v_loader is not None
    tr.v_loader = _Raises()
    with pytest.raises(AssertionError, match="iterated over the loader"):
        tr.get_validate_result(tr.model)
    tr.t_iter = tr.t_loader = tr.v_loader = None
    del tr
