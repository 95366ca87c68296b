"""cfg.dataset.device_aug_level = 3, host side (hiast_amd/sseg/datasets/device_aug.py): FDA in its sparse-DFT form.

Comparison A — device_aug.fda_u8 against augmentations.fourier_domain_adaptation: every differing byte differs by exactly
1 and lies where the float64 value before truncation (device_aug.fda_f64) is within 1e-3 of an integer; such pixels are
at most 0.5 % of the bytes (asserted first: a frame that sits on the knife edges is a bad input, not a pass).  numpy runs
the host FFT in complex64 on the float32 frame, so the host function is the noisy party at those edges.

Then the plan: plan_sample(level=3) draws what A.FDA.params draws without opening a file, leaves `random` where aug()
leaves it, flags no sample for the host (levels 1 and 2 flag every one), and execute_plan_host reproduces aug() under
comparison A; the accepted levels; the launch segments of rows that hold FDA ops."""
import random
import types

import numpy as np
import pytest

from fda_compare import comparison_a, smooth_noise

from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA

SHAPES = [(64, 96), (61, 83), (40, 72), (33, 47), (72, 40)]


@pytest.mark.parametrize("border", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fda_u8_against_the_host_fft(shape, border):
    h, w = shape
    img, tgt = smooth_noise(3 * h + border, h, w, 95.0), smooth_noise(5 * w + border, h, w, 150.0)
    beta = (border + 0.5) / min(h, w)
    assert int(np.floor(min(h, w) * beta)) == border
    host = A.fourier_domain_adaptation(img, tgt, beta)
    got = DA.fda_u8(img, tgt, border)
    assert int((got != img).sum()) > got.size // 2, "the transform moved nothing: a vacuous comparison"
    comparison_a(got, host, DA.fda_f64(img, tgt, border), "%dx%d border %d" % (h, w, border))


@pytest.mark.parametrize("border", [0, 1, 2])
def test_target_equal_to_the_image_returns_the_image(border):
    """the one deliberate difference from the host FFT, whose round-off can move a byte down by one here"""
    for h, w in SHAPES:
        img = smooth_noise(h + w, h, w, 120.0)
        assert np.array_equal(DA.fda_u8(img, img.copy(), border), img)
        host = A.fourier_domain_adaptation(img, img.copy(), (border + 0.5) / min(h, w))
        d = img.astype(np.int32) - host.astype(np.int32)
        assert d.min() >= 0 and d.max() <= 1
    flat = np.full((16, 24, 3), 77, np.uint8)
    assert np.array_equal(DA.fda_u8(flat, flat, border), flat)


def test_fda_u8_refuses_what_it_does_not_define():
    img = smooth_noise(1, 16, 16, 100.0)
    for bad in ((img, img, 3), (img, img, -1), (img, img[:8], 1), (img[:7], img[:7], 0), (img.astype(np.float32), img, 0)):
        with pytest.raises(ValueError):
            DA.fda_u8(*bad)


class CountingReader:
    def __init__(self, frames):
        self.frames, self.calls = frames, 0

    def __call__(self, path):
        self.calls += 1
        return self.frames[path]


def _fda_lists(beta_limit=0.04):
    """(['MS', 'FDA']-style list, ['FDA'] alone, the reader): 64 x 128 views, so beta < 0.04 gives borders 0, 1 and 2"""
    frames = {"ref/%d.png" % i: smooth_noise(40 + i, 50 + 7 * i, 90 + 5 * i, 150.0 + 10 * i) for i in range(4)}
    rd = CountingReader(frames)
    fda = A.FDA(sorted(frames), beta_limit=beta_limit, read_fn=rd, p=1.0)
    ms = A.flip_crop_resize(64, 128, (40, 90), 2)
    return [ms, fda], fda, rd


@pytest.mark.parametrize("which", ["MS+FDA", "FDA"])
def test_level3_plan_reproduces_aug_without_reading(which):
    """200 indices: no file read while planning, `random` left as aug() leaves it, no sample flagged at level 3 and every
    one at levels 1 and 2; the plan executed in numpy against aug(): comparison A on the FDA view, everything else equal"""
    two, alone, rd = _fda_lists()
    aug_fun = two if which == "MS+FDA" else alone
    shape = (100, 200) if which == "MS+FDA" else (64, 128)
    img, lbl = smooth_noise(9, *shape, 95.0), (smooth_noise(10, *shape, 9.0)[..., 0] % 19).astype(np.uint8)
    borders = set()
    for i in range(200):
        want_i, want_l = A.aug(aug_fun, img.copy(), lbl.copy(), i)
        state = random.getstate()
        before = rd.calls
        plan = DA.plan_sample(aug_fun, shape, i, level=3)
        assert rd.calls == before, "planning read a reference image"
        assert random.getstate() == state, i
        assert not DA.needs_host(plan), i
        for level in (1, 2):
            assert DA.needs_host(DA.plan_sample(aug_fun, shape, i, level=level)), (i, level)
        assert rd.calls == before
        op = plan[-1]["ops"][-1]
        assert op[0] == "fda" and op[1] in rd.frames and 0 <= op[2] <= 2 and len(op) == 3
        borders.add(op[2])
        if i % 10:
            continue
        got_i, got_l = DA.execute_plan_host(plan, img, lbl)
        if which == "FDA":
            want_i, want_l = [want_i], [want_l]
        assert len(got_i) == len(want_i)
        for a, b in zip(got_l, want_l):
            assert np.array_equal(a, b), i
        for a, b in zip(got_i[:-1], want_i[:-1]):
            assert np.array_equal(a, b), i
        pre = got_i[-2] if len(got_i) > 1 else img
        tgt = DA.fda_target(op[1], pre.shape, rd)
        comparison_a(got_i[-1], want_i[-1], DA.fda_f64(pre, tgt, op[2]), "%s index %d" % (which, i))
    assert borders == {0, 1, 2}, borders


def test_what_still_falls_back_at_level_3():
    """border > 2 (a user-built FDA with a large beta_limit), a view with a side below 8, and geometry after the FDA"""
    two, fda, rd = _fda_lists(beta_limit=(0.05, 0.1))                 # floor(64 * beta) >= 3
    assert all(DA.needs_host(DA.plan_sample(two, (100, 200), s, level=3)) for s in range(20))
    ok = A.FDA(sorted(rd.frames), beta_limit=0.001, read_fn=rd, p=1.0)
    ms = A.flip_crop_resize(64, 128, (40, 90), 2)
    assert not any(DA.needs_host(DA.plan_sample([ms, ok], (100, 200), s, level=3)) for s in range(20))
    assert all(DA.needs_host(DA.plan_sample([ok, ms], (100, 200), s, level=3)) for s in range(20))
    assert all(DA.needs_host(DA.plan_sample([A.resize(7, 64), ok], (100, 200), s, level=3)) for s in range(5))
    assert not any(DA.needs_host(DA.plan_sample([A.resize(8, 64), ok], (100, 200), s, level=3)) for s in range(5))
    assert rd.calls == 0
    # the draws are those of aug() whether the FDA is planned or falls back
    for aug_fun in (two, [ok, ms]):
        A.aug(aug_fun, smooth_noise(1, 100, 200, 90.0), np.zeros((100, 200), np.uint8), 5)
        state = random.getstate()
        DA.plan_sample(aug_fun, (100, 200), 5, level=3)
        assert random.getstate() == state
    assert DA.HOST_ONLY == (A.ColorJitter, A.GaussianBlur, A.FDA)
    # params() returns what it returned: beta, then the path, then the read and the resize
    random.seed(3)
    beta, path = random.uniform(0, 0.001), random.choice(ok.refs)
    random.seed(3)
    p = ok.params(np.zeros((20, 30, 3), np.uint8))
    assert sorted(p) == ["beta", "target"] and p["beta"] == beta
    assert np.array_equal(p["target"], A._resize_img(rd.frames[path], 20, 30))


def test_fda_ops_count_towards_max_ops_and_pack_their_targets():
    _, fda, rd = _fda_lists()
    img, lbl = smooth_noise(2, 64, 128, 100.0), np.zeros((64, 128), np.uint8)
    plan = DA.plan_sample([fda, fda, fda], (64, 128), 1, level=3)
    assert [len(v["ops"]) for v in plan] == [2, 1, 1] and not DA.needs_host(plan)
    item = DA.pack_sample(plan, img, lbl)
    assert rd.calls == 3 and len(item["raw"]["fda"]) == 3
    t = DA.build_batch_tables([item])
    blob, ops = t["blob"].numpy(), t["ops"].numpy()
    for k, v in enumerate(plan):
        op = v["ops"][-1]
        assert int(ops[k, 0, 2]) == 1 and int(ops[k, 0, 4]) == DA.OP_FDA == 8
        par = int(ops[k, 0, 5])
        off, border = par & ((1 << DA.FDA_BORDER_SHIFT) - 1), par >> DA.FDA_BORDER_SHIFT
        assert border == op[2] and off % 16 == 0
        want = DA.fda_target(op[1], (64, 128), rd)
        assert np.array_equal(blob[off:off + want.size].reshape(want.shape), want)
    many = DA.plan_sample(A.Compose([fda] * (DA.MAX_OPS + 1)), (64, 128), 1, level=3)
    assert DA.needs_host(many)
    assert not DA.needs_host(DA.plan_sample(A.Compose([fda] * DA.MAX_OPS), (64, 128), 1, level=3))


def test_fda_rows_are_bounds_checked_on_the_host():
    from hiast_amd import kernels as K
    _, fda, rd = _fda_lists()
    img, lbl = smooth_noise(2, 64, 128, 100.0), np.zeros((64, 128), np.uint8)
    plan = DA.plan_sample(fda, (64, 128), 1, level=3)
    t = DA.build_batch_tables([DA.pack_sample(plan, img, lbl)])
    blob_n, tabs, recs, ops = t["blob"].numel(), t["tabs"].numpy(), t["recs"].numpy(), t["ops"].numpy()
    K._aug_check_tables(blob_n, tabs, recs, ops, 64, 128, 64)
    off = int(ops[0, 0, 5]) & ((1 << 40) - 1)
    for par in (off | (3 << 40), off | (-1 << 40), (blob_n - 64 * 128 * 3 + 16) | (1 << 40), (off + 2) | (1 << 40), blob_n << 1):
        bad = ops.copy()
        bad[0, 0, 5] = par
        with pytest.raises(ValueError):
            K._aug_check_tables(blob_n, tabs, recs, bad, 64, 128, 64)
    with pytest.raises(ValueError):
        item = DA.pack_sample(plan, img, lbl)
        item["raw"]["fda"][0] = item["raw"]["fda"][0][:32]
        DA.build_batch_tables([item])


@pytest.mark.parametrize("level,ok", [(0, False), (1, True), (2, True), (3, True), (4, False)])
def test_accepted_levels(level, ok, monkeypatch):
    """dataset.device_aug_level: 3 is accepted, 0 and 4 are rejected; HIAST_DEVICE_AUG=3 selects it"""
    from torch.utils.data import Dataset
    from hiast_amd.utils.default_config import get_default_cfg
    from hiast_amd.workflows.trainer.base_trainer import BaseTrainer

    class Empty(Dataset):
        def __len__(self):
            return 4

    cfg = get_default_cfg()
    assert cfg.dataset.device_aug_level == 1 and cfg.dataset.device_aug is False
    cfg.dataset.num_workers = 0
    cfg.dataset.device_aug = True
    cfg.dataset.device_aug_level = level
    me = types.SimpleNamespace(cfg=cfg, world=1, gpu_index=0)
    monkeypatch.delenv("HIAST_DEVICE_AUG", raising=False)
    monkeypatch.delenv("HIAST_HOST_TRANSFORM", raising=False)
    ds = Empty()
    if not ok:
        with pytest.raises(ValueError):
            BaseTrainer._loader(me, ds, 2, True, True)
        return
    BaseTrainer._loader(me, ds, 2, True, True)
    assert ds.device_aug is True and ds.device_aug_level == level
    if level == 1:
        monkeypatch.setenv("HIAST_DEVICE_AUG", "3")
        BaseTrainer._loader(me, ds, 2, True, True)
        assert ds.device_aug is True and ds.device_aug_level == 3
        monkeypatch.setenv("HIAST_DEVICE_AUG", "4")
        cfg.dataset.device_aug = False
        BaseTrainer._loader(me, ds, 2, True, True)
        assert ds.device_aug is False


def test_segments_close_at_an_fda_as_at_a_blur():
    """an FDA between pointwise ops, an FDA after an Equalize, two FDAs; a row without an FDA is cut as before"""
    from hiast_amd import kernels as K
    E, C, S, B, L, F = DA.OP_EQUALIZE, DA.OP_CONTRAST, DA.OP_SAT, DA.OP_BLUR, DA.OP_LUT, DA.OP_FDA
    rows = np.zeros((5, DA.OPS_WORDS), np.int64)
    lists = [[L, F, S], [E, F], [F, F], [L, C, S, E, B], [C, F, B, E]]
    for b, ts in enumerate(lists):
        rows[b, 2] = len(ts)
        rows[b, 4:4 + 2 * len(ts):2] = ts
    segs = K._aug_segments(rows)
    assert segs[:, 0].tolist() == [[0, 1, -1, 1], [2, 3, -1, -1], [3, 3, -1, -1]]
    assert segs[:, 1].tolist() == [[0, 1, 0, 1], [2, 2, -1, -1], [2, 2, -1, -1]]
    assert segs[:, 2].tolist() == [[0, 0, -1, 0], [1, 1, -1, 1], [2, 2, -1, -1]]
    assert segs[:, 3].tolist() == [[0, 3, 1, -1], [3, 4, 3, 4], [5, 5, -1, -1]]
    assert segs[:, 4].tolist() == [[0, 1, 0, 1], [2, 2, -1, 2], [3, 4, 3, -1]]
    alone = K._aug_segments(rows[3:4])                                 # the row without an FDA, on its own: today's cut
    assert alone[:, 0].tolist() == [[0, 3, 1, -1], [3, 4, 3, 4]]


def test_gtav_dataset_hands_fda_samples_over_as_plans(tmp_path):
    """['MS', 'FDA-Target'] on a source dataset: a plan + the resized reference image at level 3, a finished sample at
    level 2 — with the same draws either way"""
    from hiast_amd.tools import synth_data
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.sseg.datasets.loader.gtav_dataset import GTAVDataset
    c = synth_data.synthetic_cfg(str(tmp_path), n_train=2, n_val=2, h=200, w=400, upscale=4)
    ds = GTAVDataset(c, c.dataset.val.json_path, c.dataset.val.image_dir, aug_type=["MS", "FDA-Target"])      # (other frames)
    ds.device_transform = ds.device_aug = True
    ds.device_aug_level = 3
    item = ds[1]
    state = random.getstate()
    assert item["plan"] is not None and [o[0] for o in item["plan"][1]["ops"]] == ["fda"]
    assert tuple(item["raw"]["fda"][0].shape) == (512, 1024, 3) and item["plan"][1]["ops"][0][2] == 0
    t = DA.build_batch_tables([item])
    assert int(t["recs"][0, DA.R_KIND]) == DA.KIND_PLAN
    ds.device_aug_level = 2
    done = ds[1]
    assert done["plan"] is None and random.getstate() == state
    img, lbl, _ = ds.load_data(1)
    y1, y2, x1, x2 = DA.plan_window(item["plan"])
    got_i, got_l = DA.execute_plan_host(item["plan"], item["raw"]["img"].numpy(), item["raw"]["lbl"].numpy(), sliced=True)
    assert np.array_equal(got_i[0], done["raw"]["views"][0].numpy()) and np.array_equal(got_l[0], done["raw"]["lbl"].numpy())
    f = DA.fda_f64(got_i[0], item["raw"]["fda"][0].numpy(), 0)
    comparison_a(got_i[1], done["raw"]["views"][1].numpy(), f, "GTAV ['MS', 'FDA-Target']")
