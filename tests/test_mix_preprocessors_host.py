"""PREPROCESSOR['ClassMix'] / ['CutMix'] on the host (no GPU): the two definitions against a per-pixel restatement that
replays the documented np.random draws, the draw accounting of run / run_plan / run_plan_index, the plan executor with a
rectangle against run() followed by the host transforms, CutMix's geometry, and the trainer's config check."""
import math

import numpy as np
import pytest

from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA
from hiast_amd.utils.default_config import get_default_cfg
from hiast_amd.utils.registry import register  # noqa: F401
from hiast_amd.utils.registry.registries import PREPROCESSOR, TRAINER

H, W, N = 24, 40, 8
# frame 0 is class-less, frame 1 holds one class, the others 3..5; the labels themselves hold every id below 20 and 255,
# so classes(j) is visibly not np.unique of the label
CLASSES = {0: [], 1: [5], 2: [0, 3, 7], 3: [1, 2, 8, 13], 4: [0, 4, 9, 11, 18], 5: [2, 5, 6], 6: [3, 10, 12, 17],
           7: [1, 7, 14, 15, 16]}


class World:
    """what a preprocessor asks of dataset_copy_from, in memory"""

    def __init__(self, shapes=None):
        self.frames = []
        for j in range(N):
            g = np.random.Generator(np.random.PCG64(900 + j))
            h, w = (H, W) if shapes is None else shapes[j]
            lbl = g.integers(0, 21, (h, w), dtype=np.uint8)
            lbl[lbl == 20] = 255
            self.frames.append((g.integers(0, 256, (h, w, 3), dtype=np.uint8), lbl))
        self.names = ["frame_%d.png" % j for j in range(N)]
        self.swc = {c: [self.names[j] for j in range(N) if c in CLASSES[j]] for c in range(19)}

    def __len__(self):
        return N

    def load_data(self, j):
        return self.frames[j][0].copy(), self.frames[j][1].copy(), self.names[j]

    def get_samples_with_class(self):
        return self.swc

    def get_file_to_idx(self, name):
        return self.names.index(name)


def _cfg(area=None):
    cfg = get_default_cfg()
    if area is not None:
        cfg.preprocessor.cut_mix.area_range = list(area)
    return cfg


def _pre(name, world=None, area=None):
    return PREPROCESSOR[name](_cfg(area), world or World(), None)


def _dest(seed=77, shape=(H, W)):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, shape + (3,), dtype=np.uint8), g.integers(0, 19, shape, dtype=np.uint8)


def _replay(name, world, seed, shape, area=(0.25, 0.5)):
    """the documented draw order, restated: -> (j | None, table, rect | None)"""
    np.random.seed(seed)
    j = np.random.randint(len(world))
    if name == "ClassMix":
        classes = sorted(c for c, names in world.swc.items() if world.names[j] in names)
        if not classes:
            return None, None, None
        chosen = np.random.choice(classes, size=(len(classes) + 1) // 2, replace=False)
        table = np.zeros(256, np.uint8)
        for c in chosen:
            table[c] = 1
        return j, table, None
    p = np.random.uniform(area[0], area[1])
    fh = math.exp(np.random.uniform(math.log(p), 0.0))
    fw = p / fh
    bh = min(shape[0], max(1, int(fh * shape[0] + 0.5)))
    bw = min(shape[1], max(1, int(fw * shape[1] + 0.5)))
    y0 = np.random.randint(0, shape[0] - bh + 1)
    x0 = np.random.randint(0, shape[1] - bw + 1)
    return j, np.ones(256, np.uint8), (y0, y0 + bh, x0, x0 + bw)


def _brute(world, img, lbl, j, table, rect):
    """per pixel: -> (img, lbl, mask)"""
    img, lbl = img.copy(), lbl.copy()
    mask = np.full(lbl.shape, 255, np.uint8)
    if j is None:
        return img, lbl, mask
    s_img, s_lbl = world.frames[j]
    for y in range(lbl.shape[0]):
        for x in range(lbl.shape[1]):
            inside = rect is None or (rect[0] <= y < rect[1] and rect[2] <= x < rect[3])
            if inside and table[s_lbl[y, x]]:
                img[y, x], lbl[y, x], mask[y, x] = s_img[y, x], s_lbl[y, x], s_lbl[y, x]
    return img, lbl, mask


def test_the_registry_holds_both():
    assert PREPROCESSOR["ClassMix"].__name__ == "ClassMix" and PREPROCESSOR["CutMix"].__name__ == "CutMix"
    assert sorted(PREPROCESSOR) == ["ClassMix", "CopyPaste", "CutMix"]


@pytest.mark.parametrize("name", ["ClassMix", "CutMix"])
def test_run_is_the_per_pixel_restatement(name):
    world = World()
    pre = _pre(name, world)
    img0, lbl0 = _dest()
    seen = set()
    for seed in range(40):
        j, table, rect = _replay(name, world, seed, (H, W))
        want = _brute(world, img0, lbl0, j, table, rect)
        np.random.seed(seed)
        got = pre.run(img0.copy(), lbl0.copy())
        for g, w, what in zip(got, want, ("image", "label", "mask")):
            assert g.dtype == np.uint8 and np.array_equal(g, w), (seed, what)
        seen.add(j)
        if j is not None:
            assert (got[2] != 255).any() and not np.array_equal(got[0], img0), seed
            if name == "ClassMix":
                n = len(CLASSES[j])
                assert int(table.sum()) == (n + 1) // 2 and set(np.flatnonzero(table)) <= set(CLASSES[j])
            else:       # a source 255 inside the rectangle is pasted, and stays 255 in the mask
                y0, y1, x0, x1 = rect
                assert np.array_equal(got[1][y0:y1, x0:x1], world.frames[j][1][y0:y1, x0:x1])
                assert np.array_equal(got[2][y0:y1, x0:x1], world.frames[j][1][y0:y1, x0:x1])
    assert {1, 2} <= seen and (None in seen) == (name == "ClassMix")       # class-less, one class, several


@pytest.mark.parametrize("name", ["ClassMix", "CutMix"])
def test_the_three_forms_spend_the_same_draws_and_agree(name):
    world = World()
    pre = _pre(name, world)
    img0, lbl0 = _dest()
    none_seen = 0
    for seed in range(30):
        np.random.seed(seed)
        r_img, r_lbl, r_mask = pre.run(img0.copy(), lbl0.copy())
        after_run = np.random.get_state()
        np.random.seed(seed)
        paste, mask = pre.run_plan(img0.copy(), lbl0.copy())
        after_plan = np.random.get_state()
        np.random.seed(seed)
        drawn = pre.run_plan_index((H, W))
        after_index = np.random.get_state()
        for other in (after_plan, after_index):
            assert after_run[0] == other[0] and np.array_equal(after_run[1], other[1]) and after_run[2:] == other[2:], seed
        assert np.array_equal(mask, r_mask)
        if paste is None:
            none_seen += 1
            assert drawn[0] is None and drawn[1] is None
            continue
        assert np.array_equal(paste[0], world.frames[drawn[0]][0]) and np.array_equal(paste[1], world.frames[drawn[0]][1])
        assert np.array_equal(paste[2], drawn[1]) and len(paste) == len(drawn) + 1
        assert DA.paste_rect(paste) == (None if name == "ClassMix" else tuple(drawn[2]))
        g_img, g_lbl = DA.execute_plan_host(DA.plan_sample(None, (H, W)), img0, lbl0, paste=paste)
        assert np.array_equal(g_img[0], r_img) and np.array_equal(g_lbl[0], r_lbl)
    assert (none_seen > 0) == (name == "ClassMix")          # frame 0, the class-less source: one draw, no paste


def test_a_source_of_another_shape_is_resized_as_for_copy_paste():
    from hiast_amd.sseg.datasets.preprocessor import CopyPaste
    world = World([(H, W)] * 4 + [(30, 50)] * 4)
    img0, lbl0 = _dest()
    for name in ("ClassMix", "CutMix"):
        pre, hits = _pre(name, world), 0
        for seed in range(12):
            j, table, rect = _replay(name, world, seed, (H, W))
            if j is None or j < 4:
                continue
            hits += 1
            s_img, s_lbl = CopyPaste.resize(world.frames[j][0], world.frames[j][1], (H, W))
            small = World()
            small.frames = list(world.frames)
            small.frames[j] = (s_img, s_lbl)
            want = _brute(small, img0, lbl0, j, table, rect)
            np.random.seed(seed)
            got = pre.run(img0.copy(), lbl0.copy())
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, seed)
        assert hits > 0


# ------------------------------------------------------------------------------------------------- plan + rectangle
RECT = (8, 16, 12, 28)                          # the CutMix rectangle of the window tests, frame coordinates
WINDOWS = [("contains the rectangle", (4, 20, 6, 34)), ("cuts its top", (10, 22, 6, 34)), ("cuts its bottom", (2, 13, 6, 34)),
           ("cuts its left", (4, 20, 17, 38)), ("cuts its right", (4, 20, 2, 21)), ("misses it", (16, 24, 0, 12)),
           ("lies inside it", (9, 15, 14, 26))]


def _window_plan(window, out, flip):
    y1, y2, x1, x2 = window
    plan = DA.plan_sample(A.resize(*out), (y2 - y1, x2 - x1))
    g = plan[0]["ops"][0][1]
    g.src, g.flip = (y1, y2, x1, x2), flip
    return plan


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flipped"])
@pytest.mark.parametrize("what,window", WINDOWS, ids=[w[0].replace(" ", "-") for w in WINDOWS])
def test_the_executor_selects_inside_the_rectangle(what, window, flip):
    """run()'s composite, then crop, flip and Pillow's resize == the plan executed with the paste and its rectangle"""
    world = World()
    img0, lbl0 = _dest()
    j, table = 4, np.zeros(256, np.uint8)
    table[[0, 4, 9, 255]] = 1
    comp_i, comp_l, _ = _brute(world, img0, lbl0, j, table, RECT)
    y1, y2, x1, x2 = window
    rw = DA.window_rect(RECT, window)
    assert (rw == (0, 0, 0, 0)) == (what == "misses it")
    for out in ((y2 - y1, x2 - x1), (7, 11)):
        plan = _window_plan(window, out, flip)
        c_i, c_l = comp_i[y1:y2, x1:x2], comp_l[y1:y2, x1:x2]
        if flip:
            c_i, c_l = c_i[:, ::-1], c_l[:, ::-1]
        want_i = A._resize_img(np.ascontiguousarray(c_i), *out)
        want_l = A._resize_mask(np.ascontiguousarray(c_l), *out)
        paste = world.frames[j] + (table, RECT)
        got_i, got_l = DA.execute_plan_host(plan, img0, lbl0, paste=paste)
        assert np.array_equal(got_i[0], want_i) and np.array_equal(got_l[0], want_l), (what, out)
        sliced = (paste[0][y1:y2, x1:x2], paste[1][y1:y2, x1:x2], table, RECT)
        s_i, s_l = DA.execute_plan_host(plan, img0[y1:y2, x1:x2], lbl0[y1:y2, x1:x2], paste=sliced, sliced=True)
        assert np.array_equal(s_i[0], want_i) and np.array_equal(s_l[0], want_l), (what, out)
        # the hand-over carries the rectangle in window coordinates behind the table, in a record of kind 3
        t = DA.build_batch_tables([DA.pack_sample(plan, img0[y1:y2, x1:x2], lbl0[y1:y2, x1:x2], sliced)])
        rec = t["recs"][0]
        tab = int(rec[DA.R_PTAB])
        assert int(rec[DA.R_KIND]) == DA.KIND_PLAN_RECT and t["recs"].shape[1] == DA.REC_WORDS
        assert np.array_equal(t["blob"].numpy()[tab:tab + 256], table)
        assert tuple(t["blob"].numpy()[tab + 256:tab + 272].view("<i4")) == rw


@pytest.mark.parametrize("name", ["ClassMix", "CutMix"])
def test_plan_equals_run_then_aug_with_the_same_seeds(name):
    world = World()
    pre = _pre(name, world)
    img0, lbl0 = _dest()
    aug = A.flip_crop_resize(H // 2, W // 2 + 3, (H // 3, H), 2)
    flips = set()
    for i in range(40):
        np.random.seed(500 + i)
        r_img, r_lbl, _ = pre.run(img0.copy(), lbl0.copy())
        want_i, want_l = A.aug(aug, r_img, r_lbl, i)
        np.random.seed(500 + i)
        paste, _ = pre.run_plan(img0.copy(), lbl0.copy())
        plan = DA.plan_sample(aug, (H, W), i)
        assert not DA.needs_host(plan)
        flips.add(plan[0]["ops"][0][1].flip)
        got_i, got_l = DA.execute_plan_host(plan, img0, lbl0, paste=paste)
        assert np.array_equal(got_i[0], want_i) and np.array_equal(got_l[0], want_l), i
    assert flips == {False, True}


def test_kinds_0_1_2_keep_their_bytes():
    """a paste without a rectangle is packed exactly as before: kind 0, a table of 256 bytes"""
    world = World()
    img0, lbl0 = _dest()
    table = np.zeros(256, np.uint8)
    table[[1, 2]] = 1
    plan = _window_plan((4, 20, 6, 34), (7, 11), False)
    sl = (slice(4, 20), slice(6, 34))
    t = DA.build_batch_tables([DA.pack_sample(plan, img0[sl], lbl0[sl], (world.frames[3][0][sl], world.frames[3][1][sl], table))])
    t4 = DA.build_batch_tables([DA.pack_sample(plan, img0[sl], lbl0[sl],
                                               (world.frames[3][0][sl], world.frames[3][1][sl], table, None))])
    assert int(t["recs"][0, DA.R_KIND]) == DA.KIND_PLAN and all(np.array_equal(t[k].numpy(), t4[k].numpy()) for k in t)
    end = int(t["recs"][0, DA.R_PTAB]) + 256
    assert t["blob"].numel() == end


# ------------------------------------------------------------------------------------------------- CutMix geometry
@pytest.mark.parametrize("shape", [(24, 40), (1024, 2048)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("area", [(0.25, 0.5), (0.3, 0.3), (1.0, 1.0), (0.05, 1.0)], ids=str)
def test_cut_mix_geometry(shape, area):
    """200 seeded draws: the rectangle inside the frame; its area within [lo, hi] widened by what rounding each side to the
    nearest pixel implies.  From |bh - fh h| <= 0.5 and |bw - fw w| <= 0.5 with fh fw = p:
    bh bw >= (fh h - 0.5)(fw w - 0.5) = p h w - 0.5 (fh h + fw w) + 0.25 and bh bw <= p h w + 0.5 (fh h + fw w) + 0.25,
    per draw; over all draws fh, fw <= 1 and lo <= p <= hi give the slack 0.5 (h + w) / (h w) + 0.25 / (h w).
    (max(1, .) never binds here: fh h >= lo h >= 1.2; min(h, .) only lowers a side that rounding cannot raise above h.)"""
    h, w = shape
    lo, hi = area
    pre = _pre("CutMix", area=area)
    slack = 0.5 * (h + w) / (h * w) + 0.25 / (h * w) + 1e-12
    for seed in range(200):
        np.random.seed(seed)
        j, table, (y0, y1, x0, x1) = pre.draw(shape)
        assert (j, (y0, y1, x0, x1)) == (_replay("CutMix", World(), seed, shape, area)[0], _replay("CutMix", World(), seed, shape, area)[2])
        assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w and table.all()
        np.random.seed(seed)
        np.random.randint(N)
        p = np.random.uniform(lo, hi)
        fh = math.exp(np.random.uniform(math.log(p), 0.0))
        fw = p / fh
        assert lo <= p <= hi and p - 1e-12 <= fh <= 1.0 and p - 1e-12 <= fw <= 1.0 + 1e-12
        bh, bw = y1 - y0, x1 - x0
        assert abs(bh - fh * h) <= 0.5 + 1e-9 and abs(bw - fw * w) <= 0.5 + 1e-9
        area_px = bh * bw
        assert (fh * h - 0.5) * (fw * w - 0.5) - 1e-6 <= area_px <= (fh * h + 0.5) * (fw * w + 0.5) + 1e-6
        assert lo - slack <= area_px / (h * w) <= hi + slack, (seed, area_px / (h * w))
        if area == (1.0, 1.0):
            assert (y0, y1, x0, x1) == (0, h, 0, w)


@pytest.mark.parametrize("area", [(0.0, 0.5), (0.6, 0.5), (0.5, 1.5), (-0.1, 0.2)], ids=str)
def test_cut_mix_refuses_a_bad_area_range(area):
    with pytest.raises(ValueError, match="area_range"):
        _pre("CutMix", area=area)


def test_default_config_has_the_new_key():
    assert list(get_default_cfg().preprocessor.cut_mix.area_range) == [0.25, 0.5]


@pytest.mark.parametrize("name", ["ClassMix", "CutMix", "CopyPaste"])
def test_the_consistency_trainer_accepts_the_type(name):
    cfg = get_default_cfg()
    cfg.dataset.target.pseudo_dir = "/nonexistent/pseudo_labels"
    cfg.cst_training.is_enabled = True
    cfg.dataset.target.aug_type = ["MS", "CCA"]
    cfg.preprocessor.type = name
    T = TRAINER["ConsistencySelfTrainingTrainer"]
    tr = object.__new__(T)
    tr.cfg = cfg
    tr.assert_cfg()
    cfg.preprocessor.type = "MixUp"
    with pytest.raises(AssertionError):
        tr.assert_cfg()
