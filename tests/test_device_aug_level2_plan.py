"""cfg.dataset.device_aug_level = 2, host side (hiast_amd/sseg/datasets/device_aug.py): the numpy restatements of
ColorJitter's steps and of GaussianBlur against the host transforms they restate (Pillow's C HSV conversion, scipy's
correlate1d, augmentations.ColorJitter / _blur_separable), the level-2 plan against augmentations.aug(), the share of
samples that still fall back, and the host-side refusal of bad level-2 op rows.  Equality everywhere: bytes for uint8,
bits for float32; no case is left out of a comparison."""
import itertools
import random

import numpy as np
import pytest
from PIL import Image

from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA


def _all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope="module")
def colours():
    return _all_colours()


def _chunked(fn, img, n=16):
    return np.concatenate([fn(c) for c in np.array_split(img.reshape(-1, 3), n)]).reshape(img.shape)


def test_hsv_restatements_equal_pillow_on_all_colours(colours):
    """item 1: every RGB triple -> HSV and every HSV triple -> RGB, 0 differing bytes"""
    want = np.array(Image.fromarray(colours).convert("HSV"))
    d = int((_chunked(DA.rgb_to_hsv_u8, colours) != want).sum())
    assert d == 0, "RGB -> HSV: %d differing bytes" % d
    back = np.asarray(Image.fromarray(colours, "HSV").convert("RGB"))
    d = int((_chunked(DA.hsv_to_rgb_u8, colours) != back).sum())
    assert d == 0, "HSV -> RGB: %d differing bytes" % d


def _frame(seed, h, w):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 20, (h, w), dtype=np.uint8)


def _smooth(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([127.5 + 127.5 * np.sin(x / 37.0 + y / 91.0), 255.0 * x / max(w - 1, 1), 255.0 * (y / max(h - 1, 1)) ** 2], -1)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


KSIZES = list(range(3, 42, 2))


@pytest.mark.parametrize("shape", [(512, 1024), (63, 125)], ids=["512x1024", "63x125"])
def test_blur_restatement_equals_scipy(shape):
    """item 2: every odd ksize 3..41 on a noise and a smooth frame; each pass bit-equal to correlate1d, the bytes equal to
    _blur_separable"""
    from scipy.ndimage import correlate1d
    h, w = shape
    assert len(KSIZES) == 20 and all(k // 2 < min(shape) for k in KSIZES)
    for name, img in (("noise", _frame(31, h, w)[0]), ("smooth", _smooth(h, w))):
        for k in KSIZES:
            wts = DA.blur_weights(k, 0)
            x0 = img.astype(np.float32)
            p1 = DA.blur_pass(x0, wts, 0)
            s1 = correlate1d(x0, wts, axis=0, mode="mirror")
            assert p1.dtype == s1.dtype == np.float32 and np.array_equal(p1.view(np.uint32), s1.view(np.uint32)), (name, k, 0)
            p2 = DA.blur_pass(p1, wts, 1)
            s2 = correlate1d(s1, wts, axis=1, mode="mirror")
            assert np.array_equal(p2.view(np.uint32), s2.view(np.uint32)), (name, k, 1)
            d = int((DA.blur_u8(img, wts) != A._blur_separable(img, wts)).sum())
            assert d == 0, "%s ksize %d: %d differing bytes" % (name, k, d)


def _factors():
    rs = random.Random(2024)
    return [0.8, 1.0, 1.2] + [rs.uniform(0.8, 1.2) for _ in range(5)]


def test_saturation_and_contrast_executors_on_all_colours(colours):
    """item 3"""
    fs = _factors()
    assert len(fs) == 8
    frames = [colours, _frame(41, 97, 131)[0], _smooth(63, 125)]
    for fr in frames:                                   # the gray means the contrast table is built from are no integers
        m = float(A._gray_cv(fr).mean())
        assert m != round(m), m
    for f in fs:
        d = int((DA.saturation_u8(colours, f) != A.ColorJitter._saturation(colours, f)).sum())
        assert d == 0, "saturation %r: %d differing bytes" % (f, d)
        for fr in frames:
            d = int((DA.contrast_lut(fr, f)[fr] != A.ColorJitter._contrast(fr, f)).sum())
            assert d == 0, "contrast %r: %d differing bytes" % (f, d)


def test_colour_jitter_plan_ops_in_every_order():
    """the four steps as plan ops against ColorJitter.apply in all 24 orders, with a hue factor whose shift is 0 modulo
    256 (the HSV round trip still runs) and one that is exactly 0 (skipped)"""
    img = _frame(51, 96, 160)[0]
    cj = A.ColorJitter()
    changed = 0
    for n, order in enumerate(itertools.permutations(range(4))):
        factors = (0.83 + 0.01 * n, 1.17 - 0.01 * n, 0.9 + 0.005 * n, (0.001, 0.0, -0.137, 0.2, 1.0, -0.001)[n % 6])
        want = cj.apply(img, [], factors=factors, order=list(order))[0]
        ops = [op for op in (DA._jitter_op(i, factors[i]) for i in order) if op is not None]
        assert len(ops) == (3 if factors[3] == 0.0 else 4)
        if factors[3] in (0.001, 1.0, -0.001):
            assert ("hue", 0) in ops
        got = DA.execute_colour_host(ops, img)
        assert int((got != want).sum()) == 0, (order, factors)
    zero = DA.hue_u8(img, 0)
    assert int((zero != A.ColorJitter._hue(img, 0.001)).sum()) == 0
    changed = int((zero != img).sum())
    assert changed > 0, "a hue shift of 0 is not the identity: the plan must keep the op"


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


LEVEL2 = ("contrast", "sat", "hue", "blur")
AUGS = [["MS", "CCA"], ["PRS-64-128", "CCA"], ["PRS-64-128", "SCA"], ["MS", "SCA"]]


@pytest.mark.parametrize("aug_type", AUGS, ids=lambda a: "+".join(a))
def test_level2_plan_reproduces_aug(tmp_path, aug_type):
    """item 4: indices 0..199: no sample flagged; every view and label of the plan, executed in numpy, equals aug(), and
    `random` is left in the same state; the dataset hands every sample over as a plan"""
    ds = _dataset(tmp_path, aug_type)
    ds.device_transform = ds.device_aug = True
    ds.device_aug_level = 2
    seen = {k: 0 for k in LEVEL2}
    for i in range(200):
        img, lbl, _ = ds.load_data(i)
        want_i, want_l = A.aug(ds.aug_fun, img.copy(), lbl.copy(), i)
        state = random.getstate()
        plan = DA.plan_sample(ds.aug_fun, img.shape[:2], i, level=2)
        assert not DA.needs_host(plan), (i, aug_type)
        assert random.getstate() == state
        for v in plan:
            for op in v["ops"]:
                if op[0] in seen:
                    seen[op[0]] += 1
        got_i, got_l = DA.execute_plan_host(plan, img, lbl)
        assert len(got_i) == len(want_i) == 2
        for a, b in zip(got_i, want_i):
            assert a.shape == b.shape and int((a != b).sum()) == 0, (i, aug_type)
        for a, b in zip(got_l, want_l):
            assert int((a != b).sum()) == 0, (i, aug_type)
        if i % 8 == 0:
            item = ds[i]
            assert item["plan"] is not None and random.getstate() == state
            y1, y2, x1, x2 = DA.plan_window(item["plan"])
            assert np.array_equal(item["raw"]["img"].numpy(), img[y1:y2, x1:x2])
            s_i, s_l = DA.execute_plan_host(item["plan"], item["raw"]["img"].numpy(), item["raw"]["lbl"].numpy(), sliced=True)
            assert all(np.array_equal(a, b) for a, b in zip(s_i + s_l, want_i + want_l))
            DA.build_batch_tables([item])
    assert all(n > 0 for n in seen.values()), seen      # (a hue shift of 0: test_colour_jitter_plan_ops_in_every_order)


def _flags(aug_fun, shape, n, **kw):
    return [DA.needs_host(DA.plan_sample(aug_fun, shape, s, **kw)) for s in range(n)]


def test_level2_leaves_no_cca_or_sca_sample_to_the_host(tmp_path):
    """item 5: seeds 0..1999"""
    ms = A.flip_crop_resize(512, 1024, (341, 1000), 2)
    cca, sca = [ms, A.complex_color_aug()], [A.resize(64, 128), A.simple_color_aug()]
    two = [DA.plan_sample(cca, (1024, 2048), s, level=2) for s in range(2000)]
    assert sum(DA.needs_host(p) for p in two) == 0
    assert sum(_flags(sca, (1024, 2048), 2000, level=2)) == 0
    # level 1 (no keyword) is what it was: exactly the samples that hold a ColorJitter or a GaussianBlur fall back
    one = _flags(cca, (1024, 2048), 2000)
    assert 0.30 <= sum(one) / 2000 <= 0.42
    for s, flagged in enumerate(one):
        ops = [op[0] for v in two[s] for op in v["ops"]]
        assert flagged == any(o in ("contrast", "blur") for o in ops), s
    assert sum(_flags(sca, (1024, 2048), 2000)) / 2000 > 0.6
    assert DA.HOST_ONLY == (A.ColorJitter, A.GaussianBlur, A.FDA)
    # FDA stays on the host at either level, and so does geometry after a pixel op
    ref = tmp_path / "ref.png"
    Image.fromarray(_frame(61, 32, 64)[0]).save(ref)
    fda = A.FDA([str(ref)], beta_limit=0.001, p=1.0)
    assert all(_flags([ms, fda], (1024, 2048), 20, level=2)) and all(_flags([ms, fda], (1024, 2048), 20))
    late = [A.Compose([A.ColorJitter(p=1.0), A.HorizontalFlip(p=1.0)])]
    assert all(_flags(late, (64, 128), 20, level=2))
    # a blur whose half width reaches across the frame has no device form
    wide = A.GaussianBlur(blur_limit=(41, 41), p=1.0)
    assert all(_flags([A.resize(16, 32), wide], (64, 128), 10, level=2))
    assert not any(_flags([A.resize(21, 32), wide], (64, 128), 10, level=2))


def test_bad_level2_rows_are_refused_on_the_host():
    """item 6: an even ksize, a half width that reaches across the frame, a non-finite factor, an unknown op type"""
    from hiast_amd import kernels as K
    img, lbl = _frame(71, 48, 96)
    plan = DA.plan_sample(None, (48, 96))
    plan[0]["ops"] += [("contrast", 1.1), ("sat", 0.9), ("hue", 17), ("blur", DA.blur_weights(9, 0))]
    t = DA.build_batch_tables([DA.pack_sample(plan, img, lbl)])
    blob_n, tabs, recs, ops = t["blob"].numel(), t["tabs"].numpy(), t["recs"].numpy(), t["ops"].numpy()
    assert [int(v) for v in ops[0, 0, 4:12:2]] == [DA.OP_CONTRAST, DA.OP_SAT, DA.OP_HUE, DA.OP_BLUR]
    assert ops[0, 0, 5:9:2].copy().view(np.float64).tolist() == [1.1, 0.9] and int(ops[0, 0, 11]) >> 32 == 9
    K._aug_check_tables(blob_n, tabs, recs, ops, 48, 96, 48)
    segs = K._aug_segments(ops[0])
    assert segs.shape == (1, 1, 4) and segs[0, 0].tolist() == [0, 3, 0, 3]

    def refused(word, value, oh=48, ow=96):
        bad = ops.copy()
        bad[0, 0, word] = value
        with pytest.raises(ValueError):
            K._aug_check_tables(blob_n, tabs, recs, bad, oh, ow, 48)
    off = int(ops[0, 0, 11]) & 0xFFFFFFFF
    refused(11, off | (8 << 32))                                    # even
    refused(11, off | (1 << 32))
    refused(11, off | (43 << 32))
    refused(11, off | (9 << 32) | 4)                                # weights that are not the symmetric ones handed over
    refused(5, np.array([np.inf], np.float64).view(np.int64)[0])
    refused(7, np.array([np.nan], np.float64).view(np.int64)[0])
    refused(9, 256)
    refused(4, 8)                                                   # unknown op type
    refused(4, 0)
    small = DA.plan_sample(None, (4, 96))                           # ksize // 2 >= min(oh, ow)
    small[0]["ops"].append(("blur", DA.blur_weights(7, 0)))
    ts = DA.build_batch_tables([DA.pack_sample(small, img[:4], lbl[:4])])
    K._aug_check_tables(ts["blob"].numel(), ts["tabs"].numpy(), ts["recs"].numpy(), ts["ops"].numpy(), 4, 96, 4)
    small[0]["ops"][-1] = ("blur", DA.blur_weights(9, 0))
    ts = DA.build_batch_tables([DA.pack_sample(small, img[:4], lbl[:4])])
    with pytest.raises(ValueError):
        K._aug_check_tables(ts["blob"].numel(), ts["tabs"].numpy(), ts["recs"].numpy(), ts["ops"].numpy(), 4, 96, 4)


def test_segments_cut_at_table_ops_and_blurs():
    """the launch rounds of a view: a second table op opens a new segment, a blur closes one"""
    from hiast_amd import kernels as K
    E, C, S, H, B, L = DA.OP_EQUALIZE, DA.OP_CONTRAST, DA.OP_SAT, DA.OP_HUE, DA.OP_BLUR, DA.OP_LUT
    rows = np.zeros((4, DA.OPS_WORDS), np.int64)
    for b, types in enumerate([[L, C, S, E, B, H], [B], [], [E, C, B, B]]):
        rows[b, 2] = len(types)
        rows[b, 4:4 + 2 * len(types):2] = types
    rows[2, 0] = DA.KIND_FINISHED
    segs = K._aug_segments(rows)
    assert segs[:, 0].tolist() == [[0, 3, 1, -1], [3, 4, 3, 4], [5, 6, -1, -1]]
    assert segs[:, 1].tolist() == [[0, 0, -1, 0], [1, 1, -1, -1], [1, 1, -1, -1]]
    assert segs[:, 2].tolist() == [[0, 0, -1, -1]] * 3
    assert segs[:, 3].tolist() == [[0, 1, 0, -1], [1, 2, 1, 2], [3, 3, -1, 3]]


def _op_rows(lists, finished=()):
    rows = np.zeros((len(lists), DA.OPS_WORDS), np.int64)
    for b, types in enumerate(lists):
        rows[b, 2] = len(types)
        rows[b, 4:4 + 2 * len(types):2] = types
    rows[list(finished), 0] = DA.KIND_FINISHED
    return rows


def test_level1_rows_are_one_segment_and_a_batch_uploads_its_views_segments_once():
    """rows of level-1 ops run through the segment kernels as ONE round (0, n, index of the Equalize | -1, -1); the
    segment tensor aug_batch_u8 uploads once per batch is the views' own segments one after the other"""
    from hiast_amd import kernels as K
    E, S, B, L, G = DA.OP_EQUALIZE, DA.OP_SAT, DA.OP_BLUR, DA.OP_LUT, DA.OP_GRAY
    rows = _op_rows([[L], [G], [E], [L, E, G], [], [L, E]], finished=[5])      # (a finished row's ops are not read)
    segs = K._aug_segments(rows)
    assert segs.dtype == np.int32 and segs.shape == (1, 6, 4)
    assert segs[0].tolist() == [[0, 1, -1, -1], [0, 1, -1, -1], [0, 1, 0, -1], [0, 3, 1, -1], [0, 0, -1, -1], [0, 0, -1, -1]]
    ops = np.stack([_op_rows([[L, E, G], [L]]), _op_rows([[S, B, E], []])])
    both, cuts = K._aug_batch_segments(ops)
    assert both.dtype == np.int32 and both.shape == (3, 2, 4) and cuts == [slice(0, 1), slice(1, 3)]
    for k in range(2):
        assert np.array_equal(both[cuts[k]], K._aug_segments(ops[k])), k
    assert both[cuts[0]][:, 0].tolist() == [[0, 3, 1, -1]]
    assert both[cuts[1]][:, 0].tolist() == [[0, 1, -1, 1], [2, 3, 2, -1]]
    # no ops and nothing finished: no colour launch and nothing to upload; a finished sample: view 1 is copied in from
    # the blob by view 1's colour launch (view 0 by the geometry)
    none, cuts = K._aug_batch_segments(np.stack([_op_rows([[], []]), _op_rows([[], []])]))
    assert none.shape == (0, 2, 4) and cuts == [None, None]
    done = np.stack([_op_rows([[], []], finished=[1])] * 2)
    one, cuts = K._aug_batch_segments(done)
    assert cuts == [None, slice(0, 1)] and one.tolist() == [[[0, 0, -1, -1]] * 2]
