"""PREPROCESSOR['ClassMix'] / ['CutMix'] on the device: hiast_aug_geometry_mix_u8 (record kinds 0..4, a select on load that
knows a rectangle) and hiast_aug_paste_mask_u8 (the copy_paste_mask of a batch in one launch) against the numpy executor,
byte for byte, in guarded buffers; the refusals of the host checks; dataset -> device batch and one trainer iteration
against the worker path, bit for bit."""
import os

import numpy as np
import pytest
import torch

import device_store_world as W
import guard_bands as G
from hiast_amd.sseg.datasets import augmentations as A
from hiast_amd.sseg.datasets import device_aug as DA
from hiast_amd.sseg.datasets import device_store as DS

pytestmark = pytest.mark.gpu

BAND = 4096
# frames 0 / 1: the sample's frame and its paste source (a row stride of 45 > cw for the store kinds); 2 / 3 keep other bytes
# beside them in the store, so a read across a frame boundary changes the result
FRAME_SHAPES = [(20, 45), (20, 45), (37, 91), (37, 91)]
WINDOWS = [(3, 10, 5, 18), (2, 18, 9, 42)]                 # 7 x 13 and 16 x 33
TABLES = {"one-class": [7], "half": list(range(10)), "all-ones": list(range(256))}


def _table(name):
    t = np.zeros(256, np.uint8)
    t[TABLES[name]] = 1
    return t


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import kernels
    assert torch.cuda.is_available()
    return kernels


@pytest.fixture(scope="module")
def frames():
    out = []
    for i, (h, w) in enumerate(FRAME_SHAPES):
        img, lbl = W.frame(140 + i, h, w)
        lbl = lbl.copy()
        lbl[lbl == 19] = 255                                 # (ids 0..18 and the ignore value)
        out.append((i, img, lbl))
    return out


@pytest.fixture(scope="module")
def store(K, frames):
    return DS.ResidentSet.from_frames(frames, "cuda")


def _plan(window, out, flip):
    y1, y2, x1, x2 = window
    plan = DA.plan_sample(A.resize(*out), (y2 - y1, x2 - x1))
    g = plan[0]["ops"][0][1]
    g.src, g.flip = (y1, y2, x1, x2), flip
    return plan


def _rects(window):
    """(what, frame rectangle): window-coordinate cases moved into the frame, + one that overhangs the window on all sides"""
    y1, y2, x1, x2 = window
    ch, cw = y2 - y1, x2 - x1
    cases = [("corner-00", (0, 1, 0, 1)), ("corner-0w", (0, 1, cw - 1, cw)), ("corner-h0", (ch - 1, ch, 0, 1)),
             ("corner-hw", (ch - 1, ch, cw - 1, cw)), ("row", (2, 3, 0, cw)), ("column", (0, ch, 4, 5)),
             ("window", (0, ch, 0, cw)), ("interior", (1, ch - 2, 2, cw - 3))]
    out = [(n, (y1 + a, y1 + b, x1 + c, x1 + d)) for n, (a, b, c, d) in cases]
    return out + [("empty", (0, 1, 0, 1)), ("overhang", (0, 20, 0, 45)), ("cut-top-left", (0, y1 + 3, 0, x1 + 5))]


def _bytes_sample(frames, plan, i, pi, table, rect, poison=False):
    y1, y2, x1, x2 = DA.plan_window(plan)
    p_img, p_lbl = frames[pi][1][y1:y2, x1:x2].copy(), frames[pi][2][y1:y2, x1:x2].copy()
    if poison:                      # outside the clipped rectangle: other image bytes, and a label every table selects
        ry0, ry1, rx0, rx1 = DA.window_rect(rect, (y1, y2, x1, x2)) if rect is not None else (0, y2 - y1, 0, x2 - x1)
        keep = np.zeros(p_lbl.shape, bool)
        keep[ry0:ry1, rx0:rx1] = True
        p_img[~keep] ^= 0xFF
        p_lbl[~keep] = 7
    paste = (p_img, p_lbl, table) if rect is None else (p_img, p_lbl, table, rect)
    return DA.pack_sample(plan, frames[i][1][y1:y2, x1:x2], frames[i][2][y1:y2, x1:x2], paste)


def _store_sample(store, plan, i, pi, table, rect):
    paste = (pi, store.frames[pi].tolist(), table) + (() if rect is None else (rect,))
    return DA.pack_store_sample(plan, i, store.frames[i].tolist(), paste)


def _want(frames, plan, i, pi, table, rect):
    paste = (frames[pi][1], frames[pi][2], table) + (() if rect is None else (rect,))
    imgs, lbls = DA.execute_plan_host(plan, frames[i][1], frames[i][2], paste=paste)
    return imgs[0], lbls[0]


def _geometry(K, samples, store=None, entry="mix"):
    """the geometry entry on one batch, outputs and tmp in guarded buffers -> (img, lbl, tables)"""
    t = DA.build_batch_tables(samples)
    _, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    K._aug_check_tables(t["blob"].numel(), t["tabs"].numpy(), t["recs"].numpy(), t["ops"].numpy(), oh, ow, max_ch,
                        None if store is None else (store.buffer.numel(), store.frames), t["blob"].numpy())
    B = len(samples)
    blob_d, tabs_d, recs_d = t["blob"].cuda(), t["tabs"].cuda(), t["recs"].cuda()
    buf = None if store is None else store.buffer
    if entry != "mix":
        img, lbl = K.aug_geometry_u8(blob_d, tabs_d, recs_d, oh, ow, max_ch, buf, host=(t["recs"], t["blob"]))
        torch.cuda.synchronize()
        return img.cpu().numpy(), lbl.cpu().numpy(), t
    carved = [G.carve(s, torch.uint8, "cuda", BAND) for s in ((B, max_ch, ow, 3), (B, oh, ow, 3), (B, oh, ow))]
    K.aug_geometry_mix_u8(blob_d, tabs_d, recs_d, oh, ow, max_ch, buf, host=(t["recs"], t["blob"]),
                          out=tuple(c[0] for c in carved))
    torch.cuda.synchronize()
    for (_, h), what in zip(carved, ("tmp", "img_out", "lbl_out")):
        G.check(h, what)
    return carved[1][0].cpu().numpy(), carved[2][0].cpu().numpy(), t


def _grid(out_of):
    """every (window, rectangle, flip, table) with the output size out_of(window)"""
    return [(win, out_of(win), what, rect, flip, tn) for win in WINDOWS for what, rect in _rects(win) for flip in (False, True)
            for tn in TABLES]


@pytest.mark.parametrize("case", ["to-5x9", "to-16x33", "identity-7x13"])
def test_geometry_mix_is_the_numpy_executor(K, frames, store, case):
    """kinds 3 (bytes) and 4 (store, row stride 45 > cw) of every rectangle / flip / table in ONE launch per kind pair; the
    same launch again with the paste source poisoned outside the clipped rectangle gives the same bytes"""
    if case == "to-5x9":                        # both windows downscaled
        grid = _grid(lambda w: (5, 9))
    elif case == "to-16x33":                    # the 7 x 13 window upscaled, the 16 x 33 window through identity tables
        grid = _grid(lambda w: (16, 33))
        assert _plan(WINDOWS[1], (16, 33), False)[0]["ops"][0][1].hk.shape[1] == 1
    else:                                       # identity tables at the small window
        grid = [g for g in _grid(lambda w: (w[1] - w[0], w[3] - w[2])) if g[0] == WINDOWS[0]]
    plans = [_plan(win, out, flip) for win, out, _, _, flip, _ in grid]
    tabs = [_table(tn) for *_, tn in grid]
    rects = [g[3] for g in grid]
    want = [_want(frames, p, 0, 1, t, r) for p, t, r in zip(plans, tabs, rects)]
    plain = [DA.execute_plan_host(p, frames[0][1], frames[0][2]) for p in plans]
    assert sum(not np.array_equal(w[0], q[0][0]) for w, q in zip(want, plain)) > len(grid) // 4      # (pasting changes bytes)
    n = len(grid)
    samples = [_bytes_sample(frames, p, 0, 1, t, r) for p, t, r in zip(plans, tabs, rects)] + \
              [_store_sample(store, p, 0, 1, t, r) for p, t, r in zip(plans, tabs, rects)]
    got_i, got_l, t = _geometry(K, samples, store)
    assert t["recs"][:, DA.R_KIND].tolist() == [DA.KIND_PLAN_RECT] * n + [DA.KIND_STORE_RECT] * n
    assert (t["recs"][n:, DA.R_STRIDE] > t["recs"][n:, DA.R_CW]).all()
    for b in range(2 * n):
        w_i, w_l = want[b % n]
        assert got_i[b].shape == w_i.shape and int((got_i[b] != w_i).sum()) == 0, ("image", b, grid[b % n][2:])
        assert int((got_l[b] != w_l).sum()) == 0, ("label", b, grid[b % n][2:])
    poisoned = [_bytes_sample(frames, p, 0, 1, t, r, poison=True) for p, t, r in zip(plans, tabs, rects)]
    assert any(not torch.equal(a["raw"]["paste_lbl"], b["raw"]["paste_lbl"]) for a, b in zip(poisoned, samples))
    pois_i, pois_l, _ = _geometry(K, poisoned)                          # (no store: it may be null without kinds 2 and 4)
    assert np.array_equal(pois_i, got_i[:n]) and np.array_equal(pois_l, got_l[:n])


def test_a_store_source_poisoned_outside_the_rectangle_changes_nothing(K, frames):
    rect = (6, 12, 15, 30)
    bad = [list(f) for f in frames]
    keep = np.zeros(FRAME_SHAPES[1], bool)
    keep[rect[0]:rect[1], rect[2]:rect[3]] = True
    bad[1][1], bad[1][2] = frames[1][1].copy(), frames[1][2].copy()
    bad[1][1][~keep] ^= 0xFF
    bad[1][2][~keep] = 7
    rs = DS.ResidentSet.from_frames([tuple(f) for f in bad], "cuda")
    grid = [(win, flip, tn) for win in WINDOWS for flip in (False, True) for tn in TABLES]
    plans = [_plan(win, (5, 9), flip) for win, flip, _ in grid]
    got_i, got_l, _ = _geometry(K, [_store_sample(rs, p, 0, 1, _table(tn), rect) for p, (_, _, tn) in zip(plans, grid)], rs)
    for b, (p, (_, _, tn)) in enumerate(zip(plans, grid)):
        w_i, w_l = _want(frames, p, 0, 1, _table(tn), rect)              # the CLEAN source
        assert np.array_equal(got_i[b], w_i) and np.array_equal(got_l[b], w_l), grid[b]
    # (and the poison is live: without the rectangle it is pasted)
    whole_i, _, _ = _geometry(K, [_store_sample(rs, plans[0], 0, 1, _table("half"), None)], rs)
    assert not np.array_equal(whole_i[0], _want(frames, plans[0], 0, 1, _table("half"), None)[0])


def test_kinds_0_to_4_in_one_batch_and_kinds_0_to_2_through_both_entries(K, frames, store):
    out, tab = (5, 9), _table("half")
    p_a, p_b = _plan(WINDOWS[0], out, False), _plan(WINDOWS[1], out, True)
    fin_i, fin_l = DA.execute_plan_host(p_b, frames[2][1][:20, :45], frames[2][2][:20, :45])
    rect = (4, 9, 8, 30)
    old = [_bytes_sample(frames, p_a, 0, 1, tab, None), DA.pack_finished(torch.from_numpy(fin_i[0]), torch.from_numpy(fin_l[0])),
           _store_sample(store, p_b, 1, 0, tab, None), _store_sample(store, p_a, 2, 3, tab, None)]
    new = [_bytes_sample(frames, p_b, 0, 1, tab, rect), _store_sample(store, p_a, 1, 0, tab, rect)]
    got_i, got_l, t = _geometry(K, old + new, store)
    assert t["recs"][:, DA.R_KIND].tolist() == [0, 1, 2, 2, 3, 4]
    want = [_want(frames, p_a, 0, 1, tab, None), (fin_i[0], fin_l[0]), _want(frames, p_b, 1, 0, tab, None),
            _want(frames, p_a, 2, 3, tab, None), _want(frames, p_b, 0, 1, tab, rect), _want(frames, p_a, 1, 0, tab, rect)]
    for b, (w_i, w_l) in enumerate(want):
        assert np.array_equal(got_i[b], w_i) and np.array_equal(got_l[b], w_l), b
    mix_i, mix_l, _ = _geometry(K, old, store)
    old_i, old_l, t_old = _geometry(K, old, store, entry="store")
    assert t_old["recs"][:, DA.R_KIND].tolist() == [0, 1, 2, 2]
    assert np.array_equal(mix_i, old_i) and np.array_equal(mix_l, old_l) and np.array_equal(mix_i, got_i[:4])
    two_i, two_l, _ = _geometry(K, old[:2])
    plain_i, plain_l, _ = _geometry(K, old[:2], entry="plain")
    assert np.array_equal(two_i, plain_i) and np.array_equal(two_l, plain_l)
    # the batch wrappers route by kind: the same bytes through aug_batch_store_u8
    views, lbl = K.aug_batch_store_u8(t["blob"], t["tabs"], t["recs"], t["ops"], 5, 9, int(t["meta"][3]), "cuda", store)
    torch.cuda.synchronize()
    assert np.array_equal(views[0].cpu().numpy(), got_i) and np.array_equal(lbl.cpu().numpy(), got_l)


UNKNOWN = {"hiast_aug_geometry_u8": (2, 3, 4), "hiast_aug_geometry_store_u8": (3, 4), "hiast_aug_geometry_mix_u8": (2, 4)}


@pytest.mark.parametrize("out", [(5, 9), (8, 12)])          # the 1-byte and the 4-byte form of the vertical pass
@pytest.mark.parametrize("entry", sorted(UNKNOWN))
def test_a_record_kind_the_entry_does_not_know_is_left_alone(K, frames, store, entry, out):
    """the C entries themselves, no host check in front: one sample of a kind the entry knows beside one of every kind it does
    not (for hiast_aug_geometry_mix_u8: the store kinds, with a null store).  The unknown samples' rows of tmp, img_out and
    lbl_out keep their prefill, the known sample is the numpy executor's, the guard bands are intact.  The blob is padded so
    that every offset of an unknown record, taken for a blob offset, has a whole window and oh*ow*3 bytes behind it: a kernel
    that mistakes such a record for another kind fails by bytes, not by a fault"""
    from hiast_amd import _lib
    tab, rect, fill = _table("half"), (4, 9, 8, 30), 0xA5
    wins = [WINDOWS[0], (0, 20, 0, 45)]                                     # 7 x 13 and 20 x 45 (store row stride 45)
    plans = [_plan(wins[k % 2], out, bool(k % 2)) for k in range(4)]
    make = {0: lambda p: _bytes_sample(frames, p, 0, 1, tab, None), 2: lambda p: _store_sample(store, p, 0, 1, tab, None),
            3: lambda p: _bytes_sample(frames, p, 0, 1, tab, rect), 4: lambda p: _store_sample(store, p, 0, 1, tab, rect)}
    known = {"hiast_aug_geometry_u8": 0, "hiast_aug_geometry_store_u8": 2, "hiast_aug_geometry_mix_u8": 3}[entry]
    kinds = (known,) + UNKNOWN[entry]
    t = DA.build_batch_tables([make[k](p) for k, p in zip(kinds, plans)])
    assert t["recs"][:, DA.R_KIND].tolist() == list(kinds)
    _, oh, ow, max_ch, _ = (int(v) for v in t["meta"])
    assert (oh, ow) == out and max_ch == 20
    B = len(kinds)
    reach = int(t["recs"][1:, DA.R_IMG:DA.R_PTAB + 1].max()) + 20 * 45 * 3 + oh * ow * 3 + DA.MIX_TABLE_BYTES
    pad = (torch.arange(max(0, reach - t["blob"].numel())) % 160).to(torch.uint8)       # (never the prefill's value)
    blob_d = torch.cat([t["blob"], pad]).cuda()
    assert blob_d.data_ptr() % 4 == 0
    tabs_d, recs_d = t["tabs"].cuda(), t["recs"].cuda()
    carved = [G.carve(s, torch.uint8, "cuda", BAND) for s in ((B, max_ch, ow, 3), (B, oh, ow, 3), (B, oh, ow))]
    for c, _ in carved:
        c.fill_(fill)
    tmp, img, lbl = (c for c, _ in carved)
    stores = {"hiast_aug_geometry_u8": (), "hiast_aug_geometry_store_u8": (store.buffer.data_ptr(),),
              "hiast_aug_geometry_mix_u8": (0,)}[entry]
    rc = getattr(_lib.load(), entry)(recs_d.data_ptr(), blob_d.data_ptr(), *stores, tabs_d.data_ptr(), tmp.data_ptr(),
                                     img.data_ptr(), lbl.data_ptr(), B, max_ch, oh, ow, K._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (_, h), what in zip(carved, ("tmp", "img_out", "lbl_out")):
        G.check(h, what)
    for b in range(1, B):
        for c, what in zip((tmp, img, lbl), ("tmp", "img_out", "lbl_out")):
            assert int((c[b] != fill).sum()) == 0, (what, "written for the unknown kind", kinds[b])
    w_i, w_l = _want(frames, plans[0], 0, 1, tab, rect if known == 3 else None)
    assert np.array_equal(img[0].cpu().numpy(), w_i) and np.array_equal(lbl[0].cpu().numpy(), w_l)
    assert int((tmp[0, :7] != fill).sum()) > 0                              # (and the known sample went through tmp)


def test_refusals_launch_nothing(K, frames, store):
    from hiast_amd import _lib
    tab, rect = _table("half"), (4, 9, 8, 30)
    plan = _plan(WINDOWS[1], (5, 9), False)
    for sample, st in ((_bytes_sample(frames, plan, 0, 1, tab, rect), None), (_store_sample(store, plan, 0, 1, tab, rect), store)):
        t = DA.build_batch_tables([sample])
        kind = int(t["recs"][0, DA.R_KIND])
        assert kind == (DA.KIND_PLAN_RECT if st is None else DA.KIND_STORE_RECT)
        max_ch = int(t["meta"][3])
        dev = [t[k].cuda() for k in ("blob", "tabs", "recs")]
        free = torch.cuda.memory_allocated()
        for buf in (None, store.buffer):                      # hiast_aug_geometry_u8 and hiast_aug_geometry_store_u8
            with pytest.raises(_lib.HiastLibraryError, match="code -1"):
                K.aug_geometry_u8(*dev, 5, 9, max_ch, buf, host=(t["recs"], t["blob"]))
        assert torch.cuda.memory_allocated() == free          # refused before the outputs were allocated
        lib = _lib.load()
        chk = lambda recs, blob, mk: lib.hiast_aug_records_check(recs.data_ptr(), blob.data_ptr(), blob.numel(), 1, mk)  # noqa: E731
        assert chk(t["recs"], t["blob"], 4) == 0 and chk(t["recs"], t["blob"], 2) == -1 and chk(t["recs"], t["blob"], 1) == -1
        off = int(t["recs"][0, DA.R_PTAB])
        run = (lambda b, r=t["recs"]: K.aug_batch_u8(b, t["tabs"], r, t["ops"], 5, 9, max_ch, "cuda")) if st is None else \
            (lambda b, r=t["recs"]: K.aug_batch_store_u8(b, t["tabs"], r, t["ops"], 5, 9, max_ch, "cuda", store))
        ch, cw = WINDOWS[1][1] - WINDOWS[1][0], WINDOWS[1][3] - WINDOWS[1][2]
        for bad_rect in ((0, ch + 1, 0, cw), (0, ch, 0, cw + 1), (-1, ch, 0, cw), (5, 4, 0, cw), (0, ch, 9, 8)):
            blob = t["blob"].clone()
            blob[off + 256:off + 272] = torch.from_numpy(np.array(bad_rect, "<i4").view(np.uint8).copy())
            assert chk(t["recs"], blob, 4) == -1, bad_rect
            with pytest.raises(ValueError, match="rectangle"):
                run(blob)
        short = t["blob"][:off + 256 + 12].clone()            # a blob too short for table + 16 bytes
        assert chk(t["recs"], short, 4) == -1
        with pytest.raises(ValueError, match="paste table"):
            run(short)
        none = t["recs"].clone()                              # a rectangle kind without a paste source
        none[0, DA.R_PIMG] = -1
        assert chk(none, t["blob"], 4) == -1
        with pytest.raises(ValueError, match="without a paste source"):
            run(t["blob"], none)
        assert torch.cuda.memory_allocated() == free


# ------------------------------------------------------------------------------------------------- copy_paste_mask
MASK_H = 6


def _mask_rects(h, w):
    return [(0, 1, 0, 1), (0, 1, w - 1, w), (h - 1, h, 0, 1), (h - 1, h, w - 1, w), (2, 3, 0, w), (0, h, w // 2, w // 2 + 1),
            (0, h, 0, w), (3, 3, 0, w), (1, h - 1, w // 3, w - w // 4)]


@pytest.mark.parametrize("w", [1, 15, 16, 17, 40])
def test_paste_mask_is_the_host_mask(K, w):
    """B = 3 frames in one launch: two sources with different tables and rectangles and a -1 source; widths at which a
    frame of the output is 16-byte aligned (16, 40), is not (1, 15, 17: frames 1 and 2), and ends in a tail (all but 16)"""
    h = MASK_H
    fr = []
    for i in range(4):
        img, lbl = W.frame(300 + 10 * w + i, h, w)
        lbl = lbl.copy()
        lbl[lbl == 19] = 255
        fr.append((i, img, lbl))
    rs = DS.ResidentSet.from_frames(fr, "cuda")
    tables = [_table("half"), _table("all-ones"), _table("one-class")]
    blob = torch.from_numpy(np.concatenate(tables)).cuda()
    rects = _mask_rects(h, w)
    for k, rect in enumerate(rects):
        other = rects[(k + 3) % len(rects)]
        rows = [(int(rs.frames[3, 1]), 256 * (k % 3), *rect, 2, 0), (-1, 0, 0, 0, 0, 0, 0, 0),
                (int(rs.frames[1, 1]), 256 * ((k + 1) % 3), *other, 1, 0)]
        out, hd = G.carve((3, h, w), torch.uint8, "cuda", BAND)
        K.paste_mask_u8(rs.buffer, blob, np.array(rows, np.int64), out)
        torch.cuda.synchronize()
        G.check(hd, "copy_paste_mask")
        got = out.cpu().numpy()
        for (src, tab, y0, y1, x0, x1, f, _), si in zip(rows, (3, None, 1)):
            want = np.full((h, w), 255, np.uint8)
            if si is not None:
                box = np.zeros((h, w), bool)
                box[y0:y1, x0:x1] = True
                s = fr[si][2]
                want = np.where((tables[tab // 256][s] != 0) & box, s, 255).astype(np.uint8)
            assert np.array_equal(got[f], want), (w, rect, f)
    bads = [[(0, 0, 0, h, 0, w, 3, 0)],                                         # a frame `out` does not have
            [(0, 768 - 255, 0, h, 0, w, 0, 0)],                                 # a table that runs past the blob
            [(0, 0, 0, h + 1, 0, w, 0, 0)], [(0, 0, 2, 1, 0, w, 0, 0)],         # a rectangle outside the frame / reversed
            [(int(rs.buffer.numel()) - h * w + 1, 0, 0, h, 0, w, 0, 0)],        # a source that runs past the store
            [(0, 0, 0, h, 0, w, 1, 0), (-1, 0, 0, 0, 0, 0, 1, 0)]]              # one frame written twice
    for bad in bads:
        out, hd = G.carve((3, h, w), torch.uint8, "cuda", BAND)
        with pytest.raises(ValueError):
            K.paste_mask_u8(rs.buffer, blob, np.array(bad, np.int64), out)
        torch.cuda.synchronize()
        G.check_untouched(hd, "a refused copy_paste_mask")


# ------------------------------------------------------------------------------------------------- dataset to batch
N, N_VAL = 8, 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from hiast_amd.utils.registry.registries import MODEL
    root = str(tmp_path_factory.mktemp("mix_preprocessors"))
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
    cfg.dataset.device_aug_level = 2
    cfg.work_dir = os.path.join(root, "work")
    # the mixing preprocessors do not read the generator's class confidences: the trainer must build without the file
    os.remove(os.path.join(cfg.dataset.target.pseudo_dir, "..", "class_mean_probabilities.npy"))
    return cfg


def _dataset(cfg, name, level):
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    from hiast_amd.utils.registry.registries import PREPROCESSOR
    t = cfg.dataset.target
    ds = CityscapesDataset(cfg, t.json_path, t.image_dir, pseudo_dir=t.pseudo_dir, aug_type=["MS", "CCA"])
    ds.set_preprocessor(PREPROCESSOR[name](cfg, ds, None))
    ds.device_transform = True
    ds.device_aug_level = level
    return ds


def _items(ds, table, seed, device_aug=True):
    ds.__dict__.pop("store_table", None)
    ds.device_aug = device_aug
    if table is not None:
        ds.store_table = table
    W.seed_all(seed)
    return [ds[i] for i in range(len(ds))]


def _assemble(items, rs):
    from hiast_amd.sseg.datasets import utils as du
    batch = DA.collate(items)
    imgs, lbls = du.assemble_device_batch(batch, torch.device("cuda"), rs)
    torch.cuda.synchronize()
    return batch, imgs, lbls


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["ClassMix", "CutMix"])
def test_dataset_to_device_batch_is_the_worker_path(K, world, name, level):
    """['MS', 'CCA'] + the preprocessor: the worker path (host composite, host transforms) against the device path without
    a store, with every frame resident and with five of eight resident — views, label and copy_paste_mask, bit for bit"""
    from torch.utils.data import default_collate
    from hiast_amd.sseg.datasets import utils as du
    ds = _dataset(world, name, level)
    stores = [None, DS.DeviceStore("cuda", 1 << 24).place(ds, 2)]
    assert stores[1].all_resident()
    ds.__dict__.pop("store_table", None)
    part = DS.DeviceStore("cuda", 5 * DS.frame_bytes(64, 128) + 100).place(ds, 2)
    assert [part.resident(i) for i in range(N)] == [i < 5 for i in range(N)]
    stores.append(part)
    for seed in (5, 6):
        worker = default_collate(_items(ds, None, seed, device_aug=False))
        w_imgs, w_lbls = du.to_device_batch(worker["images"], worker["labels"], torch.device("cuda"))
        assert worker["copy_paste_mask"].dtype == torch.uint8 and bool((worker["copy_paste_mask"] != 255).any())
        for rs in stores:
            items = _items(ds, None if rs is None else rs.table, seed)
            batch, imgs, lbls = _assemble(items, rs)
            kinds = batch["device_aug"]["recs"][:, DA.R_KIND].tolist()
            assert len(imgs) == len(w_imgs) == 2
            for x, y in zip(imgs, w_imgs):
                assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (seed, kinds)
            for x, y in zip(lbls, w_lbls):
                assert x.dtype == y.dtype == torch.uint8 and torch.equal(x, y), (seed, kinds)
            assert torch.equal(batch["copy_paste_mask"].cpu(), worker["copy_paste_mask"]), (seed, kinds)
            rect_kinds = {DA.KIND_PLAN_RECT, DA.KIND_STORE_RECT}
            if name == "CutMix":
                assert set(kinds) <= rect_kinds | {DA.KIND_FINISHED} and set(kinds) & rect_kinds, kinds
            else:
                assert not set(kinds) & rect_kinds, kinds
            if rs is not None:
                assert (DA.KIND_STORE_RECT if name == "CutMix" else DA.KIND_STORE) in kinds, kinds
                assert batch["copy_paste_mask"].is_cuda
            if rs is part and level == 2:       # (level 2 plans every 'CCA' sample: frames 5..7 travel as bytes)
                assert (DA.KIND_PLAN_RECT if name == "CutMix" else DA.KIND_PLAN) in kinds, kinds


@pytest.mark.parametrize("name", ["ClassMix", "CutMix"])
def test_one_training_iteration_is_bit_equal_to_the_worker_path(K, world, name):
    from hiast_amd.utils.registry.registries import TRAINER
    runs = []
    for device_aug, gb in ((False, 0.0), (True, 0.01)):
        c = world.clone()
        c.preprocessor.type = name
        c.dataset.device_aug, c.dataset.device_store_gb = device_aug, gb
        c.freeze()
        W.seed_all(9)
        tr = TRAINER[c.trainer](c, 0)
        assert type(tr.preprocessor).__name__ == name and tr.class_value is None
        assert (tr.device_store is not None) == (gb > 0) and bool(getattr(tr.t_dataset, "device_aug", False)) == device_aug
        seen, fetch = [], tr.next_target_batch
        tr.next_target_batch = lambda: (seen.append(fetch()), seen[-1])[1]
        W.seed_all(9)
        out = tr.train()
        if not getattr(out, "backward_done", False):
            sum(torch.mean(v) for v in out.values()).backward()
        torch.cuda.synchronize()
        if device_aug:
            kinds = seen[0]["device_aug"]["recs"][:, DA.R_KIND].tolist()
            assert tr.store_of("t_dataset").all_resident()
            assert kinds == [DA.KIND_STORE_RECT if name == "CutMix" else DA.KIND_STORE] * 2, kinds
        else:
            assert "device_aug" not in seen[0]
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
