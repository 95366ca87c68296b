"""BaseDataset (reference: sseg/datasets/loader/base_dataset.py:15-178): same constructor,
__getitem__ dict keys ('images', 'labels', 'image_paths'[, 'copy_paste_mask']), pseudo-label file
naming (<stem>_pseudo_label.png), samples_with_class.json handling and load-failure fallback."""
import json
import os
import os.path as osp

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from hiast_amd.sseg.datasets import augmentations, device_aug, utils


class BaseDataset(Dataset):

    def __init__(self, cfg, json_path, image_dir, pseudo_dir=None, aug_type=[], num_classes=19):
        self.cfg = cfg
        self.pseudo_dir = pseudo_dir
        self.num_classes = num_classes
        self.preprocessor = None
        self.aug_fun = utils.get_aug_fun(aug_type, self.build_aug_fun)
        self.img_path_list, self.lbl_path_list, self.city_list = utils.get_path_list(json_path, image_dir)
        assert len(self.img_path_list) == len(self.lbl_path_list), "images and labels should have the same number"
        self.file_to_idx = {p.split("/")[-1]: i for i, p in enumerate(self.img_path_list)}
        if self.pseudo_dir is not None:
            root = self.pseudo_dir.split(self.pseudo_dir.split("/")[-1])[0]     # parent of the label dir
            self.samples_with_class = self.stat_samples_with_class(root)

    def __len__(self):
        return len(self.img_path_list)

    def __getitem__(self, index):
        if self.preprocessor is not None:
            return self.get_item_with_copy_paste(index)
        return self.original_get_item(index)

    def get_file_to_idx(self, file_name):
        return self.file_to_idx[file_name]

    def get_samples_with_class(self):
        return self.samples_with_class

    def get_aug(self):
        return self.aug_fun

    def get_city_list(self):
        return self.city_list

    def stat_samples_with_class(self, data_root):
        """per class: file names sorted by pixel count, lowest 10 % dropped (base_dataset.py:61-77)"""
        with open(osp.join(data_root, "samples_with_class.json")) as f:
            raw = {int(k): v for k, v in json.load(f).items()}
        out = {}
        for c in range(self.cfg.dataset.num_classes):
            names = [fn.split("/")[-1] for fn, _ in sorted(raw.get(c, []), key=lambda it: it[1])]
            out[c] = names[round(len(names) * 0.1):]
        return out

    def _safe_load(self, index):
        try:
            return self.load_data(index), index
        except Exception as e:   # same recovery as the reference: neighbour index
            print("## {} in loading {}: {}".format(repr(e), index, self.img_path_list[index]))
            index = index - 1 if index > 0 else index + 1
            return self.load_data(index), index

    def _device_aug_on(self):
        """cfg.dataset.device_aug (set by the trainer's loader): workers draw the plan, the device executes it; only with
        device_transform, i.e. for consumers that take uint8 batches"""
        return bool(getattr(self, "device_aug", False)) and bool(getattr(self, "device_transform", False))

    def _device_aug_item(self, img, lbl, path, seed, paste):
        """the sample as plan + the bytes the plan reads (device_aug.pack_sample), or — a plan with a transform that has no
        device form — as finished uint8 views from the host code, the draws spent once either way"""
        import random
        if seed is not None:
            random.seed(seed)
        state = random.getstate()
        plan = device_aug.plan_sample(self.aug_fun, img.shape[:2], level=int(getattr(self, "device_aug_level", 1)))
        cp_mask = None
        if device_aug.needs_host(plan):
            random.setstate(state)
            if paste:
                img, lbl, cp_mask = self.preprocessor.run(img, lbl)
            img, lbl = augmentations.aug(self.aug_fun, img, lbl)
            out = device_aug.pack_finished(*utils.transform(img, lbl, raw_u8=True))
        else:
            y1, y2, x1, x2 = device_aug.plan_window(plan)
            src = None
            if paste:
                src, cp_mask = self.preprocessor.run_plan(img, lbl)
                if src is not None:
                    src = (src[0][y1:y2, x1:x2], src[1][y1:y2, x1:x2]) + tuple(src[2:])
            out = device_aug.pack_sample(plan, img[y1:y2, x1:x2], lbl[y1:y2, x1:x2], src)
        out["image_paths"] = path
        if cp_mask is not None:
            out["copy_paste_mask"] = torch.from_numpy(cp_mask)
        return out

    def _store_item(self, index, seed, paste):
        """the sample as a plan over device-resident frames (device_store.py: `store_table`, attached by the trainer's
        loader), nothing loaded, or None: the frame or the CopyPaste source is not resident, the source has another shape
        (it would need CopyPaste.resize), or the plan needs the host.  The draws are those of _device_aug_item from the same
        generators in the same order; before None is returned `random` and `np.random` are put back as they were found,
        so the caller's bytes path spends them once."""
        import random
        table = getattr(self, "store_table", None)
        if table is None or not self._device_aug_on() or not 0 <= index < len(table) or int(table[index, 0]) < 0:
            return None
        row = table[index].tolist()
        state, np_state = random.getstate(), (np.random.get_state() if paste else None)
        if seed is not None:
            random.seed(seed)
        plan = device_aug.plan_sample(self.aug_fun, (row[2], row[3]), level=int(getattr(self, "device_aug_level", 1)))
        ok, src = not device_aug.needs_host(plan), None
        if ok and paste:
            pre = self.preprocessor       # (CutMix sizes its rectangle by the frame's shape: the residency row has it)
            drawn = pre.run_plan_index((row[2], row[3])) if getattr(pre, "plan_takes_shape", False) else pre.run_plan_index()
            p_index, p_table = drawn[:2]
            if p_index is not None:
                p_row = table[p_index].tolist()
                ok = self.preprocessor.dataset_copy_from is self and p_row[0] >= 0 and p_row[2:] == row[2:]
                src = (p_index, p_row, p_table) + tuple(drawn[2:])
        if not ok:
            random.setstate(state)
            if paste:
                np.random.set_state(np_state)
            return None
        out = device_aug.pack_store_sample(plan, index, row, src)
        out["image_paths"] = self.img_path_list[index]
        if paste:
            out["copy_paste_mask"] = None       # cut from the resident source label on the device (assemble_device_batch)
        return out

    def frame_shape(self, index):
        """(H, W) of what load_data(index) returns, from the image's header alone (load_data resizes the label to the image)"""
        with Image.open(self.img_path_list[index]) as im:
            return im.size[1], im.size[0]

    def original_get_item(self, index):
        out = self._store_item(index, index, False)
        if out is not None:
            return out
        (img, lbl, path), index = self._safe_load(index)
        if self._device_aug_on():
            return self._device_aug_item(img, lbl, path, index, False)
        img, lbl = augmentations.aug(self.aug_fun, img, lbl, index)
        img, lbl = utils.transform(img, lbl, raw_u8=getattr(self, "device_transform", False))
        return {"images": img, "labels": lbl, "image_paths": path}

    def get_item_with_copy_paste(self, index):
        out = self._store_item(index, None, True)
        if out is not None:
            return out
        (img, lbl, path), index = self._safe_load(index)
        if self._device_aug_on():
            return self._device_aug_item(img, lbl, path, None, True)
        img, lbl, cp_mask = self.preprocessor.run(img, lbl)
        img, lbl = augmentations.aug(self.aug_fun, img, lbl)
        img, lbl = utils.transform(img, lbl, raw_u8=getattr(self, "device_transform", False))
        out = {"images": img, "labels": lbl, "image_paths": path}
        if cp_mask is not None:     # native-resolution map of the pasted classes (255 elsewhere); int64 as the reference,
            m = torch.from_numpy(cp_mask)           # uint8 for device_transform consumers (8x fewer bytes per sample)
            out["copy_paste_mask"] = m if getattr(self, "device_transform", False) else m.long()
        return out

    def _decoded_cache(self):
        """cfg.dataset.decoded_cache_dir (optional): decoded uint8 arrays are kept as raw files and re-read instead of
        decoding the PNG again (decoded_cache.py); created lazily, i.e. inside each DataLoader worker"""
        c = self.__dict__.get("_dcache", False)
        if c is False:
            d = getattr(self.cfg.dataset, "decoded_cache_dir", None)
            c = None
            if d:
                from hiast_amd.sseg.datasets.decoded_cache import DecodedCache
                c = DecodedCache(d, getattr(self.cfg.dataset, "decoded_cache_gb", 16.0))
            self.__dict__["_dcache"] = c
        return c

    def set_preprocessor(self, preprocessor):
        self.preprocessor = preprocessor
        print("%% use {}".format(type(preprocessor).__name__))

    def read_label(self, path):
        raise NotImplementedError

    def build_aug_fun(self, aug_type):
        raise NotImplementedError

    def load_data(self, index):
        """-> (uint8 HxWx3 image, uint8 HxW label, image path); with `pseudo_dir`, the label is the
        generator's <stem>_pseudo_label.png (base_dataset.py:158-178)"""
        img_path = self.img_path_list[index]
        cache = self._decoded_cache()
        dec_img = lambda p: np.array(Image.open(p).convert("RGB"), dtype=np.uint8)      # noqa: E731
        dec_lbl = lambda p: np.array(Image.open(p), dtype=np.uint8)                     # noqa: E731
        img = cache.load(img_path, dec_img) if cache else dec_img(img_path)
        if self.pseudo_dir is not None:
            stem = os.path.splitext(os.path.basename(img_path))[0]
            lp = os.path.join(self.pseudo_dir, stem + "_pseudo_label.png")
            lbl = cache.load(lp, dec_lbl) if cache else dec_lbl(lp)
        elif cache and self.lbl_path_list[index] is not None and os.path.exists(self.lbl_path_list[index]):
            lbl = cache.load(self.lbl_path_list[index], self.read_label,     # (the id-mapped label, as read_label returns it)
                             salt="%s/%d" % (type(self).__name__, self.num_classes))
        else:
            lbl = self.read_label(self.lbl_path_list[index])
        if lbl is None:
            lbl = np.full(img.shape[:2], 255, dtype=np.uint8)
        if lbl.shape != img.shape[:2]:
            lbl = np.asarray(Image.fromarray(lbl).resize((img.shape[1], img.shape[0]), Image.NEAREST))
        return img, lbl, img_path
