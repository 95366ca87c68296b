"""Shared by tests/test_device_store_plan.py and tests/test_gpu_device_store.py: a seeded synthetic Cityscapes-like target
set on disk whose frames may differ in size, with hand-written generator artefacts (pseudo-labels = the labels, every class
'hard' in turn), as tests/test_gpu_device_aug.py::world builds for one size; and small helpers around the device store."""
import json
import os
import random

import numpy as np
import torch


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def frame(seed, h, w):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 20, (h, w), dtype=np.uint8)


def make_world(root, shapes, val_shapes=((64, 128),), seed=1):
    """-> cfg of a target set with one frame per entry of `shapes` ((h, w) each) and a validation set of `val_shapes`,
    CopyPaste artefacts beside the pseudo-labels"""
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.tools import synth_data
    cfg = synth_data.synthetic_cfg(root, n_train=len(shapes), n_val=len(val_shapes), h=64, w=128, seed=seed)
    for split, key, shp in (("train", "target", shapes), ("val", "val", val_shapes)):
        node = getattr(cfg.dataset, key)
        for i, (e, (h, w)) in enumerate(zip(json.load(open(node.json_path)), shp)):
            if (h, w) != (64, 128):                              # rewrite this frame at its own size
                img, lbl = synth_data.make_sample(seed * 7919 + 31 * i + len(split), h, w)
                Image.fromarray(img).save(os.path.join(node.image_dir, e["image_name"]))
                Image.fromarray(lbl, mode="L").save(os.path.join(node.image_dir, e["mask_name"]))
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
    cfg.dataset.target.pseudo_dir = pdir
    cfg.preprocessor.type = "CopyPaste"
    return cfg


def target_dataset(cfg, aug_type, copy_paste, level=1):
    """the target set as the trainer's loader sets it up for the device-side sample path"""
    from hiast_amd.sseg.datasets.preprocessor import CopyPaste
    from hiast_amd.sseg.datasets.loader.cityscapes_dataset import CityscapesDataset
    t = cfg.dataset.target
    ds = CityscapesDataset(cfg, t.json_path, t.image_dir, pseudo_dir=t.pseudo_dir, aug_type=aug_type)
    if copy_paste:
        ds.set_preprocessor(CopyPaste(cfg, ds, np.load(os.path.join(t.pseudo_dir, "..", "class_mean_probabilities.npy"))))
    ds.device_transform = ds.device_aug = True
    ds.device_aug_level = level
    return ds


def same(a, b):
    """deep equality of plans / samples: dicts, sequences, numpy arrays, tensors, Geometry objects, scalars"""
    from hiast_amd.sseg.datasets.device_aug import Geometry
    if isinstance(a, Geometry):
        return isinstance(b, Geometry) and same(vars(a), vars(b))
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if callable(a) and callable(b):          # (an FDA op's reader: the same function of the same transform)
        return True
    return type(a) is type(b) and a == b


def arrays_of(x):
    """every numpy array / tensor inside a sample, as (path, number of bytes)"""
    out = []

    def walk(v, path):
        from hiast_amd.sseg.datasets.device_aug import Geometry
        if isinstance(v, torch.Tensor):
            out.append((path, v.numel() * v.element_size()))
        elif isinstance(v, np.ndarray):
            out.append((path, v.nbytes))
        elif isinstance(v, dict):
            for k, w in v.items():
                walk(w, path + (k,))
        elif isinstance(v, (list, tuple)):
            for i, w in enumerate(v):
                walk(w, path + (i,))
        elif isinstance(v, Geometry):
            return                              # the plan's tables travel in every form of the sample
    walk(x, ())
    return out
