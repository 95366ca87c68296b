"""What validation costs inside a training run, through the trainer's own validate_all (student and EMA model): the
validation set read through the DataLoader (every frame decoded and uploaded again, twice per validation) against the
same set resident in the device store (cfg.dataset.device_store_gb).  One process, one box: the loader path
first, then the store path, each validate_all timed twice (the first call loads kernels and starts the workers).
    python tools/bench_validation.py [n_val=500] [workers=14] [batch=6] [native_h=1024] [native_w=2048] [store_gb=6]
The reference's recipe (sl_*.yaml): 8000 iterations at batch 6, validation every 400 iterations = 20 validate_all calls on
the 500 Cityscapes validation frames at val.resize_size [768, 1536]."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

LOG = os.environ.get("HIAST_LOG")        # progress also goes to this file
_print = print


def print(*a, **k):     # noqa: A001
    _print(*a, **k)
    if LOG:
        with open(LOG, "a") as f:
            _print(*a, file=f)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hiast_amd.utils.registry import register  # noqa: E402,F401
from hiast_amd.utils.registry.registries import MODEL, TRAINER  # noqa: E402
from hiast_amd.tools import synth_data  # noqa: E402

n_val = int(sys.argv[1]) if len(sys.argv) > 1 else 500
nw = int(sys.argv[2]) if len(sys.argv) > 2 else 14
bs = int(sys.argv[3]) if len(sys.argv) > 3 else 6
nh = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
nwid = int(sys.argv[5]) if len(sys.argv) > 5 else 2048
store_gb = float(sys.argv[6]) if len(sys.argv) > 6 else 6.0

root = tempfile.mkdtemp(prefix="hiast_val_")
try:
    from PIL import Image
    t0 = time.time()
    cfg = synth_data.synthetic_cfg(root, n_train=bs, n_val=n_val, h=nh, w=nwid, upscale=2, procs=min(max(nw, 1), 14))
    print("wrote %d + %d synthetic %dx%d frames in %.1fs" % (bs, n_val, nwid, nh, time.time() - t0), flush=True)
    pdir = cfg.pseudo_policy.save_dir               # generator artefacts by hand: pseudo-labels = the labels
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
    torch.manual_seed(888)
    ck = os.path.join(root, "warmup.pth")
    torch.save(MODEL["SelfTrainingSegmentor"](cfg).state_dict(), ck)
    cfg.trainer = "ConsistencySelfTrainingTrainer"
    cfg.train.resume_from = ck
    cfg.train.gpu_num, cfg.train.batch_size, cfg.train.total_iter = 1, bs, 10 ** 6
    cfg.train.iter_report = cfg.train.iter_val = 10 ** 6
    cfg.dataset.num_workers = nw
    cfg.dataset.target.pseudo_dir = pdir
    cfg.dataset.target.aug_type = ["MS", "CCA"]
    cfg.dataset.val.resize_size = [768, 1536]
    cfg.cst_training.is_enabled = True
    cfg.preprocessor.type = "CopyPaste"
    cfg.work_dir = os.path.join(root, "work")

    results = {}
    for tag, gb in (("loader", 0.0), ("device store", store_gb)):
        cfg.dataset.device_store_gb = gb
        t0 = time.time()
        tr = TRAINER[cfg.trainer](cfg, 0)
        torch.cuda.synchronize()
        built = time.time() - t0
        if gb > 0:
            rs = tr.store_of("_v_dataset")
            print("%s: trainer built in %.1f s, the fill included; %.1f MB held, %d of %d validation frames resident, "
                  "validation %s" % (tag, built, tr.device_store.bytes_held() / 1e6, int((rs.frames[:, 0] >= 0).sum()), n_val,
                                     "reads the store" if tr.v_resident is not None else "FALLS BACK to the loader"), flush=True)
        else:
            print("%s: trainer built in %.1f s" % (tag, built), flush=True)
        for rep in range(2):
            t0 = time.time()
            a = tr.get_validate_result(tr.model)
            torch.cuda.synchronize()
            t1 = time.time()
            b = tr.get_validate_result(tr.ema_model)
            torch.cuda.synchronize()
            t2 = time.time()
            tr.validate_all(rep + 1)
            torch.cuda.synchronize()
            t3 = time.time()
            print("%s, pass %d: get_validate_result student %.2f s, EMA %.2f s; validate_all (both, with the checkpoints it "
                  "writes) %.2f s = %.1f ms per frame and model" % (tag, rep, t1 - t0, t2 - t1, t3 - t2,
                                                                     (t3 - t2) / (2 * n_val) * 1e3), flush=True)
            results[tag] = (a[0], b[0], t3 - t2)
        tr.t_iter = tr.t_loader = tr.v_loader = None
        del tr
        import gc
        gc.collect()
        torch.cuda.empty_cache()
    same = all(np.array_equal(x, y) for x, y in zip(results["loader"][:2], results["device store"][:2]))
    print("IoU vectors of the two paths %s" % ("are equal, student and EMA" if same else "DIFFER"), flush=True)
    tl, ts = results["loader"][2], results["device store"][2]
    print("validate_all on %d frames at %d workers: loader %.2f s, device store %.2f s (%.2fx); over the 20 validations of "
          "the reference's recipe: %.0f s against %.0f s" % (n_val, nw, tl, ts, tl / ts, 20 * tl, 20 * ts), flush=True)
finally:
    shutil.rmtree(root, ignore_errors=True)
