"""Level 3 of the device-side sample path (cfg.dataset.device_aug_level: 3): what FDA costs on the device and what it
buys through the DataLoader.

    python tools/bench_fda.py [kernel] [loader] [workers=14] [batches=28] [N=16]

kernel: hiast_aug3_fda_u8 (its three launches, event-timed as one call) at B = 8 for 512 x 1024 views and GTAV's native
        1052 x 1914 frame, borders 0, 1 and 2, every sample with an FDA op.
loader: a ['MS', 'FDA-Target'] GTAV-size source dataset (N synthetic 1052 x 1914 frames) through the DataLoader with
        device_aug at level 2 (every sample finished by a worker: the host FFT) against level 3 (plans; the device
        runs the FDA), batch 8, batches handed to the device as the trainer hands them (batch_to_device); wall time
        from the first request over two rounds of the workers, so prefetched batches do not flatter either level."""
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hiast_amd import kernels as K  # noqa: E402
from hiast_amd.sseg.datasets import device_aug as DA  # noqa: E402

args = sys.argv[1:]
modes = [a for a in args if a in ("kernel", "loader")] or ["kernel", "loader"]
nums = [int(a) for a in args if a.isdigit()]
workers, batches, N = (nums + [14, 28, 16][len(nums):])[:3]
B = 8


def bench_kernel():
    dev = torch.device("cuda")
    print("hiast_aug3_fda_u8, B = %d, uint8 HWC views, every sample with an FDA op (median of 20 calls after 3)" % B)
    for H, W in ((512, 1024), (1052, 1914)):
        g = torch.Generator().manual_seed(H)
        img0 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
        blob = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, generator=g).to(dev)
        for border in (0, 1, 2):
            rows = np.zeros((B, DA.OPS_WORDS), np.int64)
            rows[:, 2], rows[:, 4] = 1, DA.OP_FDA
            rows[:, 5] = np.arange(B, dtype=np.int64) * (H * W * 3) | (border << DA.FDA_BORDER_SHIFT)
            seg = torch.from_numpy(K._aug_segments(rows)[0]).to(dev)
            ops = torch.from_numpy(rows).to(dev)
            img = img0.to(dev)
            times = []
            for it in range(23):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                K.aug3_fda_u8(img, ops, seg, blob)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            t = float(np.median(times[3:]))
            nbytes = 3 * B * H * W * 3 + B * H * W * 3           # view + target read, view read again and written
            print("  %4d x %4d  border %d: %7.1f us per batch = %6.1f us per sample  (%.0f GB/s of the %d MB it moves)"
                  % (H, W, border, t * 1e3, t * 1e3 / B, nbytes / t / 1e6, nbytes >> 20), flush=True)


def bench_loader():
    from torch.utils.data import DataLoader
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.sseg.datasets import utils as du
    from hiast_amd.sseg.datasets.loader.gtav_dataset import GTAVDataset
    from hiast_amd.tools import synth_data
    root = tempfile.mkdtemp(prefix="hiast_fda_")
    try:
        cfg = synth_data.synthetic_cfg(root, n_train=N, n_val=1, h=1052, w=1914, upscale=2, procs=min(workers, 14))
        dev = torch.device("cuda")
        print("['MS', 'FDA-Target'] GTAV source set, %d frames of 1052 x 1914, batch %d, %d workers, the first %d batches"
              % (N, B, workers, batches), flush=True)
        for level in (2, 3):
            ds = GTAVDataset(cfg, cfg.dataset.target.json_path, cfg.dataset.target.image_dir, aug_type=["MS", "FDA-Target"])
            ds.img_path_list = ds.img_path_list * 64
            ds.lbl_path_list = ds.lbl_path_list * 64
            ds.device_transform = ds.device_aug = True
            ds.device_aug_level = level
            dl = DataLoader(ds, batch_size=B, shuffle=True, drop_last=True, num_workers=workers, collate_fn=DA.collate,
                            pin_memory=True, persistent_workers=workers > 0)
            torch.cuda.synchronize()
            t0 = time.time()                    # from the first request: the workers' prefetch queues hide nothing
            it = iter(dl)
            finished, wait, hand = 0, 0.0, 0.0
            for i in range(batches):
                a = time.time()
                batch = next(it)
                b = time.time()
                finished += int((batch["device_aug"]["recs"][:, DA.R_KIND] == DA.KIND_FINISHED).sum())
                imgs, lbls = du.batch_to_device(batch, dev)
                wait, hand = wait + b - a, hand + time.time() - b
            torch.cuda.synchronize()
            dt = (time.time() - t0) / batches
            print("  level %d: %7.1f ms per batch = %6.1f images/s  (%d of %d samples finished by a worker; main process: %.1f ms "
                  "per batch waiting for the workers, %.1f ms handing the batch to the device)"
                  % (level, dt * 1e3, B / dt, finished, batches * B, wait / batches * 1e3, hand / batches * 1e3), flush=True)
            del it, dl
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_fda.py needs the GPU"
    if "kernel" in modes:
        bench_kernel()
    if "loader" in modes:
        bench_loader()
