"""Device-resident frames (cfg.dataset.device_store_gb / HIAST_DEVICE_STORE_GB; off by default): the decoded frames of a
dataset stay in device memory, so a training sample travels as a plan of a few hundred bytes (device_aug.py, record kind 2)
and a validation batch as a set of offsets (kernels.normalize_gather_u8).  The draws and the kernels' arithmetic are those of
the bytes path; every batch is byte-identical to what the loader delivers.

    DeviceStore(device, budget_bytes)      the process's one budget; place(dataset, num_workers) -> ResidentSet
    ResidentSet                            one dataset's frames: ONE uint8 device buffer (one base pointer per launch) and the
                                           residency table, int64 [n, 4] = (image offset, label offset, H, W) per dataset
                                           index, offset -1 = not resident; in shared host memory, attached to the dataset
                                           (`dataset.store_table`) before its loader's first iterator exists, constant afterwards

A frame is the image uint8 [H][W][3] followed by the label uint8 [H][W] — what load_data returns, so the pseudo-label of a
target set with pseudo_dir —, each 16-byte aligned.  Frames go in in index order and placement stops at the first frame that
would exceed what is left of the budget: the first k frames are resident.  The sizes come from the image headers
(BaseDataset.frame_shape) so that the buffer is allocated once, at its final size; a frame whose load raises, or whose
decoded shape is not its header's, keeps its room and stays non-resident.  Each rank keeps its own store."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ALIGN = 16
# decode threads of a fill: at most min(16, max(1, num_workers)), and no more than this — 500 frames of 2048x1024 filled in 9 s
# on 4 threads and in 31 s on 14 (profiles/device_store_timing.txt): beyond a few, the threads wait for one another
FILL_THREADS = 4
T_IMG, T_LBL, T_H, T_W = range(4)


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def frame_bytes(h, w):
    """what a resident frame of h x w takes: image and label, each padded to 16 bytes"""
    return _align(int(h) * int(w) * 3) + _align(int(h) * int(w))


class ResidentSet:
    """one dataset's resident frames.  `buffer`: uint8 [bytes] on the store's device; `table`: int64 [n, 4] in shared host
    memory (see the module text)"""

    def __init__(self, buffer, table):
        self.buffer, self.table = buffer, table
        self.frames = table.numpy()

    @classmethod
    def from_frames(cls, frames, device, n=None, alloc=None):
        """frames: [(index, image uint8 [H, W, 3], label uint8 [H, W])] in placement order -> a set of n dataset indices
        (default: as many as frames) holding exactly these"""
        n = len(frames) if n is None else n
        table = torch.full((n, 4), -1, dtype=torch.int64)
        off = 0
        for i, img, lbl in frames:
            h, w = lbl.shape
            table[i] = torch.tensor([off, off + _align(h * w * 3), h, w])
            off += frame_bytes(h, w)
        buf = (alloc or _alloc_on(device))(max(off, ALIGN))
        rs = cls(buf, table.share_memory_())
        for i, img, lbl in frames:
            rs.write(i, img, lbl)
        return rs

    def resident(self, index):
        return index >= 0 and int(self.frames[index, T_IMG]) >= 0

    def all_resident(self):
        return len(self.frames) > 0 and bool((self.frames[:, T_IMG] >= 0).all())

    def bytes_held(self):
        return int(self.buffer.numel())

    def write(self, index, img, lbl, stage=None):
        """copy a decoded frame to its place (through `stage`, a pinned uint8 buffer, when given)"""
        io, lo, h, w = (int(v) for v in self.frames[index])
        img = np.ascontiguousarray(img, np.uint8).reshape(-1)
        lbl = np.ascontiguousarray(lbl, np.uint8).reshape(-1)
        if img.size != h * w * 3 or lbl.size != h * w:
            raise ValueError("device_store: frame %d is not %dx%d" % (index, h, w))
        for off, a in ((io, img), (lo, lbl)):
            src = torch.from_numpy(a)
            if stage is not None:
                stage[:a.size].copy_(src)
                self.buffer[off:off + a.size].copy_(stage[:a.size], non_blocking=True)
                torch.cuda.current_stream(self.buffer.device).synchronize()     # (the staging buffer is written again next)
            else:
                self.buffer[off:off + a.size].copy_(src)

    def image(self, index):
        io, _, h, w = (int(v) for v in self.frames[index])
        return self.buffer[io:io + h * w * 3].view(h, w, 3)

    def label(self, index):
        _, lo, h, w = (int(v) for v in self.frames[index])
        return self.buffer[lo:lo + h * w].view(h, w)


def _alloc_on(device):
    return lambda nbytes: torch.empty((int(nbytes),), dtype=torch.uint8, device=device)


class DeviceStore:
    """DeviceStore(device, budget_bytes): one budget per process, spent by place() in the order of the calls (the trainer
    places the validation set first — small, and read by both models —, then the target set, then a source set).  `alloc`:
    nbytes -> uint8 tensor (default: torch.empty on `device`; a CPU device gives a host-backed store for tests)"""

    def __init__(self, device, budget_bytes, alloc=None):
        self.device = torch.device(device)
        self.budget = int(budget_bytes)
        self.alloc = alloc or _alloc_on(self.device)
        self.sets = {}                     # id(dataset) -> ResidentSet

    def bytes_held(self):
        return sum(rs.bytes_held() for rs in self.sets.values())

    def of(self, dataset):
        return self.sets.get(id(dataset))

    def place(self, dataset, num_workers=1):
        """fill eagerly (the calling process decodes, on min(FILL_THREADS, 16, max(1, num_workers)) threads, through the
        dataset's own load_data: the decoded cache is used when configured), attach the residency table to the dataset and
        return the ResidentSet; a second call for the same dataset returns the first one's"""
        if id(dataset) in self.sets:
            return self.sets[id(dataset)]
        n = len(dataset)
        table = torch.full((n, 4), -1, dtype=torch.int64)
        left, off = self.budget - self.bytes_held(), 0
        for i in range(n):
            try:
                h, w = dataset.frame_shape(i)
            except Exception as e:          # (an unreadable header: load_data would raise too)
                print("## device_store: {} in sizing {}".format(repr(e), i))
                continue
            need = frame_bytes(h, w)
            if off + need > left:
                break                       # the first frame that would exceed the budget ends the placement
            table[i] = torch.tensor([off, off + _align(h * w * 3), h, w])
            off += need
        rs = ResidentSet(self.alloc(off) if off else torch.empty((0,), dtype=torch.uint8, device=self.device), table)
        self._fill(dataset, rs, min(FILL_THREADS, 16, max(1, int(num_workers))))
        table.share_memory_()
        rs.frames = table.numpy()
        self.sets[id(dataset)] = rs
        dataset.store_table = table
        return rs

    def _fill(self, dataset, rs, threads):
        todo = [i for i in range(len(rs.frames)) if rs.frames[i, T_IMG] >= 0]
        cuda = rs.buffer.is_cuda
        local = threading.local()

        def one(i):
            try:
                img, lbl, _ = dataset.load_data(i)
                if cuda and getattr(local, "stage", None) is None:
                    biggest = max(int(rs.frames[j, T_H]) * int(rs.frames[j, T_W]) * 3 for j in todo)
                    local.stage = torch.empty((biggest,), dtype=torch.uint8).pin_memory()
                rs.write(i, img, lbl, getattr(local, "stage", None))
                return i, None
            except Exception as e:          # left non-resident: the worker path loads (and recovers) as it does today
                return i, e
        with ThreadPoolExecutor(threads) as pool:
            for i, err in pool.map(one, todo):
                if err is not None:
                    print("## device_store: {} in loading {}: not resident".format(repr(err), i))
                    rs.frames[i, :2] = -1
