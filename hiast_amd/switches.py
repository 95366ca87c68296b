"""Path-selecting environment switches of the training step, read ONCE at import.

Each of them changes which autograd path (and, under SyncBN, which sequence of collectives) a forward / backward takes.  Looked
up per call they could differ between the ranks of a job, or between a forward and its backward — mismatched collective order on
the statistics communicator is a hang.  Tests flip them with `monkeypatch.setitem(switches.SWITCHES, name, value)`."""
import os

_NAMES = ("HIAST_NO_BN_MASK", "HIAST_NO_BN_BWD_FUSION", "HIAST_LIB_WGRAD", "HIAST_NO_WGROUP", "HIAST_NO_XSUM",
          "HIAST_NO_IDT_HANDOFF", "HIAST_LIB_STEM",
          "HIAST_NO_BN3_FUSION",      # bn3's backward sums from a pass of their own, not from the next block's conv1 data gradient
          "HIAST_LIB_DGRAD_S2",       # the library's data gradient for the strided 3x3
          "HIAST_NO_ASYNC_STAT")      # SyncBN backward: the exchange inside the BatchNorm's backward (changes the collective order)
SWITCHES = {n: os.environ.get(n, "0") == "1" for n in _NAMES}
# opt-IN paths (off unless set to "1"), kept apart from the opt-outs above; read once and flipped by tests the same way
_OPT_IN_NAMES = ("HIAST_DISC_HIP", "HIAST_DISC_HIP_16BIT")
OPT_IN = {n: os.environ.get(n, "0") == "1" for n in _OPT_IN_NAMES}
# opt-in SIZES (0 = off), read once and flipped by tests the same way.  HIAST_DEVICE_STORE_GB: GB of device memory per process
# for decoded frames that stay resident (sseg/datasets/device_store.py); overrides cfg.dataset.device_store_gb when > 0
_SIZE_NAMES = ("HIAST_DEVICE_STORE_GB",)
SIZES = {n: float(os.environ.get(n, "0") or 0) for n in _SIZE_NAMES}


def on(name):
    return OPT_IN[name] if name in OPT_IN else SWITCHES[name]


def device_store_bytes(cfg):
    """the budget of the device store in bytes: HIAST_DEVICE_STORE_GB if > 0, else cfg.dataset.device_store_gb; 0 = off"""
    gb = SIZES["HIAST_DEVICE_STORE_GB"]
    if not gb > 0:
        gb = float(getattr(cfg.dataset, "device_store_gb", 0) or 0)
    return int(gb * (1 << 30)) if gb > 0 else 0
