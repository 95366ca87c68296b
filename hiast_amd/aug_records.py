"""The K15 hand-over tables as Python reads them (include/hiast_hip.h HIAST_AUG_*, HIAST_STORE_*, HIAST_MIX_*; csrc/aug_records.h
is the C side): the words of a sample's record row, the record kinds, the op types of a view's row and their limits.  Pure
constants with no imports, so that hiast_amd.kernels (which checks and launches the tables) and
hiast_amd.sseg.datasets.device_aug (which plans and builds them in DataLoader workers) share ONE definition without either
importing the other's dependencies."""

# one int64 record row per sample (offsets into the batch's uint8 blob / int32 table blob)
R_KIND, R_IMG, R_LBL, R_PIMG, R_PLBL, R_PTAB, R_CH, R_CW, R_FLIP, R_HLO, R_HN, R_HK, R_HT, R_VLO, R_VN, R_VK, R_VT, R_NX, \
    R_NY = range(19)
R_STRIDE = 19                # KIND_STORE: the frame's width in pixels, the row stride of a window read in place
REC_WORDS = 20
KIND_PLAN, KIND_FINISHED, KIND_STORE = 0, 1, 2
# kind 0 / kind 2 whose paste is confined to a rectangle (CutMix): the paste table's 256 bytes are followed by ry0, ry1, rx0,
# rx1 as little-endian int32 in WINDOW coordinates, clipped (an empty rectangle has ry0 == ry1)
KIND_PLAN_RECT, KIND_STORE_RECT = 3, 4
RECT_KINDS = (KIND_PLAN_RECT, KIND_STORE_RECT)
RECT_BYTES = 16
MIX_TABLE_BYTES = 256 + RECT_BYTES

# per (view, sample): kind, offset of the finished view, n ops, 0, then (type, parameter) x MAX_OPS
MAX_OPS = 8                  # colour ops per view the device record holds (after composing neighbouring LUTs)
OPS_WORDS = 4 + 2 * MAX_OPS
OP_LUT, OP_GRAY, OP_EQUALIZE = 1, 2, 3
OP_CONTRAST, OP_SAT, OP_HUE, OP_BLUR = 4, 5, 6, 7        # level 2 (plan_sample(level=2)): ColorJitter's steps, GaussianBlur
MAX_KSIZE = 41
OP_FDA = 8                                               # level 3: blob offset of the target view | border << 40
FDA_MAX_BORDER, FDA_BORDER_SHIFT, FDA_MIN_SIDE = 2, 40, 8
