"""The stem, pooling, packing and table entries of the C ABI by argument NAME (a plain helper module, the scheme of bn_calls.py): one
table, used by the host-side refusal tests (placeholder addresses, nothing is launched) and by the guard-band tests on the device
(carved buffers)."""
import ctypes

import numpy as np

E_ARG, E_RANGE = -1, -2
BF16, SPLIT, FP16 = 1, 2, 3                    # HIAST_FMT_*
FMT = {"bf16": BF16, "split": SPLIT, "fp16": FP16}
DTYPE = {"fp32": 0, "bf16": 1, "fp16": 2}      # hiast_stem_tail's input code (hiast_bn_act_nhwc_infer: 0 and 1 only)

ENTRIES = {
    "stem_eval": ("hiast_stem_eval", "x w gamma beta mean var eps out fmt B H W stream"),
    "stem_tail": ("hiast_stem_tail", "x dtype gamma beta mean var eps out fmt B H W C stream"),
    "split_planes": ("hiast_split_planes", "x planes M C inverse stream"),
    "pack": ("hiast_pack_conv_weight", "w N K taps fmt transpose wp wpt stream"),
    "pack_multi": ("hiast_pack_conv_weight_multi", "table chunk_tensor chunk_start n_chunks max_taps stream"),
    "bn_infer": ("hiast_bn_act_nhwc_infer", "x y gamma beta mean var eps relu M C dtype stream"),
    "pool_fwd": ("hiast_maxpool3x3s2_nhwc_fwd", "x y idx B H W C fmt stream"),
    "pool_bwd": ("hiast_maxpool3x3s2_nhwc_bwd", "dy idx dx B H W C fmt stream"),
    "normalize_u8": ("hiast_normalize_u8", "img out B HW mean std stream"),      # mean, std: HOST float[3]
    "ema": ("hiast_ema_update", "table chunk_tensor chunk_start n_chunks decay one_minus_decay stream"),
    "multi_copy": ("hiast_multi_copy", "table n_tensors stream"),
    "confusion": ("hiast_confusion_hist", "pred target N K inter area_pred area_tgt stream"),
}
# pointers an entry refuses as NULL (E_ARG) whatever the other arguments are (pack: wpt only with transpose 2, listed below)
REQUIRED = {
    "stem_eval": "x w mean var out", "stem_tail": "x mean var out", "split_planes": "x planes", "pack": "w wp",
    "pack_multi": "table chunk_tensor chunk_start", "bn_infer": "x y mean var", "pool_fwd": "x y idx", "pool_bwd": "dy idx dx",
    "normalize_u8": "img out mean std", "ema": "table chunk_tensor chunk_start", "multi_copy": "table",
    "confusion": "pred target inter area_pred area_tgt",
}
# pointers an entry wants aligned, and to how many bytes (E_RANGE otherwise); everything else may sit at any address its element
# type allows (pack: a misaligned wp / wpt only selects the elementwise kernel)
ALIGNED = {
    "stem_eval": {"out": 8}, "stem_tail": {"x": 16, "out": 16}, "split_planes": {"x": 16, "planes": 16},
    "bn_infer": {"x": 16, "y": 16}, "pool_fwd": {"x": 16, "y": 16, "idx": 8}, "pool_bwd": {"dy": 16, "dx": 16, "idx": 8},
}
POINTERS = set("x w gamma beta mean var out planes wp wpt table chunk_tensor chunk_start y idx dy dx img std pred target inter "
               "area_pred area_tgt stream".split())
# positive extents (E_ARG when <= 0)
EXTENTS = {
    "stem_eval": "B H W", "stem_tail": "B H W C", "split_planes": "M C", "pack": "N K taps", "pack_multi": "n_chunks max_taps",
    "bn_infer": "M C", "pool_fwd": "B H W C", "pool_bwd": "B H W C", "normalize_u8": "B HW", "ema": "n_chunks",
    "multi_copy": "n_tensors", "confusion": "N K",
}
BASE = dict(B=2, H=9, W=14, C=64, M=64, N=64, K=64, taps=9, fmt=BF16, dtype=1, transpose=0, inverse=0, eps=1e-5, relu=1, HW=64,
            n_chunks=2, max_taps=9, decay=0.5, one_minus_decay=0.5, n_tensors=2)


def args_of(entry):
    return ENTRIES[entry][1].split()


def _addr(v):
    return v if isinstance(v, int) else v.data_ptr()


def call(lib, entry, **kw):
    """kw: every argument of the entry by name; pointers as int addresses, device tensors, ctypes arrays (the host vectors of
    hiast_normalize_u8) or None"""
    fn, names = ENTRIES[entry]
    vals = []
    for n in names.split():
        v = kw[n]
        if n in POINTERS and not isinstance(v, ctypes.Array):
            v = ctypes.c_void_p(0 if v is None else _addr(v))
        vals.append(v)
    return getattr(lib, fn)(*vals)


def placeholders(entry):
    """a valid argument set whose pointers are distinct 4096-byte aligned addresses that are never dereferenced"""
    kw = {}
    for i, n in enumerate(args_of(entry)):
        kw[n] = 4096 * (i + 1) if n in POINTERS else BASE[n]
    kw.update(stream=None)
    if entry == "confusion":
        kw.update(K=19)
    return kw


def refused_calls(entry):
    """-> [(what, changed arguments, expected code)] for one entry, each refused BEFORE any launch; shared with the device test,
    which runs them on carved buffers.  A value "+n" moves a pointer n bytes on."""
    names = args_of(entry)
    out = [("null " + n, {n: None}, E_ARG) for n in REQUIRED[entry].split()]
    for n in EXTENTS[entry].split():
        out.append((n + " = 0", {n: 0}, E_ARG))
        out.append((n + " = -1", {n: -1}, E_ARG))
    for n, a in ALIGNED.get(entry, {}).items():
        out.append(("%s at addr+%d" % (n, a // 2), {n: "+%d" % (a // 2)}, E_RANGE))
    if entry in ("stem_eval", "stem_tail", "pack"):
        out += [("fmt %d" % f, {"fmt": f}, E_RANGE) for f in (0, 4, -1)]
    if entry in ("pool_fwd", "pool_bwd"):
        out += [("fmt %d" % f, {"fmt": f}, E_RANGE) for f in (0, SPLIT, 4)]
        out.append(("C = 12", {"C": 12}, E_RANGE))
        out.append(("B H W C = 2^40", dict(B=65536, H=4096, W=4096, C=1), E_RANGE))      # C % 8 fails first: same code
        out.append(("B H W C = 2^43", dict(B=65536, H=4096, W=4096, C=8), E_RANGE))
        out.append(("B H W C = 2^40 exactly", dict(B=32768, H=2048, W=2048, C=8), E_RANGE))
    if entry == "stem_eval":
        out.append(("3 B H W = 2^31 + 65536", dict(B=1, H=32768, W=21846), E_RANGE))
        out.append(("3 B H W = 3 * 2^30", dict(B=2 ** 15, H=2 ** 15, W=1), E_RANGE))
    if entry == "stem_tail":
        out += [("dtype 3", {"dtype": 3}, E_RANGE), ("dtype -1", {"dtype": -1}, E_RANGE), ("C = 12", {"C": 12}, E_RANGE),
                ("C = 48 with split planes", {"C": 48, "fmt": SPLIT}, E_RANGE),
                ("B H W C = 2^43", dict(B=65536, H=4096, W=4096, C=8), E_RANGE),
                ("B H W C = 2^40 exactly", dict(B=32768, H=2048, W=2048, C=8), E_RANGE),
                # G = 16385 is odd: need = G exceeds the cap of 16384 blocks, and 289 G / 256 > 16384 blocks are wanted
                ("need above the grid cap", dict(B=1, H=33, W=33, C=8 * 16385), E_RANGE)]
    if entry == "split_planes":
        out += [("C = 48", {"C": 48}, E_RANGE), ("C = 8", {"C": 8}, E_RANGE)]
    if entry == "pack":
        out += [("transpose 3", {"transpose": 3}, E_RANGE), ("transpose -1", {"transpose": -1}, E_RANGE),
                ("transpose 2 without wpt", {"transpose": 2, "wpt": None}, E_ARG)]
        out += [(what + " (split planes)", dict(ch, fmt=SPLIT), E_RANGE) for what, ch in split_pack_refusals()]
    if entry == "pack_multi":
        out.append(("max_taps 10", {"max_taps": 10}, E_RANGE))
    if entry == "bn_infer":
        out += [("dtype %d" % d, {"dtype": d}, E_RANGE) for d in (2, 3, -1)]
        out += [("C = 12, bf16 rows", {"C": 12, "dtype": 1}, E_RANGE), ("C = 6, fp32 rows", {"C": 6, "dtype": 0}, E_RANGE)]
    if entry == "normalize_u8":
        out.append(("B = 65536", {"B": 65536}, E_RANGE))
    if entry == "confusion":
        out.append(("K = 1025", {"K": 1025}, E_RANGE))
    assert all(set(ch) <= set(names) for _, ch, _ in out), entry
    return out


def split_pack_refusals():
    """the split-plane shapes hiast_pack_conv_weight refuses: a form it writes whose reduction channel count is no multiple of 32
    (the lo half of a ragged last slab would land in the next row — behind wp for the last one)"""
    return [("K = 48, forward", dict(N=64, K=48, transpose=0)), ("K = 48, both", dict(N=64, K=48, transpose=2)),
            ("N = 48, adjoint", dict(N=48, K=64, transpose=1)), ("N = 48, both", dict(N=48, K=64, transpose=2)),
            ("K = 3, forward", dict(N=64, K=3, taps=49, transpose=0)), ("N = 19, adjoint", dict(N=19, K=256, taps=1, transpose=1))]


def apply_change(kw, change):
    kw = dict(kw)
    for n, v in change.items():
        kw[n] = _addr(kw[n]) + int(v[1:]) if isinstance(v, str) else v
    return kw


# ------------------------------------------------------------------------------------------------ the record tables
PACK_REC = np.dtype([("w", np.int64), ("wp", np.int64), ("wpt", np.int64), ("N", np.int32), ("K", np.int32), ("taps", np.int32),
                     ("planes", np.int32), ("mode", np.int32), ("pad", np.int32)])         # hiast_pack_rec
CHUNK = 65536                                                                                # elements per block of hiast_ema_update


def ema_tables(pairs):
    """[(ema address, p address, n)] -> (records int64 [T][3], chunk_tensor int32, chunk_start int64) as numpy"""
    recs = np.asarray(pairs, np.int64).reshape(-1, 3)
    ct = [i for i, (_, _, n) in enumerate(pairs) for _ in range(0, n, CHUNK)]
    cs = [s for _, _, n in pairs for s in range(0, n, CHUNK)]
    return recs, np.asarray(ct, np.int32), np.asarray(cs, np.int64)


def pack_tables(recs):
    """[(w, wp, wpt | 0, N, K, taps, fmt, mode)] -> (records, chunk_tensor, chunk_start, max taps): one block per 64 x 64 tile"""
    host = np.zeros(len(recs), PACK_REC)
    ct, cs = [], []
    for i, r in enumerate(recs):
        host[i] = tuple(r) + (0,)
        N, K = r[3], r[4]
        assert N % 64 == 0 and K % 64 == 0 and r[5] <= 9
        for tile in range((N // 64) * (K // 64)):
            ct.append(i)
            cs.append(tile)
    return host, np.asarray(ct, np.int32), np.asarray(cs, np.int64), max(r[5] for r in recs)
