"""The head and pseudo-label entries of the C ABI by argument NAME (a plain helper module): one table, used by the host-side
refusal tests (placeholder addresses, nothing is launched) and by the guard-band tests on the device (carved buffers).

Three kinds of pointer arguments: DEVICE pointers (int address, tensor or None), HOST int arrays (`dil`, `hs`, `wss`, `Hs`, `Ws`:
a tuple or None; the entries read them on the host, some of them before their last check, so they are always real) and HOST
arrays of device pointers (`z`, `zf`: a list of addresses / tensors / None entries, or None)."""
import ctypes

E_ARG, E_RANGE, E_WS = -1, -2, -3
BF16, SPLIT, FP16 = 1, 2, 3              # HIAST_FMT_*; 0 = fp32 rows (hiast_aspp2_fwd only)
MAX_CLASSES = 32
DIL = (6, 12, 18, 24)

_W8 = "w0 w1 w2 w3 b0 b1 b2 b3 "
ENTRIES = {
    "aspp_pack": ("hiast_aspp_pack_weights", _W8 + "Cin Cout wpack stream"),
    "aspp_fwd": ("hiast_aspp_fwd", "x wpack y B Cin h w Cout dil ws ws_bytes stream"),
    "aspp_bwd_data": ("hiast_aspp_bwd_data", "dy wpack dx B Cin h w Cout dil stream"),
    "aspp_bwd_weight": ("hiast_aspp_bwd_weight", "x dy dw0 dw1 dw2 dw3 db B Cin h w Cout dil ws ws_bytes stream"),
    "aspp2_pack": ("hiast_aspp2_pack_weights", _W8 + "Cin Cout wt wd bias stream"),
    "aspp2_fwd": ("hiast_aspp2_fwd", "x dtype wt bias y B Cin h w Cout dil ws ws_bytes stream"),
    "aspp2_bwd": ("hiast_aspp2_bwd", "x dy wd dx dw0 dw1 dw2 dw3 db B Cin h w Cout dil fmt ws ws_bytes stream"),
    "up_fwd": ("hiast_upsample_bilinear_ac_fwd", "x y B C h w H W stream"),
    "up_bwd": ("hiast_upsample_bilinear_ac_bwd", "gout gin B C h w H W stream"),
    "pass1": ("hiast_plabel_pass1", "logits B C h w H W maxprob argmax hist ws ws_bytes stream"),
    "pass2": ("hiast_plabel_pass2", "maxprob argmax thr B C HW plbl count sumprob stream"),
    "strided_hist": ("hiast_plabel_strided_hist", "maxprob argmax N C interval rank_offset class_total hist ws ws_bytes stream"),
    "tta": ("hiast_tta_fused", "z zf hs wss Hs Ws n_scales B C H W probsum label stream"),
}
HOST_INTS = set("dil hs wss Hs Ws".split())
HOST_PTRS = set("z zf".split())
POINTERS = set("w0 w1 w2 w3 b0 b1 b2 b3 wpack x y dy dx dw0 dw1 dw2 dw3 db ws wt wd bias gout gin logits maxprob argmax hist thr "
               "plbl count sumprob rank_offset class_total probsum label stream".split())
# device / host pointers an entry refuses as NULL (E_ARG) whatever the other arguments are
REQUIRED = {
    "aspp_pack": _W8 + "wpack", "aspp_fwd": "x wpack y dil", "aspp_bwd_data": "dy wpack dx dil",
    "aspp_bwd_weight": "x dy dw0 dw1 dw2 dw3 db dil ws", "aspp2_pack": _W8 + "wt bias", "aspp2_fwd": "x wt bias y dil ws",
    "aspp2_bwd": "dy dil ws", "up_fwd": "x y", "up_bwd": "gout gin", "pass1": "logits maxprob argmax hist",
    "pass2": "maxprob argmax plbl count sumprob", "strided_hist": "maxprob argmax hist ws", "tta": "z hs wss Hs Ws",
}
# extents an entry refuses when they are not positive (E_ARG)
EXTENTS = {
    "aspp_pack": "Cin Cout", "aspp_fwd": "B Cin h w Cout", "aspp_bwd_data": "B Cin h w Cout", "aspp_bwd_weight": "B Cin h w Cout",
    "aspp2_pack": "Cin Cout", "aspp2_fwd": "B Cin h w Cout", "aspp2_bwd": "B Cin h w Cout", "up_fwd": "B C h w H W",
    "up_bwd": "B C h w H W", "pass1": "B C h w H W", "pass2": "B C HW", "strided_hist": "N C interval", "tta": "n_scales B C H W",
}
# the valid call the refusals start from (the device test carves its buffers for these extents)
BASE = {
    "aspp_pack": dict(Cin=64, Cout=19), "aspp_fwd": dict(B=1, Cin=64, h=9, w=17, Cout=19, dil=DIL),
    "aspp_bwd_data": dict(B=1, Cin=256, h=9, w=17, Cout=19, dil=DIL),
    "aspp_bwd_weight": dict(B=1, Cin=64, h=9, w=17, Cout=19, dil=DIL), "aspp2_pack": dict(Cin=128, Cout=19),
    "aspp2_fwd": dict(B=1, Cin=128, h=9, w=17, Cout=19, dil=DIL, dtype=BF16),
    "aspp2_bwd": dict(B=1, Cin=128, h=9, w=17, Cout=19, dil=DIL, fmt=BF16), "up_fwd": dict(B=1, C=2, h=3, w=4, H=9, W=13),
    "up_bwd": dict(B=1, C=2, h=3, w=4, H=9, W=13), "pass1": dict(B=1, C=19, h=3, w=4, H=9, W=13),
    "pass2": dict(B=1, C=19, HW=64), "strided_hist": dict(N=4097, C=19, interval=3),
    "tta": dict(n_scales=1, B=1, C=19, H=9, W=13, hs=(3,), wss=(4,), Hs=(9,), Ws=(13,)),
}


def args_of(entry):
    return ENTRIES[entry][1].split()


def _addr(v):
    return 0 if v is None else (v if isinstance(v, int) else v.data_ptr())


def call(lib, entry, **kw):
    """kw: every argument of the entry by name"""
    fn, names = ENTRIES[entry]
    vals, keep = [], []
    for n in names.split():
        v = kw[n]
        if n in HOST_INTS:
            v = None if v is None else (ctypes.c_int * len(v))(*[int(i) for i in v])
            keep.append(v)
        elif n in HOST_PTRS:
            v = None if v is None else (ctypes.c_void_p * len(v))(*[_addr(p) or None for p in v])
            keep.append(v)
        elif n in POINTERS:
            v = ctypes.c_void_p(_addr(v))
        vals.append(v)
    return getattr(lib, fn)(*vals)


def workspace_need(lib, entry, kw):
    """bytes of workspace the entry's header asks for with these extents (0: the entry takes none)"""
    if entry in ("aspp_fwd", "aspp_bwd_weight"):
        return lib.hiast_aspp_workspace_bytes(kw["B"], kw["Cin"], kw["h"], kw["w"], kw["Cout"])
    if entry in ("aspp2_fwd", "aspp2_bwd"):
        return lib.hiast_aspp2_workspace_bytes(kw["B"], kw["Cin"], kw["h"], kw["w"], kw["Cout"], int(entry == "aspp2_bwd"))
    if entry == "pass1":
        return lib.hiast_plabel_pass1_workspace_bytes(kw["C"])
    if entry == "strided_hist":
        return lib.hiast_plabel_strided_hist_workspace_bytes(kw["N"], kw["C"])
    return 0


def aspp_splitk(B, Cin, h, w, Cout):
    """pick_splitk of aspp.hip without its tuning override: doubled while the grid has fewer than 1024 blocks and half the
    channel range is still a whole number of 64-channel chunks; at most 8"""
    px = 256
    blocks = -(-h * w // px) * B
    s = 1
    while blocks * s < 1024 and s < 8 and (Cin // (s * 2)) % 64 == 0 and Cin // (s * 2) >= 64:
        s *= 2
    return s


def aspp_wgrad_nsplit(B, h, w):
    """wgrad_nsplit of aspp.hip: pixel splits of the weight gradient, at least 32 16-pixel steps each, at most 16"""
    total = B * h * ((w + 15) // 16)
    s = 16
    while s > 1 and total // s < 32:
        s >>= 1
    return s


def used_bytes(kind, kw):
    if kind == "splitk":
        return aspp_splitk(kw["B"], kw["Cin"], kw["h"], kw["w"], kw["Cout"]) * kw["B"] * kw["Cout"] * kw["h"] * kw["w"] * 4
    assert kind == "wgrad"
    return aspp_wgrad_nsplit(kw["B"], kw["h"], kw["w"]) * 33 * 32 * kw["Cin"] * 4


def placeholders(lib, entry):
    """a valid argument set whose device pointers are distinct 4096-byte aligned addresses that are never dereferenced"""
    kw = {}
    for i, n in enumerate(args_of(entry)):
        kw[n] = 4096 * (i + 1) if n in POINTERS else 0
    kw.update(BASE[entry], stream=None)
    if entry == "tta":
        kw.update(z=[4096 * 50], zf=[4096 * 51])
    if "ws_bytes" in kw:
        kw["ws_bytes"] = workspace_need(lib, entry, kw)
    return kw


def refused_calls(entry):
    """-> [(what, changed arguments, expected code)] for one entry: calls its header and its code refuse before any launch.
    Shared with the device test, which runs them on carved buffers.  Values "+4": the address 4 bytes on; "+2": 2 bytes on;
    ("need", d): the workspace size of the entry's *_workspace_bytes for the CHANGED extents, plus d; ("splitk", d) and
    ("wgrad", d): the bytes hiast_aspp_fwd / hiast_aspp_bwd_weight actually use (below), plus d."""
    names = args_of(entry)
    out = [("null " + n, {n: None}, E_ARG) for n in REQUIRED[entry].split()]
    for n in EXTENTS[entry].split():
        for v in (0, -1):
            out.append(("%s = %d" % (n, v), {n: v}, E_ARG))
    if entry.startswith("aspp"):
        step = 128 if entry.startswith("aspp2") else 64
        out.append(("Cin = %d" % (step + step // 2), {"Cin": step + step // 2}, E_RANGE))
        out.append(("Cout = 33", {"Cout": 33}, E_RANGE))
        if "B" in names:
            out.append(("B = 65536", {"B": 65536}, E_RANGE))
    if entry == "aspp_fwd":
        # split-K is 2 here (one block of pixels, Cin / 2 = 64 is still a chunk): the partial sums need a workspace
        out.append(("no workspace with split-K 2", {"Cin": 128, "ws": None, "ws_bytes": 0}, E_WS))
        out.append(("split-K workspace one byte short", {"Cin": 128, "ws_bytes": ("splitk", -1)}, E_WS))
        # an image of 4096 x 256 x 513 fp32 = 2.004 GiB: beyond the 32-bit byte offsets of the 16-row forward kernel.  (Split-K
        # is 2 for this shape as well: without the range check it is refused for its missing workspace.)
        out.append(("image above 2 GiB", dict(B=1, Cin=4096, h=256, w=513, Cout=19, ws=None, ws_bytes=0), E_RANGE))
    if entry == "aspp_bwd_data":
        for Cin in (64, 320):
            out.append(("Cin = %d" % Cin, {"Cin": Cin}, E_RANGE))
        out.append(("Cout = 21", {"Cout": 21}, E_RANGE))
    if entry == "aspp_bwd_weight":
        out.append(("Cout = 20", {"Cout": 20}, E_RANGE))
        out.append(("dilation 65", {"dil": (6, 12, 18, 65)}, E_RANGE))
        out.append(("dilation 0", {"dil": (6, 0, 18, 24)}, E_ARG))
        out.append(("dilation -1", {"dil": (-1, 12, 18, 24)}, E_ARG))
        out.append(("workspace one byte short", {"ws_bytes": ("wgrad", -1)}, E_WS))
    if entry == "aspp2_fwd":
        for dt in (-1, 4):
            out.append(("dtype %d" % dt, {"dtype": dt}, E_RANGE))
        out.append(("workspace 257 bytes short", {"ws_bytes": ("need", -257)}, E_WS))
        for n in ("x", "wt", "ws"):
            out.append((n + " at addr+4", {n: "+4"}, E_RANGE))
    if entry == "aspp2_bwd":
        for fmt in (0, SPLIT, 4, -1):
            out.append(("fmt %d" % fmt, {"fmt": fmt}, E_RANGE))
        out.append(("weight gradients without x", {"x": None}, E_ARG))
        out.append(("weight gradients without dw2", {"dw2": None}, E_ARG))
        out.append(("weight gradients without db", {"db": None}, E_ARG))
        out.append(("dx without wd", {"wd": None}, E_ARG))
        out.append(("workspace 257 bytes short", {"ws_bytes": ("need", -257)}, E_WS))
        for n in ("x", "ws", "wd", "dx"):
            out.append((n + " at addr+4", {n: "+4"}, E_RANGE))
    if entry in ("up_fwd", "up_bwd"):
        out.append(("B C = 65536", {"B": 32768, "C": 2}, E_RANGE))
        out.append(("H = 65536", {"H": 65536}, E_RANGE))
        out.append(("h = 65536", {"h": 65536, "H": 65535}, E_RANGE))
    if entry == "pass1":
        for C in (5, 33):
            out.append(("C = %d" % C, {"C": C}, E_RANGE))
        out.append(("H < h", {"H": 2}, E_RANGE))
        out.append(("W < w", {"W": 3}, E_RANGE))
        out.append(("B = 65536", {"B": 65536}, E_RANGE))
        out.append(("workspace one byte short", {"ws_bytes": ("need", -1)}, E_WS))
        out.append(("workspace at addr+2", {"ws": "+2", "ws_bytes": 1 << 30}, E_WS))
    if entry == "pass2":
        out.append(("C = 33", {"C": MAX_CLASSES + 1}, E_RANGE))
        out.append(("B = 65536", {"B": 65536}, E_RANGE))
    if entry == "strided_hist":
        out.append(("C = 33", {"C": MAX_CLASSES + 1, "ws_bytes": 1 << 30}, E_RANGE))
        out.append(("workspace one byte short", {"ws_bytes": ("need", -1)}, E_WS))
    if entry == "tta":
        out.append(("neither probsum nor label", {"probsum": None, "label": None}, E_ARG))
        out.append(("9 scales", {"n_scales": 9}, E_RANGE))
        out.append(("B = 65536", {"B": 65536}, E_RANGE))
        out.append(("H = 65536", {"H": 65536}, E_RANGE))
        out.append(("C = 5", {"C": 5}, E_RANGE))
        out.append(("Hs < hs", {"Hs": (2,)}, E_ARG))
        out.append(("Ws < ws", {"Ws": (3,)}, E_ARG))
        out.append(("hs = 0", {"hs": (0,)}, E_ARG))
        out.append(("z[0] NULL", {"z": [None]}, E_ARG))
    return out


def apply_change(lib, entry, kw, change):
    kw = dict(kw)
    for n, v in change.items():
        if isinstance(v, str) and v[0] == "+":
            kw[n] = _addr(kw[n]) + int(v[1:])
        elif not isinstance(v, tuple) or n in HOST_INTS:
            kw[n] = v
    for n, v in change.items():
        if isinstance(v, tuple) and n not in HOST_INTS:
            kw[n] = (workspace_need(lib, entry, kw) if v[0] == "need" else used_bytes(v[0], kw)) + v[1]
    return kw
