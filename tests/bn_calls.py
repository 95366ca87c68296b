"""The BatchNorm entries of the C ABI by argument NAME (a plain helper module): one table, used by the host-side refusal tests
(placeholder addresses, nothing is launched) and by the guard-band tests on the device (carved buffers)."""
import ctypes

E_ARG, E_RANGE, E_WS = -1, -2, -3
BF16, FP16 = 1, 3                    # HIAST_FMT_* of the channels-last entries
FMT = {"bf16": BF16, "fp16": FP16}
DTYPE = {"fp32": 0, "bf16": 1, "fp16": 2}      # dtype of the NCHW entries

ENTRIES = {
    "nhwc_stats": ("hiast_bn_nhwc_stats", "x M C sums ws ws_bytes fmt stream"),
    "nhwc_stats_from_partial": ("hiast_bn_nhwc_stats_from_partial", "partial nblk C sums stream"),
    "nhwc_apply": ("hiast_bn_nhwc_apply", "x res y gamma beta run_mean run_var sums count momentum eps relu save_mean save_invstd "
                                          "M C mask fmt stream"),
    "nhwc_apply_partial": ("hiast_bn_nhwc_apply_partial", "x res y gamma beta run_mean run_var partial nblk count momentum eps "
                                                          "relu save_mean save_invstd M C mask fmt stream"),
    "nhwc_bwd_stats": ("hiast_bn_nhwc_bwd_stats", "dy y x gamma beta save_mean save_invstd relu M C sums ws ws_bytes fmt stream"),
    "nhwc_bwd_apply": ("hiast_bn_nhwc_bwd_apply", "dy y x gamma beta save_mean save_invstd sums count relu dx dres dgamma dbeta "
                                                  "M C fmt stream"),
    "stats": ("hiast_bn_stats", "x B C HW dtype part stream"),
    "apply": ("hiast_bn_act_apply", "x res y gamma beta run_mean run_var part npart count momentum eps relu save_mean save_invstd "
                                    "B C HW dtype stream"),
    "bwd_stats": ("hiast_bn_act_bwd_stats", "dy y x save_mean save_invstd relu B C HW dtype part stream"),
    "bwd_apply": ("hiast_bn_act_bwd_apply", "dy y x gamma save_mean save_invstd part npart count relu dx dres dgamma dbeta "
                                            "B C HW dtype stream"),
}
# pointers an entry refuses as NULL (E_ARG) whatever the other arguments are (hiast_bn_act_apply: in training mode; a NULL part
# selects inference, which wants the running statistics instead)
REQUIRED = {
    "nhwc_stats": "x sums ws", "nhwc_stats_from_partial": "partial sums", "nhwc_apply": "x y sums save_mean save_invstd",
    "nhwc_apply_partial": "x y partial save_mean save_invstd", "nhwc_bwd_stats": "dy x save_mean save_invstd sums ws",
    "nhwc_bwd_apply": "dy x save_mean save_invstd sums dx", "stats": "x part", "apply": "x y save_mean save_invstd",
    "bwd_stats": "dy x save_mean save_invstd part", "bwd_apply": "dy x save_mean save_invstd part dx",
}
# activation pointers an entry wants 16-byte aligned (E_RANGE otherwise); y only for the gate that reads it as activations
ALIGNED = {
    "nhwc_stats": "x", "nhwc_apply": "x res y", "nhwc_apply_partial": "x res y", "nhwc_bwd_stats": "dy x y",
    "nhwc_bwd_apply": "dy x y dx dres",
}
POINTERS = set("x res y gamma beta run_mean run_var sums save_mean save_invstd mask partial ws dy dx dres dgamma dbeta part "
               "stream".split())


def args_of(entry):
    return ENTRIES[entry][1].split()


def call(lib, entry, **kw):
    """kw: every argument of the entry by name; pointers as int addresses, device tensors or None"""
    fn, names = ENTRIES[entry]
    vals = []
    for n in names.split():
        v = kw[n]
        if n in POINTERS:
            v = ctypes.c_void_p(0 if v is None else (v if isinstance(v, int) else v.data_ptr()))
        vals.append(v)
    return getattr(lib, fn)(*vals)


def placeholders(entry, M=64, C=64, B=2, HW=64):
    """a valid argument set whose pointers are distinct 16-byte aligned addresses that are never dereferenced"""
    kw = {}
    for i, n in enumerate(args_of(entry)):
        kw[n] = 4096 * (i + 1) if n in POINTERS else 0
    kw.update(stream=None)
    for n, v in dict(M=M, C=C, B=B, HW=HW, fmt=BF16, dtype=1, count=float(M), npart=B, nblk=4, momentum=0.1, eps=1e-5, relu=1,
                     ws_bytes=1 << 30).items():
        if n in kw:
            kw[n] = v
    if "HW" in kw:
        kw["count"] = float(B * HW)
    return kw


def refused_calls(entry):
    """-> [(what, changed arguments, expected code)] for one entry; shared with the device test, which runs them on carved
    buffers"""
    names = args_of(entry)
    out = []
    for n in REQUIRED[entry].split():
        out.append(("null " + n, {n: None}, E_ARG))
    if "y" in names and "relu" in names and entry != "nhwc_apply" and entry != "nhwc_apply_partial" and entry != "apply":
        for gate in ((1, 3) if entry.startswith("nhwc_") else (1,)):
            out.append(("gate %d without y" % gate, {"y": None, "relu": gate}, E_ARG))
    if entry.startswith("nhwc_"):
        for C in (0, 4, 24, 4096):
            out.append(("C = %d" % C, {"C": C}, E_RANGE))
        if "fmt" in names:
            for fmt in (0, 2, 4, -1):
                out.append(("fmt %d" % fmt, {"fmt": fmt}, E_RANGE))
        if entry in ("nhwc_bwd_stats", "nhwc_bwd_apply"):
            for gate in (-1, 4):
                out.append(("gate %d" % gate, {"relu": gate}, E_RANGE))
        for n in ALIGNED.get(entry, "").split():
            out.append((n + " at addr+2", {n: "+2"}, E_RANGE))
        if "ws_bytes" in names:
            out.append(("workspace one byte short", {"ws_bytes": "need-1"}, E_WS))
        if "M" in names:
            out.append(("M = 0", {"M": 0}, E_ARG))
        if "count" in names:
            out.append(("count = 0", {"count": 0.0}, E_ARG))
    else:
        out.append(("dtype 3", {"dtype": 3}, E_RANGE))
        out.append(("dtype -1", {"dtype": -1}, E_RANGE))
        out.append(("B = 65536", {"B": 65536}, E_RANGE))
        out.append(("B = 0", {"B": 0}, E_ARG))
        if "count" in names:
            for cnt in (0.0, -1.0):
                out.append(("count = %g" % cnt, {"count": cnt}, E_ARG))
        if entry == "apply":
            out.append(("inference without running statistics", {"part": None, "run_mean": None}, E_ARG))
    return out


def apply_change(kw, change, need_ws):
    kw = dict(kw)
    for n, v in change.items():
        if v == "+2":
            kw[n] = (kw[n] if isinstance(kw[n], int) else kw[n].data_ptr()) + 2
        elif v == "need-1":
            kw[n] = need_ws - 1
        else:
            kw[n] = v
    return kw
