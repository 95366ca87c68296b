"""The loss and discriminator-input entries of the C ABI (st_loss.hip, dinput.hip) by argument NAME (a plain helper module): one
table, used by the host-side tests (placeholder addresses, nothing is launched) and by the guard-band tests on the device (carved
buffers).  Pointers are int addresses, device tensors or None."""
import ctypes

E_ARG, E_RANGE, E_WS = -1, -2, -3
SOFTCE, CE, KLDIV, MSE = 0, 1, 2, 3                  # HIAST_CST_*
REGIONS = ("ignored", "confident", "all")            # region 0, 1, 2
IGNORE = 255

_LOSS = "logits teacher plbl is_i64 B C h w H W region "
ENTRIES = {
    "fwd": ("hiast_st_loss_fwd", _LOSS + "sums ws ws_bytes stream"),
    "bwd": ("hiast_st_loss_bwd", _LOSS + "sums coef dlogits ws ws_bytes stream"),
    "cst_fwd": ("hiast_st_loss_cst_fwd", _LOSS + "kind sums ws ws_bytes stream"),
    "cst_bwd": ("hiast_st_loss_cst_bwd", _LOSS + "kind sums coef dlogits ws ws_bytes stream"),
    "ws_bytes": ("hiast_st_loss_workspace_bytes", "B C h w H W"),
    "dinput_fwd": ("hiast_dinput_fwd", "logits mode out B C h w H W stream"),
    "dinput_bwd": ("hiast_dinput_bwd", "logits mode gout scratch dlogits B C h w H W stream"),
    "up_bwd": ("hiast_upsample_bilinear_ac_bwd", "gout gin B C h w H W stream"),
}
# eight symbols: the seven of st_loss.hip / dinput.hip and hiast_upsample_bilinear_ac_bwd, which hiast_dinput_bwd ends in
# (scratch -> dlogits)
ALL_SYMBOLS = sorted(fn for fn, _ in ENTRIES.values())
POINTERS = set("logits teacher plbl sums coef dlogits ws out gout scratch gin stream".split())


def args_of(entry):
    return ENTRIES[entry][1].split()


def call(lib, entry, **kw):
    """kw: every argument of the entry by name"""
    fn, names = ENTRIES[entry]
    vals = []
    for n in names.split():
        v = kw[n]
        if n in POINTERS:
            v = ctypes.c_void_p(0 if v is None else (v if isinstance(v, int) else v.data_ptr()))
        vals.append(v)
    return getattr(lib, fn)(*vals)


def workspace_bytes(lib, B, C, h, w, H, W):
    return int(lib.hiast_st_loss_workspace_bytes(B, C, h, w, H, W))


def loss_call(lib, bwd, cst_entry, **kw):
    """hiast_st_loss_fwd / _bwd, or the _cst_ entry of the same pass (which takes `kind`); kw may hold the arguments of both"""
    entry = ("cst_" if cst_entry else "") + ("bwd" if bwd else "fwd")
    assert cst_entry or kw.get("kind", 0) == 0
    return call(lib, entry, **{n: kw[n] for n in args_of(entry)})


def loss_refusals():
    """-> [(what, changed arguments, expected code, the changed geometry makes hiast_st_loss_workspace_bytes return 0)]: calls
    that loss_check / loss_geom / loss_dispatch of st_loss.hip refuse on the host, before any launch.  They start from a valid
    call with B = 1, C = 19, (h, w, H, W) = (2, 3, 4, 5), region 0, kind 0, a teacher, and a workspace of the valid call's
    size; ws_bytes "need": the size for the CHANGED extents (+ d)."""
    R, A, W_ = E_RANGE, E_ARG, E_WS
    return [
        ("w = 1, W = 257", dict(w=1, W=257), R, True),
        ("w = 2, W = 256", dict(w=2, W=256), R, True),
        ("(2,9,2,2034)", dict(h=2, w=9, H=2, W=2034), R, True),
        ("H < h", dict(h=5, H=4), R, True),
        ("W < w", dict(w=6, W=5), R, True),
        ("C = 3", dict(C=3), R, False),
        ("C = 20", dict(C=20), R, False),
        ("region 3", dict(region=3), R, False),
        ("region -1", dict(region=-1), R, False),
        ("kind 4", dict(kind=4), R, False),
        ("kind -1", dict(kind=-1), R, False),
        ("kind 1 without a teacher", dict(kind=1, teacher=None), A, False),
        ("kind 2 without a teacher", dict(kind=2, teacher=None), A, False),
        ("kind 3 without a teacher", dict(kind=3, teacher=None), A, False),
        ("B = 65536", dict(B=65536), R, False),
        ("B = 0", dict(B=0), A, False),
        ("workspace one byte short", dict(ws_bytes=("need", -1)), W_, False),
        ("workspace NULL", dict(ws=None), A, False),
        ("logits NULL", dict(logits=None), A, False),
        ("plbl NULL", dict(plbl=None), A, False),
        ("sums NULL", dict(sums=None), A, False),
        ("coef NULL", dict(coef=None), A, False),            # bwd only
        ("dlogits NULL", dict(dlogits=None), A, False),      # bwd only
    ]


LOSS_BASE = dict(is_i64=0, B=1, C=19, h=2, w=3, H=4, W=5, region=0, kind=0)


def dinput_refusals():
    """-> [(what, changed arguments, expected code)] from a valid call with B = 1, C = 19, (h, w, H, W) = (2, 3, 4, 5), mode 0"""
    return [
        ("mode 2", dict(mode=2), E_ARG),
        ("mode -1", dict(mode=-1), E_ARG),
        ("C = 3", dict(C=3), E_RANGE),
        ("B C = 65536", dict(B=4096, C=16), E_RANGE),
        ("H = 65536", dict(H=65536), E_RANGE),
        ("W = 0", dict(W=0), E_ARG),
        ("logits NULL", dict(logits=None), E_ARG),
        ("out / gout NULL", dict(out=None, gout=None), E_ARG),
        ("scratch NULL", dict(scratch=None), E_ARG),         # bwd only
        ("dlogits NULL", dict(dlogits=None), E_ARG),         # bwd only
    ]


DINPUT_BASE = dict(mode=0, B=1, C=19, h=2, w=3, H=4, W=5)
