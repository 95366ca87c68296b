"""Host side of the weight-gradient entries (hiast_amd/csrc/wgrad.hip, wgrad_small.hip, stem_train.hip), without a GPU: which
calls are refused, with which code and in which order of the checks, and how many workspace bytes the size entries ask for.

Every launch-entry call below is REFUSED: the library returns before its first HIP call, so the operands are literal fake
addresses (non-NULL, 16-byte aligned unless a case says otherwise) that nothing dereferences.  Never add a case that the
library accepts: it would launch a kernel on those addresses.  Codes are literals: -1 = HIAST_E_ARG, -2 = HIAST_E_RANGE,
-3 = HIAST_E_WS.

The codes and sizes are RECORDED: they are what the library answered before wgrad.hip got its one job check (DESIGN.md,
"One job check, one reduce body"), with no device visible (the planners then split for 256 CUs, the MI355X's count) and
HIAST_WGROUP_RATIO unset.  A row that breaks two rules pins which check comes first in that entry; the single launch and
the grouped launch do NOT agree on that (the grouped entry plans — shapes and workspace — before it looks at the
operand pointers), and both orders are part of the C ABI's behaviour."""
import ctypes

import pytest

DY, XA, DW, WS = 0x10000, 0x20000, 0x30000, 0x40000
BF16, SPLIT, FP16 = 1, 2, 3
HUGE = 1 << 40                     # a workspace size no plan exceeds


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    lib = _lib.load()
    # the sizes below are those of a 256-CU plan: a CU reserve (or another chip) must fail here, not as forty wrong sizes
    assert lib.hiast_get_reserve_cus() == 0
    assert lib.hiast_device_cus() in (0, 256)
    return lib


# ---- hiast_conv_wgrad_nhwc / hiast_conv_wgrad_small_nhwc (same argument list) --------------------------------------------
CONV_ARGS = ("dy", "x", "dw", "B", "H", "W", "Cin", "Cout", "taps", "stride", "dil", "fmt", "ws", "ws_bytes", "stream")
# a 1x1 256 -> 256 weight gradient on one 16 x 32 map, bf16 rows, one split of 256 KiB.  NOT refused by itself.
WGRAD_BASE = dict(dy=DY, x=XA, dw=DW, B=1, H=16, W=32, Cin=256, Cout=256, taps=1, stride=1, dil=1, fmt=BF16, ws=WS,
                  ws_bytes=HUGE, stream=None)

WGRAD_REFUSED = [
    # one broken rule each
    ("fmt 0", dict(fmt=0), -2),
    ("split planes", dict(fmt=SPLIT), -2),
    ("dy NULL", dict(dy=None), -1),
    ("x NULL", dict(x=None), -1),
    ("dw NULL", dict(dw=None), -1),
    ("workspace NULL", dict(ws=None), -1),
    ("B 0", dict(B=0), -1),
    ("H 0", dict(H=0), -1),
    ("W -1", dict(W=-1), -1),
    ("stride 0", dict(stride=0), -1),
    ("dil 0", dict(dil=0), -1),
    ("3x3 dil 0", dict(taps=9, dil=0), -1),
    ("Cin % 256", dict(Cin=128), -2),
    ("Cin % 256, 384", dict(Cin=384), -2),
    ("Cout % 256", dict(Cout=64), -2),
    ("taps 3", dict(taps=3), -2),
    ("taps 0", dict(taps=0), -2),
    ("strided 1x1", dict(stride=2), -2),
    ("dy misaligned", dict(dy=DY + 8), -2),
    ("x misaligned", dict(x=XA + 2), -2),
    ("dw misaligned", dict(dw=DW + 4), -2),
    ("workspace misaligned", dict(ws=WS + 8), -2),
    ("dy of 2 GiB", dict(B=64, H=256, W=256, Cout=256), -2),                      # 2^22 pixels x 256 x 2 bytes
    ("x of 2 GiB", dict(B=8, H=256, W=256, Cin=2048), -2),
    ("x of 2 GiB, 3x3 stride 2 (the input map counts)", dict(B=8, H=256, W=256, Cin=2048, taps=9, stride=2), -2),
    ("M = 2^24", dict(B=1 << 16, H=16, W=16), -2),
    ("3x3: Wo 3", dict(taps=9, H=8, W=3), -2),
    ("3x3 stride 2: Wo 3", dict(taps=9, H=8, W=6, stride=2), -2),
    ("workspace one byte short", dict(ws_bytes=256 * 256 * 4 - 1), -3),
    ("workspace 0", dict(ws_bytes=0), -3),
    ("3x3 workspace one byte short", dict(taps=9, ws_bytes=9 * 256 * 256 * 4 - 1), -3),
    ("two splits, workspace for one", dict(H=32, ws_bytes=256 * 256 * 4), -3),     # M = 1024: 2 splits
    # two broken rules: the first check in the entry's order decides
    ("fmt before dy NULL", dict(fmt=0, dy=None), -2),
    ("fmt before workspace NULL", dict(fmt=SPLIT, ws=None), -2),
    ("fmt before B 0", dict(fmt=0, B=0), -2),
    ("x NULL before B 0 (same code)", dict(x=None, B=0), -1),
    ("dw NULL before Cin % 256", dict(dw=None, Cin=128), -1),
    ("workspace NULL before strided 1x1", dict(ws=None, stride=2), -1),
    ("dy NULL before dy-sized limits", dict(dy=None, B=1 << 16, H=16, W=16), -1),
    ("B 0 before Cin % 256", dict(B=0, Cin=128), -1),
    ("stride 0 before taps", dict(stride=0, taps=3), -1),
    ("dil 0 before x misaligned", dict(dil=0, x=XA + 8), -1),
    ("B 0 before dy misaligned", dict(B=0, dy=DY + 8), -1),
    ("H 0 before workspace misaligned", dict(H=0, ws=WS + 4), -1),
    ("Cout % 256 before short workspace", dict(Cout=64, ws_bytes=0), -2),
    ("M = 2^24 before short workspace", dict(B=1 << 16, H=16, W=16, ws_bytes=0), -2),
    ("3x3 Wo 3 before short workspace", dict(taps=9, H=8, W=3, ws_bytes=0), -2),
    ("dy misaligned before short workspace", dict(dy=DY + 8, ws_bytes=0), -2),
    ("workspace misaligned before short workspace", dict(ws=WS + 8, ws_bytes=255), -2),
]


@pytest.mark.parametrize("what,over,code", WGRAD_REFUSED, ids=[c[0] for c in WGRAD_REFUSED])
def test_conv_wgrad_refuses(lib, what, over, code):
    assert over and code in (-1, -2, -3)
    a = dict(WGRAD_BASE, **over)
    assert lib.hiast_conv_wgrad_nhwc(*[a[k] for k in CONV_ARGS]) == code


# a 1x1 64 -> 64 weight gradient on the same map (H, W: the INPUT map).  NOT refused by itself.
SMALL_BASE = dict(WGRAD_BASE, Cin=64, Cout=64)

SMALL_REFUSED = [
    ("stride 0", dict(stride=0), -2),
    ("strided 1x1 (the caller subsamples)", dict(stride=2), -2),
    ("fmt 0", dict(fmt=0), -2),
    ("split planes", dict(fmt=SPLIT), -2),
    ("dy NULL", dict(dy=None), -1),
    ("x NULL", dict(x=None), -1),
    ("dw NULL", dict(dw=None), -1),
    ("workspace NULL", dict(ws=None), -1),
    ("B 0", dict(B=0), -1),
    ("H -1 (the output map is 0 rows)", dict(H=-1), -1),
    ("W -3", dict(W=-3), -1),
    ("dil 0", dict(dil=0), -1),
    ("Cin 96", dict(Cin=96), -2),
    ("Cin 32", dict(Cin=32), -2),
    ("Cout 192", dict(Cout=192), -2),
    ("Cout 4096", dict(Cout=4096), -2),
    ("taps 3", dict(taps=3), -2),
    ("M = 2^24", dict(B=1 << 16, H=16, W=16), -2),
    ("dy misaligned", dict(dy=DY + 8), -2),
    ("x misaligned", dict(x=XA + 2), -2),
    ("dw misaligned", dict(dw=DW + 4), -2),
    ("workspace misaligned", dict(ws=WS + 8), -2),
    ("workspace one byte short", dict(ws_bytes=64 * 128 * 4 - 1), -3),
    ("workspace 0", dict(ws_bytes=0), -3),
    ("3x3 workspace 0", dict(taps=9, ws_bytes=0), -3),
    # two broken rules
    ("stride 0 before fmt (same code)", dict(stride=0, fmt=0), -2),
    ("strided 1x1 before dy NULL", dict(stride=2, dy=None), -2),
    ("stride 0 before B 0", dict(stride=0, B=0), -2),
    ("fmt before x NULL", dict(fmt=0, x=None), -2),
    ("fmt before dil 0", dict(fmt=SPLIT, dil=0), -2),
    ("dw NULL before Cin 96", dict(dw=None, Cin=96), -1),
    ("workspace NULL before M = 2^24", dict(ws=None, B=1 << 16, H=16, W=16), -1),
    ("B 0 before Cout 192", dict(B=0, Cout=192), -1),
    ("dil 0 before taps 3", dict(dil=0, taps=3), -1),
    ("B 0 before dy misaligned", dict(B=0, dy=DY + 8), -1),
    ("dil 0 before workspace misaligned", dict(dil=0, ws=WS + 8), -1),
    ("Cin 96 before short workspace", dict(Cin=96, ws_bytes=0), -2),
    ("x misaligned before short workspace", dict(x=XA + 8, ws_bytes=0), -2),
    ("workspace misaligned before short workspace", dict(ws=WS + 4, ws_bytes=0), -2),
]


@pytest.mark.parametrize("what,over,code", SMALL_REFUSED, ids=[c[0] for c in SMALL_REFUSED])
def test_conv_wgrad_small_refuses(lib, what, over, code):
    assert over and code in (-1, -2, -3)
    a = dict(SMALL_BASE, **over)
    assert lib.hiast_conv_wgrad_small_nhwc(*[a[k] for k in CONV_ARGS]) == code


# ---- hiast_conv_wgrad_group_nhwc -----------------------------------------------------------------------------------------
JOB_FIELDS = ("dy", "x", "dw", "B", "H", "W", "Cin", "Cout", "taps", "stride", "dil")
# the job of WGRAD_BASE, and a 3x3 256 -> 256 job on the same map.  NOT refused, alone or together.
JOB1 = dict(dy=DY, x=XA, dw=DW, B=1, H=16, W=32, Cin=256, Cout=256, taps=1, stride=1, dil=1)
JOB9 = dict(dy=DY + 0x100000, x=XA + 0x100000, dw=DW + 0x100000, B=1, H=16, W=32, Cin=256, Cout=256, taps=9, stride=1, dil=2)
GROUP_CALL = dict(fmt=BF16, ws=WS, ws_bytes=HUGE)
ONE_SPLIT_1, ONE_SPLIT_9 = 256 * 256 * 4, 9 * 256 * 256 * 4            # M = 512: one split per job

JOB_RULES = [
    # (what, fields of the bad job, fields of the call, code): one broken rule each
    ("fmt 0", {}, dict(fmt=0), -2),
    ("split planes", {}, dict(fmt=SPLIT), -2),
    ("workspace NULL", {}, dict(ws=None), -1),
    ("B 0", dict(B=0), {}, -1),
    ("H 0", dict(H=0), {}, -1),
    ("W -1", dict(W=-1), {}, -1),
    ("stride 0", dict(stride=0), {}, -1),
    ("dil 0", dict(dil=0), {}, -1),
    ("Cin % 256", dict(Cin=128), {}, -2),
    ("Cout % 256", dict(Cout=64), {}, -2),
    ("taps 3", dict(taps=3), {}, -2),
    ("strided 1x1", dict(taps=1, stride=2), {}, -2),
    ("dy of 2 GiB", dict(B=64, H=256, W=256), {}, -2),
    ("x of 2 GiB", dict(B=8, H=256, W=256, Cin=2048), {}, -2),
    ("M = 2^24", dict(B=1 << 16, H=16, W=16), {}, -2),
    ("3x3: Wo 3", dict(taps=9, H=8, W=3), {}, -2),
    ("3x3 stride 2: Wo 3", dict(taps=9, H=8, W=6, stride=2), {}, -2),
    ("more than 64 tiles (6 bits of the block map)", dict(Cin=2048, Cout=2048, taps=9), {}, -2),
    ("dy NULL", dict(dy=None), {}, -1),
    ("x NULL", dict(x=None), {}, -1),
    ("dw NULL", dict(dw=None), {}, -1),
    ("dy misaligned", dict(dy=DY + 8), {}, -2),
    ("x misaligned", dict(x=XA + 2), {}, -2),
    ("dw misaligned", dict(dw=DW + 4), {}, -2),
    ("workspace misaligned", {}, dict(ws=WS + 8), -2),
    ("workspace 0", {}, dict(ws_bytes=0), -3),
    # two broken rules: the grouped entry plans before it looks at the jobs' pointers
    ("fmt before workspace NULL", {}, dict(fmt=0, ws=None), -2),
    ("fmt before B 0", dict(B=0), dict(fmt=0), -2),
    ("workspace NULL before Cin % 256", dict(Cin=128), dict(ws=None), -1),
    ("B 0 before Cin % 256", dict(B=0, Cin=128), {}, -1),
    ("Cin % 256 before dy NULL", dict(Cin=128, dy=None), {}, -2),
    ("M = 2^24 before x NULL", dict(B=1 << 16, H=16, W=16, x=None), {}, -2),
    ("B 0 before dy misaligned", dict(B=0, dy=DY + 8), {}, -1),
    ("3x3 Wo 3 before short workspace", dict(taps=9, H=8, W=3), dict(ws_bytes=0), -2),
    ("short workspace before dy NULL", dict(dy=None), dict(ws_bytes=0), -3),
    ("short workspace before dw misaligned", dict(dw=DW + 4), dict(ws_bytes=0), -3),
    ("short workspace before workspace misaligned", {}, dict(ws=WS + 8, ws_bytes=255), -3),
    ("dy NULL before x misaligned", dict(dy=None, x=XA + 8), {}, -1),
    ("dw NULL before workspace misaligned", dict(dw=None), dict(ws=WS + 8), -1),
]


def _group_call(lib, jobs, call):
    from hiast_amd import _lib
    arr = (_lib.WgradJob * len(jobs))(*[_lib.WgradJob(*[j[f] for f in JOB_FIELDS]) for j in jobs])
    c = dict(GROUP_CALL, **call)
    return lib.hiast_conv_wgrad_group_nhwc(ctypes.addressof(arr), len(jobs), c["fmt"], c["ws"], c["ws_bytes"], None)


@pytest.mark.parametrize("what,bad,call,code", JOB_RULES, ids=[c[0] for c in JOB_RULES])
def test_conv_wgrad_group_refuses(lib, what, bad, call, code):
    """the bad job alone, first of two and second of two"""
    assert (bad or call) and code in (-1, -2, -3)
    for jobs in ([dict(JOB1, **bad)], [dict(JOB1, **bad), JOB9], [JOB9, dict(JOB1, **bad)]):
        assert _group_call(lib, jobs, call) == code, len(jobs)


GROUP_REFUSED = [
    # rules of the group as a whole, and rows where BOTH jobs break a rule: the first job's decides within the plan, and the
    # plan of all jobs comes before any pointer
    ("jobs NULL", None, {}, -1),
    ("no job", [], {}, -1),
    ("five jobs", [JOB1] * 5, {}, -1),
    ("five jobs before a bad shape", [dict(JOB1, Cin=128)] * 5, {}, -1),
    ("fmt before five jobs", [JOB1] * 5, dict(fmt=0), -2),
    ("first job Cin % 256, second B 0", [dict(JOB1, Cin=128), dict(JOB9, B=0)], {}, -2),
    ("first job B 0, second Cin % 256", [dict(JOB1, B=0), dict(JOB9, Cin=128)], {}, -1),
    ("first job dy NULL, second Cin % 256", [dict(JOB1, dy=None), dict(JOB9, Cin=128)], {}, -2),
    ("first job dy misaligned, second dw NULL", [dict(JOB1, dy=DY + 8), dict(JOB9, dw=None)], {}, -1),
    ("first job dy NULL, second dw misaligned", [dict(JOB1, dy=None), dict(JOB9, dw=DW + 4)], {}, -1),
    ("workspace for the first job only", [JOB1, JOB9], dict(ws_bytes=ONE_SPLIT_1), -3),
    ("workspace one byte short of both", [JOB1, JOB9], dict(ws_bytes=ONE_SPLIT_1 + ONE_SPLIT_9 - 1), -3),
    ("one job, one byte short", [JOB9], dict(ws_bytes=ONE_SPLIT_9 - 1), -3),
]


@pytest.mark.parametrize("what,jobs,call,code", GROUP_REFUSED, ids=[c[0] for c in GROUP_REFUSED])
def test_conv_wgrad_group_refuses_as_a_whole(lib, what, jobs, call, code):
    if jobs is None:
        c = dict(GROUP_CALL, **call)
        assert lib.hiast_conv_wgrad_group_nhwc(None, 1, c["fmt"], c["ws"], c["ws_bytes"], None) == code
        assert lib.hiast_conv_wgrad_group_workspace_bytes(None, 1) == 0
    else:
        assert _group_call(lib, jobs, call) == code


# ---- hiast_stem_wgrad ----------------------------------------------------------------------------------------------------
STEM_ARGS = ("x", "dy", "dw", "fmt", "B", "H", "W", "ws", "ws_bytes", "stream")
STEM_BASE = dict(x=XA, dy=DY, dw=DW, fmt=BF16, B=1, H=32, W=64, ws=WS, ws_bytes=HUGE, stream=None)        # NOT refused
STEM_REFUSED = [
    ("x NULL", dict(x=None), -1),
    ("dy NULL", dict(dy=None), -1),
    ("dw NULL", dict(dw=None), -1),
    ("workspace NULL", dict(ws=None), -1),
    ("fmt 0", dict(fmt=0), -2),
    ("split planes", dict(fmt=SPLIT), -2),
    ("dy misaligned", dict(dy=DY + 8), -2),
    ("workspace misaligned", dict(ws=WS + 4), -2),
    ("B 0", dict(B=0), -1),
    ("H 0", dict(H=0), -1),
    ("W -2", dict(W=-2), -1),
    ("an image batch of 2^31 elements", dict(B=1 << 17, H=64, W=128), -2),
    ("workspace 0", dict(ws_bytes=0), -3),
    ("workspace one byte short", dict(ws_bytes=4 * 64 * 7 * 32 * 4 - 1), -3),         # 2 x 2 tiles of 8 x 16 outputs
    # two broken rules
    ("x NULL before fmt", dict(x=None, fmt=0), -1),
    ("workspace NULL before dy misaligned", dict(ws=None, dy=DY + 8), -1),
    ("fmt before B 0", dict(fmt=SPLIT, B=0), -2),
    ("dy misaligned before B 0", dict(dy=DY + 8, B=0), -2),
    ("workspace misaligned before H 0", dict(ws=WS + 8, H=0), -2),
    ("B 0 before short workspace", dict(B=0, ws_bytes=0), -1),
    ("2^31 elements before short workspace", dict(B=1 << 17, H=64, W=128, ws_bytes=0), -2),
    ("workspace misaligned before short workspace", dict(ws=WS + 8, ws_bytes=0), -2),
]


@pytest.mark.parametrize("what,over,code", STEM_REFUSED, ids=[c[0] for c in STEM_REFUSED])
def test_stem_wgrad_refuses(lib, what, over, code):
    assert over and code in (-1, -2, -3)
    a = dict(STEM_BASE, **over)
    assert lib.hiast_stem_wgrad(*[a[k] for k in STEM_ARGS]) == code


# ---- workspace sizes -----------------------------------------------------------------------------------------------------
# (B, Ho, Wo, Cin, Cout, taps) -> bytes = splits x Cout x taps x Cin x 4.  The trunk's layer3 / layer4 shapes on the bench's
# map (8 x 64 x 128) and on one image, the maps of tests/test_gpu_conv_extents.py's exact cases, the entry's smallest maps,
# and the shapes that must give 0.  (The size entry knows the OUTPUT map only: it cannot see the limits that need the input
# map or the stride, and answers for shapes the launch then refuses.)
WS_SIZES = [
    ((8, 64, 128, 1024, 256, 1), 64 * 1024 * 256 * 4),
    ((8, 64, 128, 256, 256, 9), 28 * 9 * 256 * 256 * 4),
    ((8, 64, 128, 256, 1024, 1), 64 * 1024 * 256 * 4),
    ((8, 64, 128, 512, 256, 1), 64 * 512 * 256 * 4),
    ((8, 64, 128, 512, 1024, 1), 32 * 512 * 1024 * 4),
    ((8, 64, 128, 2048, 512, 1), 16 * 2048 * 512 * 4),
    ((8, 64, 128, 512, 512, 9), 7 * 9 * 512 * 512 * 4),
    ((8, 64, 128, 512, 2048, 1), 16 * 2048 * 512 * 4),
    ((8, 64, 128, 1024, 512, 1), 32 * 1024 * 512 * 4),
    ((8, 64, 128, 1024, 2048, 1), 8 * 1024 * 2048 * 4),
    ((8, 64, 128, 256, 512, 1), 64 * 256 * 512 * 4),
    ((1, 64, 128, 1024, 256, 1), 16 * 1024 * 256 * 4),                 # 8192 pixels: at most 16 ranges of 512
    ((1, 64, 128, 256, 256, 9), 16 * 9 * 256 * 256 * 4),
    ((1, 64, 128, 512, 512, 9), 7 * 9 * 512 * 512 * 4),
    ((1, 64, 128, 512, 2048, 1), 16 * 2048 * 512 * 4),
    ((1, 64, 128, 1024, 2048, 1), 8 * 1024 * 2048 * 4),
    ((1, 53, 107, 256, 256, 1), 11 * 256 * 256 * 4),                   # 5671 pixels: 11 ranges
    ((1, 53, 107, 256, 256, 9), 11 * 9 * 256 * 256 * 4),
    ((1, 53, 107, 512, 256, 1), 11 * 512 * 256 * 4),
    ((1, 53, 107, 512, 512, 9), 7 * 9 * 512 * 512 * 4),
    ((1, 128, 256, 256, 256, 1), 64 * 256 * 256 * 4),                  # one tile: the cap of 64 ranges
    ((2, 9, 4, 256, 256, 9), 9 * 256 * 256 * 4),
    ((1, 1, 1, 256, 256, 1), 256 * 256 * 4),
    ((1, 8, 3, 256, 256, 9), 9 * 256 * 256 * 4),                       # (Wo = 3: the launch refuses it)
    ((1 << 16, 16, 16, 256, 256, 1), 64 * 256 * 256 * 4),              # (M = 2^24: the launch refuses it)
    ((0, 64, 128, 256, 256, 1), 0),
    ((8, 0, 128, 256, 256, 1), 0),
    ((8, 64, -1, 256, 256, 1), 0),
    ((8, 64, 128, 128, 256, 1), 0),
    ((8, 64, 128, 256, 384, 1), 0),
    ((8, 64, 128, 256, 256, 3), 0),
    ((8, 64, 128, 256, 256, 0), 0),
    ((8, 64, 128, 64, 64, 9), 0),
]

# hiast_conv_wgrad_small_workspace_bytes(B, Ho, Wo, Cin, Cout, taps): the layers below 256 channels on the bench's maps
# (layer1 8 x 128 x 256, layer2 8 x 64 x 128) and on the ragged map of the small tests
SMALL_SIZES = [
    ((8, 128, 256, 64, 64, 1), 16777216),
    ((8, 128, 256, 64, 64, 9), 16384000),
    ((8, 128, 256, 64, 256, 1), 16777216),
    ((8, 128, 256, 256, 64, 1), 16777216),
    ((8, 128, 256, 256, 128, 1), 33554432),
    ((8, 64, 128, 256, 128, 1), 16777216),
    ((8, 64, 128, 128, 128, 9), 31850496),
    ((8, 64, 128, 128, 512, 1), 33554432),
    ((8, 64, 128, 512, 128, 1), 33554432),
    ((8, 64, 128, 128, 128, 1), 8388608),
    ((1, 27, 45, 64, 64, 1), 65536),
    ((1, 27, 45, 64, 64, 9), 327680),
    ((1, 27, 45, 64, 256, 1), 131072),
    ((1, 27, 45, 256, 64, 1), 131072),
    ((1, 27, 45, 128, 128, 9), 1179648),
    ((1, 27, 45, 128, 512, 1), 524288),
    ((8, 64, 128, 256, 256, 1), 33554432),                             # (a K9d shape: this entry takes it as well)
    ((0, 64, 128, 64, 64, 1), 0),
    ((8, 64, 128, 96, 64, 1), 0),
    ((8, 64, 128, 64, 192, 1), 0),
    ((8, 64, 128, 64, 4096, 1), 0),
    ((8, 64, 128, 64, 64, 3), 0),
    ((1 << 16, 16, 16, 64, 64, 1), 0),
]


def _l3(B, H, W):
    return [(B, H, W, 256, 1024, 1, 1, 1), (B, H, W, 256, 256, 9, 1, 2), (B, H, W, 1024, 256, 1, 1, 1)]


def _l4(B, H, W):
    return [(B, H, W, 512, 2048, 1, 1, 1), (B, H, W, 512, 512, 9, 1, 4), (B, H, W, 2048, 512, 1, 1, 1)]


# jobs (B, H, W, Cin, Cout, taps, stride, dil) -> bytes = Σ splits x Cout x taps x Cin x 4 with ONE split count per launch
# (HIAST_WGROUP_RATIO unset)
GROUP_SIZES = [
    (_l3(8, 64, 128), 15 * 17 * 65536 * 4),                            # 17 tiles x 15 ranges = 255 blocks
    (_l3(1, 64, 128), 15 * 17 * 65536 * 4),
    ([_l4(8, 64, 128)[0], _l4(8, 64, 128)[2]], 8 * 32 * 65536 * 4),    # layer4's 1x1 pair: 32 tiles x 8 ranges
    (_l4(8, 64, 128), 3 * 68 * 65536 * 4),
    (_l3(8, 64, 128)[:1], 64 * 4 * 65536 * 4),
    (_l3(8, 64, 128)[1:2], 28 * 9 * 65536 * 4),
    (_l3(8, 64, 128) + [(8, 64, 128, 512, 256, 1, 1, 1)], 13 * 19 * 65536 * 4),
    ([(1, 53, 107, 512, 256, 1, 1, 1), (1, 53, 107, 256, 256, 9, 1, 1)], 11 * 11 * 65536 * 4),
    ([(2, 13, 21, 512, 256, 1, 1, 1), (1, 21, 37, 256, 256, 9, 1, 2)], 1 * 11 * 65536 * 4),       # M = 546 and 777: one range
    ([], 0),
    (_l3(8, 64, 128) + _l3(8, 64, 128)[:2], 0),                        # five jobs
    ([(8, 64, 128, 2048, 2048, 9, 1, 1)], 0),                          # 576 tiles
    ([(8, 64, 128, 256, 256, 1, 2, 1)], 0),                            # strided 1x1
    ([(8, 64, 128, 256, 256, 1, 1, 1), (8, 64, 128, 128, 256, 1, 1, 1)], 0),
    ([(8, 64, 128, 256, 256, 1, 1, 1), (0, 64, 128, 256, 256, 1, 1, 1)], 0),
    ([(1, 8, 3, 256, 256, 9, 1, 1)], 0),                               # Wo = 3: the plan sees the whole job, unlike the single size entry
    ([(1 << 16, 16, 16, 256, 256, 1, 1, 1)], 0),
]


def test_workspace_sizes(lib):
    from hiast_amd import _lib
    for args, want in WS_SIZES:
        assert lib.hiast_conv_wgrad_workspace_bytes(*args) == want, args
    for args, want in SMALL_SIZES:
        assert lib.hiast_conv_wgrad_small_workspace_bytes(*args) == want, args
    for jobs, want in GROUP_SIZES:
        arr = (_lib.WgradJob * max(1, len(jobs)))(*[_lib.WgradJob(DY, XA, DW, *j) for j in jobs])
        assert lib.hiast_conv_wgrad_group_workspace_bytes(ctypes.addressof(arr), len(jobs)) == want, jobs
    # the stem: 64 x 7 x 32 floats per block, one block per 8 x 16 tile of the output map up to two per CU
    assert lib.hiast_stem_wgrad_workspace_bytes(1, 32, 64) == 4 * 64 * 7 * 32 * 4
    assert lib.hiast_stem_wgrad_workspace_bytes(2, 67, 101) == 2 * 5 * 4 * 64 * 7 * 32 * 4
    assert lib.hiast_stem_wgrad_workspace_bytes(8, 512, 1024) == 512 * 64 * 7 * 32 * 4
    for bad in ((0, 32, 64), (1, 0, 64), (1, 32, -1), (1 << 17, 64, 128)):
        assert lib.hiast_stem_wgrad_workspace_bytes(*bad) == 0
