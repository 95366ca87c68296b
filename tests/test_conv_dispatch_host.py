"""Host side of the trunk-convolution dispatch (hiast_amd/csrc/igemm.hip), without a GPU: which calls are refused, with which
code and in which order of the checks, and how many statistics rows the row-count entries promise.

Every launch-entry call below is REFUSED: the library returns before its first HIP call, so the operands are literal fake
addresses (non-NULL, 16-byte aligned unless a case says otherwise) that nothing dereferences.  Never add a case that the
library accepts: it would launch a kernel on those addresses.  Codes are literals: -1 = HIAST_E_ARG, -2 = HIAST_E_RANGE.

"M is no multiple of the output map" can only be reached from the C ABI through hiast_igemm_bn_act with stride -2 (the other
entries compute M from the map themselves); that case is in the table.

The tuning variables HIAST_IGEMM_* / HIAST_XCONV* are taken to be unset, as tests/test_abi.py takes them."""
import pytest

X, WP, Y, RES, GATE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
GAMMA, BETA, MEAN, VAR, STATS = 0x60000, 0x61000, 0x62000, 0x63000, 0x70000
BF16, SPLIT, FP16 = 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


# ---- hiast_igemm_bn_act --------------------------------------------------------------------------------------------------
BN_ACT_ARGS = ("x", "wp", "gamma", "beta", "mean", "var", "eps", "res", "relu", "y", "B", "H", "W", "Cin", "Cout", "taps", "stride",
               "dil", "fmt", "out_f32", "stats", "stats_rows", "res_gate", "gate_mask", "stream")
# a 1x1 64 -> 64 convolution on one 16 x 16 map (M = 256: one block row of the tile kernel), bf16 rows.  NOT refused by itself.
BN_ACT_BASE = dict(x=X, wp=WP, gamma=None, beta=None, mean=None, var=None, eps=1e-5, res=None, relu=0, y=Y, B=1, H=16, W=16,
                   Cin=64, Cout=64, taps=1, stride=1, dil=1, fmt=BF16, out_f32=0, stats=None, stats_rows=0, res_gate=None,
                   gate_mask=0, stream=None)
BN = dict(gamma=GAMMA, beta=BETA, mean=MEAN, var=VAR)
XCONV_SHAPE = dict(B=2, H=64, W=64, Cin=256, Cout=1024)            # M = 8192: the statistics launch goes to xconv

BN_ACT_REFUSED = [
    # one broken rule each
    ("fmt 0", dict(fmt=0), -2),
    ("fmt 4", dict(fmt=4), -2),
    ("x NULL", dict(x=None), -1),
    ("wp NULL", dict(wp=None), -1),
    ("y NULL", dict(y=None), -1),
    ("mean without var", dict(mean=MEAN), -1),
    ("B 0", dict(B=0), -1),
    ("H 0", dict(H=0), -1),
    ("Cin 0", dict(Cin=0), -1),
    ("Cout 0", dict(Cout=0), -1),
    ("K % 64", dict(Cin=96), -2),
    ("K % 64, split planes", dict(Cin=48, fmt=SPLIT), -2),
    ("N % 64", dict(Cout=96), -2),
    ("taps 3", dict(taps=3), -2),
    ("taps 0", dict(taps=0), -2),
    ("fp32 output with a residual", dict(out_f32=1, res=RES), -2),
    ("statistics with ReLU", dict(stats=STATS, stats_rows=1, relu=1), -2),
    ("statistics with a residual", dict(stats=STATS, stats_rows=1, res=RES), -2),
    ("statistics with BatchNorm", dict(stats=STATS, stats_rows=1, **BN), -2),
    ("statistics with split planes", dict(stats=STATS, stats_rows=1, fmt=SPLIT), -2),
    ("statistics with fp32 output", dict(stats=STATS, stats_rows=1, out_f32=1), -2),
    ("gate without residual", dict(res_gate=GATE, gate_mask=1), -2),
    ("gate with split planes", dict(res_gate=GATE, gate_mask=1, res=RES, fmt=SPLIT), -2),
    ("gate with ReLU", dict(res_gate=GATE, gate_mask=1, res=RES, relu=1), -2),
    ("gate with BatchNorm", dict(res_gate=GATE, gate_mask=1, res=RES, **BN), -2),
    ("value gate misaligned", dict(res_gate=GATE + 8, gate_mask=0, res=RES), -2),
    ("x misaligned", dict(x=X + 8), -2),
    ("wp misaligned", dict(wp=WP + 4), -2),
    ("y misaligned", dict(y=Y + 2), -2),
    ("residual misaligned", dict(res=RES + 8), -2),
    ("strided 1x1", dict(stride=2), -2),
    ("3x3 dilation 0", dict(taps=9, dil=0), -1),
    ("3x3 dilation -1", dict(taps=9, dil=-1), -1),
    ("M no multiple of the output map (stride -2: H x W is the output map)", dict(taps=9, stride=-2), -1),
    ("stride -2 in split planes", dict(taps=9, stride=-2, fmt=SPLIT), -1),
    ("M beyond 2^31 - 512", dict(B=32768, H=256, W=256), -2),
    ("operand of 2 GiB", dict(B=8, H=256, W=256, Cin=2048), -2),
    ("operand of 2 GiB, 3x3 stride 2 (input map counts)", dict(B=8, H=256, W=256, Cin=2048, taps=9, stride=2), -2),
    ("weight of 2 GiB", dict(Cin=16384, Cout=16384, taps=9), -2),
    ("statistics rows: tile kernel writes 1", dict(stats=STATS, stats_rows=2), -1),
    ("statistics rows: 0", dict(stats=STATS, stats_rows=0), -1),
    ("statistics rows: xconv never writes 7 (a multiple of 8)", dict(stats=STATS, stats_rows=7, **XCONV_SHAPE), -1),
    ("statistics rows: xconv, fp16", dict(stats=STATS, stats_rows=7, fmt=FP16, **XCONV_SHAPE), -1),
    # two broken rules: the first check in the library's order decides
    ("B 0 before strided 1x1", dict(B=0, stride=2), -1),
    ("strided 1x1 before x NULL", dict(stride=2, x=None), -2),
    ("strided 1x1 before fmt", dict(stride=2, fmt=0), -2),
    ("fmt before x NULL", dict(fmt=0, x=None), -2),
    ("statistics with ReLU before x NULL", dict(stats=STATS, stats_rows=1, relu=1, x=None), -2),
    ("statistics with BatchNorm before mean without var", dict(stats=STATS, stats_rows=1, mean=MEAN), -2),
    ("gate without residual before mean without var", dict(res_gate=GATE, gate_mask=1, mean=MEAN), -2),
    ("gate with BatchNorm before y NULL", dict(res_gate=GATE, gate_mask=1, res=RES, y=None, **BN), -2),
    ("x NULL before K % 64", dict(x=None, Cin=96), -1),
    ("mean without var before N % 64", dict(mean=MEAN, Cout=96), -1),
    ("Cin 0 before taps", dict(Cin=0, taps=3), -1),
    ("taps before dilation", dict(taps=3, dil=0), -2),
    ("N % 64 before dilation", dict(Cout=96, taps=9, dil=0), -2),
    ("fp32 output with a residual before dilation", dict(out_f32=1, res=RES, taps=9, dil=0), -2),
    ("x misaligned before dilation", dict(x=X + 8, taps=9, dil=0), -2),
    ("x misaligned before the stride -2 map", dict(x=X + 8, taps=9, stride=-2), -2),
    ("dilation before operand of 2 GiB", dict(B=8, H=256, W=256, Cin=2048, taps=9, dil=0), -1),
    ("operand of 2 GiB before statistics rows", dict(B=8, H=256, W=256, Cin=2048, stats=STATS, stats_rows=0), -2),
    ("y misaligned before statistics rows", dict(y=Y + 8, stats=STATS, stats_rows=2), -2),
]


@pytest.mark.parametrize("what,over,code", BN_ACT_REFUSED, ids=[c[0] for c in BN_ACT_REFUSED])
def test_igemm_bn_act_refuses(lib, what, over, code):
    assert over and code in (-1, -2)
    a = dict(BN_ACT_BASE, **over)
    assert lib.hiast_igemm_bn_act(*[a[k] for k in BN_ACT_ARGS]) == code


def test_launch_checks_the_row_count_of_the_form_it_takes(lib):
    """1024 -> 256 on M = 4096 (16 tiles of 256 rows): the thread's tile-form hint decides between 16 rows of 256 and 32 of 128,
    and the launch refuses the row count of the OTHER form (it uses the same rule as hiast_igemm_stats_rows)"""
    shape = dict(B=1, H=64, W=64, Cin=1024, Cout=256, stats=STATS)
    try:
        for half, rows, other in ((1, 32, 16), (0, 16, 32)):
            lib.hiast_igemm_set_half(half)
            assert lib.hiast_igemm_stats_rows(4096, 1024, 256, 1, BF16) == rows
            a = dict(BN_ACT_BASE, stats_rows=other, **shape)
            assert lib.hiast_igemm_bn_act(*[a[k] for k in BN_ACT_ARGS]) == -1
    finally:
        lib.hiast_igemm_set_half(-1)


# ---- hiast_igemm_dgrad_bn_stats ------------------------------------------------------------------------------------------
DGRAD_BN_ARGS = ("dy", "wpt", "da", "B", "H", "W", "Cin", "Cout", "taps", "dil", "bn_x", "gamma", "beta", "save_mean", "save_invstd",
                 "partial", "partial_rows", "fmt", "stream")
DGRAD_BN_BASE = dict(dy=X, wpt=WP, da=Y, B=1, H=16, W=16, Cin=64, Cout=64, taps=1, dil=1, bn_x=RES, gamma=GAMMA, beta=BETA,
                     save_mean=MEAN, save_invstd=VAR, partial=STATS, partial_rows=1, fmt=BF16, stream=None)      # NOT refused
DGRAD_BN_REFUSED = [
    ("split planes", dict(fmt=SPLIT), -2),
    ("fmt 0", dict(fmt=0), -2),
    ("B 0", dict(B=0), -1),
    ("bn_x NULL", dict(bn_x=None), -1),
    ("save_mean NULL", dict(save_mean=None), -1),
    ("save_invstd NULL", dict(save_invstd=None), -1),
    ("partial NULL", dict(partial=None), -1),
    ("save_mean misaligned", dict(save_mean=MEAN + 4), -2),
    ("gamma misaligned", dict(gamma=GAMMA + 8), -2),
    ("Cout % 8", dict(Cout=68), -2),
    ("dy NULL", dict(dy=None), -1),
    ("da NULL", dict(da=None), -1),
    ("Cin % 64", dict(Cin=96), -2),
    ("Cout % 64", dict(Cout=96), -2),
    ("taps 3", dict(taps=3), -2),
    ("bn_x misaligned", dict(bn_x=RES + 8), -2),
    ("3x3 dilation 0", dict(taps=9, dil=0), -1),
    ("operand of 2 GiB", dict(B=8, H=256, W=256, Cin=2048), -2),
    ("partial rows: the tile kernel writes 1", dict(partial_rows=3), -1),
    ("partial rows: 0", dict(partial_rows=0), -1),
    ("fmt before B 0", dict(fmt=SPLIT, B=0), -2),
    ("B 0 before bn_x NULL", dict(B=0, bn_x=None), -1),
    ("bn_x NULL before save_mean misaligned", dict(bn_x=None, save_mean=MEAN + 4), -1),
    ("beta misaligned before dy NULL", dict(beta=BETA + 4, dy=None), -2),
    ("Cout % 8 before dy NULL", dict(Cout=68, dy=None), -2),
    ("dy NULL before Cin % 64", dict(dy=None, Cin=96), -1),
    ("bn_x misaligned before dilation", dict(bn_x=RES + 8, taps=9, dil=0), -2),
    ("dilation before partial rows", dict(taps=9, dil=0, partial_rows=3), -1),
]


@pytest.mark.parametrize("what,over,code", DGRAD_BN_REFUSED, ids=[c[0] for c in DGRAD_BN_REFUSED])
def test_igemm_dgrad_bn_stats_refuses(lib, what, over, code):
    assert over and code in (-1, -2)
    a = dict(DGRAD_BN_BASE, **over)
    assert lib.hiast_igemm_dgrad_bn_stats(*[a[k] for k in DGRAD_BN_ARGS]) == code


# ---- hiast_igemm_dgrad_s2 ------------------------------------------------------------------------------------------------
DGRAD_S2_ARGS = ("dy", "wpt", "dx", "B", "H", "W", "Cin", "Cout", "fmt", "stream")
DGRAD_S2_BASE = dict(dy=X, wpt=WP, dx=Y, B=1, H=16, W=16, Cin=64, Cout=64, fmt=BF16, stream=None)                 # NOT refused
DGRAD_S2_REFUSED = [
    ("split planes", dict(fmt=SPLIT), -2),
    ("fmt 4", dict(fmt=4), -2),
    ("B 0", dict(B=0), -1),
    ("W 0", dict(W=0), -1),
    ("dy NULL", dict(dy=None), -1),
    ("wpt NULL", dict(wpt=None), -1),
    ("dx NULL", dict(dx=None), -1),
    ("Cout % 64 (the reduction)", dict(Cout=96), -2),
    ("Cin % 64 (the output channels)", dict(Cin=96), -2),
    ("Cin 0", dict(Cin=0), -1),
    ("dx misaligned", dict(dx=Y + 8), -2),
    ("operand of 2 GiB (the half-size map counts)", dict(B=8, H=512, W=512, Cout=2048), -2),
    ("fmt before B 0", dict(fmt=SPLIT, B=0), -2),
    ("B 0 before dy NULL", dict(B=0, dy=None), -1),
    ("dy NULL before Cout % 64", dict(dy=None, Cout=96), -1),
]


@pytest.mark.parametrize("what,over,code", DGRAD_S2_REFUSED, ids=[c[0] for c in DGRAD_S2_REFUSED])
def test_igemm_dgrad_s2_refuses(lib, what, over, code):
    assert over and code in (-1, -2)
    a = dict(DGRAD_S2_BASE, **over)
    assert lib.hiast_igemm_dgrad_s2(*[a[k] for k in DGRAD_S2_ARGS]) == code


# ---- row counts ----------------------------------------------------------------------------------------------------------
def tile_rows(M, Cout, taps, half, cosched):
    """block rows of the tile kernel for a statistics launch: 256-row tiles, or 128 x 128 tiles for the 1x1 launches with
    Cout % 128 == 0 and M >= 4096 that the hint forces there, or, without a hint, that leave the chip at most a quarter full
    (<= 64 tiles of 256 rows) or at most half full when the thread does not co-schedule two launch sequences"""
    bm = 256
    if taps == 1 and Cout % 128 == 0 and M >= 4096:
        tiles = -(-M // 256) * (Cout // 256 if Cout % 256 == 0 else Cout // 128)
        if half == 1 or (half == -1 and (tiles <= 64 or (tiles <= 128 and cosched != 1))):
            bm = 128
    return -(-M // bm)


def xconv_rows(lib, M, Cout):
    """panel streams of xconv (the relations of tests/test_abi.py): the planned CUs over the 512-column groups, in whole rounds
    of the 8 XCDs, at least 8, and no more than the 64-row panels need"""
    cus = (lib.hiast_device_cus() if lib.hiast_device_cus() >= 8 else 256) - lib.hiast_get_reserve_cus()
    streams = max(8, cus // (Cout // 512) // 8 * 8)
    panels = -(-M // 64)
    return min(streams, (panels + 7) // 8 * 8)


MS = (4095, 4096, 4160, 32768, 65536)
SHAPES = ((64, 64), (128, 128), (256, 1024), (1024, 256), (512, 640))


@pytest.mark.parametrize("cosched", (-1, 1))
@pytest.mark.parametrize("half", (-1, 0, 1))
def test_row_counts(lib, half, cosched):
    try:
        lib.hiast_igemm_set_half(half)
        lib.hiast_igemm_set_cosched(cosched)
        for M in MS:
            for Cin, Cout in SHAPES:
                for taps in (1, 9):
                    want = tile_rows(M, Cout, taps, half, cosched)
                    assert lib.hiast_igemm_dgrad_bn_stats_rows(M, Cin, Cout, taps) == want, (M, Cin, Cout, taps)
                    for fmt in (BF16, SPLIT, FP16):
                        # the expanding 1x1 shape on 16-bit rows from 4096 pixels on: xconv, whatever the hints say
                        xconv = fmt != SPLIT and taps == 1 and Cin == 256 and Cout % 512 == 0 and M >= 4096
                        got = lib.hiast_igemm_stats_rows(M, Cin, Cout, taps, fmt)
                        assert got == (xconv_rows(lib, M, Cout) if xconv else want), (M, Cin, Cout, taps, fmt)
    finally:
        lib.hiast_igemm_set_half(-1)
        lib.hiast_igemm_set_cosched(-1)


def test_row_counts_literals(lib):
    """a few entries of the grid above as plain numbers (hints unset), and the degenerate arguments"""
    assert lib.hiast_igemm_stats_rows(4095, 1024, 256, 1, BF16) == 16          # below 4096 pixels: 256-row tiles
    assert lib.hiast_igemm_stats_rows(4096, 1024, 256, 1, BF16) == 32          # 16 tiles: a quarter of the chip, 128-row tiles
    assert lib.hiast_igemm_stats_rows(4160, 1024, 256, 1, FP16) == 33
    assert lib.hiast_igemm_stats_rows(32768, 1024, 256, 1, BF16) == 256        # 128 tiles, alone: 128-row tiles
    assert lib.hiast_igemm_stats_rows(65536, 1024, 256, 1, BF16) == 256        # 256 tiles: 256-row tiles
    assert lib.hiast_igemm_stats_rows(4096, 1024, 256, 9, BF16) == 16          # 3x3: never
    assert lib.hiast_igemm_stats_rows(4096, 512, 640, 1, BF16) == 32           # 640 = 5 x 128: 80 tiles, 128-row tiles alone
    assert lib.hiast_igemm_stats_rows(4096, 64, 64, 1, BF16) == 16             # 64 columns: no 128 x 128 form
    assert lib.hiast_igemm_stats_rows(4096, 256, 1024, 1, SPLIT) == 32         # split planes: not xconv
    assert lib.hiast_igemm_dgrad_bn_stats_rows(4096, 256, 1024, 1) == 32       # the backward-statistics launch never goes to xconv
    assert lib.hiast_igemm_dgrad_bn_stats_rows(65536, 256, 1024, 1) == 256
    for bad in ((0, 64, 64), (-5, 64, 64), (4096, 0, 64), (4096, 64, 0)):
        assert lib.hiast_igemm_stats_rows(bad[0], bad[1], bad[2], 1, BF16) == 0
    assert lib.hiast_igemm_dgrad_bn_stats_rows(0, 64, 64, 1) == 0
