"""Host side of the loss / discriminator-input tests (no GPU): the float64 reference of tests/loss_ref.py against torch float64 in
an independent formulation, its error bounds against a float32 restatement of the kernels' order (inside as written, outside for
six deliberate errors), the bounds against the tolerances the older tests use, a float32 restatement of loss_geom / band_start
swept over the geometries, and the argument checks of the entries (refusals happen before any launch, so placeholder addresses
are never dereferenced)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cst_kinds_util as CU
import head_ref
import loss_calls as LC
import loss_ref as R
import synth
from oracle import losses_ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    return _lib.load()


def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all()
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())


# ------------------------------------------------------------------------------------------------ weights and bands
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (1, 256), (2, 255), (9, 2033), (5, 42), (8, 24), (254, 254), (40, 300), (9, 65), (5, 33),
                                        (512, 711), (7, 4), (5, 3)])
def test_weights_are_those_of_src_of(n_in, n_out):
    """lerp_matrix64 holds head_ref.lerp_matrix's float32 weights; the one difference is a clamped cell (i0 == i1), whose l0 + l1
    head_ref rounds to float32 once more.  band_starts is band_start for every j, and a band is the rows that share i0."""
    m64, m32 = R.lerp_matrix64(n_in, n_out), head_ref.lerp_matrix(n_in, n_out).astype(np.float64)
    i0, i1, l0, l1 = R.src_of(n_in, n_out)
    merged = np.zeros_like(m64, bool)
    merged[np.arange(n_out)[i0 == i1], i0[i0 == i1]] = True
    assert np.array_equal(m64[~merged], m32[~merged]) and (np.abs(m64 - m32)[merged] <= R.U).all()
    assert ((i1 == i0) == (i0 == n_in - 1)).all() and (i0 >= 0).all() and (i1 <= n_in - 1).all()
    bs = R.band_starts(n_in, n_out)
    s = R.scale_of(n_in, n_out)
    assert [R.band_start(s, j, n_in, n_out) for j in range(n_in + 1)] == list(bs)
    assert (np.diff(bs) >= 0).all() and bs[0] == 0 and bs[-1] == n_out
    for j in range(n_in):
        assert (i0[bs[j]:bs[j + 1]] == j).all()


def test_clamped_column_with_a_weight_exists_only_above_the_last_cell():
    """x1 = x0 (the clamp at w - 1) carries a weight l1 != 0 only where float32 sw · (W - 1) lands ABOVE w - 1; on the first nine
    geometries it never does, on the two clamp geometries (512 -> 711) the last column / row has l1 = 2^-15"""
    for (h, w, H, W) in R.GEOMETRIES:
        if (h, w, H, W) in R.CLAMP_GEOMETRIES:
            continue
        for n_in, n_out in ((h, H), (w, W)):
            i0, i1, _, l1 = R.src_of(n_in, n_out)
            assert not l1[i0 == i1].any()
    assert set(R.CLAMP_GEOMETRIES) <= set(R.GEOMETRIES)
    i0, i1, _, l1 = R.src_of(512, 711)
    assert i0[-1] == i1[-1] == 511 and l1[-1] == np.float32(2.0 ** -15)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("region", [0, 1, 2])
def test_reference_equals_torch_float64(variant, region):
    """sums, counts and the gradient against F.interpolate + autograd in float64 (oracle/losses_ref.py for slots 0-2,
    cst_kinds_util.closed_form for the consistency kinds): 2e-6 relative, what torch's float64 weights differ from the float32
    ones by (1e-5 for the discriminator map below, whose small probabilities carry the logits' difference in full)"""
    name, kind, teacher, _ = variant
    B, C, h, w, H, W = 3, 9, 4, 5, 9, 14
    z, zt, lbl = R.loss_inputs(77, B, C, h, w, H, W)
    geo = R.Geometry(h, w, H, W)
    ref = R.loss_reference(geo, z, zt if teacher else None, lbl, kind, region, R.COEF)
    pl = torch.from_numpy(lbl.astype(np.int64))
    zl, zf, ztf = CU.upsample_inputs(torch.from_numpy(z), torch.from_numpy(zt), (H, W))
    s = losses_ref.st_loss_sums(zl, None, pl, (H, W), LC.REGIONS[region])
    if not teacher:
        num, cnt = torch.zeros((), dtype=torch.float64), 0.0
    elif kind == R.SOFTCE:
        m = CU.region_mask(pl, LC.REGIONS[region]).unsqueeze(1)
        t = -torch.log_softmax(zf, 1) * F.softmax(ztf, 1).double() * m
        num, cnt = t.sum(), float((t != 0).sum())
    else:
        num, cnt, _ = CU.closed_form(CU.KINDS[kind - 1], zf, ztf, pl, LC.REGIONS[region])
        cnt = float(cnt)
    want = [float(v.detach()) for v in (s["ce"], s["kld"], s["ent"], num, s["n_conf"], s["n_ign"])] + [cnt]
    assert np.array_equal(ref["sums"][4:], want[4:])
    np.testing.assert_allclose(ref["sums"][:4], want[:4], rtol=2e-6)
    c = R.COEF
    L = c[0] * s["ce"] / s["n_conf"] + c[1] * s["kld"] / (C * s["n_conf"]) + c[2] * s["ent"] / (C * s["n_ign"])
    if teacher:
        L = L + c[3] * num / cnt
    L.backward()
    np.testing.assert_allclose(ref["grad"], zl.grad.numpy(), rtol=2e-6, atol=2e-6 * float(zl.grad.abs().max()))
    assert (ref["grad_bound"] > 0).all() and (ref["sum_bound"][:3] > 0).all()


def test_dinput_reference_equals_torch_float64():
    from oracle import warmup_ref
    B, C, h, w, H, W = 2, 9, 4, 5, 9, 14
    z, g = synth.logits_lr(78, B, C, h, w, 3.0), synth.normal_f32(79, (B, C, H, W))
    geo = R.Geometry(h, w, H, W)
    for mode in (0, 1):
        ref = R.dinput_reference(geo, z, mode, g)
        zt = torch.from_numpy(z).double().requires_grad_(True)
        want = warmup_ref.discriminator_input(zt, (H, W), bool(mode))
        np.testing.assert_allclose(ref["out"], want.detach().numpy(), rtol=1e-5, atol=1e-9)
        want.backward(torch.from_numpy(g).double())
        np.testing.assert_allclose(ref["dlogits"], zt.grad.numpy(), rtol=1e-5, atol=1e-5 * float(zt.grad.abs().max()))
        assert (ref["out_bound"] > 0).all() and (ref["scratch_bound"] > 0).all()


# ------------------------------------------------------------------------------------------------ order restatement, mutants
def _case(geom, C, variant, region, coef=R.COEF, seed=None, p_ignore=0.4):
    name, kind, teacher, B = variant
    h, w, H, W = geom
    z, zt, lbl = R.loss_inputs(R.case_seed(geom, C) if seed is None else seed, B, C, h, w, H, W, p_ignore)
    zt = zt if teacher else None
    ref = R.loss_reference(R.Geometry(*geom), z, zt, lbl, kind, region)
    assert ref["gap_ok"] and ref["min_prod"] >= R.MIN_PROD, (geom, C, name, region)
    coef = R.usable_coef(ref["sums"], coef)
    ref = R.loss_reference(R.Geometry(*geom), z, zt, lbl, kind, region, coef)
    return (h, w, H, W, z, zt, lbl, kind, region, coef, ref["sums"]), ref


@pytest.mark.parametrize("geom", list(R.GEOMETRIES), ids=lambda g: "x".join(map(str, g)))
def test_kernel_order_in_float32_is_inside_the_bounds(geom):
    """every variant at the smallest and the largest class count, the region rotating; counts exact.  (512,2,711,3), whose 711
    rows the restatement walks one by one in Python, at C = 2 only: its 19-class kernels run on the device"""
    for C in ((2,) if geom[2] > 256 else (2, 19)):
        for variant in R.VARIANTS:
            region = (variant[1] + C + len(variant[0])) % 3
            args, ref = _case(geom, C, variant, region)
            sums, d = R.kernel_order_f32(*args)
            assert np.array_equal(sums[4:], ref["sums"][4:]), (geom, C, variant[0])
            assert _ratio(sums[:4], ref["sums"][:4], ref["sum_bound"]) <= 1.0, (geom, C, variant[0], "sums")
            assert _ratio(d, ref["grad"], ref["grad_bound"]) <= 1.0, (geom, C, variant[0], "gradient")


# mutant -> its named case: (geometry, C, variant index, region)
MUTANT_CASES = {
    "no_seam": ((4, 40, 9, 300), 19, 1, 2),                 # two tile blocks: cell 33 is shared
    "no_clamped_band": ((512, 2, 711, 3), 2, 1, 2),         # float32 sh · (H - 1) = 511 + 2^-15: the last row has l1 != 0 on row h - 1
    "x1_unclamped": ((2, 512, 2, 711), 2, 1, 2),            # the same for the last column
    "ent_no_H": ((5, 9, 33, 65), 19, 0, 0),
    "ce_own_mask": ((5, 9, 33, 65), 9, 2, 0),
    "kld_single_softmax": ((5, 9, 33, 65), 19, 3, 2),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_fall_outside_the_bounds(mutant):
    geom, C, vi, region = MUTANT_CASES[mutant]
    assert R.loss_geom(*geom) is not None
    assert geom in R.GEOMETRIES                             # every named case also runs on the device
    args, ref = _case(geom, C, R.VARIANTS[vi], region)
    sums, d = R.kernel_order_f32(*args)
    assert _ratio(sums[:4], ref["sums"][:4], ref["sum_bound"]) <= 1.0 and _ratio(d, ref["grad"], ref["grad_bound"]) <= 1.0
    sums_m, d_m = R.kernel_order_f32(*args, mutant=mutant)
    rg = _ratio(d_m, ref["grad"], ref["grad_bound"])
    assert rg > 1.0, (mutant, rg)
    if mutant in ("ce_own_mask", "kld_single_softmax"):     # these change the forward too
        assert _ratio(sums_m[3], ref["sums"][3], ref["sum_bound"][3]) > 1.0 or sums_m[6] != ref["sums"][6]


@pytest.mark.parametrize("mutant", ["x1_unclamped", "no_clamped_band"])
def test_clamp_mutants_pass_the_old_tolerance_and_miss_the_cell_bounds(mutant):
    """the reason for per-cell bounds: a clamp mutant is wrong by less than 1e-4 of the largest gradient, the tolerance of
    test_gpu_kernels.py::test_st_loss_fwd_bwd, and still outside the bound of the cells it touches"""
    geom, C, vi, region = MUTANT_CASES[mutant]
    args, ref = _case(geom, C, R.VARIANTS[vi], region)
    _, d = R.kernel_order_f32(*args, mutant=mutant)
    assert np.abs(d - ref["grad"]).max() <= 1e-4 * np.abs(ref["grad"]).max()
    bad = np.abs(d - ref["grad"]) > ref["grad_bound"]
    assert bad.any()
    last = bad[..., -1] if mutant == "x1_unclamped" else bad[:, :, -1]
    assert int(last.sum()) == int(bad.sum()), "cells other than the clamped column / row are outside their bounds"


def test_seam_mutant_is_wrong_in_the_shared_cell_only():
    """without the seam term of the combine only the column of the cell two tile blocks share is wrong (there by far more than
    any tolerance: the older test on its two-block shape sees it too)"""
    args, ref = _case((4, 40, 9, 300), 19, R.VARIANTS[1], 2)
    _, d = R.kernel_order_f32(*args, mutant="no_seam")
    bad = np.abs(d - ref["grad"]) > ref["grad_bound"]
    assert bad.any() and not bad[..., :33].any() and not bad[..., 34:].any()


@pytest.mark.parametrize("geom", list(R.GEOMETRIES), ids=lambda g: "x".join(map(str, g)))
def test_input_conditions_hold_for_every_device_case(geom):
    """what the device test asserts before it compares counts exactly, checked here first for every class count, variant and
    region it runs: no counted product below 1e-30 in float64, and the CE kind's arg-max gap"""
    geo = R.Geometry(*geom)
    for C in R.GEOMETRIES[geom]:
        for name, kind, teacher, B in R.VARIANTS:
            z, zt, lbl = R.loss_inputs(R.case_seed(geom, C), B, C, *geom)
            for region in range(3):
                ref = R.loss_reference(geo, z, zt if teacher else None, lbl, kind, region)
                assert ref["gap_ok"], (geom, C, name, region)
                assert ref["min_prod"] >= R.MIN_PROD, (geom, C, name, region, ref["min_prod"])
                assert np.isfinite(ref["sums"]).all() and (ref["sums"][4] + ref["sums"][5] == lbl.size)


# ------------------------------------------------------------------------------------------------ not looser than today
@pytest.mark.parametrize("shape", [(2, 19, 5, 9, 33, 65), (2, 19, 16, 32, 128, 256), (1, 9, 7, 7, 50, 50)])
@pytest.mark.parametrize("region", [0, 1, 2])
def test_bounds_are_at_or_below_the_older_tolerances(shape, region):
    """the inputs of test_gpu_kernels.py::test_st_loss_fwd_bwd: sums 2e-5 relative, gradient 1e-4 of its maximum"""
    B, C, h, w, H, W = shape
    z, zt = synth.logits_lr(700, B, C, h, w, 2.5), synth.logits_lr(701, B, C, h, w, 2.5)
    lbl = synth.pseudo_labels(702, B, H, W, C, 0.4, np.uint8)
    ref = R.loss_reference(R.Geometry(h, w, H, W), z, zt, lbl, R.SOFTCE, region, (2.0, 0.3, 0.5, 0.5))
    assert (ref["sum_bound"] <= 2e-5 * np.abs(ref["sums"][:4])).all(), ref["sum_bound"] / np.abs(ref["sums"][:4])
    assert ref["grad_bound"].max() <= 1e-4 * np.abs(ref["grad"]).max(), ref["grad_bound"].max() / np.abs(ref["grad"]).max()


# ------------------------------------------------------------------------------------------------ geometry
LARGEST_W = {1: 256, 2: 255, 3: 509, 4: 763, 5: 1017, 6: 1271, 7: 1525, 8: 1779, 9: 2033}


def test_geometry_sweep(lib):
    """every 1 <= w <= W <= 320: the restatement accepts what the library accepts, with the same workspace size; an accepted
    geometry keeps every tile block within 256 columns, the blocks tile [0, W) and every column's x0 lies in its block; a refused
    one has workspace_bytes == 0"""
    accepted = refused = 0
    for W in range(1, 321):
        for w in range(1, W + 1):
            g = R.loss_geom(2, w, 3, W)
            need = lib.hiast_st_loss_workspace_bytes(1, 19, 2, w, 3, W)
            assert need == R.workspace_bytes(1, 19, 2, w, 3, W), (w, W)
            if g is None:
                assert need == 0
                refused += 1
            else:
                assert need > 0
                R.check_tiling(w, W, g["TI"])
                accepted += 1
    assert accepted > 0 and refused > 0


def test_largest_accepted_width(lib):
    """the largest W the entries take for w = 1 .. 16 (pinned for w <= 9), the pairs around it, and their tiling"""
    for w in range(1, 17):
        ok = [W for W in range(w, 4200) if lib.hiast_st_loss_workspace_bytes(1, 2, 1, w, 1, W) > 0]
        assert ok == [W for W in range(w, 4200) if R.loss_geom(1, w, 1, W) is not None]
        top = max(ok)
        if w in LARGEST_W:
            assert top == LARGEST_W[w], (w, top)
        for W in (top - 1, top):
            if W >= w:
                g = R.loss_geom(1, w, 1, W)
                if g is not None:
                    R.check_tiling(w, W, g["TI"])
        assert R.loss_geom(1, w, 1, top + 1) is None and lib.hiast_st_loss_workspace_bytes(3, 19, 2, w, 2, top + 1) == 0
    assert R.loss_geom(2, 9, 2, 2033)["TI"] == 1 and R.loss_geom(2, 254, 2, 254) == dict(sh=1, sw=1, TI=253, nxb=2)
    assert R.Geometry(8, 5, 24, 42).empty_bands == (1, 1)
    for geom in R.GEOMETRIES:
        g = R.loss_geom(*geom)
        assert g is not None and R.check_tiling(geom[1], geom[3], g["TI"]) <= 256
    for h, w, H, W in [(5, 4, 4, 9), (4, 6, 9, 5)]:              # H < h, W < w: no size either
        assert R.loss_geom(h, w, H, W) is None and lib.hiast_st_loss_workspace_bytes(1, 19, h, w, H, W) == 0


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_exported_with_the_header_arity(lib):
    from hiast_amd import _lib
    from test_abi import declared_arity
    arity = declared_arity()
    assert len(LC.ALL_SYMBOLS) == 8 and len(LC.ENTRIES) == 8
    for fn, names in LC.ENTRIES.values():
        assert hasattr(lib, fn) and arity[fn] == len(names.split()) == len(_lib.SIGNATURES[fn][1]), fn


def _placeholders(entry, base):
    kw = {n: 4096 * (i + 1) if n in LC.POINTERS else 0 for i, n in enumerate(LC.args_of(entry))}
    kw.update({k: v for k, v in base.items() if k in kw}, stream=None)
    return kw


@pytest.mark.parametrize("entry", ["fwd", "bwd", "cst_fwd", "cst_bwd"])
def test_loss_entries_refuse_before_any_launch(lib, entry):
    base = _placeholders(entry, LC.LOSS_BASE)
    dims = lambda kw: [kw[n] for n in "B C h w H W".split()]
    base["ws_bytes"] = LC.workspace_bytes(lib, *dims(base))
    assert base["ws_bytes"] > 0
    n = 0
    for what, change, code, zero_ws in LC.loss_refusals():
        if any(k not in base for k in change):
            continue                                         # an argument this entry does not take
        kw = dict(base, **{k: v for k, v in change.items() if k != "ws_bytes"})
        need = LC.workspace_bytes(lib, *dims(kw))
        assert (need == 0) == zero_ws, (what, need)
        if isinstance(change.get("ws_bytes"), tuple):
            kw["ws_bytes"] = need + change["ws_bytes"][1]
        elif 0 < need < (1 << 30):
            kw["ws_bytes"] = need
        assert LC.call(lib, entry, **kw) == code, (entry, what)
        n += 1
    assert n >= 15


@pytest.mark.parametrize("entry", ["dinput_fwd", "dinput_bwd"])
def test_dinput_entries_refuse_before_any_launch(lib, entry):
    base = _placeholders(entry, LC.DINPUT_BASE)
    n = 0
    for what, change, code in LC.dinput_refusals():
        if not any(k in base for k in change):
            continue
        assert LC.call(lib, entry, **dict(base, **{k: v for k, v in change.items() if k in base})) == code, (entry, what)
        n += 1
    assert n >= 7
