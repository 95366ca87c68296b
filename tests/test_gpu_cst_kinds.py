"""The consistency kinds of the fused self-training loss (cfg.cst_training.cst_loss.type 'CE', 'KLDIV', 'MSE';
hiast_st_loss_cst_fwd / _bwd, include/hiast_hip.h HIAST_CST_*) on the device: against oracle.losses_ref.registry_loss
(pinned to the reference, tests/golden/loss_registry.npz) on the upsampled tensors, against the reference's own outputs,
bit-equality of the SoftCE kind with the existing entries, the argument checks, and the public interface (segmentor paths,
trainer iterations eager and from the captured graph).

Bounds of (a) are those of tests/test_gpu_kernels.py::test_st_loss_fwd_bwd (same kernel family, same kind of oracle):
counts equal, numerator 2e-5 relative, gradient 1e-4 of its maximum."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import synth
import cst_kinds_util as U
from oracle import losses_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ (a) against the oracle
SHAPES = [(3, 19, 5, 9, 33, 65),        # odd bands, three images
          (1, 9, 7, 7, 50, 50),         # single image
          (3, 16, 4, 40, 9, 300),       # more than one block along X in both kernels: TI = 33, two tile columns, W > 256
          (2, 2, 6, 6, 6, 6)]           # identity upsample, smallest class count
COEF = (2.0, 0.3, 0.5, 0.5)             # the other three terms are live beside the consistency term
SEED = 5220                             # (seeds for which the arg-max gap condition holds on every shape; asserted below)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    B, C, h, w, H, W = shape
    z = synth.logits_lr(SEED, B, C, h, w, 2.5)
    zt = synth.logits_lr(SEED + 1, B, C, h, w, 2.5)
    plbl = synth.pseudo_labels(SEED + 2, B, H, W, C, 0.4, np.int64)
    return z, zt, plbl


@functools.lru_cache(maxsize=None)
def _expected(shape, kind, region):
    """float64 oracle, once per (shape, kind, region): numerator, count, d(Σ COEF_i loss_i)/d low-res logits, and whether
    the teacher's arg-max is safe in fp32"""
    B, C, h, w, H, W = shape
    z, zt, plbl = _inputs(shape)
    pl = torch.from_numpy(plbl)
    zl, zf, ztf = U.upsample_inputs(torch.from_numpy(z), torch.from_numpy(zt), (H, W))
    num, cnt, loss = U.expected(kind, zf, U.target_of(kind, ztf), pl, region)
    L = losses_ref.st_losses(zl, None, pl, (H, W), region, 1.0, 1.0, 1.0, 0.0)
    (COEF[0] * L["target_seg_loss"] + COEF[1] * L["kld_confident_loss"] + COEF[2] * L["ent_ignored_loss"]
     + COEF[3] * loss).backward()
    return num, cnt, zl.grad.numpy().copy(), U.argmax_gap_ok(ztf)


@pytest.mark.parametrize("ldt", [np.uint8, np.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("region", U.REGIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("kind", U.KINDS)
def test_sums_counts_gradient(K, kind, shape, region, ldt):
    B, C, h, w, H, W = shape
    z, zt, plbl = _inputs(shape)
    num, cnt, gref, gap_ok = _expected(shape, kind, region)
    if kind == "CE":
        assert gap_ok, "the two largest teacher logits are closer than 32 * 2^-23 * max|zt| somewhere: pick another seed"
    a, b, c = dev(z), dev(zt), dev(plbl.astype(ldt))
    sums = K.st_loss_fwd(a, b, c, H, W, region, cst_kind=kind)
    base = K.st_loss_fwd(a, b, c, H, W, region)
    got, want0 = sums.cpu().numpy(), base.cpu().numpy()
    print("%s %s %s: count %d / %d, numerator rel.err %.3g" % (kind, shape, region, got[6], cnt,
                                                                abs(got[3] - num) / abs(num)))
    for k in (0, 1, 2, 4, 5, 7):                                 # the other slots do not depend on the kind
        assert got[k].tobytes() == want0[k].tobytes(), k
    assert got[6] == cnt and cnt > 0
    assert abs(got[3] - num) <= 2e-5 * abs(num)
    coef = torch.tensor(COEF, dtype=torch.float32).cuda()
    d = K.st_loss_bwd(a, b, c, H, W, region, sums, coef, cst_kind=kind).cpu().numpy()
    err = np.abs(d - gref).max() / np.abs(gref).max()
    print("   gradient err / max %.3g" % err)
    assert err <= 1e-4


# --------------------------------------------------------------------------------- (b) against the reference's own outputs
@pytest.mark.parametrize("name", ["mse_refer_ign", "ce_refer_conf", "ce_refer_ign"])
def test_against_reference_outputs(K, golden, name):
    """tests/golden/loss_registry.npz: LOSS['MSE'] / LOSS['CE'] of the reference with refer_labels + region, value and
    gradient, 2 x 19 x 12 x 20 with an identity upsample.  The teacher logits are built so that the kernel's own softmax /
    arg-max reproduces the case's target: log(soft) for MSE, 10 x one-hot of the hard labels (255 -> 0, as the generator
    substitutes) for CE.  KLDIV has no such case: the fixture's KLDIV target is a tensor of normal deviates, not a
    distribution, and the kernel's target softmax(softmax(teacher logits)) — the double softmax of trainer + loss — cannot
    be made equal to softmax(target) from it."""
    from make_golden import LOSS_REGISTRY_CASES, loss_registry_inputs
    g = golden("loss_registry")
    _, kind, use_w, use_refer, region, ign = [c for c in LOSS_REGISTRY_CASES if c[0] == name][0]
    assert not use_w and use_refer and ign == 255
    z, hard, soft, refer, _ = loss_registry_inputs(name)
    B, C, H, W = z.shape
    if kind == "MSE":
        zt = np.log(soft).astype(np.float32)
    else:
        lbl = hard.copy()
        lbl[lbl == 255] = 0
        zt = (10.0 * np.eye(C, dtype=np.float32)[lbl]).transpose(0, 3, 1, 2).copy()
    a, b, c = dev(z), dev(zt), dev(refer)
    sums = K.st_loss_fwd(a, b, c, H, W, region, cst_kind=kind)
    s = sums.cpu().numpy()
    val, want = s[3] / s[6], float(g["val_" + name])
    print(name, val, want)
    assert abs(val - want) <= 2e-5 * abs(want)
    coef = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float32).cuda()
    d = K.st_loss_bwd(a, b, c, H, W, region, sums, coef, cst_kind=kind).cpu().numpy()
    gr = g["grad_" + name]
    assert np.abs(d - gr).max() <= 2e-4 * np.abs(gr).max()


# ------------------------------------------------------------------------------------------ (c) bits, (d) argument checks
def test_softce_kind_is_the_existing_path_and_all_kinds_repeat(K):
    B, C, h, w, H, W = 2, 19, 16, 32, 128, 256
    z = synth.logits_lr(5300, B, C, h, w, 2.5)
    zt = synth.logits_lr(5301, B, C, h, w, 2.5)
    plbl = synth.pseudo_labels(5302, B, H, W, C, 0.4, np.uint8)
    a, b, c = dev(z), dev(zt), dev(plbl)
    coef = torch.tensor([1, .1, 1, .5], dtype=torch.float32).cuda()
    s0 = K.st_loss_fwd(a, b, c, H, W, "ignored")
    d0 = K.st_loss_bwd(a, b, c, H, W, "ignored", s0, coef)
    s1 = K.st_loss_fwd(a, b, c, H, W, "ignored", cst_kind=0, cst_entry=True)
    d1 = K.st_loss_bwd(a, b, c, H, W, "ignored", s1, coef, cst_kind=0, cst_entry=True)
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    for kind in U.KINDS:
        r = []
        for _ in range(2):
            s = K.st_loss_fwd(a, b, c, H, W, "ignored", cst_kind=kind)
            r.append((s, K.st_loss_bwd(a, b, c, H, W, "ignored", s, coef, cst_kind=kind)))
        assert torch.equal(r[0][0].view(torch.int64), r[1][0].view(torch.int64)), kind
        assert torch.equal(r[0][1].view(torch.int32), r[1][1].view(torch.int32)), kind
        assert bool(torch.isfinite(r[0][1]).all()) and not torch.equal(r[0][1], d0), kind


def test_argument_checks(K):
    """an unknown kind is HIAST_E_RANGE (-2), a kind other than SoftCE without a teacher HIAST_E_ARG (-1); neither launches:
    the outputs keep their sentinel"""
    from hiast_amd import _lib
    lib = _lib.load()
    B, C, h, w, H, W = 1, 19, 4, 4, 8, 8
    z = dev(synth.logits_lr(5400, B, C, h, w, 2.5))
    plbl = dev(synth.pseudo_labels(5401, B, H, W, C, 0.4, np.uint8))
    ws = K.st_loss_workspace(B, C, h, w, H, W, z.device)
    sums = torch.full((8,), -7.0, dtype=torch.float64, device=z.device)
    d = torch.full_like(z, -7.0)
    coef = torch.ones(4, dtype=torch.float32, device=z.device)
    P, st = K._ptr, K._stream()
    geom = (0, B, C, h, w, H, W, 0)
    for kind, teacher, want in ((4, z, -2), (-1, z, -2), (1, None, -1), (3, None, -1)):
        assert lib.hiast_st_loss_cst_fwd(P(z), P(teacher), P(plbl), *geom, kind, P(sums), P(ws), ws.numel() * 8, st) == want
        assert lib.hiast_st_loss_cst_bwd(P(z), P(teacher), P(plbl), *geom, kind, P(sums), P(coef), P(d), P(ws),
                                         ws.numel() * 8, st) == want
    ok = sums.clone()                 # (the same call with a kind that needs no teacher goes through)
    assert lib.hiast_st_loss_cst_fwd(P(z), P(None), P(plbl), *geom, 0, P(ok), P(ws), ws.numel() * 8, st) == 0
    torch.cuda.synchronize()
    assert bool((ok != -7.0).all())
    assert bool((sums == -7.0).all()) and bool((d == -7.0).all())
    with pytest.raises(_lib.HiastLibraryError):
        K.st_loss_fwd(z, None, plbl, H, W, "ignored", cst_kind="MSE")


# ------------------------------------------------------------------------------------------- (e) the public interface
def _segmentor(kind):
    from hiast_amd.utils.default_config import get_default_cfg
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    c = get_default_cfg()
    c.model.type = "SelfTrainingSegmentor"
    c.cst_training.is_enabled = True
    c.cst_training.cst_loss.type = kind
    c.cst_training.cst_loss.weight = 0.5
    c.cst_training.cst_loss.region = "ignored"
    return MODEL["SelfTrainingSegmentor"](c)


@pytest.mark.parametrize("kind", U.KINDS)
def test_segmentor_paths_agree(K, kind):
    """compute_loss_lowres (fused, low-res logits) against the reference-compatible compute_loss on the same logits
    upsampled by upsample_logits, the target built as the reference's trainer builds it: the four losses within 2e-5
    relative, the gradients w.r.t. the low-res student logits within 2e-4 of their maximum"""
    from hiast_amd.sseg.models.segmentors.self_training_segmentor import upsample_logits
    seg = _segmentor(kind)
    B, C, h, w, H, W = 2, 19, 9, 17, 65, 129
    z = dev(synth.logits_lr(5500, B, C, h, w, 2.5))
    zt = dev(synth.logits_lr(5511, B, C, h, w, 2.5))
    plbl = dev(synth.pseudo_labels(5502, B, H, W, C, 0.4, np.int64))
    with torch.no_grad():
        zt_full = upsample_logits(zt, (H, W))
        target = zt_full.argmax(dim=1) if kind == "CE" else torch.softmax(zt_full, dim=1)
    if kind == "CE":
        assert U.argmax_gap_ok(zt_full.cpu())
    out = []
    for lowres in (True, False):
        zl = z.clone().requires_grad_(True)
        if lowres:
            L = seg.compute_loss_lowres(zl, plbl, (H, W), zt)
        else:
            L = seg.compute_loss(upsample_logits(zl, (H, W)), plbl, target)
        sum(L.values()).backward()
        out.append(({k: float(v.detach()) for k, v in L.items()}, zl.grad.cpu().numpy()))
    (La, ga), (Lb, gb) = out
    assert set(La) == set(Lb) == {"target_seg_loss", "kld_confident_loss", "ent_ignored_loss", "cst_loss"}
    for k in La:
        print(kind, k, La[k], Lb[k])
        assert np.isfinite(La[k]) and abs(La[k] - Lb[k]) <= 2e-5 * abs(Lb[k]), k
    assert np.abs(ga - gb).max() <= 2e-4 * np.abs(gb).max()


H_IMG, W_IMG, N_IMG = 400, 800, 8


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a target set with hand-written generator artefacts (pseudo-labels = the labels), as tests/test_gpu_device_aug.py"""
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    from hiast_amd.tools import synth_data
    root = str(tmp_path_factory.mktemp("cst_kinds"))
    cfg = synth_data.synthetic_cfg(root, n_train=N_IMG, n_val=1, h=H_IMG, w=W_IMG, upscale=4)
    pdir = cfg.pseudo_policy.save_dir
    os.makedirs(pdir, exist_ok=True)
    swc = {c: [] for c in range(19)}
    for e in json.load(open(cfg.dataset.target.json_path)):
        lbl = np.array(Image.open(os.path.join(cfg.dataset.target.image_dir, e["mask_name"])))
        stem = os.path.splitext(os.path.basename(e["image_name"]))[0]
        Image.fromarray(lbl).save(os.path.join(pdir, stem + "_pseudo_label.png"))
        for c in range(19):
            if (lbl == c).any():
                swc[c].append([os.path.basename(e["image_name"]), int((lbl == c).sum())])
    with open(os.path.join(pdir, "..", "samples_with_class.json"), "w") as f:
        json.dump(swc, f)
    np.save(os.path.join(pdir, "..", "class_mean_probabilities.npy"), np.linspace(0.55, 0.95, 19))
    torch.manual_seed(31)
    ck = os.path.join(root, "init.pth")
    torch.save(MODEL["SelfTrainingSegmentor"](cfg).state_dict(), ck)
    cfg.train.resume_from = ck
    cfg.train.amp_dtype = "bf16"
    cfg.trainer = "ConsistencySelfTrainingTrainer"
    cfg.dataset.target.pseudo_dir = pdir
    cfg.dataset.target.aug_type = ["MS", "CCA"]
    cfg.cst_training.is_enabled = True
    cfg.cst_training.cst_loss.weight = 0.5
    cfg.preprocessor.type = "CopyPaste"
    cfg.train.gpu_num, cfg.train.batch_size, cfg.train.total_iter = 1, 4, 1
    cfg.train.iter_report = cfg.train.iter_val = 10 ** 6
    cfg.train.lr = 3e-6
    cfg.work_dir = os.path.join(root, "work")
    return cfg


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize("kind", U.KINDS)
def test_trainer_iterations_eager_and_captured(K, world, kind, monkeypatch):
    """ConsistencySelfTrainingTrainer.train() with cst_loss.type = kind until GraphedTrainStep replays its captured graph
    (WARM eager iterations, then capture + replay): finite losses, and the replayed iteration's cst_loss bit-equal to the
    same iteration of a trainer with HIAST_GRAPH_TRAIN=0 started from the same state with the same seeds"""
    from hiast_amd.utils.registry.registries import TRAINER
    from hiast_amd.workflows.trainer.consistency_self_training_trainer import GraphedTrainStep
    n_iter = GraphedTrainStep.WARM + 1
    last = []
    for graphed in (True, False):
        monkeypatch.setenv("HIAST_GRAPH_TRAIN", "1" if graphed else "0")
        c = world.clone()
        c.cst_training.cst_loss.type = kind
        c.freeze()
        _seed(9)
        tr = TRAINER[c.trainer](c, 0)
        assert tr.graph_train_enabled() is graphed
        _seed(9)
        for _ in range(n_iter):
            out = tr.train()
            torch.cuda.synchronize()
            out = {k: v.detach().float().cpu().clone() for k, v in out.items()}
            assert "cst_loss" in out and all(bool(torch.isfinite(v).all()) for v in out.values()), out
        if graphed:
            assert tr._graphed_step.graph is not None, "the iteration was not captured"
        last.append(out)
        tr.t_iter = tr.t_loader = None
        del tr
    print(kind, {k: float(v) for k, v in last[0].items()})
    for k in last[0]:
        assert torch.equal(last[0][k].view(torch.int32), last[1][k].view(torch.int32)), k
