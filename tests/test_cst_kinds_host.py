"""The consistency kinds of the fused loss on the CPU: the per-(image, pixel) closed forms that the HIP kernel implements
(M-weighted CE, double-softmax KLDIV, raw-logit MSE and their gradients; include/hiast_hip.h HIAST_CST_*) against
oracle.losses_ref.registry_loss + autograd, which is pinned to the reference's own outputs — this proves the separation of
CE's [B,B,H,W] broadcast (losses.py:86-87) before any kernel runs — and the host-side mapping of cst_loss.type."""
import numpy as np
import pytest
import torch

import synth
import cst_kinds_util as U

B, C, H, W = 3, 19, 12, 20


@pytest.fixture(scope="module")
def inputs():
    z = torch.from_numpy(synth.normal_f32(4100, (B, C, H, W), 2.5)).double()
    zt = torch.from_numpy(synth.normal_f32(4101, (B, C, H, W), 2.5))
    plbl = torch.from_numpy(synth.pseudo_labels(4102, B, H, W, C, 0.4, np.int64))     # ~40 % ignored, per image
    return z, zt, plbl


def test_labels_give_every_M(inputs):
    """M (images of the batch whose mask holds at a pixel position) takes every value 0..B in both label regions"""
    _, _, plbl = inputs
    for region in ("ignored", "confident"):
        assert sorted(set(U.region_mask(plbl, region).sum(0).flatten().tolist())) == list(range(B + 1))


@pytest.mark.parametrize("region", U.REGIONS)
@pytest.mark.parametrize("kind", U.KINDS)
def test_closed_forms_match_the_registry_oracle(inputs, kind, region):
    z, zt, plbl = inputs
    zl = z.clone().requires_grad_(True)
    target = U.target_of(kind, zt)
    num, cnt, loss = U.expected(kind, zl, target, plbl, region)
    loss.backward()
    n, c, g = U.closed_form(kind, z, zt, plbl, region)
    assert int(c) == cnt and cnt > 0
    assert abs(float(n) - num) <= 1e-12 * abs(num)
    gref = zl.grad
    assert float((g - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
    if kind == "CE" and region != "all":
        # the broadcast is real: the per-image masking one might expect gives another value
        l = torch.nn.functional.cross_entropy(z, target, reduction="none")
        own = (l * U.region_mask(plbl, region)).sum()
        assert abs(float(own) - num) > 1e-3 * abs(num)


def test_kernels_table_and_segmentor_mapping():
    from hiast_amd import kernels as K
    from hiast_amd.utils.default_config import get_default_cfg
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    assert K.CST_KINDS == {"SoftCE": 0, "CE": 1, "KLDIV": 2, "MSE": 3}
    c = get_default_cfg()
    c.model.type = "SelfTrainingSegmentor"
    c.cst_training.is_enabled = True
    c.cst_training.cst_loss.weight = 0.5
    seg = MODEL["SelfTrainingSegmentor"](c)
    for name in K.CST_KINDS:
        c.cst_training.cst_loss.type = name
        w = seg._weights(True)
        assert w[3] == 0.5 and w[4] is True and w[5] == name
    c.cst_training.cst_loss.type = "BCEWithLogits"
    with pytest.raises(ValueError, match="SoftCE, CE, KLDIV, MSE"):
        seg._weights(True)
    assert seg._weights(False)[4] is False            # no teacher: the type is not consulted
    c.cst_training.cst_loss.type = "SoftCE"
    c.model.predictor.seg_loss.type = "SoftCE"        # a soft loss on hard pseudo-labels stays refused
    with pytest.raises(NotImplementedError):
        seg._weights(True)
