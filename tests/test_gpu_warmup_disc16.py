"""The adversarial warm-up iteration under apex O1 (autocast) with HIAST_DISC_HIP=1 and HIAST_DISC_HIP_16BIT=1: the
discriminator's convolutions run on the library's own matrix-core kernels in the autocast type, so not one aten convolution
with a 4x4 weight is left in the iteration (forward, both backward passes, both optimiser steps).  Without the second switch
the discriminator under autocast is MIOpen's — or, with HIAST_DISC_HIP=1 alone, the own kernels in fp32, a type the reference
does not train the discriminator in."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H_IMG, W_IMG = 128, 256


def _trainer(root, amp_dtype):
    """one AdversarialWarmupTrainer on a tiny synthetic dataset: the recipe of tests/test_gpu_disc_conv.py's fixture, with
    apex_opt O1 and the given 16-bit type"""
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL, TRAINER
    from hiast_amd.tools import synth_data
    from make_golden import seeded_state_dict
    cfg = synth_data.synthetic_cfg(root, n_train=4, n_val=2, h=H_IMG, w=W_IMG)
    cfg.train.apex_opt = "O1"
    cfg.train.amp_dtype = amp_dtype
    cfg.dataset.source.type = "Cityscapes"
    cfg.dataset.source.json_path = cfg.dataset.target.json_path
    cfg.dataset.source.image_dir = cfg.dataset.target.image_dir
    cfg.dataset.source.aug_type = ["PRS-%d-%d" % (H_IMG, W_IMG)]
    cfg.dataset.target.aug_type = ["PRS-%d-%d" % (H_IMG, W_IMG)]
    m = MODEL["SourceOnlySegmentor"](cfg)
    sd = {"seg_model." + k: v for k, v in seeded_state_dict(m.seg_model, 778).items()}
    m.load_state_dict(sd)
    m = m.cuda()
    ds = np.stack([synth_data.make_sample(5 + i, H_IMG, W_IMG)[0].astype(np.float32).transpose(2, 0, 1) for i in range(2)]) / 255.0
    synth_data.calibrate_bn(m, torch.from_numpy((ds - 0.45) / 0.225).cuda())
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    del m
    ck = os.path.join(root, "imagenet_like.pth")
    torch.save(sd, ck)
    cfg.train.resume_from = ck
    cfg.train.gpu_num = 1
    cfg.train.batch_size = 2
    cfg.train.iter_report = 1
    cfg.trainer = "AdversarialWarmupTrainer"
    cfg.model.type = "AdversarialWarmupSegmentor"
    cfg.model.discriminator.is_enabled = True
    cfg.model.discriminator.D_loss.type = "BCEWithLogits"
    cfg.model.predictor.ent_loss.weight = 3.0
    cfg.train.total_iter = 2
    cfg.train.iter_val = 2
    cfg.work_dir = os.path.join(root, "work")
    cfg.freeze()
    torch.manual_seed(21)
    return TRAINER[cfg.trainer](cfg, 0)


def _count_disc_convs(fn):
    """the dispatch-mode counter of tests/test_gpu_disc_conv.py: aten convolution / convolution_backward calls whose weight is
    [*, *, 4, 4], autograd's backward included"""
    from torch.utils._python_dispatch import TorchDispatchMode
    seen = []

    class DiscConvCounter(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "convolution" in str(func):
                if any(isinstance(a, torch.Tensor) and a.dim() == 4 and tuple(a.shape[2:]) == (4, 4) for a in args[:3]):
                    seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with DiscConvCounter():
        out = fn()
    torch.cuda.synchronize()
    return out, seen


@pytest.mark.parametrize("amp_dtype", ["bf16", "fp16"])
def test_o1_warmup_iteration_runs_no_library_convolution_in_the_discriminator(tmp_path, monkeypatch, amp_dtype):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import functional as HF, switches as SW
    from hiast_amd.sseg.datasets import utils as du
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP", True)
    monkeypatch.setitem(SW.OPT_IN, "HIAST_DISC_HIP_16BIT", True)
    tr = _trainer(str(tmp_path), amp_dtype)
    assert tr.amp_dtype is (torch.bfloat16 if amp_dtype == "bf16" else torch.float16)
    net = tr.model.module
    s_img, s_lbl = du.batch_to_device(tr.next_source_batch(), tr.device)
    t_img, _ = du.batch_to_device(tr.next_target_batch(), tr.device)
    launches = {"fwd": 0, "fmt": set()}
    orig = HF.K.disc_conv16_fwd

    def spy(x, weight, bias, leaky, fmt):
        launches["fwd"] += 1
        launches["fmt"].add(fmt)
        return orig(x, weight, bias, leaky, fmt)

    monkeypatch.setattr(HF.K, "disc_conv16_fwd", spy)

    def iteration():
        losses = tr.train_on(s_img, s_lbl, t_img)
        vals = {k: float(torch.mean(v.detach().float())) for k, v in losses.items()}
        tr.update_model(tr.g_optimizer, tr.d_optimizer, losses)
        return vals

    d0 = net.D.conv1.weight.detach().clone()
    if amp_dtype == "fp16":
        # dynamic loss scaling settles first: from 2^16 the scaler halves its scale and skips the step on every overflow, and
        # the discriminator moves once a step is applied (the normal start of an fp16 run, not a retry of a failure)
        assert tr.scaler is not None
        for n in range(20):
            iteration()
            if not torch.equal(d0, net.D.conv1.weight.detach()):
                break
        assert not torch.equal(d0, net.D.conv1.weight.detach()), "no optimiser step was applied in 20 iterations"
        print("disc_conv16 trainer fp16: first applied step after %d iteration(s), loss scale now %g" % (
            n + 1, float(tr.scaler.get_scale())))
        d0 = net.D.conv1.weight.detach().clone()
    else:
        assert tr.scaler is None
    launches["fwd"] = 0
    vals, seen = _count_disc_convs(iteration)
    assert seen == [], seen                                   # the feature: not one aten convolution left in the discriminator
    assert launches["fwd"] == 15 and launches["fmt"] == {tr.amp_dtype}, launches       # 3 passes x 5 layers, in the autocast type
    assert set(vals) == {"source_seg_loss", "adv_loss", "D_loss", "target_ent_loss"}
    for k, v in vals.items():
        print("disc_conv16 trainer %s %-16s %.9g" % (amp_dtype, k, v))
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert all(torch.isfinite(p).all() for p in net.D.parameters())
    assert not torch.equal(d0, net.D.conv1.weight.detach()), "discriminator did not move"
