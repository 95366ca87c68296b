"""CPU-side checks of the fused SGD / AdamW steps (K13b / K13c): the two element rules, restated in numpy float32 in the
operation order the kernels use, against torch's single-tensor optimisers; the argument checks of FusedSGD; what
init_optimizers builds for CPU parameters; the two entries of the C ABI.  No GPU is needed."""
import os
import re
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(3,), (70, 11), (4, 5, 3, 3)]
LRS = [2.5e-4, 1e-2, 2.5e-4]          # the two param groups of the GPU trajectory test
STEPS = 6
# float32 parameters of magnitude ~1 move by lr * O(1) per step; torch's CPU kernels may contract a multiply and an add
# (p + alpha*buf, lerp) where the restatement rounds twice: half an ulp of the product per step, i.e. <= 6e-8 * lr-sized
# terms over six steps — far inside the tolerance of the GPU tests, which is what this file pins the formulas for
RTOL, ATOL = 2e-6, 2e-7


def sgd_rule(p, g, buf, lr, mu, wd, inv_scale=F(1)):
    """hiast_sgd_step, element rule; buf None = momentum 0"""
    g = g * F(inv_scale)
    if wd != 0:
        g = g + F(wd) * p
    if buf is None:
        return p - F(lr) * g, None
    buf = buf * F(mu) + g
    return p - F(lr) * buf, buf


def adamw_rule(p, g, m, v, lr, step, beta1, beta2, eps, wd, inv_scale=F(1)):
    """hiast_adamw_step, element rule; the scalars are formed as the host / the kernel form them"""
    decay = F(1.0 - lr * wd)
    omb1, omb2 = F(1.0 - beta1), F(1.0 - beta2)
    bc1, bc2_sqrt = F(1.0 - beta1 ** step), F(np.sqrt(1.0 - beta2 ** step))
    g = g * F(inv_scale)
    p = p * decay
    m = m + (g - m) * omb1
    v = v * F(beta2) + omb2 * g * g
    step_size = F(lr) / bc1
    p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + F(eps)))
    return p, m, v


def _inputs():
    ps = [synth.normal_f32(2100 + i, s) for i, s in enumerate(SHAPES)]
    gs = [[synth.normal_f32(2200 + 10 * t + i, s) for i, s in enumerate(SHAPES)] for t in range(STEPS)]
    return ps, gs


def _torch_params(ps):
    return [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]


def _groups(tp, wd0):
    """group 0: tensors 0 and 2 (lr 2.5e-4, weight decay wd0); group 1: tensor 1 (lr 1e-2, no weight decay)"""
    return [{"params": [tp[0], tp[2]], "lr": LRS[0], "weight_decay": wd0}, {"params": [tp[1]], "lr": LRS[1], "weight_decay": 0.0}]


@pytest.mark.parametrize("mu", [0.9, 0.0])
def test_sgd_rule_restated_in_float32_matches_torch_sgd(mu):
    ps, gs = _inputs()
    tp = _torch_params(ps)
    opt = torch.optim.SGD(_groups(tp, 5e-4), lr=1.0, momentum=mu, foreach=False)
    wds = [5e-4, 0.0, 5e-4]
    bufs = [None if mu == 0 else np.zeros_like(p) for p in ps]
    for t in range(STEPS):
        for i, q in enumerate(tp):
            sits_out = t == 1 and i == 2
            q.grad = None if sits_out else torch.from_numpy(gs[t][i].copy())
            if not sits_out:
                ps[i], bufs[i] = sgd_rule(ps[i], gs[t][i], bufs[i], LRS[i], mu, wds[i])
        opt.step()
        for i, q in enumerate(tp):
            assert ps[i].dtype == np.float32
            assert np.allclose(ps[i], q.detach().numpy(), rtol=RTOL, atol=ATOL), (t, i)
    for i, q in enumerate(tp):
        if mu == 0:
            assert "momentum_buffer" not in opt.state[q] or opt.state[q]["momentum_buffer"] is None
        else:
            ref = opt.state[q]["momentum_buffer"].numpy()
            assert np.allclose(bufs[i], ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())


def test_adamw_rule_restated_in_float32_matches_torch_adamw():
    ps, gs = _inputs()
    tp = _torch_params(ps)
    b1, b2, eps = 0.9, 0.999, 1e-8
    opt = torch.optim.AdamW(_groups(tp, 5e-4), lr=1.0, betas=(b1, b2), eps=eps, foreach=False)
    wds = [5e-4, 0.0, 5e-4]
    ms, vs, steps = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps], [0, 0, 0]
    for t in range(STEPS):
        for i, q in enumerate(tp):
            sits_out = t == 1 and i == 2
            q.grad = None if sits_out else torch.from_numpy(gs[t][i].copy())
            if not sits_out:
                steps[i] += 1
                ps[i], ms[i], vs[i] = adamw_rule(ps[i], gs[t][i], ms[i], vs[i], LRS[i], steps[i], b1, b2, eps, wds[i])
        opt.step()
        for i, q in enumerate(tp):
            assert ps[i].dtype == np.float32
            assert np.allclose(ps[i], q.detach().numpy(), rtol=RTOL, atol=ATOL), (t, i)
    for i, q in enumerate(tp):
        st = opt.state[q]
        assert float(st["step"]) == steps[i]
        for got, key in ((ms[i], "exp_avg"), (vs[i], "exp_avg_sq")):
            ref = st[key].numpy()
            assert np.allclose(got, ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max()), (i, key)


def test_loss_scale_in_the_rules_is_a_plain_multiplication():
    """a power-of-two loss scale leaves no trace: the rule on (g * scale, 1 / scale) gives the bits of the rule on g"""
    ps, gs = _inputs()
    p, g = ps[1], gs[0][1]
    a = sgd_rule(p, g, np.zeros_like(p), 1e-2, 0.9, 5e-4)
    b = sgd_rule(p, g * F(1024), np.zeros_like(p), 1e-2, 0.9, 5e-4, inv_scale=1.0 / 1024)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    a = adamw_rule(p, g, np.zeros_like(p), np.zeros_like(p), 1e-2, 1, 0.9, 0.999, 1e-8, 5e-4)
    b = adamw_rule(p, g * F(1024), np.zeros_like(p), np.zeros_like(p), 1e-2, 1, 0.9, 0.999, 1e-8, 5e-4, inv_scale=1.0 / 1024)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_fused_sgd_refuses_nesterov_and_dampening():
    from hiast_amd.utils.utils import FusedSGD
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    opt = FusedSGD(p, lr=0.1, momentum=0.9, weight_decay=5e-4)         # construction itself needs no device
    assert opt._step_supports_amp_scaling
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (0.1, 0.9, 0.0, 5e-4, False)


def test_fused_adamw_shares_fused_adams_bookkeeping():
    from hiast_amd.utils import utils
    assert issubclass(utils.FusedAdamW, utils.FusedAdam)
    for name in ("_fold_steps", "applied_steps", "state_dict", "load_state_dict", "step"):
        assert getattr(utils.FusedAdamW, name) is getattr(utils.FusedAdam, name), name
    opt = utils.FusedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    assert opt.defaults["weight_decay"] == torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))]).defaults["weight_decay"]


class _Seg(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 7))

    def get_optimizer_params(self, lr):
        return [{"params": [self.a], "lr": lr}, {"params": [self.b], "lr": 10 * lr}, {"params": [self.c], "lr": 10 * lr}]


class _Net(torch.nn.Module):
    """the surface init_optimizers needs: seg_model.get_optimizer_params(lr) -> three LR groups"""

    def __init__(self):
        super().__init__()
        self.seg_model = _Seg()


@pytest.mark.parametrize("switch", [None, "1"])
def test_init_optimizers_keeps_torchs_classes_for_cpu_parameters(monkeypatch, switch):
    from hiast_amd.utils import utils
    if switch is None:
        monkeypatch.delenv("HIAST_TORCH_OPTIM", raising=False)
    else:
        monkeypatch.setenv("HIAST_TORCH_OPTIM", switch)
    for kind, cls in (("SGD", torch.optim.SGD), ("Adam", torch.optim.Adam), ("AdamW", torch.optim.AdamW)):
        cfg = ns(train=ns(optimizer=kind, lr=2.5e-4), model=ns(discriminator=ns(is_enabled=False)))
        opt, d_opt = utils.init_optimizers(cfg, _Net())
        assert type(opt) is cls and d_opt is None
        assert [g["lr"] for g in opt.param_groups] == [2.5e-4, 2.5e-3, 2.5e-3]
        assert all(g["weight_decay"] == 0.0005 for g in opt.param_groups)
        if kind == "SGD":
            assert all(g["momentum"] == 0.9 for g in opt.param_groups)


def test_the_switch_is_not_one_of_the_kernel_switches():
    """HIAST_TORCH_OPTIM is read where the optimiser is built; the set in hiast_amd.switches is for the kernel paths"""
    from hiast_amd import switches as SW
    assert "HIAST_TORCH_OPTIM" not in SW._NAMES + SW._OPT_IN_NAMES


def test_sgd_and_adamw_entries_are_exported_with_the_headers_arity():
    import __graft_entry__ as ge
    ge.build()
    from hiast_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "hiast_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in (("hiast_sgd_step", 8), ("hiast_adamw_step", 9)):
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, txt, flags=re.S)
        assert m is not None, name
        assert m.group(1).count(",") + 1 == n_args == len(_lib.SIGNATURES[name][1]), name
    assert lib.hiast_version() == 6
    # the records the Python side fills are the header's structs, field for field
    from hiast_amd import kernels as K
    assert K.SgdPlan.REC.itemsize == 40 and K.AdamWPlan.REC.itemsize == 64 and K.AdamPlan.REC.itemsize == 56
    assert K.AdamWPlan.REC.names[:8] == K.AdamPlan.REC.names[:8] and K.AdamWPlan.REC.names[9] == "decay"
    assert [K.AdamWPlan.REC.fields[n][1] for n in K.AdamWPlan.REC.names[:8]] == \
           [K.AdamPlan.REC.fields[n][1] for n in K.AdamPlan.REC.names[:8]]
    # refused before anything is launched: no table, no chunks (needs no device)
    assert lib.hiast_sgd_step(None, None, None, 1, 0.9, 0.0, None, None) == -1
    assert lib.hiast_adamw_step(None, None, None, 1, 0.9, 0.999, 1e-8, None, None) == -1
