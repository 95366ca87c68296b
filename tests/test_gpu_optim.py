"""The fused SGD / AdamW steps (K13b hiast_sgd_step, K13c hiast_adamw_step) on the device, through the C ABI: trajectories
against torch's CPU optimisers, the loss scale handled on the device, no host wait, the extents of every load and store, and
the interchange with torch.optim (state_dict, init_optimizers, the packed-weight caches).

Shapes are those at which the multi-tensor chunk walk can go wrong, not the workload's: no whole float4 ((1,), (3,)),
exactly one 64Ki chunk, a chunk boundary with a ragged tail ((65537,), (70001,)), many chunks ((64, 256, 3, 3)) and a view
that starts one element into its storage (not 16-byte aligned: the scalar path)."""
import copy

import numpy as np
import pytest
import torch

import guard_bands as gb
import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (65536,), (65537,), (70001,), (64, 256, 3, 3), (1029,)]
UNALIGNED = 6                                  # SHAPES[UNALIGNED] lives one element into its storage
GROUP_OF = [0, 1, 0, 1, 0, 1, 0]               # two param groups ...
LRS, WDS = (2.5e-4, 1e-2), (5e-4, 0.0)         # ... with their own lr and weight decay
SITS_OUT = (1, 3)                              # (step, tensor): grad is None
RTOL, ATOL = 2e-6, 2e-7                        # parameters (the tolerances of the FusedAdam tests)
KINDS = ("sgd", "adamw")


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from hiast_amd import kernels
    return kernels


def _offset_by_one(t):
    """the same values in a tensor whose first element sits 4 bytes into a fresh storage"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dev_params(values, unaligned=UNALIGNED):
    out = []
    for i, a in enumerate(values):
        t = torch.from_numpy(a.copy()).cuda()
        out.append(torch.nn.Parameter(_offset_by_one(t) if i == unaligned else t))
    assert out[unaligned].data_ptr() % 16 == 4
    return out


def _groups(ps):
    return [{"params": [p for p, k in zip(ps, GROUP_OF) if k == j], "lr": LRS[j], "weight_decay": WDS[j]} for j in (0, 1)]


def _make(kind, ps, fused, **kw):
    from hiast_amd.utils import utils
    if kind == "sgd":
        kw.setdefault("momentum", 0.9)
        return utils.FusedSGD(_groups(ps), lr=1.0, **kw) if fused else torch.optim.SGD(_groups(ps), lr=1.0, foreach=False, **kw)
    return (utils.FusedAdamW(_groups(ps), lr=1.0, betas=(0.9, 0.999), **kw) if fused else
            torch.optim.AdamW(_groups(ps), lr=1.0, betas=(0.9, 0.999), foreach=False, **kw))


STATE_KEYS = {"sgd": ("momentum_buffer",), "adamw": ("exp_avg", "exp_avg_sq")}


def _assert_close(own, ref, kind, what):
    """parameters and state of a fused optimiser on the device against a torch optimiser (any device)"""
    ps_own = [p for g in own.param_groups for p in g["params"]]
    ps_ref = [p for g in ref.param_groups for p in g["params"]]
    for i, (a, b) in enumerate(zip(ps_own, ps_ref)):
        d = (a.detach().cpu() - b.detach().cpu()).abs().max()
        assert torch.allclose(a.detach().cpu(), b.detach().cpu(), rtol=RTOL, atol=ATOL), (what, i, float(d))
    for i, (a, b) in enumerate(zip(ps_own, ps_ref)):
        for key in STATE_KEYS[kind]:
            if key not in ref.state.get(b, {}):        # (.get: indexing the defaultdict would create the entry)
                assert key not in own.state.get(a, {}), (what, i, key)
                continue
            r, o = ref.state[b][key].cpu(), own.state[a][key].cpu()
            assert torch.allclose(o, r, rtol=1e-5, atol=1e-6 * float(r.abs().max())), (what, i, key)


@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_matches_torch_on_the_cpu(K, kind):
    """six steps, two param groups (lr 2.5e-4 with weight decay 5e-4, lr 1e-2 without), one tensor without a gradient at
    step 1, one parameter and its gradient off the 16-byte grid"""
    vals = [synth.normal_f32(2300 + i, s) for i, s in enumerate(SHAPES)]
    pa = _dev_params(vals)
    pb = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in vals]
    own, ref = _make(kind, pa, True), _make(kind, pb, False)
    for step in range(6):
        for i, (a, b) in enumerate(zip(pa, pb)):
            g = torch.from_numpy(synth.normal_f32(2400 + 10 * step + i, SHAPES[i]))
            if (step, i) == SITS_OUT:
                a.grad = b.grad = None
                continue
            b.grad = g
            a.grad = _offset_by_one(g.cuda()) if i == UNALIGNED else g.cuda()
        own.step()
        ref.step()
        _assert_close(own, ref, kind, "step %d" % step)
    if kind == "adamw":
        sa, sb = own.state_dict()["state"], ref.state_dict()["state"]
        assert sorted(sa) == sorted(sb)
        assert all(float(sa[k]["step"]) == float(sb[k]["step"]) for k in sb)
        assert sorted(float(st["step"]) for st in sa.values()) == [5.0] + [6.0] * 6        # one tensor sat out a step


def test_sgd_without_momentum_keeps_no_state(K):
    vals = [synth.normal_f32(2500 + i, s) for i, s in enumerate(SHAPES)]
    pa = _dev_params(vals)
    pb = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in vals]
    own, ref = _make("sgd", pa, True, momentum=0.0), _make("sgd", pb, False, momentum=0.0)
    for step in range(3):
        for i, (a, b) in enumerate(zip(pa, pb)):
            g = torch.from_numpy(synth.normal_f32(2600 + 10 * step + i, SHAPES[i]))
            b.grad = g
            a.grad = _offset_by_one(g.cuda()) if i == UNALIGNED else g.cuda()
        own.step()
        ref.step()
        _assert_close(own, ref, "sgd", "step %d" % step)
    assert all(p not in own.state for p in pa)
    assert own.state_dict()["state"] == {} == ref.state_dict()["state"]


def _scaler():
    sc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=1000)
    sc.scale(torch.zeros((), device="cuda"))        # (the scale tensor is created lazily by the first scale() call)
    return sc


@pytest.mark.parametrize("kind", KINDS)
def test_loss_scale_is_handled_on_the_device(K, kind):
    """under torch.amp.GradScaler scaled gradients give the update torch makes on the unscaled ones; a step with an inf
    gradient (steps 1 and 4) changes NOTHING — parameters and every state tensor keep their bits — and halves the scale;
    the next good step continues as torch does; AdamW's applied-step count leaves the skipped steps out"""
    shapes = [(3,), (65537,), (64, 32, 3, 3), (1029,)]
    gen = torch.Generator().manual_seed(5)
    vals = [torch.randn(s, generator=gen).numpy() for s in shapes]
    pa = _dev_params(vals, unaligned=3)
    pb = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in vals]
    kw = dict(lr=1e-2, weight_decay=5e-4)
    from hiast_amd.utils import utils
    if kind == "sgd":
        own, ref = utils.FusedSGD(pa, momentum=0.9, **kw), torch.optim.SGD(pb, momentum=0.9, foreach=False, **kw)
    else:
        own, ref = utils.FusedAdamW(pa, **kw), torch.optim.AdamW(pb, foreach=False, **kw)
    scaler = _scaler()
    applied = 0
    for it in range(6):
        gs = [torch.randn(s, generator=gen) for s in shapes]
        overflow = it in (1, 4)
        scale = float(scaler.get_scale())
        for i, (p, g) in enumerate(zip(pa, gs)):
            sg = g.cuda() * scale
            if overflow:
                sg.view(-1)[min(3, sg.numel() - 1)] = float("inf")
            p.grad = _offset_by_one(sg) if i == 3 else sg
        before = [p.detach().clone() for p in pa]
        state = [[own.state[p][k].clone() for k in STATE_KEYS[kind]] for p in pa] if applied else None
        scaler.step(own)
        scaler.update()
        if overflow:
            assert all(torch.equal(a.view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(before, pa)), it
            assert state is not None
            for p, old in zip(pa, state):
                for k, o in zip(STATE_KEYS[kind], old):
                    assert torch.equal(o.view(torch.int32), own.state[p][k].view(torch.int32)), (it, k)
            assert float(scaler.get_scale()) == scale * 0.5
        else:
            applied += 1
            for p, g in zip(pb, gs):
                p.grad = g.clone()
            ref.step()
            _assert_close(own, ref, kind, "iteration %d" % it)
            assert float(scaler.get_scale()) == scale
        if kind == "adamw":
            assert own.applied_steps() == applied
    assert applied == 4
    if kind == "adamw":
        sd = own.state_dict()
        assert all(float(st["step"]) == applied for st in sd["state"].values())
    else:
        assert float(own._ctl[0]) == 2.0        # SGD keeps no step count: the device's count of skipped steps is all there is


def test_scaler_step_does_not_wait_for_the_device(K):
    """GradScaler.step on a stock optimiser reads found_inf on the host (`found_inf.item()`: aten._local_scalar_dense of a
    DEVICE tensor, which waits for everything queued before it) once per iteration; on FusedSGD / FusedAdamW it reads no
    device scalar at all.  (Scalars of host tensors — FusedAdam's per-tensor 'step' — wait for nothing and are not counted;
    they are listed in the assertion message.)"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from hiast_amd.utils import utils

    class ScalarReads(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.device, self.host = 0, 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "_local_scalar_dense" in str(func):
                if args[0].is_cuda:
                    self.device += 1
                else:
                    self.host += 1
            return func(*args, **(kwargs or {}))

    shapes = [(3,), (65537,), (32, 16, 3, 3)]

    def run(make):
        ps = [torch.nn.Parameter(torch.from_numpy(synth.normal_f32(2700 + i, s)).cuda()) for i, s in enumerate(shapes)]
        opt, scaler = make(ps), _scaler()
        reads = []
        for it in range(2):                     # (the first step also creates state and plans)
            for i, p in enumerate(ps):
                p.grad = torch.from_numpy(synth.normal_f32(2800 + 10 * it + i, shapes[i])).cuda() * 1024.0
            with ScalarReads() as mode:
                scaler.step(opt)
            scaler.update()
            reads.append((mode.device, mode.host))
        torch.cuda.synchronize()
        return reads

    fused_sgd = run(lambda ps: utils.FusedSGD(ps, lr=1e-2, momentum=0.9, weight_decay=5e-4))
    fused_adamw = run(lambda ps: utils.FusedAdamW(ps, lr=1e-3, weight_decay=5e-4))
    stock = run(lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=5e-4))
    assert all(d == 0 for d, _ in fused_sgd), fused_sgd
    assert all(d == 0 for d, _ in fused_adamw), fused_adamw
    assert all(d >= 1 for d, _ in stock), stock          # the detector sees the wait it is there to see


def _carved(values, offset):
    """values in a poisoned allocation -> (tensor, handle); offset: the tensor starts one element into the payload"""
    n = values.numel() + (1 if offset else 0)
    pay, h = gb.carve((n,), torch.float32, "cuda", 4096)
    t = pay[1:] if offset else pay
    gb.fill(t, values.cuda())
    return t, h


def _bits(t):
    return t.view(torch.int32).clone()


@pytest.mark.parametrize("kind", ["sgd", "sgd0", "adamw"])
def test_extents_in_poisoned_allocations(K, kind):
    """p, g and the state tensors of every shape sit inside poison: one launch over all of them (loss scale 4 from the
    control block) leaves every guard band and every g bit-unchanged and reads no poison; a skipped launch leaves p and the
    state bit-unchanged as well"""
    n_state = {"sgd": 1, "sgd0": 0, "adamw": 2}[kind]
    ts, hs = [], []
    for i, s in enumerate(SHAPES):
        off = i == UNALIGNED
        n = int(np.prod(s))
        row = [torch.from_numpy(synth.normal_f32(2900 + 10 * i + j, (n,))) for j in range(2)]
        row += [torch.from_numpy(np.abs(synth.normal_f32(2950 + 10 * i + j, (n,)))) for j in range(n_state)]
        carved = [_carved(v, off) for v in row]
        ts.append([t for t, _ in carved])
        hs.append([h for _, h in carved])
        if off:
            assert all(t.data_ptr() % 16 == 4 for t in ts[-1])
    numels = [t[0].numel() for t in ts]
    lrs = [LRS[k] for k in GROUP_OF]
    ctl = torch.zeros(8, dtype=torch.float32, device="cuda")
    scale = torch.full((1,), 4.0, device="cuda")
    col = lambda j: [t[j] for t in ts]

    def launch():
        if kind == "adamw":
            K.adamw_step(plan, col(0), col(1), col(2), col(3), lrs, [1.0] * len(ts), [1.0] * len(ts), 0.9, 0.999, 1e-8, 5e-4,
                         ctl=ctl, steps=[1.0] * len(ts))
        else:
            K.sgd_step(plan, col(0), col(1), col(2) if kind == "sgd" else None, lrs, 0.9 if kind == "sgd" else 0.0, 5e-4,
                       ctl=ctl)

    def check_bands():
        for i, row in enumerate(hs):
            for j, h in enumerate(row):
                gb.check(h, "%s tensor %d operand %d" % (kind, i, j))
            if i == UNALIGNED:      # the element in front of an offset tensor belongs to nobody
                for h in row:
                    first = h.raw[h.band:h.band + 4]
                    assert bool((first == gb.FILL).all()), "tensor %d: the element in front of the view was written" % i

    plan = (K.AdamWPlan if kind == "adamw" else K.SgdPlan)(numels, torch.device("cuda"))
    before = [[_bits(t) for t in row] for row in ts]
    K.adam_prepare(ctl, scale, torch.zeros(1, device="cuda"))
    launch()
    torch.cuda.synchronize()
    check_bands()
    for i, row in enumerate(ts):
        assert torch.equal(_bits(row[1]), before[i][1]), "g of tensor %d was written" % i
        assert all(gb.finite(t) for t in row), "tensor %d: poison was read" % i
        assert not torch.equal(_bits(row[0]), before[i][0]), "p of tensor %d did not move" % i
        for j in range(2, 2 + n_state):
            assert not torch.equal(_bits(row[j]), before[i][j]), "state %d of tensor %d did not move" % (j, i)
    after = [[_bits(t) for t in row] for row in ts]
    K.adam_prepare(ctl, scale, torch.ones(1, device="cuda"))            # found_inf: the launch must touch nothing
    launch()
    torch.cuda.synchronize()
    check_bands()
    assert float(ctl[0]) == 1.0 and float(ctl[1]) == 1.0
    for i, row in enumerate(ts):
        for j, t in enumerate(row):
            assert torch.equal(_bits(t), after[i][j]), "skipped step changed operand %d of tensor %d" % (j, i)


def test_entries_refuse_missing_tables(K):
    from hiast_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for n_chunks, table in ((0, t.data_ptr()), (-1, t.data_ptr()), (1, None)):
        assert lib.hiast_sgd_step(table, t.data_ptr(), t.data_ptr(), n_chunks, 0.9, 0.0, None, None) == -1
        assert lib.hiast_adamw_step(table, t.data_ptr(), t.data_ptr(), n_chunks, 0.9, 0.999, 1e-8, None, None) == -1
    p = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError):
        K.sgd_step(K.SgdPlan([8], p.device), [p], [p.double()], None, [0.1], 0.0, 0.0)
    with pytest.raises(ValueError):
        K.adamw_step(K.AdamWPlan([8], p.device), [p], [p[:4]], [p], [p], [0.1], [1.0], [1.0], 0.9, 0.999, 1e-8, 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_goes_to_torch_and_back(K, kind):
    """fused -> torch.optim of the same name -> fused: after each hand-over one further step on both sides agrees"""
    shapes = [(3,), (65537,), (16, 8, 3, 3)]
    from hiast_amd.utils import utils
    kw = dict(lr=1e-2, weight_decay=5e-4)
    mk_own = (lambda ps: utils.FusedSGD(ps, momentum=0.9, **kw)) if kind == "sgd" else (lambda ps: utils.FusedAdamW(ps, **kw))
    mk_ref = (lambda ps: torch.optim.SGD(ps, momentum=0.9, **kw)) if kind == "sgd" else (lambda ps: torch.optim.AdamW(ps, **kw))
    new = lambda src: [torch.nn.Parameter(p.detach().clone()) for p in src]

    def give(ps, it):
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(synth.normal_f32(3100 + 10 * it + i, shapes[i])).cuda()

    pa = [torch.nn.Parameter(torch.from_numpy(synth.normal_f32(3000 + i, s)).cuda()) for i, s in enumerate(shapes)]
    own = mk_own(pa)
    for it in range(2):
        give(pa, it)
        own.step()
    pb = new(pa)
    ref = mk_ref(pb)
    ref.load_state_dict(copy.deepcopy(own.state_dict()))       # (as a checkpoint would: load_state_dict may alias tensors)
    give(pa, 2)
    give(pb, 2)
    own.step()
    ref.step()
    _assert_close(own, ref, kind, "fused -> torch")
    pc = new(pb)
    back = mk_own(pc)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    give(pb, 3)
    give(pc, 3)
    ref.step()
    back.step()
    _assert_close(back, ref, kind, "torch -> fused")
    if kind == "adamw":
        assert back.applied_steps() == 4 and all(float(st["step"]) == 4 for st in back.state_dict()["state"].values())


def test_init_optimizers_builds_the_fused_classes_on_the_device(K, monkeypatch):
    from types import SimpleNamespace as ns
    from hiast_amd.utils import utils
    from test_optim_host import _Net
    net = _Net().cuda()
    cfg = lambda kind: ns(train=ns(optimizer=kind, lr=2.5e-4), model=ns(discriminator=ns(is_enabled=False)))
    monkeypatch.delenv("HIAST_TORCH_OPTIM", raising=False)
    for kind, cls in (("SGD", utils.FusedSGD), ("Adam", utils.FusedAdam), ("AdamW", utils.FusedAdamW)):
        opt, _ = utils.init_optimizers(cfg(kind), net)
        assert type(opt) is cls, kind
        assert [g["lr"] for g in opt.param_groups] == [2.5e-4, 2.5e-3, 2.5e-3]
        assert all(g["weight_decay"] == 0.0005 for g in opt.param_groups)
    assert all(g["momentum"] == 0.9 for g in utils.init_optimizers(cfg("SGD"), net)[0].param_groups)
    monkeypatch.setenv("HIAST_TORCH_OPTIM", "1")
    for kind, cls in (("SGD", torch.optim.SGD), ("Adam", utils.FusedAdam), ("AdamW", torch.optim.AdamW)):
        assert type(utils.init_optimizers(cfg(kind), net)[0]) is cls, kind


def test_packed_weight_follows_a_fused_sgd_step(K):
    """the kernel writes through raw pointers; the packed copies of the trunk weights are cached on Parameter._version"""
    from hiast_amd.utils import utils
    from hiast_amd.sseg.models.modules.resnet import packed_weight
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).cuda()
    wp0 = packed_weight(conv, K.FMT_BF16)
    assert packed_weight(conv, K.FMT_BF16) is wp0
    opt = utils.FusedSGD([conv.weight], lr=0.1, momentum=0.9, weight_decay=5e-4)
    conv.weight.grad = torch.from_numpy(synth.normal_f32(3200, tuple(conv.weight.shape))).cuda()
    v0 = conv.weight._version
    opt.step()
    assert conv.weight._version > v0
    wp1 = packed_weight(conv, K.FMT_BF16)
    assert wp1 is not wp0 and not torch.equal(wp1, wp0)
    assert torch.equal(wp1, K.pack_conv_weight(conv.weight, K.FMT_BF16))
