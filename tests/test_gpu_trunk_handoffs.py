"""The hand-offs between the autograd nodes of the 16-bit training trunk (functional.IdentityLink / BnBwdLink / SharedInputLink,
the grouped weight gradient, the side-stream helper): every forward / backward issues the kernel entry points it issued when
golden/trunk_backward_calls.json was recorded (from the commit before the links replaced the per-block dicts), in the same order
and on the same stream — and after each backward no link holds a tensor any more."""
import json
import os

import pytest
import torch
import torch.nn as nn

from hiast_amd import switches as SW

pytestmark = pytest.mark.gpu

ENTRIES = ("igemm_bn_act", "igemm_dgrad_bn_stats", "xconv_dgrad_gated_bn_stats", "igemm_dgrad_s2", "bn_nhwc_stats",
           "bn_nhwc_stats_from_partial", "bn_nhwc_apply", "bn_nhwc_apply_partial", "bn_nhwc_bwd_stats", "bn_nhwc_bwd_apply",
           "conv_wgrad_nhwc", "conv_wgrad_small_nhwc", "conv_wgrad_group", "pack_conv_weight")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk_backward_calls.json")
OFF = ("HIAST_NO_IDT_HANDOFF", "HIAST_NO_BN_BWD_FUSION", "HIAST_NO_XSUM", "HIAST_NO_WGROUP", "HIAST_NO_BN_MASK")


def _net(kind):
    """-> (blocks, input shape) at the smallest shapes where each path still arms"""
    from hiast_amd.sseg.models.modules.resnet import Bottleneck
    if kind == "identity2":     # M = 4096: the minimum of the gated conv1 data gradient + bn3 sums; the full weight-gradient group
        return nn.Sequential(Bottleneck(1024, 256, 1, 2), Bottleneck(1024, 256, 1, 2)), (1, 1024, 64, 64)
    if kind == "entry_s1":      # stride-1 downsample: conv1 and the downsample convolution share their input
        down = nn.Sequential(nn.Conv2d(512, 1024, 1, stride=1, bias=False), nn.BatchNorm2d(1024))
        return nn.Sequential(Bottleneck(512, 256, 1, 1, down)), (1, 512, 24, 40)
    if kind == "entry_s2":      # own strided data gradient, the subsample node, the small weight gradients
        down = nn.Sequential(nn.Conv2d(256, 512, 1, stride=2, bias=False), nn.BatchNorm2d(512))
        return nn.Sequential(Bottleneck(256, 128, 2, 1, down)), (1, 256, 32, 48)
    assert kind == "layer4"     # only the 1x1 pair is grouped
    return nn.Sequential(Bottleneck(2048, 512, 1, 4)), (1, 2048, 16, 24)


# name -> (blocks, switches set, variant)
CASES = {k: (k, (), "") for k in ("identity2", "entry_s1", "entry_s2", "layer4")}
CASES["entry_s1_retain"] = ("entry_s1", (), "retain")               # a second backward over the retained graph
CASES["identity2_pruned"] = ("identity2", (), "pruned")             # the block input needs no gradient; two iterations
CASES["entry_s1_down_bn_eval"] = ("entry_s1", (), "down_bn_eval")   # no taker: conv1 returns its own gradient
for _k in ("identity2", "entry_s1"):
    for _s in OFF:
        CASES["%s_%s" % (_k, _s)] = (_k, (_s,), "")
CASES["identity2_side_stream"] = ("identity2", (), "overlap")       # the grouped launch on the side stream
CASES["entry_s2_side_stream"] = ("entry_s2", (), "overlap")         # ... and the per-convolution launches


def run_case(name, after_backward=None):
    """one case -> the ordered [entry name, "main" | "side"] list of its forwards and backwards.  Only spellings that the
    recorded commit has too (it is run there to record the list); after_backward(net): called after every backward.
    The inference-mode BatchNorm of `down_bn_eval` has no backward: the pass ends there with NotImplementedError, after
    conv1's (the downsample leg, created first, runs last) — the list then ends with ["raised", "NotImplementedError"]."""
    from hiast_amd import functional as HF
    from hiast_amd import kernels as K
    kind, switches, variant = CASES[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net, shape = _net(kind)
    net = net.to(dev).train()
    if variant == "down_bn_eval":
        net[0].downsample[1].eval()
    x0 = torch.randn(shape, device=dev).half().contiguous(memory_format=torch.channels_last)
    main = torch.cuda.current_stream()
    calls, real, saved = [], {}, {s: SW.SWITCHES[s] for s in switches}

    def spy(entry):
        def f(*a, **k):
            calls.append([entry, "main" if torch.cuda.current_stream() == main else "side"])
            return real[entry](*a, **k)
        return f
    overlap = HF._wgrad_overlap[0]
    try:
        for e in ENTRIES:
            real[e] = getattr(K, e)
            setattr(K, e, spy(e))
        for s in switches:
            SW.SWITCHES[s] = True
        HF._wgrad_overlap[0] = variant == "overlap"
        for _ in range(2 if variant == "pruned" else 1):
            net.zero_grad()
            src = x0.clone().requires_grad_(variant != "pruned")
            with torch.autocast("cuda", dtype=torch.float16):
                y = net(src if variant == "pruned" else src * 1.0)
            gy = torch.randn_like(y)
            try:
                for i in range(2 if variant == "retain" else 1):
                    y.backward(gy, retain_graph=(variant == "retain" and i == 0))
                    HF.wgrad_stream_join()
                    if after_backward is not None:
                        after_backward(net)
            except NotImplementedError:
                if variant != "down_bn_eval":
                    raise
                calls.append(["raised", "NotImplementedError"])
                if after_backward is not None:
                    after_backward(net)
            torch.cuda.synchronize()
            grads = [p.grad for p in net.parameters()] + ([] if variant == "pruned" else [src.grad])
            if variant != "down_bn_eval":       # (the pass that ended early has delivered only some of them)
                assert all(g is not None for g in grads), name
            assert all(bool(torch.isfinite(g).all()) for g in grads if g is not None), name
    finally:
        HF._wgrad_overlap[0] = overlap
        for e, f in real.items():
            setattr(K, e, f)
        SW.SWITCHES.update(saved)
    return calls


@pytest.fixture(scope="module")
def golden_calls():
    from hiast_amd import kernels as K
    with open(GOLDEN) as f:
        gold = json.load(f)
    prev = K.reserve_cus(0)         # the grouping decision depends on the CU count: recorded, and run, without a CU reserve
    try:
        assert K.grid_cus() == gold["grid_cus"], (
            "golden/trunk_backward_calls.json was recorded on %d CUs, this device has %d: which convolutions share a "
            "weight-gradient launch depends on it, record the list again on this device" % (gold["grid_cus"], K.grid_cus()))
        yield gold["cases"]
    finally:
        K.reserve_cus(prev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_trunk_issues_the_recorded_calls_and_leaves_no_link_holding_a_tensor(name, golden_calls, monkeypatch):
    from hiast_amd import functional as HF
    links, jobs = [], []

    def tracked(cls):
        def make(*a, **k):
            links.append(cls(*a, **k))
            return links[-1]
        return make
    for cls in ("IdentityLink", "BnBwdLink", "SharedInputLink"):
        monkeypatch.setattr(HF, cls, tracked(getattr(HF, cls)))
    real_wg = HF.wgroup_weights

    def wgroup_weights(convs, x):
        out = real_wg(convs, x)
        jobs.extend(w[0] for w in out if w is not None)
        return out
    monkeypatch.setattr(HF, "wgroup_weights", wgroup_weights)
    seen = [0]

    def after_backward(net):
        seen[0] += 1
        assert links, "the blocks created no link"
        for ln in links:
            held = {a: getattr(ln, a) for a in ("gated", "dx", "partial", "sums") if getattr(ln, a, None) is not None}
            assert not held, (type(ln).__name__, sorted(held))
        assert all(j is None for js in jobs for j in js), "a weight-gradient group still holds operands"
    calls = run_case(name, after_backward)
    assert seen[0] >= 1
    want = golden_calls[name]
    assert len(calls) == len(want) and calls == want, next(
        ("call %d: %s, recorded %s" % (i, a, b) for i, (a, b) in enumerate(zip(calls, want)) if a != b),
        "%d calls, recorded %d" % (len(calls), len(want)))
