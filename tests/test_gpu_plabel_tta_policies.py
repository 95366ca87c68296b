"""pseudo_policy.tta on the MI355X: the IAS, CT and CBST generators with two resized views and their mirror images, through
HipPlabelEngine (views built with the validator's resample and torch.flip, forwards through GraphedEval, hiast_plabel_pass1_tta),
against the replay of the oracle chain (tests/plabel_tta_inputs.py) through oracle/ias_ref.py.  The model is a head-only stub that
picks its logits by frame index and view shape; the dataset stub writes the frame index k into the frame and k + 0.5 into its last
column, so the stub can tell a view from its mirror image."""
import os

import numpy as np
import pytest
import torch

import plabel_tta_inputs as P

pytestmark = pytest.mark.gpu

NB, B, C, H, W = 3, 2, 19, 33, 65
SIZES = ((17, 33), (49, 97))
POLICIES = ["IAS", "CT", "CBST"]


class _Items(torch.utils.data.Dataset):
    """item i is frame pos[i]: the image carries that index, and index + 0.5 in its last column"""

    def __init__(self, pos):
        self.pos = pos
        self.device_transform = False

    def __len__(self):
        return len(self.pos)

    def __getitem__(self, i):
        k = int(self.pos[i])
        img = torch.full((3, H, W), float(k))
        img[:, :, -1] = k + 0.5
        return {"images": img, "image_paths": "data/cityscapes/leftImg8bit/train/x/img_%03d_leftImg8bit.png" % k}


class _HeadOnly(torch.nn.Module):
    """model stub: the low-res head output of frame k for the view of the shape it is handed, or for that view's mirror image"""

    def __init__(self, z_by_view):
        super().__init__()
        self.z, self.seen = z_by_view, []

    def forward(self, imgs, lowres=True):
        first, last = imgs[:, 0, 0, 0], imgs[:, 0, 0, -1]
        mirror = bool((first > last).all())
        assert mirror or bool((first < last).all())
        idx = torch.minimum(first, last).round().long()
        key = (int(imgs.shape[2]), int(imgs.shape[3]), mirror)
        self.seen.append(key + (int(imgs.shape[0]),))
        return {"logits_lowres": self.z[key][idx].contiguous(), "size": tuple(imgs.shape[2:])}


def _frames():
    """logits of all NB * B frames per (view, mirror) + the generator's frame order"""
    zs, zfs = P.view_logits(4300, NB * B, C, SIZES, True)
    z = {}
    for (Hs, Ws), a, f in zip(SIZES, zs, zfs):
        z[(Hs, Ws, False)], z[(Hs, Ws, True)] = np.array(a), np.array(f)
    return z


def _cfg(tmp_path, policy, name):
    from hiast_amd.utils.default_config import get_default_cfg
    c = get_default_cfg()
    c.pseudo_policy.type = policy
    c.pseudo_policy.batch_size = B
    c.pseudo_policy.resize_size = [H, W]
    c.pseudo_policy.ct.threshold = 0.9
    c.pseudo_policy.cbst.p, c.pseudo_policy.cbst.sample_interval = 0.2, 4
    c.pseudo_policy.save_dir = str(tmp_path / name / "pseudo_labels")
    c.dataset.num_workers = 0
    return c


def _run(tmp_path, policy, name, z, tta=True):
    from PIL import Image
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import PSEUDO_POLICY
    from hiast_amd.workflows.pseudo_label_generator import HipPlabelEngine, ShardedBatchSampler
    c = _cfg(tmp_path, policy, name)
    if tta:
        c.pseudo_policy.tta.resize_sizes = [list(s) for s in SIZES]
        c.pseudo_policy.tta.is_flip = True
    # the generator walks a seeded permutation: lay the frames out so that it meets them in index order
    order = ShardedBatchSampler(NB * B, B, 0, 1, True, c.train.random_seed).order
    pos = np.empty(NB * B, np.int64)
    pos[np.asarray(order)] = np.arange(NB * B)
    model = _HeadOnly({k: torch.from_numpy(v).cuda() for k, v in z.items()})
    gen = PSEUDO_POLICY[policy](c, engine=HipPlabelEngine(model, torch.device("cuda", 0), C), dataset=_Items(pos))
    gen.run()
    root = str(tmp_path / name)
    files = {n: open(os.path.join(root, n), "rb").read() for n in sorted(os.listdir(root)) if n.endswith(".npy")}
    pngs = {n: open(os.path.join(c.pseudo_policy.save_dir, n), "rb").read() for n in sorted(os.listdir(c.pseudo_policy.save_dir))}
    maps = np.stack([np.array(Image.open(os.path.join(c.pseudo_policy.save_dir, "img_%03d_leftImg8bit_pseudo_label.png" % k)))
                     for k in range(NB * B)])
    return c, gen, model, root, files, pngs, maps


@pytest.mark.parametrize("policy", POLICIES)
def test_generators_with_views_equal_the_oracle_replay(tmp_path, policy, monkeypatch):
    from oracle import ias_ref
    monkeypatch.setenv("HIAST_CBST_QUANTILE", "float16")       # numpy-2 evaluation, as ias_ref.cbst_threshold does it
    monkeypatch.delenv("HIAST_GEN_LANES", raising=False)
    z = _frames()
    c, gen, model, root, files, pngs, maps = _run(tmp_path, policy, "lanes", z)
    assert gen.engine.views and gen.engine.group(B, (H, W)) == 1
    # every forward saw one view of one loader batch; 33 x 65 frames are below the validator's 4096-pixel condition: no forward
    # holds a view and its mirror image together
    assert {s[:3] for s in model.seen} == set(z) and {s[3] for s in model.seen} == {B}
    assert len(model.seen) == (2 if policy == "CBST" else 1) * NB * 2 * len(SIZES)

    # the oracle replay
    batches = []
    for t in range(NB):
        sl = slice(t * B, (t + 1) * B)
        mp, am, _, _ = P.oracle_chain([z[(s[0], s[1], False)][sl] for s in SIZES], [z[(s[0], s[1], True)][sl] for s in SIZES],
                                      SIZES, H, W)
        batches.append((mp, am.astype(np.int64)))
    names = lambda t: ["img_%03d" % (t * B + b) for b in range(B)]
    cpg = c.preprocessor.copy_paste.gamma
    if policy == "IAS":
        st = ias_ref.IASState(C, c.pseudo_policy.ias.alpha, c.pseudo_policy.ias.beta, c.pseudo_policy.ias.gamma, cpg)
    else:
        thr = 0.9 * np.ones(C) if policy == "CT" else ias_ref.cbst_threshold(batches, C, 0.2, 4)
        st = ias_ref.ConstantPolicyState(C, thr, cpg)
    want = np.concatenate([st.step(mp, am, names(t)) for t, (mp, am) in enumerate(batches)])
    assert np.array_equal(maps, want), "pseudo-label maps differ from the replay on %d pixels" % int((maps != want).sum())
    assert float((want != 255).mean()) > 0.05 and float((want == 255).mean()) > 0.05          # both outcomes occur
    assert np.array_equal(np.load(os.path.join(root, "statics_class.npy")), st.statics_class)
    got_thr = np.load(os.path.join(root, "class_threshold.npy"))
    assert np.array_equal(got_thr.view(np.uint64), np.asarray(st.class_threshold, np.float64).view(np.uint64))
    assert np.allclose(np.load(os.path.join(root, "class_mean_probabilities.npy")), st.class_mean_probs, rtol=1e-6)

    # one forward stream instead of two: the same bytes in every artefact
    monkeypatch.setenv("HIAST_GEN_LANES", "1")
    _, _, _, _, files1, pngs1, _ = _run(tmp_path, policy, "single", z)
    assert files1 == files and pngs1 == pngs


def test_defaults_never_reach_the_new_entry(tmp_path, monkeypatch):
    """tta keys at their defaults: one forward per batch at the frame's own size and hiast_plabel_pass1, as before"""
    from hiast_amd import kernels as K
    calls = []
    real = K.plabel_pass1_tta
    monkeypatch.setattr(K, "plabel_pass1_tta", lambda *a, **k: calls.append(1) or real(*a, **k))
    z = _frames()
    z[(H, W, False)] = np.array(P.view_logits(4301, NB * B, C, ((H, W),), False)[0][0])
    c, gen, model, root, files, pngs, maps = _run(tmp_path, "CT", "off", z, tta=False)
    assert not gen.engine.views and calls == []
    assert [s[:3] for s in model.seen] == [(H, W, False)] * NB
    from oracle import cref, ias_ref
    st = ias_ref.ConstantPolicyState(C, 0.9 * np.ones(C), c.preprocessor.copy_paste.gamma)
    want = np.concatenate([st.step(mp, am.astype(np.int64), ["img_%03d" % (t * B + b) for b in range(B)]) for t, (mp, am) in
                           enumerate(cref.plabel_stage_a(z[(H, W, False)][t * B:(t + 1) * B], H, W) for t in range(NB))])
    assert np.array_equal(maps, want)
    # and with them set, the same generator does
    _run(tmp_path, "CT", "on", _frames())
    assert len(calls) == NB


def test_a_view_and_its_mirror_image_in_one_forward_give_the_same_bits(tmp_path, monkeypatch):
    """frames whose 1/8 map has 4096 pixels or more: the engine puts a view and its mirror image into ONE forward (the validator's
    condition).  With the real trunk, 512 x 512 frames, the native view and a resized one: maxprob, argmax and hist are bit for bit
    those of separate forwards (HIAST_VAL_BATCH_FLIP=0), and the label is the validator's hiast_tta_fused label of the same views."""
    from hiast_amd import functional as HF, kernels as K
    from hiast_amd.utils.registry import register  # noqa: F401
    from hiast_amd.utils.registry.registries import MODEL
    from hiast_amd.tools import synth_data
    from hiast_amd.workflows.pseudo_label_generator import HipPlabelEngine
    from make_golden import seeded_state_dict
    Hh = Ww = 512
    sizes = [(512, 512), (576, 576)]
    cfg = synth_data.synthetic_cfg(str(tmp_path), n_train=1, n_val=1, h=Hh, w=Ww)
    m = MODEL["SelfTrainingSegmentor"](cfg)
    m.load_state_dict({"seg_model." + k: v for k, v in seeded_state_dict(m.seg_model, 778).items()})
    m = m.cuda().eval()
    ds = np.stack([synth_data.make_sample(15 + i, Hh, Ww)[0].astype(np.float32).transpose(2, 0, 1) for i in range(2)]) / 255.0
    xs = torch.from_numpy((ds - 0.45) / 0.225).cuda()
    synth_data.calibrate_bn(m, xs)
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append(int(args[0].shape[0])))
    eng = HipPlabelEngine(m, torch.device("cuda", 0), cfg.dataset.num_classes, sizes=sizes, flip=True)
    out = {}
    for tag, env in (("one", "1"), ("two", "0")):
        monkeypatch.setenv("HIAST_VAL_BATCH_FLIP", env)
        del seen[:]
        st = eng.begin(xs)
        torch.cuda.synchronize()
        out[tag] = (st["mp"], st["am"], st["hist"], list(seen))
    hook.remove()
    assert out["one"][3] == [4, 4] and out["two"][3] == [2, 2, 2, 2]
    for a, b in zip(out["one"][:3], out["two"][:3]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert int(out["one"][2].sum()) == 2 * Hh * Ww and float(out["one"][0].max()) <= 1.0
    # the validator's tail on the same views
    with torch.no_grad():
        zs, zfs = [], []
        for s in sizes:
            v = xs if s == (Hh, Ww) else HF.upsample_bilinear_ac(xs, s)
            zs.append(m(v, lowres=True)["logits_lowres"].float().contiguous())
            zfs.append(m(torch.flip(v, dims=[3]), lowres=True)["logits_lowres"].float().contiguous())
    probs, label = K.tta_fused(zs, zfs, sizes, Hh, Ww, want_probs=True)
    assert torch.equal(label, out["two"][1])
    mean = torch.minimum(probs.max(1).values / 4.0, torch.ones((), device="cuda"))
    assert torch.equal(mean.view(torch.uint8), out["two"][0].view(torch.uint8))
