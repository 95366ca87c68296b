"""Expected values of the fused loss's consistency kinds (CE, KLDIV, MSE), shared by tests/test_cst_kinds_host.py and
tests/test_gpu_cst_kinds.py.  TEST INFRASTRUCTURE ONLY.

`expected` builds them from what is already pinned to the reference: oracle.losses_ref.registry_loss
(tests/golden/loss_registry.npz) on the upsampled tensors.  `closed_form` is the per-(image, pixel) restatement the HIP
kernel implements (include/hiast_hip.h, HIAST_CST_*), in torch float64 (or any dtype it is asked for)."""
import torch
import torch.nn.functional as F

from oracle import losses_ref

KINDS = ("CE", "KLDIV", "MSE")
REGIONS = ("ignored", "confident", "all")


def region_mask(plbl, region):
    if region == "ignored":
        return plbl == 255
    if region == "confident":
        return plbl != 255
    assert region == "all"
    return torch.ones_like(plbl, dtype=torch.bool)


def upsample_inputs(z_lr, zt_lr, size):
    """student logits upsampled in float64 (requires_grad on the LOW-RES leaf), teacher logits upsampled in fp32 — as
    oracle.losses_ref.st_loss_sums does"""
    zl = z_lr.double().clone().requires_grad_(True)
    z = F.interpolate(zl, size=size, mode="bilinear", align_corners=True)
    zt = F.interpolate(zt_lr.float(), size=size, mode="bilinear", align_corners=True)
    return zl, z, zt


def target_of(kind, zt_full):
    """what the reference's trainer hands to compute_loss (consistency_self_training_trainer.py:113-119): the arg-max for
    'CE', the softmax (fp32) otherwise; registry_loss applies KLDIV's second softmax itself"""
    if kind == "CE":
        return zt_full.argmax(dim=1)
    return F.softmax(zt_full, dim=1).double()


def masked_tensor(kind, z, target, plbl, region):
    """the per-element tensor of losses.py:75-88 after the multiplication by the mask ([B,B,H,W] for CE)"""
    if kind == "CE":
        t = F.cross_entropy(z, target, reduction="none")
    elif kind == "KLDIV":
        t = F.kl_div(F.log_softmax(z, dim=1), F.softmax(target, dim=1), reduction="none")
    else:
        t = F.mse_loss(z, target, reduction="none")
    return t * region_mask(plbl, region).unsqueeze(1)


def expected(kind, z, target, plbl, region):
    """-> (numerator, count, loss) of LOSS[kind](z, target, refer_labels=plbl, region=region): the loss IS
    registry_loss's value; numerator and count are the sum and the number of non-zero elements of the masked tensor,
    checked to reproduce that value"""
    loss = losses_ref.registry_loss(kind, z, target, refer_labels=plbl, region=region)
    t = masked_tensor(kind, z.detach(), target, plbl, region)
    num, cnt = t.sum(), (t != 0).sum()
    assert abs(float(num / cnt) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    return float(num), int(cnt), loss


def closed_form(kind, z, zt_or_q1, plbl, region, teacher_is_logits=True):
    """per-(image, pixel) closed forms -> (numerator, count, d(numerator / count)/dz with the count held constant).
    z [B,C,H,W]; zt_or_q1: teacher logits (softmax / arg-max taken here) or, with teacher_is_logits=False, the target
    the trainer would pass (hard labels [B,H,W] for CE, probabilities otherwise)."""
    mask = region_mask(plbl, region).to(z.dtype)                 # [B,H,W]
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    if kind == "CE":
        yt = zt_or_q1.argmax(dim=1) if teacher_is_logits else zt_or_q1
        l = -logp.gather(1, yt.unsqueeze(1)).squeeze(1)          # [B,H,W]
        M = mask.sum(0, keepdim=True)                            # [1,H,W]: images whose mask holds at this position
        num = (l * M).sum()
        cnt = ((l != 0).to(z.dtype) * M).sum()
        onehot = torch.zeros_like(z).scatter_(1, yt.unsqueeze(1), 1.0)
        grad = M.unsqueeze(1) * (p - onehot) / cnt
        return num, cnt, grad
    q1 = (torch.softmax(zt_or_q1, dim=1) if teacher_is_logits else zt_or_q1).to(z.dtype)
    m = mask.unsqueeze(1)
    if kind == "KLDIV":
        q = torch.softmax(q1, dim=1)                             # the reference's second softmax (losses.py:21-23)
        t = q * (torch.log(q) - logp) * m
        g = m * (p * q.sum(1, keepdim=True) - q)
    else:
        t = (z - q1) ** 2 * m
        g = m * 2.0 * (z - q1)
    cnt = (t != 0).sum().to(z.dtype)
    return t.sum(), cnt, g / cnt


def argmax_gap_ok(zt_full):
    """the kernel's fp32 arg-max must be the oracle's: the two largest upsampled teacher logits differ by at least
    32 * 2^-23 * max|zt| at every pixel (two nested fp32 lerps stay within a few ulp of that scale)"""
    top2 = zt_full.double().topk(2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1]).min()
    return float(gap) >= 32.0 * 2.0 ** -23 * float(zt_full.abs().max())
