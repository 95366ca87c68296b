"""FCDiscriminator (reference: sseg/models/modules/discriminator.py:7-33): five 4x4 stride-2 convolutions,
C -> 64 -> 128 -> 256 -> 512 -> 1, LeakyReLU(0.2) between them; state-dict names conv1..conv4, classifier.
31 GFLOP per 512x1024 image (4 % of one trunk forward).

Default: the convolutions go through MIOpen via PyTorch-ROCm (F.conv2d, in the autocast type).  HIAST_DISC_HIP=1 (opt-in,
hiast_amd/switches.py) routes every layer whose input is a float32 device tensor through the library's own 4x4 / stride-2
kernels instead (HF.disc_conv4x4s2 = hiast_disc_conv_fwd / _dgrad / _wgrad): bias and LeakyReLU in the forward
epilogue, the activation's backward in the gradient kernels' prologue, fp32 arithmetic also under autocast, and no
weight-gradient launch when the weights are detached (`params=`).  HIAST_DISC_HIP_16BIT=1 (opt-in, only with HIAST_DISC_HIP=1
and only under device autocast with float16 or bfloat16) takes the same kernels' matrix-core form in the autocast type
(hiast_disc_conv16_*): operands rounded to that type as they are staged, fp32 accumulation, activations and gradients still
stored in fp32 — the arithmetic of the reference's apex-O1 discriminator.  Without autocast, or with HIAST_DISC_HIP=1 alone,
the fp32 kernels run."""
import torch
from torch import nn
from torch.nn import functional as F

from hiast_amd import switches as SW

__all__ = ["build_discriminator", "FCDiscriminator"]


def _own_fmt():
    """operand type of the own kernels: None = fp32; the autocast type when HIAST_DISC_HIP_16BIT is on and device autocast is
    enabled with float16 or bfloat16"""
    if SW.on("HIAST_DISC_HIP_16BIT") and torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt in (torch.float16, torch.bfloat16):
            return dt
    return None


class FCDiscriminator(nn.Module):

    def __init__(self, num_classes, ndf=64):
        super().__init__()
        chans = [num_classes, ndf, ndf * 2, ndf * 4, ndf * 8]
        for i in range(4):
            setattr(self, "conv%d" % (i + 1), nn.Conv2d(chans[i], chans[i + 1], kernel_size=4, stride=2, padding=1))
        self.classifier = nn.Conv2d(ndf * 8, 1, kernel_size=4, stride=2, padding=1)
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x, params=None):
        """params: optional {name: tensor} overriding the module's own (used with detached weights when only the
        gradient w.r.t. the input is wanted)"""
        for name in ("conv1", "conv2", "conv3", "conv4", "classifier"):
            m = getattr(self, name)
            wgt = m.weight if params is None else params[name + ".weight"]
            b = m.bias if params is None else params[name + ".bias"]
            if SW.on("HIAST_DISC_HIP"):
                from hiast_amd import functional as HF
                if HF.disc_conv_ok(x, wgt):
                    x = HF.disc_conv4x4s2(x, wgt, b, name != "classifier", _own_fmt())
                    continue
            x = F.conv2d(x, wgt, b, stride=2, padding=1)
            if name != "classifier":
                x = F.leaky_relu(x, 0.2, inplace=True)
        return x


def build_discriminator(input_channels):
    return FCDiscriminator(input_channels)
