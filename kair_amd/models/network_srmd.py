"""SRMD — super-resolution for multiple degradations (Zhang, Zuo, Zhang, CVPR 2018); the reference's
models/network_srmd.py restated (the reference sources were not at hand):

    model = Sequential(conv(in_nc -> nc) + ReLU, [conv(nc -> nc) + ReLU] x (nb-2), conv(nc -> out_nc*upscale^2),
                       PixelShuffle(upscale))
    forward(x [B, in_nc, h, w]) = model(x)

The input is the LR image followed by its degradation map: the 15 PCA coefficients of the 15 x 15 blur kernel and,
for SRMD (not for the noise-free SRMDNF), the noise level, each stretched over h x w
(utils_sisr.srmd_degradation_map).  in_nc = C + 16 (SRMD) or C + 15 (SRMDNF).  No BatchNorm, no residual.
state_dict keys are model.{0, 2, ..., 2(nb-1)}.{weight, bias}, so srmd_x4.pth / srmdnf_x4.pth style checkpoints load.

`forward` on HIP tensors runs the whole network as one autograd node on SRMDEngine (engine/dncnn_engine.py: DnCNN's
layer loop on the LR grid, the last conv storing through the PixelShuffle); the input gets no gradient.  On CPU tensors
with CPU parameters it runs the module list with torch ops, as DnCNN does -- never a substitute for a device call.

Departures from the reference: act_mode 'R' and upsample_mode 'pixelshuffle' only (the reference's defaults and the
published models), upscale 2 / 3 / 4, out_nc * upscale^2 <= 48.
"""
import torch.nn as nn

from ..engine.dncnn_engine import SRMDEngine
from .network_dncnn import _Base, _layers


class SRMD(_Base):
    residual = False

    def __init__(self, in_nc=19, out_nc=3, nc=128, nb=12, upscale=4, act_mode="R", upsample_mode="pixelshuffle",
                 compute_dtype="fp32"):
        if upscale not in (2, 3, 4):
            raise NotImplementedError(f"kair_amd SRMD: upscale must be 2, 3 or 4 (got {upscale})")
        if act_mode != "R":
            raise NotImplementedError(f"kair_amd SRMD: act_mode 'R' only (got {act_mode!r})")
        if upsample_mode != "pixelshuffle":
            raise NotImplementedError(f"kair_amd SRMD: upsample_mode 'pixelshuffle' only (got {upsample_mode!r})")
        if nc % 8:
            raise NotImplementedError(f"kair_amd SRMD: nc must be a multiple of 8 (got {nc})")
        if nb < 3:
            raise NotImplementedError(f"kair_amd SRMD: nb must be >= 3 (got {nb})")
        if out_nc * upscale * upscale > 48:
            raise NotImplementedError(f"kair_amd SRMD: out_nc * upscale^2 must be <= 48 (got {out_nc * upscale ** 2})")
        super().__init__(in_nc, out_nc * upscale * upscale, nc, nb, act_mode, compute_dtype)
        self.model.append(nn.PixelShuffle(upscale))
        self.in_nc, self.out_nc, self.upscale = in_nc, out_nc, upscale

    def engine(self):
        if self._engine is None or self._engine.net_ref() is not self:
            self._engine = SRMDEngine(self, self.compute_dtype)
        return self._engine
