"""IMDN -- the lightweight information multi-distillation network (Hui et al., ACM MM 2019; AIM 2019); the reference's
models/network_imdn.py and basicblock.IMDBlock restated from upstream cszn/KAIR (the reference sources were not at
hand, and the restatement has not been checked against them):

    model = sequential(conv(in_nc -> nc), ShortcutBlock(sequential(IMDBlock x nb, conv(nc -> nc))),
                       conv(nc -> out_nc r^2), PixelShuffle(r))
    IMDBlock, d = nc / 4, r = nc - d:
        (d1, r1) = split(lrelu(conv1(x)));  (d2, r2) = split(lrelu(conv2(r1)));  (d3, r3) = split(lrelu(conv3(r2)))
        d4 = conv4(r3);   out = x + conv1x1(cat(d1, d2, d3, d4))
    conv1: nc -> nc, conv2 / conv3: r -> nc, conv4: r -> d (no activation), conv1x1: 4d -> nc (1 x 1, no activation);
    LeakyReLU slope 0.05.  KAIR's block has no channel-attention layer.

state_dict keys: model.0.*, model.1.sub.{i}.conv{1,2,3}.0.*, model.1.sub.{i}.conv4.*, model.1.sub.{i}.conv1x1.*,
model.1.sub.{nb}.*, model.2.*.  IMDN(3, 3, 64, 8, 4) has 893,936 parameters, the published figure.

`forward` on HIP tensors runs the whole network as one autograd node on ResSREngine (engine/ressr_engine.py); on CPU
tensors with CPU parameters it runs the module list with torch ops -- never a substitute for a device call.

Departures from the reference: act_mode 'L' and upsample_mode 'pixelshuffle' only (the reference's defaults), upscale
2 / 3 / 4, out_nc * upscale^2 <= 48, nc a multiple of 32 (so d is a multiple of 8).
"""
import torch
import torch.nn as nn

from .network_msrresnet import ShortcutBlock, _ResSRBase, conv3, sequential


class IMDBlock(nn.Module):
    def __init__(self, nc=64, negative_slope=0.05):
        super().__init__()
        self.d_nc, self.r_nc = nc // 4, nc - nc // 4
        act = lambda: nn.LeakyReLU(negative_slope, inplace=True)
        self.conv1 = nn.Sequential(conv3(nc, nc), act())
        self.conv2 = nn.Sequential(conv3(self.r_nc, nc), act())
        self.conv3 = nn.Sequential(conv3(self.r_nc, nc), act())
        self.conv4 = conv3(self.r_nc, self.d_nc)
        self.conv1x1 = nn.Conv2d(4 * self.d_nc, nc, 1, 1, 0, bias=True)

    def forward(self, x):
        d1, r1 = torch.split(self.conv1(x), (self.d_nc, self.r_nc), dim=1)
        d2, r2 = torch.split(self.conv2(r1), (self.d_nc, self.r_nc), dim=1)
        d3, r3 = torch.split(self.conv3(r2), (self.d_nc, self.r_nc), dim=1)
        d4 = self.conv4(r3)
        return x + self.conv1x1(torch.cat((d1, d2, d3, d4), dim=1))


class IMDN(_ResSRBase):
    NAME = "IMDN"

    def __init__(self, in_nc=3, out_nc=3, nc=64, nb=8, upscale=4, act_mode="L", upsample_mode="pixelshuffle",
                 negative_slope=0.05, compute_dtype="fp32"):
        if act_mode != "L":
            raise NotImplementedError(f"kair_amd IMDN: act_mode 'L' only (got {act_mode!r})")
        if upsample_mode != "pixelshuffle":
            raise NotImplementedError(f"kair_amd IMDN: upsample_mode 'pixelshuffle' only (got {upsample_mode!r})")
        if upscale not in (2, 3, 4):
            raise NotImplementedError(f"kair_amd IMDN: upscale must be 2, 3 or 4 (got {upscale})")
        if nc % 32:
            raise NotImplementedError(f"kair_amd IMDN: nc must be a multiple of 32 (got nc {nc})")
        if out_nc * upscale * upscale > 48:
            raise NotImplementedError(f"kair_amd IMDN: out_nc * upscale^2 must be <= 48 (got {out_nc * upscale ** 2})")
        if nb < 1:
            raise NotImplementedError(f"kair_amd IMDN: nb must be >= 1 (got nb {nb})")
        super().__init__(compute_dtype)
        body = sequential(*[IMDBlock(nc, negative_slope) for _ in range(nb)], conv3(nc, nc))
        self.model = sequential(conv3(in_nc, nc), ShortcutBlock(body), conv3(nc, out_nc * upscale * upscale),
                                nn.PixelShuffle(upscale))
        self.in_nc, self.out_nc, self.nc, self.nb, self.upscale = in_nc, out_nc, nc, nb, upscale
        self.negative_slope = negative_slope

    def engine_spec(self):
        m = list(self.model)
        sub = list(m[1].sub)
        return {"head": m[0], "body_tail": sub[-1], "up": [], "hr": None, "last": m[2], "ps": self.upscale, "act": 2,
                "slope": self.negative_slope,
                "blocks": [("imd", b.conv1[0], b.conv2[0], b.conv3[0], b.conv4, b.conv1x1) for b in sub[:-1]]}
