"""MSRResNet -- the modified SRResNet (no BatchNorm) PSNR baseline; the reference's models/network_msrresnet.py
(MSRResNet0) and the basicblock.py pieces it uses, restated from upstream cszn/KAIR (the reference sources were not at
hand, and the restatement has not been checked against them):

    model = sequential(conv(in_nc -> nc),
                       ShortcutBlock(sequential(ResBlock x nb, conv(nc -> nc))),      x + sub(x)
                       [Upsample(2, nearest), conv(nc -> nc), ReLU] x (1 for x2, 2 for x4)   ('upconv'), or
                       [conv(nc -> r^2 nc), PixelShuffle(r), ReLU], r = 2 (x2; twice for x4) or 3   ('pixelshuffle')
                       conv(nc -> nc), ReLU, conv(nc -> out_nc, bias=False))
    ResBlock(x) = x + res(x),  res = Sequential(conv, ReLU, conv)

basicblock.sequential flattens nested Sequentials, so the state_dict keys are model.0.{weight,bias},
model.1.sub.{i}.res.{0,2}.{weight,bias} (i < nb), model.1.sub.{nb}.{weight,bias}, the upsampling convs at model.3 (and
model.6 for x4; 'pixelshuffle': model.2 and model.5, the conv leading its block), the tail convs at model.{5,7} (x2,
x3) or model.{8,10} (x4); the last conv has no bias.
MSRResNet0(3, 3, 64, 16, 4) has 1,332,928 parameters (derived from the layer list above, not from the reference).

`forward` on HIP tensors runs the whole network as one autograd node on ResSREngine (engine/ressr_engine.py); the input
gets no gradient.  On CPU tensors with CPU parameters it runs the module list with torch ops -- never a substitute for
a device call.

Departures from the reference: act_mode 'R' only; upsample_mode 'upconv' at x2 and x4 and 'pixelshuffle' at x2, x3 and
x4 ('convtranspose' and 'upconv' x3 raise NotImplementedError); nc a multiple of 8.  MSRResNet1 (the bilinear-base variant kept upstream for the
original checkpoints) is not built.
"""
import torch.nn as nn

from ..engine.base import ConvNetFunction


def sequential(*args):
    """basicblock.sequential: one flat nn.Sequential of the modules, nested Sequentials unpacked."""
    mods = []
    for m in args:
        if isinstance(m, nn.Sequential):
            mods.extend(m.children())
        elif isinstance(m, nn.Module):
            mods.append(m)
    return nn.Sequential(*mods)


def conv3(cin, cout, bias=True):
    return nn.Conv2d(cin, cout, 3, 1, 1, bias=bias)


class ShortcutBlock(nn.Module):
    """basicblock.ShortcutBlock: x + sub(x)."""

    def __init__(self, submodule):
        super().__init__()
        self.sub = submodule

    def forward(self, x):
        return x + self.sub(x)


class ResBlock(nn.Module):
    """basicblock.ResBlock, mode 'CRC': x + conv(ReLU(conv(x)))."""

    def __init__(self, nc):
        super().__init__()
        self.res = nn.Sequential(conv3(nc, nc), nn.ReLU(inplace=True), conv3(nc, nc))

    def forward(self, x):
        return x + self.res(x)


class _ResSRBase(nn.Module):
    """What the residual SR networks share: `model`, the engine cache, the device / host split of forward."""
    NAME = "ResSR"

    def __init__(self, compute_dtype):
        super().__init__()
        self.compute_dtype = compute_dtype
        self._engine = None

    def engine_spec(self):
        raise NotImplementedError

    def engine(self):
        from ..engine.ressr_engine import ResSREngine
        if self._engine is None or self._engine.net_ref() is not self:
            self._engine = ResSREngine(self, self.compute_dtype, self.engine_spec())
        return self._engine

    def _apply(self, fn, *args, **kwargs):
        self._engine = None
        return super()._apply(fn, *args, **kwargs)

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        self._engine = None
        return self

    def forward(self, x):
        if x.is_cuda:
            return ConvNetFunction.run(self.engine(), x, list(self.parameters()))
        if next(self.parameters()).is_cuda:
            raise RuntimeError(f"kair_amd {self.NAME}: CPU input for a network on the HIP device")
        return self.model(x)


class MSRResNet0(_ResSRBase):
    NAME = "MSRResNet"

    def __init__(self, in_nc=3, out_nc=3, nc=64, nb=16, upscale=4, act_mode="R", upsample_mode="upconv",
                 compute_dtype="fp32"):
        name = self.NAME
        if act_mode != "R":
            raise NotImplementedError(f"kair_amd {name}: act_mode 'R' only (got {act_mode!r})")
        if upsample_mode not in ("upconv", "pixelshuffle"):
            raise NotImplementedError(f"kair_amd {name}: upsample_mode 'upconv' or 'pixelshuffle' (got {upsample_mode!r})")
        if upscale not in ((2, 4) if upsample_mode == "upconv" else (2, 3, 4)):
            raise NotImplementedError(f"kair_amd {name}: {upsample_mode!r} upscales by 2{'' if upsample_mode == 'upconv' else ', 3'}"
                                      f" or 4 (got upscale {upscale})")
        if nc % 8:
            raise NotImplementedError(f"kair_amd {name}: nc must be a multiple of 8 (got nc {nc})")
        if nb < 1:
            raise NotImplementedError(f"kair_amd {name}: nb must be >= 1 (got nb {nb})")
        super().__init__(compute_dtype)
        body = sequential(*[ResBlock(nc) for _ in range(nb)], conv3(nc, nc))
        ups = []
        self.up_r = [3] if upscale == 3 else [2] * (upscale // 2)
        for r in self.up_r:
            if upsample_mode == "upconv":
                ups += [nn.Upsample(scale_factor=2, mode="nearest"), conv3(nc, nc), nn.ReLU(inplace=True)]
            else:
                ups += [conv3(nc, nc * r * r), nn.PixelShuffle(r), nn.ReLU(inplace=True)]
        self.upsample_mode = upsample_mode
        self.model = sequential(conv3(in_nc, nc), ShortcutBlock(body), *ups, conv3(nc, nc), nn.ReLU(inplace=True),
                                conv3(nc, out_nc, bias=False))
        self.in_nc, self.out_nc, self.nc, self.nb, self.upscale = in_nc, out_nc, nc, nb, upscale

    def engine_spec(self):
        m = list(self.model)
        convs = [x for x in m[2:] if isinstance(x, nn.Conv2d)]
        sub = list(m[1].sub)
        return {"head": m[0], "blocks": [("res", b.res[0], b.res[2]) for b in sub[:-1]], "body_tail": sub[-1],
                "up": convs[:-2],
                "up_r": self.up_r if self.upsample_mode == "pixelshuffle" else None, "hr": convs[-2], "last": convs[-1], "ps": 0, "act": 1, "slope": 0.0}
