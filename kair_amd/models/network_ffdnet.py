"""FFDNet — the reference's models/network_ffdnet.py, restated (the reference sources were not at hand):

    model = Sequential(conv(in_nc*4+1 -> nc) + act, [conv(nc -> nc) (+ BatchNorm2d) + act] x (nb-2), conv(nc -> out_nc*4))
    forward(x [B, in_nc, h, w], sigma [B, 1, 1, 1]):
        x = ReplicationPad2d((0, ceil(w/2)*2 - w, 0, ceil(h/2)*2 - h))(x)
        x = pixel_unshuffle(x, 2);  x = cat((x, sigma.repeat(1, 1, H/2, W/2)), 1)
        x = model(x);  x = PixelShuffle(2)(x)[..., :h, :w]

`model` is DnCNN's flattened Sequential (network_dncnn._layers), so the state_dict keys are model.{0,2,4,...}.{weight,
bias} for act_mode 'R'.  The output is the clean image: no residual subtraction.

`forward` on HIP tensors runs the whole network as one autograd node on FFDNetEngine (engine/dncnn_engine.py: the
PixelUnshuffle head kair_ffd_pack, DnCNN's layer loop over the half grid, the PixelShuffle store); neither x nor sigma
gets a gradient.  On CPU tensors with CPU parameters it runs the forward above with torch ops, as DnCNN runs config 1
on the host -- never a substitute for a device call.
"""
import torch
import torch.nn.functional as F

from ..engine.base import ConvNetFunction
from ..engine.dncnn_engine import FFDNetEngine
from .network_dncnn import _Base, _layers


class FFDNet(_Base):
    residual = False
    sf = 2

    def __init__(self, in_nc=1, out_nc=1, nc=64, nb=15, act_mode="R", compute_dtype="fp32"):
        if nc % 8:
            raise NotImplementedError(f"kair_amd FFDNet: nc must be a multiple of 8 (got {nc})")
        if 4 * out_nc > 16:
            raise NotImplementedError(f"kair_amd FFDNet: 4 * out_nc must be <= 16 (got out_nc {out_nc})")
        if nb < 2:
            raise NotImplementedError(f"kair_amd FFDNet: nb must be >= 2 (got {nb})")
        if "I" in act_mode:
            raise NotImplementedError("kair_amd FFDNet: InstanceNorm ('I') is not on the MI355X path")
        super().__init__(in_nc * 4 + 1, out_nc * 4, nc, nb, act_mode, compute_dtype)
        self.in_nc, self.out_nc = in_nc, out_nc

    def engine(self):
        if self._engine is None or self._engine.net_ref() is not self:
            self._engine = FFDNetEngine(self, self.compute_dtype)
        return self._engine

    def forward(self, x, sigma):
        if x.is_cuda:
            return ConvNetFunction.run(self.engine(), x, list(self.parameters()), sigma)
        if next(self.parameters()).is_cuda:
            raise RuntimeError("kair_amd FFDNet: CPU input for a network on the HIP device")
        B, _, h, w = x.shape
        sigma = torch.as_tensor(sigma, dtype=x.dtype).reshape(-1)
        if sigma.numel() not in (1, B):
            raise ValueError(f"kair_amd FFDNet: sigma holds {sigma.numel()} levels for a batch of {B}")
        x = F.pad(x, (0, -w % 2, 0, -h % 2), mode="replicate")
        x = F.pixel_unshuffle(x, 2)
        m = sigma.view(-1, 1, 1, 1).expand(B, 1, x.shape[2], x.shape[3])
        x = self.model(torch.cat((x, m), 1))
        return F.pixel_shuffle(x, 2)[..., :h, :w]
