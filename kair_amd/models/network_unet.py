"""DRUNet — the UNetRes module tree of the reference's models/network_unet.py (the class define_G binds for net_type
'drunet'; the Gaussian denoiser behind DPIR).

Same submodule names and parameter shapes (m_head, m_down1-3, m_body, m_up3-1, m_tail, all bias-free), so
`state_dict` and drunet_gray.pth / drunet_color.pth style checkpoints interchange with the reference.  The input
is the noisy image with the noise-level map as its last channel (utils_image.add_noise_map); H and W must be
multiples of 8 (utils_model.test_mode(net, L, mode=1, modulo=8) pads and crops, as the reference's scripts do).
`forward` runs the whole network as one autograd node on the HIP step program (kair_amd/engine/drunet_engine.py, the
ResUNet program it shares with USRNet's prior); there is no CPU path.
"""
import torch.nn as nn

from ..engine.base import ConvNetFunction
from ..engine.drunet_engine import DRUNetEngine
from .network_usrnet import ResBlock, _seq


class UNetRes(nn.Module):
    """network_unet.py UNetRes: x1 = m_head(x0), x_{l+1} = m_down_l(x_l), x = m_body(x4), x = m_up3(x + x4),
    m_up2(x + x3), m_up1(x + x2), m_tail(x + x1).  compute_dtype is the engine option ('bf16' MFMA operands with fp32
    accumulation, 'fp32' exact-MFMA parity mode, 'fp32x3' three fp16-pair MFMA products)."""

    def __init__(self, in_nc=1, out_nc=1, nc=(64, 128, 256, 512), nb=4, act_mode="R", downsample_mode="strideconv",
                 upsample_mode="convtranspose", compute_dtype="fp32"):
        super().__init__()
        if act_mode != "R":
            raise NotImplementedError("kair_amd DRUNet: act_mode 'R' only (options/train_drunet.json)")
        if downsample_mode != "strideconv" or upsample_mode != "convtranspose":
            raise NotImplementedError("kair_amd DRUNet: strideconv / convtranspose only (options/train_drunet.json)")
        if nb < 1:
            raise NotImplementedError("kair_amd DRUNet: nb >= 1")
        if len(nc) != 4:
            raise NotImplementedError("kair_amd DRUNet: four channel counts (three down / up stages)")
        if in_nc > 8 or out_nc > 8:
            raise NotImplementedError("kair_amd DRUNet: in_nc <= 8 and out_nc <= 8")
        if any(c % 8 for c in nc):
            raise NotImplementedError("kair_amd DRUNet: every nc must be a multiple of 8")
        rb = lambda c: [ResBlock(c, act_mode) for _ in range(nb)]   # noqa: E731
        self.m_head = nn.Conv2d(in_nc, nc[0], 3, 1, 1, bias=False)
        self.m_down1 = nn.Sequential(*rb(nc[0]), nn.Conv2d(nc[0], nc[1], 2, 2, 0, bias=False))
        self.m_down2 = nn.Sequential(*rb(nc[1]), nn.Conv2d(nc[1], nc[2], 2, 2, 0, bias=False))
        self.m_down3 = nn.Sequential(*rb(nc[2]), nn.Conv2d(nc[2], nc[3], 2, 2, 0, bias=False))
        self.m_body = _seq(*rb(nc[3]))
        self.m_up3 = nn.Sequential(nn.ConvTranspose2d(nc[3], nc[2], 2, 2, 0, bias=False), *rb(nc[2]))
        self.m_up2 = nn.Sequential(nn.ConvTranspose2d(nc[2], nc[1], 2, 2, 0, bias=False), *rb(nc[1]))
        self.m_up1 = nn.Sequential(nn.ConvTranspose2d(nc[1], nc[0], 2, 2, 0, bias=False), *rb(nc[0]))
        self.m_tail = nn.Conv2d(nc[0], out_nc, 3, 1, 1, bias=False)
        self.compute_dtype = compute_dtype
        self._engine = None

    def engine(self):
        if self._engine is None or self._engine.net_ref() is not self:
            self._engine = DRUNetEngine(self, self.compute_dtype)
        return self._engine

    def _apply(self, fn, *args, **kwargs):
        self._engine = None
        return super()._apply(fn, *args, **kwargs)

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        self._engine = None
        return self

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("kair_amd DRUNet runs on the MI355X (HIP) only; got a CPU tensor (no CPU fallback)")
        return ConvNetFunction.run(self.engine(), x, list(self.parameters()))
