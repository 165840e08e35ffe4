"""DRUNet (UNetRes, the reference's models/network_unet.py) step program for MI355X: one pass of the shared ResUNet
program (kair_amd/engine/resunet.py) over the [noisy image | noise-level map] input.

  xin = NHWC rows of 8 channels of x [B, in_nc, H, W]       kair_image_to_nhwc (pad channels zero)
  E   = ResUNet(xin)                                         -> NCHW image written by the tail conv's epilogue

UNetRes.forward does no padding of its own (the reference's test scripts pad through utils_model.test_mode with
modulo 8), so H and W must be multiples of 8.  The input gets no gradient: the head conv's dgrad is not issued.
"""
import torch

from .. import _hip as H
from .resunet import C8, ResUNetProgram


class DRUNetEngine(ResUNetProgram):
    NAME = "DRUNet"
    COMPUTE_DTYPES = ("bf16", "fp32", "fp32x3")

    def __init__(self, net, compute_dtype="fp32"):
        super().__init__(net, compute_dtype)
        if net.m_head.in_channels > C8 or net.m_tail.out_channels > C8:
            raise NotImplementedError("kair_amd DRUNet: in_nc <= 8 and out_nc <= 8")
        self.init_resunet(net)

    def convs(self):
        return self.resunet_convs()

    def _build_plan(self, key, infer):
        B, Hh, Ww = key
        M = self.unet_levels(B, Hh, Ww)
        T, e = self.tdt, self._e
        P = {"B": B, "H": Hh, "W": Ww, "Hp": Hh, "Wp": Ww, "M": M}
        P["xin"] = e(M[0], C8, dt=T)
        P["S"] = self.unet_state(M)
        P["E"] = e(B, self.out_nc, Hh, Ww)
        if not infer:
            P["gE"] = torch.zeros(M[0], C8, device=self.device, dtype=T)
            P["G"] = self.unet_grad_scratch(M)
            P["loss"], P["loss_ws"] = e(1), e(1024)
            P["wg_ws"] = e(self.wgrad_ws_size(self.unet_wgrad_shapes(M)))
        return P

    def forward(self, x, drop_scales=None):
        """x [B, in_nc, H, W] fp32 NCHW.  Returns the NCHW output buffer."""
        B, C, Hh, Ww = x.shape
        if C != self.in_nc:
            raise ValueError(f"kair_amd DRUNet: {C} input channels, network has {self.in_nc}")
        if Hh % 8 or Ww % 8:
            raise ValueError(f"kair_amd DRUNet: H and W must be multiples of 8 (got {Hh} x {Ww}); pad the input, e.g. "
                             "utils_model.test_mode(net, L, mode=1, modulo=8)")
        P = self.plan(B, Hh, Ww)
        self.pack()
        self.cur = P
        self._ax = self.X3_AEXP   # fp32x3: forward operands are activations
        H.image_to_nhwc(x.contiguous(), P["xin"], C8, None, 1.0, B, C, Hh, Ww)
        self._unet_fwd(P, P["S"], P["xin"], P["E"])
        return P["E"]

    def backward_from_loss(self, H_img, grads, loss_weight=1.0, charb_eps=None, loss_type=None):
        P = self.cur
        self.pixel_loss(P, P["E"], H_img, P["gE"], C8, loss_weight, self.out_nc, P["H"], P["W"], charb_eps=charb_eps,
                        loss_type=loss_type)
        P["e_g"] = self._x3_grad_exp(P["B"] * self.out_nc * P["H"] * P["W"], loss_weight, loss_type)
        self.backward(grads, P)
        return P["loss"]

    def backward_from_grad(self, gE, grads):
        P = self.cur
        H.image_to_nhwc(gE.contiguous(), P["gE"], C8, None, 1.0, P["B"], self.out_nc, P["H"], P["W"])
        self._x3_set_grad_exp(P, gE)
        self.backward(grads, P)

    def backward(self, grads, P):
        self._ax = P.get("e_g", 0)   # fp32x3: backward GEMM A operands are data gradients
        self._unet_bwd(P, P["S"], P["xin"], P["gE"], None, grads, acc=False)
