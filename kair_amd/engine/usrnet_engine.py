"""USRNet step program for MI355X.

Reference: /root/reference/models/network_usrnet_v1.py (the torch.fft restatement of the
network_usrnet.py that define_G binds, select_network.py:167-178): p2o :48-69, upsample :72-82,
ResUNet :109-166, DataNet :179-194, HyPaNet :204-216, USRNet.forward :237-262.

Program per forward (B patches, LQ h x w, scale sf, HR H = h*sf, W = w*sf):
  ab = HyPaNet([sigma, sf])                                   one-block kernel, [B, 2n]
  FB = fft2(p2o(k)), invW = alias-mean |FB|^2                 rows pass + column pass
  FBFy = conj(FB) * fft2(upsample(x, sf))                     rows pass + column pass
  x = nearest-upsample(x)
  n times:  z = DataNet(x; alpha_i)     rows -> columns (closed form, inverse columns) -> inverse rows
            xin = [z, beta_i]           NHWC rows of 8 channels (the 4-channel cat, padded)
            x = ResUNet(xin)            -> NCHW image written by the tail conv's epilogue
ResUNet: the program shared with DRUNet (kair_amd/engine/resunet.py: packs, buffers, forward and
backward passes); this engine owns HyPaNet, the FFT passes, the replicate pad / crop / fold and the
iteration loop.  The ResUNet weights are shared by the n iterations, so their gradients accumulate.

Maps are NHWC fp32 token rows (ReLU outputs and GEMM-only operands in the compute dtype), complex
planes float2 [planes][W][H] (kair_hip.h).  An HR size that is not a multiple of 8 runs the ResUNet on
the replicate-padded grid (v1:148-151) and crops its output (v1:164) -- kair_usr_pad, with the zero pad
(crop adjoint) of the output gradient and the fold (replicate adjoint) of the input gradient in
backward.  B*Hp*Wp < 2^24.
"""
import torch

from .. import _hip as H
from .resunet import C8, ResUNetProgram


class USRNetEngine(ResUNetProgram):
    NAME = "USRNet"
    COMPUTE_DTYPES = ("bf16", "fp32", "fp32x3")

    def __init__(self, net, compute_dtype="bf16"):
        # fp32x3 (EngineBase): the ResUNet products in the split-fp16 arithmetic (split in the GEMM kernels, weights
        # packed as fp16 pairs, the launches through _nt / _wgrad); the FFT / DataNet / HyPaNet passes are the fp32
        # engine's
        super().__init__(net, compute_dtype)
        p = net.p
        self.n = net.n
        if p.m_head.in_channels != p.m_tail.out_channels + 1 or p.m_head.in_channels > C8:
            raise NotImplementedError("kair_amd USRNet: in_nc must be out_nc + 1 <= 8")
        self.hyp = [net.h.mlp[0], net.h.mlp[2], net.h.mlp[4]]
        self.hc, self.no = self.hyp[0].out_channels, self.hyp[2].out_channels
        if self.no != 2 * self.n or self.hyp[0].in_channels != 2:
            raise NotImplementedError("kair_amd USRNet: HyPaNet must map 2 -> 2 * n_iter")
        self.init_resunet(p)

    def convs(self):
        return self.resunet_convs()

    def _hyp(self):
        return [t for m in self.hyp for t in (m.weight, m.bias)]

    # ------------------------------------------------------------------------------------
    def _build_plan(self, key, infer):
        B, h, w, sf, kh, kw = key
        Hh, Ww = h * sf, w * sf
        Hp, Wp = -(-Hh // 8) * 8, -(-Ww // 8) * 8   # the ResUNet's grid (ReplicationPad2d, v1:148-151)
        pad = (Hp, Wp) != (Hh, Ww)
        M = self.unet_levels(B, Hp, Wp)
        T, e, C = self.tdt, self._e, self.out_nc
        planes = B * C
        P = {"B": B, "h": h, "w": w, "sf": sf, "H": Hh, "W": Ww, "Hp": Hp, "Wp": Wp, "pad": pad, "M": M}
        Mu = B * Hh * Ww   # pixels of the HR grid
        cplx = planes * Hh * Ww * 2
        P["T"], P["FBFy"] = e(cplx), e(cplx)
        P["FB"] = e(B * Hh * Ww * 2)
        P["invW"] = e(B * (Hh // sf) * (Ww // sf))
        P["ab"], P["gab"], P["sig"] = e(B, self.no), e(B, self.no), e(B)
        P["x0"], P["z"] = e(B, C, Hh, Ww), e(B, C, Hh, Ww)
        its = []
        for _ in range(self.n):
            its.append({"FR": e(cplx), "xin": e(M[0], C8, dt=T), "xout": e(B, C, Hh, Ww),
                        "xin_u": e(Mu, C8, dt=T) if pad else None, "xout_p": e(B, C, Hp, Wp) if pad else None,
                        **self.unet_state(M)})
        P["it"] = its
        P["gE"] = torch.zeros(Mu, C8, device=self.device, dtype=T)
        P["gxin"] = e(M[0], C8)
        if pad:   # the output gradient on the padded grid (zeros outside), the input gradient folded back
            P["gE_p"], P["gxin_u"] = e(M[0], C8, dt=T), e(Mu, C8)
        P["G"] = self.unet_grad_scratch(M)
        P["a_ws"] = e(planes * (Ww // sf))
        P["cs_ws"] = e(B * H.USR_CHAN_CHUNKS)
        P["loss"], P["loss_ws"] = e(1), e(1024)
        P["wg_ws"] = e(self.wgrad_ws_size(self.unet_wgrad_shapes(M)))
        return P

    # ------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------
    def forward(self, x, k, sf, sigma):
        """x [B, C, h, w], k [B, 1, kh, kw], sigma [B, 1, 1, 1] (device fp32).  Returns the NCHW
        output buffer of the last iteration."""
        B, C, h, w = x.shape
        if C != self.out_nc:
            raise ValueError(f"kair_amd USRNet: {C} input channels, network has {self.out_nc}")
        if k.dim() != 4 or k.shape[0] != B or k.shape[1] != 1:
            raise NotImplementedError("kair_amd USRNet: one blur kernel per image, k of shape [B, 1, kh, kw]")
        kh, kw = k.shape[-2:]
        P = self.plan(B, h, w, sf, kh, kw)
        self.pack()
        self.cur = P
        self._ax = self.X3_AEXP   # fp32x3: forward operands are activations
        x = x.contiguous().float()
        k = k.contiguous().float()
        P["x_in"], P["k_in"] = x, k
        P["sig"].copy_(sigma.reshape(B).float())
        Hh, Ww, planes = P["H"], P["W"], B * C
        H.hypanet_fwd(P["sig"], float(sf), *self._hyp(), self.hc, self.no, B, P["ab"])
        H.usr_fft_rows(k, H.USR_SRC_PSF, 1, 0, kh, kw, 1, P["FB"], B, Hh, Ww)
        H.usr_fft_cols(H.USR_COL_FB, P["FB"], P["FB"], None, None, None, P["invW"], None, 0, None, B, 1, Hh, Ww, sf)
        H.usr_fft_rows(x, H.USR_SRC_ZUP, C, 0, 0, 0, sf, P["FBFy"], planes, Hh, Ww)
        H.usr_fft_cols(H.USR_COL_FBFY, P["FBFy"], P["FBFy"], P["FB"], None, None, P["invW"], None, 0, None, planes, C,
                       Hh, Ww, sf)
        H.usr_upsample_nearest(x, P["x0"], planes, h, w, sf)
        xc = P["x0"]
        for i in range(self.n):
            S = P["it"][i]
            self._datanet_fwd(P, S, xc, i)
            self._prior_fwd(P, S)
            xc = S["xout"]
        return xc

    def _datanet_fwd(self, P, S, xc, i):
        B, C, Hh, Ww, sf = P["B"], self.out_nc, P["H"], P["W"], P["sf"]
        planes, ab = B * C, P["ab"]
        H.usr_fft_rows(xc, H.USR_SRC_NCHW, C, 0, 0, 0, 1, P["T"], planes, Hh, Ww)
        H.usr_fft_cols(H.USR_COL_DATA_FWD, P["T"], P["T"], P["FB"], P["FBFy"], S["FR"], P["invW"], ab[:, i], self.no, None,
                       planes, C, Hh, Ww, sf)
        H.usr_ifft_rows(P["T"], P["z"], False, C, 0, 1.0 / (Hh * Ww), planes, Hh, Ww)
        if P["pad"]:
            H.usr_pack_input(P["z"], ab[:, self.n + i], self.no, S["xin_u"], C8, B, C, Hh * Ww)
            H.usr_pad(S["xin_u"], S["xin"], H.USR_PAD_REPLICATE, C8, B, Hh, Ww, P["Hp"], P["Wp"])
        else:
            H.usr_pack_input(P["z"], ab[:, self.n + i], self.no, S["xin"], C8, B, C, Hh * Ww)

    def _prior_fwd(self, P, S):
        """x = ResUNet(xin) on the (padded) grid, cropped back to the HR size."""
        xo = S["xout_p"] if P["pad"] else S["xout"]
        self._unet_fwd(P, S, S["xin"], xo)
        if P["pad"]:   # x[..., :h, :w] (v1:164)
            H.usr_pad(xo, S["xout"], H.USR_CROP_NCHW, 0, P["B"] * self.out_nc, P["H"], P["W"], P["Hp"], P["Wp"])

    # ------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------
    def backward_from_loss(self, H_img, grads, loss_weight=1.0, charb_eps=None, loss_type=None):
        P = self.cur
        self.pixel_loss(P, P["it"][-1]["xout"], H_img, P["gE"], C8, loss_weight, self.out_nc, P["H"], P["W"],
                        charb_eps=charb_eps, loss_type=loss_type)
        P["e_g"] = self._x3_grad_exp(P["B"] * self.out_nc * P["H"] * P["W"], loss_weight, loss_type)
        self.backward(grads, P)
        return P["loss"]

    def backward_from_grad(self, gE, grads):
        P = self.cur
        H.image_to_nhwc(gE.contiguous(), P["gE"], C8, None, 1.0, P["B"], self.out_nc, P["H"], P["W"])
        self._x3_set_grad_exp(P, gE)
        self.backward(grads, P)

    def backward(self, grads, P):
        B, C, Hh, Ww, sf, n = P["B"], self.out_nc, P["H"], P["W"], P["sf"], self.n
        planes, inv_n = B * C, 1.0 / (Hh * Ww)
        ab, gab = P["ab"], P["gab"]
        # fp32x3: backward GEMM A operands are data gradients.  One exponent serves every stage (measured at
        # n_iter = 6, DESIGN.md 3a "USRNet": the bars hold with two orders of magnitude to spare)
        self._ax = P.get("e_g", 0)
        for i in range(n - 1, -1, -1):
            S = P["it"][i]
            gE = P["gE"]
            if P["pad"]:   # adjoint of the crop: the output gradient on the padded grid, zeros outside
                H.usr_pad(gE, P["gE_p"], H.USR_PAD_ZERO, C8, B, Hh, Ww, P["Hp"], P["Wp"])
                gE = P["gE_p"]
            self._unet_bwd(P, S, S["xin"], gE, P["gxin"], grads, acc=i < n - 1)
            gxin = P["gxin"]
            if P["pad"]:   # adjoint of the replicate pad: pad pixels' gradients onto the edge they copied
                gxin = P["gxin_u"]
                H.usr_pad(P["gxin"], gxin, H.USR_PAD_FOLD, C8, B, Hh, Ww, P["Hp"], P["Wp"])
            # beta_i: channel C of the ResUNet input gradient, summed over pixels
            H.usr_chan_sum(gxin, C8, C, Hh * Ww, B, P["cs_ws"], gab[:, n + i], self.no)
            # DataNet_i backward: dL/dx_{i-1} (skipped for i = 0: the upsampled LQ needs none) and dL/dalpha_i
            H.usr_fft_rows(gxin, H.USR_SRC_NHWC, C, C8, 0, 0, 1, P["T"], planes, Hh, Ww)
            H.usr_fft_cols(H.USR_COL_DATA_BWD, P["T"], P["T"] if i > 0 else None, P["FB"], P["FBFy"], S["FR"], P["invW"],
                           ab[:, i], self.no, P["a_ws"], planes, C, Hh, Ww, sf)
            H.usr_seg_sum(P["a_ws"], C * (Ww // sf), B, inv_n, gab[:, i], self.no)
            if i > 0:
                H.usr_ifft_rows(P["T"], P["gE"], True, C, C8, inv_n, planes, Hh, Ww)
        hp = self._hyp()
        H.hypanet_bwd(P["sig"], float(sf), *hp, self.hc, self.no, B, gab, *[grads[t] for t in hp])

