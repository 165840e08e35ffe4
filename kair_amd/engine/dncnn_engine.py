"""DnCNN / FDnCNN / FFDNet / SRMD step program for MI355X.

Reference: /root/reference/models/network_dncnn.py:40-71 (DnCNN, out = x - model(x)), 128-149
(FDnCNN, out = model(x)); layers from basicblock.conv (basicblock.py:61-98).  SURVEY §8 row a14.  IRCNN, the same
file's third class (restated in network_dncnn.IRCNN), is the same loop with a dilation per conv.

Per body layer: implicit-GEMM 3x3 conv (bias in the epilogue) -> fp32 pre-norm rows z ->
BatchNorm (batch statistics + running-stat update in train mode, running statistics in eval) with
the activation fused into the normalise pass -> compute-dtype activation rows for the next conv.
Without BN the activation is fused into the conv epilogue.  Backward: BN backward fuses the
activation gate and the two per-channel reductions; conv input / weight / bias gradients as in the
other conv programs.

FFDNetEngine (below) runs the same layer loop over the half grid behind a PixelUnshuffle head (kair_ffd_pack) and a
PixelShuffle store; SRMDEngine runs it on the LR grid with a last conv of up to 48 columns behind a PixelShuffle(2 / 3 / 4)
store.  DnCNNEngine keeps what differs in the methods after convs().
"""
import torch
import torch.nn as nn

from .. import _hip as H
from .base import ConvEngineBase, _Conv, _rup


class DnCNNEngine(ConvEngineBase):
    COMPUTE_DTYPES = ("bf16", "fp32")

    def __init__(self, net, compute_dtype="bf16", residual=True, dil_kernel=True):
        """dil_kernel: bf16 engines run the dilated convs inside kair_conv3x3_dil's contract (IRCNN's 64 -> 64 layers,
        forward and input gradient) on that kernel; False, like every other dilated conv, on the dilated im2col
        operand of kair_gemm_nt (H.im2col(..., dil=d)).  Layers without dilation do not read it."""
        super().__init__(net, compute_dtype)
        self.residual = residual
        self.dil_kernel = bool(dil_kernel)
        mods = self._conv_modules(net)
        self.device = mods[0].weight.device
        layers, i = [], 0
        while i < len(mods):
            conv = mods[i]
            if not isinstance(conv, nn.Conv2d) or conv.kernel_size != (3, 3) or conv.stride != (1, 1):
                raise NotImplementedError("kair_amd DnCNN: 3x3 / stride 1 convs only")
            d = conv.dilation[0]
            if conv.dilation != (d, d) or conv.padding != (d, d) or not 1 <= d <= 4:
                raise NotImplementedError("kair_amd DnCNN: padding == dilation == (d, d) with d in 1..4 only (got padding "
                                          f"{conv.padding}, dilation {conv.dilation})")
            i += 1
            bn, act, slope = None, 0, 0.0
            if i < len(mods) and isinstance(mods[i], nn.BatchNorm2d):
                bn = mods[i]
                i += 1
            if i < len(mods) and isinstance(mods[i], (nn.ReLU, nn.LeakyReLU)):
                act = 1 if isinstance(mods[i], nn.ReLU) else 2
                slope = mods[i].negative_slope if act == 2 else 0.0
                i += 1
            layers.append((conv, bn, act, slope))
        self.in_ch = layers[0][0].in_channels
        self.out_ch = layers[-1][0].out_channels
        self.nc = layers[0][0].out_channels
        if self.nc % 8:
            raise NotImplementedError("kair_amd DnCNN: nc multiple of 8, out_nc <= 16")
        self.Cout_p = self._out_width()
        self.Cin_p = _rup(self.in_ch, 8)
        self.layers = []
        for li, (conv, bn, act, slope) in enumerate(layers):
            cop = self.Cout_p if li == len(layers) - 1 else conv.out_channels
            cip = self.Cin_p if li == 0 else conv.in_channels
            self.layers.append((_Conv(self, conv, cop, cip, need_dgrad=li > 0, dil=conv.dilation[0],
                                      dil_kernel=self.dil_kernel and li > 0), bn, act, slope))

    def convs(self):
        return [c for c, _, _, _ in self.layers]

    # ---- what a network with another head / tail overrides (FFDNetEngine, SRMDEngine) ----------
    def _conv_modules(self, net):
        """The modules of the conv stack, in order."""
        return list(net.model)

    def _out_width(self):
        """The padded width of the last conv's output rows (and of the gradient rows P['dEf'] / P['dn'])."""
        if self.out_ch > 16:
            raise NotImplementedError("kair_amd DnCNN: nc multiple of 8, out_nc <= 16")
        return 16

    def _grid(self, key):
        """The conv grid (rows, columns) of the plan keyed (B, h, w): the image itself."""
        return key[1], key[2]

    def _out_image(self, P, key):
        B, Hh, Ww = key
        return self._e(B, self.out_ch, Hh, Ww)

    def _pack_input(self, P, x, *cond):
        H.image_to_nhwc(x, P["xin"], self.Cin_p, None, 1.0, P["B"], self.in_ch, P["H"], P["W"])

    def _out_epilogue(self, P, c):
        return H.epilogue(P["E"], mode=H.OUT_NCHW, ldo=0, bias=c.bp, img=(None, 1.0, self.out_ch, P["H"], P["W"]))

    def _loss(self, P, H_img, loss_weight, charb_eps, loss_type=None):
        self.pixel_loss(P, P["E"], H_img, P["dEf"], self.Cout_p, loss_weight, self.out_ch, P["H"], P["W"],
                        charb_eps=charb_eps, loss_type=loss_type)

    def _pack_grad(self, P, gE):
        H.image_to_nhwc(gE.contiguous(), P["dEf"], self.Cout_p, None, 1.0, P["B"], self.out_ch, P["H"], P["W"])

    def _build_plan(self, key, infer):
        B = key[0]
        Hh, Ww = self._grid(key)
        T, e, nc = self.tdt, self._e, self.nc
        M = B * Hh * Ww
        P = {"B": B, "H": Hh, "W": Ww, "M": M}
        P["xin"] = e(M, self.Cin_p, dt=T)
        n_mid = len(self.layers) - 1
        P["a"] = [e(M, nc, dt=T) for _ in range(n_mid)]
        P["z"] = [e(M, nc) if bn is not None else None for _, bn, _, _ in self.layers[:n_mid]]
        P["mean"] = [e(nc) if bn is not None else None for _, bn, _, _ in self.layers[:n_mid]]
        P["rstd"] = [e(nc) if bn is not None else None for _, bn, _, _ in self.layers[:n_mid]]
        P["E"] = self._out_image(P, key)
        P["dEf"] = torch.zeros(M, self.Cout_p, device=self.device)
        P["dn"] = e(M, self.Cout_p, dt=T)
        P["G"], P["dz"] = e(M, nc), e(M, nc, dt=T)
        P["dzf"] = e(M, nc)   # fp32 gradient rows before the compute-dtype cast (bias gradients)
        P["bn_ws"] = e(H.bn_ws(nc))
        P["loss"], P["loss_ws"] = e(1), e(1024)
        P["colsum_ws"] = e(H.colsum_ws(max(c.Cop for c in self.convs())))
        shapes = [(M, c.Cop, 9 * c.Cip) for c, _, _, _ in self.layers]
        P["wg_ws"] = e(self.wgrad_ws_size(shapes))
        return P

    def _conv_fwd(self, P, c, src, ldsrc, Cs, out, bias, act=H.ACT_NONE, slope=0.0):
        """A body conv's forward product into the rows `out`: kair_conv3x3_dil where the layer is packed for it, else
        the implicit GEMM over the (dilated) im2col operand."""
        if c.dil_fast:
            H.conv3x3_dil(src, ldsrc, c.dil, False, c.Wk15, 15, bias, out, P["B"], P["H"], P["W"], Cs, c.Cop, act=act,
                          slope=slope)
        else:
            self._nt(H.im2col(src, P["H"], P["W"], Cs, ld=ldsrc, dil=c.dil), c.fwd(),
                     H.epilogue(out, bias=bias, act=act, slope=slope), P["M"], c.Cop, 9 * c.Cip)

    def forward(self, x, *cond):
        """cond: the network's extra forward inputs (FFDNet: sigma); the trainer's drop-path slot (None) otherwise."""
        B, _, h, w = x.shape
        P = self.plan(B, h, w)
        self.pack()
        nc = self.nc
        M, Hh, Ww = P["M"], P["H"], P["W"]
        x = x.contiguous()
        self.cur = P
        P["x"] = x
        training = self.net_ref().training
        self._pack_input(P, x, *cond)
        src, ldsrc, Cs = P["xin"], self.Cin_p, self.Cin_p
        for li, (c, bn, act, slope) in enumerate(self.layers[:-1]):
            a = P["a"][li]
            if bn is None:
                self._conv_fwd(P, c, src, ldsrc, Cs, a, c.bp,
                               (H.ACT_RELU if act == 1 else H.ACT_LEAKY) if act else H.ACT_NONE, slope)
            else:
                z = P["z"][li]
                self._conv_fwd(P, c, src, ldsrc, Cs, z, c.bp)
                H.bn_fwd(z, nc, a, nc, M, nc, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                         training, P["mean"][li], P["rstd"][li], act, slope, P["bn_ws"])
                if training:
                    bn.num_batches_tracked.add_(1)
            src, ldsrc, Cs = a, nc, nc
        c = self.layers[-1][0]
        self._nt(H.im2col(src, Hh, Ww, nc, dil=c.dil), c.fwd(), self._out_epilogue(P, c), M, c.Cop, 9 * nc)
        if self.residual:
            H.axpby(P["E"], x, 1.0, -1.0)     # x - model(x)
        return P["E"]

    def backward_from_loss(self, H_img, grads, loss_weight=1.0, charb_eps=None, loss_type=None):
        P = self.cur
        self._loss(P, H_img, loss_weight, charb_eps, loss_type)
        self.backward(grads, P)
        return P["loss"]

    def backward_from_grad(self, gE, grads):
        P = self.cur
        self._pack_grad(P, gE)
        self.backward(grads, P)

    def backward(self, grads, P):
        cd, nc, Co = self.cd, self.nc, self.Cout_p
        Hh, Ww, M = P["H"], P["W"], P["M"]
        # d model(x) = -dE for DnCNN (out = x - model(x)), dE for FDnCNN
        H.act_grad_cast(P["dEf"], Co, None, 0, P["dn"], Co, M, Co, 0, 0.0, -1.0 if self.residual else 1.0)
        c = self.layers[-1][0]
        G = P["G"]
        self._nt(H.im2col(P["dn"], Hh, Ww, Co, flip=True, dil=c.dil), H.rows(c.Wd), H.epilogue(G), M, nc, 9 * Co)
        self.conv_wgrad(P, c, P["dn"], Co, H.im2col(P["a"][-1], Hh, Ww, nc, dil=c.dil), M, grads)
        for li in range(len(self.layers) - 2, -1, -1):
            c, bn, act, slope = self.layers[li]
            a, dz = P["a"][li], P["dz"]
            if bn is not None:
                dzf = dz if cd == H.F32 else P["dzf"]
                H.bn_bwd(P["z"][li], nc, a, nc, G, nc, dzf, nc, M, nc, bn.weight, P["mean"][li], P["rstd"][li], act, slope,
                         grads[bn.weight], grads[bn.bias], False, P["bn_ws"])
                if cd != H.F32:
                    H.row_copy(dzf, nc, M, nc, H.copy_desc(dz))
                bs = (dzf, nc)
            else:
                bs = self.gate_cast(P, G, nc, a, nc, dz, nc, M, nc, act, slope)
            if li > 0:
                if c.dil_fast:   # the input gradient on the flipped taps, fp32 rows for gate_cast
                    H.conv3x3_dil(dz, nc, c.dil, True, c.Wk16, 16, None, G, P["B"], Hh, Ww, nc, nc)
                else:
                    self._nt(H.im2col(dz, Hh, Ww, nc, flip=True, dil=c.dil), H.rows(c.Wd), H.epilogue(G), M, nc, 9 * nc)
                self.conv_wgrad(P, c, dz, nc, H.im2col(P["a"][li - 1], Hh, Ww, nc, dil=c.dil), M, grads, *bs)
            else:
                self.conv_wgrad(P, c, dz, nc, H.im2col(P["xin"], Hh, Ww, self.Cin_p, dil=c.dil), M, grads, *bs)


class IRCNNEngine(DnCNNEngine):
    """IRCNN (network_dncnn.IRCNN): DnCNN's layer loop with a dilation per conv, no BatchNorm, out = x - model(x)."""

    def grad_segments(self):
        """One gradient segment: 0.19 M parameters are one all-reduce bucket."""
        return [list(self.net_ref().parameters())]


class FFDNetEngine(DnCNNEngine):
    """FFDNet (the restated reference forward, network_ffdnet.FFDNet): DnCNN's layer loop over the half grid.

    head: kair_ffd_pack -- ReplicationPad2d to even sizes, PixelUnshuffle(2) and the per-sample noise level as channel
          4 in_nc of the packed rows, one launch;
    tail: the last conv stores through KAIR_OUT_PSHUF_NCHW (ps_r = 2) straight into the NCHW image; an odd h or w
          stores into a plan-owned padded image whose [..., :h, :w] view is the output.
    Plans are keyed (B, h, w); the conv grid is ceil(h/2) x ceil(w/2).  out = model(x): no residual."""

    def __init__(self, net, compute_dtype="bf16"):
        super().__init__(net, compute_dtype, residual=False)
        if (self.in_ch - 1) % 4 or self.out_ch % 4:
            raise NotImplementedError("kair_amd FFDNet: the first conv reads 4 in_nc + 1 channels, the last writes 4 out_nc")
        self.img_in, self.img_out = (self.in_ch - 1) // 4, self.out_ch // 4

    def _grid(self, key):
        return (key[1] + 1) // 2, (key[2] + 1) // 2

    def _out_image(self, P, key):
        B, h, w = key
        P["h"], P["w"] = h, w
        P["Epad"] = self._e(B, self.img_out, 2 * P["H"], 2 * P["W"])
        return P["Epad"][..., :h, :w]   # (the whole image when h and w are even)

    def sigma_rows(self, sigma, B):
        """[B, 1, 1, 1], [B] or one element (broadcast) -> [B] fp32 on the device."""
        s = torch.as_tensor(sigma, dtype=torch.float32, device=self.device).reshape(-1)
        if s.numel() == 1 and B > 1:
            s = s.expand(B)
        if s.numel() != B:
            raise ValueError(f"kair_amd FFDNet: sigma holds {s.numel()} levels for a batch of {B}")
        return s.contiguous()

    def _pack_input(self, P, x, sigma=None):
        if sigma is None:
            raise ValueError("kair_amd FFDNet: forward(x, sigma) needs the noise level")
        P["sigma"] = self.sigma_rows(sigma, P["B"])
        H.ffd_pack(x, P["sigma"], P["xin"], self.Cin_p, P["B"], self.img_in, P["h"], P["w"])

    def _out_epilogue(self, P, c):
        return H.epilogue(P["Epad"], mode=H.OUT_PSHUF_NCHW, ldo=0, bias=c.bp, ps=(2, P["H"], P["W"]),
                          img=(None, 1.0, self.img_out, P["H"], P["W"]))

    def _loss(self, P, H_img, loss_weight, charb_eps, loss_type=None):
        if P["h"] % 2 or P["w"] % 2:
            raise ValueError(f"kair_amd FFDNet: the fused loss needs even sizes (got {P['h']} x {P['w']}); odd sizes run "
                             "forward and the autograd backward")
        self.pixel_loss(P, P["Epad"], H_img, P["dEf"], 16, loss_weight, self.img_out, P["h"], P["w"], ps_r=2,
                        charb_eps=charb_eps, loss_type=loss_type)

    def _pack_grad(self, P, gE):
        H.ffd_pack(gE.contiguous(), None, P["dEf"], 16, P["B"], self.img_out, P["h"], P["w"])


class SRMDEngine(DnCNNEngine):
    """SRMD (network_srmd.SRMD): DnCNN's layer loop on the LR grid, no BatchNorm, no residual.

    head: the LR image and its degradation-map channels arrive as one [B, in_nc, h, w] tensor; kair_image_to_nhwc packs
          it into rows of _rup(in_nc, 8) channels (24 for 16..19), pad channels zero;
    tail: the last conv has _rup(out_nc r^2, 16) output columns (16 / 32 / 48) and stores through KAIR_OUT_PSHUF_NCHW
          (ps_r = r) straight into the [B, out_nc, r h, r w] image.  The HR-grid gradient reaches it as pre-shuffle rows
          [M, Cop]: the fused pixel losses write them (ps_r = r, pad columns zero), an upstream autograd gradient goes
          through pixel_unshuffle and kair_image_to_nhwc (outside any captured step).
    Plans are keyed (B, h, w) of the LR input."""

    def __init__(self, net, compute_dtype="bf16"):
        self.r = int(net.upscale)
        super().__init__(net, compute_dtype, residual=False)
        if self.out_ch % (self.r * self.r):
            raise NotImplementedError("kair_amd SRMD: the last conv writes out_nc * upscale^2 channels")
        self.img_out = self.out_ch // (self.r * self.r)

    def _conv_modules(self, net):
        mods = list(net.model)
        if not isinstance(mods[-1], nn.PixelShuffle) or mods[-1].upscale_factor != self.r:
            raise NotImplementedError("kair_amd SRMD: the conv stack ends in PixelShuffle(upscale)")
        return mods[:-1]

    def _out_width(self):
        if self.out_ch > 48:
            raise NotImplementedError(f"kair_amd SRMD: out_nc * upscale^2 must be <= 48 (got {self.out_ch})")
        return _rup(self.out_ch, 16)

    def grad_segments(self):
        """One gradient segment: 1.5 M parameters are one all-reduce bucket."""
        return [list(self.net_ref().parameters())]

    def _out_image(self, P, key):
        B, h, w = key
        return self._e(B, self.img_out, self.r * h, self.r * w)

    def _out_epilogue(self, P, c):
        return H.epilogue(P["E"], mode=H.OUT_PSHUF_NCHW, ldo=0, bias=c.bp, ps=(self.r, P["H"], P["W"]),
                          img=(None, 1.0, self.img_out, P["H"], P["W"]))

    def _loss(self, P, H_img, loss_weight, charb_eps, loss_type=None):
        self.pixel_loss(P, P["E"], H_img, P["dEf"], self.Cout_p, loss_weight, self.img_out, self.r * P["H"],
                        self.r * P["W"], ps_r=self.r, charb_eps=charb_eps, loss_type=loss_type)

    def _pack_grad(self, P, gE):
        rows = torch.nn.functional.pixel_unshuffle(gE.contiguous(), self.r).contiguous()   # [B, out_nc r^2, h, w]
        H.image_to_nhwc(rows, P["dEf"], self.Cout_p, None, 1.0, P["B"], self.out_ch, P["H"], P["W"])
