"""SwinIR reconstruction tails (network_swinir.py:815-836): P['fb'] (conv_after_body + long skip) -> the image
P['E'], and back from P['dE'] to P['dfb'].  One class per upsampler owns that tail's layer objects, plan buffers and
launch sequences; SwinIREngine holds `tail = make_tail(self, net)` and never asks which kind it is.

Every method takes the engine: a tail must not store it (SwinIR._apply / set_compute_dtype drop the engine and count
on refcounting to release its plans' HBM at once, which an engine <-> tail cycle would leave to the collector).
"""
import math

import torch

from .. import _hip as H
from .base import _Conv, _rup

NF = 64   # the tail's feature width (num_feat, network_swinir.py:741)


class _Tail:
    MODS = ()   # the network's tail modules, in registration order

    def params(self, net):
        """The tail's parameters: what grad_segments() appends after norm and conv_after_body."""
        return [p for name in self.MODS for p in getattr(net, name).parameters()]

    def plan_forward(self, eng, P, e):
        pass

    def colsum_widths(self):
        """Np of every eng._bias_colsum the tail's backward can issue (sizes P['colsum_ws'])."""
        return []

    def loss(self, eng, P, H_img, wr, charb_eps, loss_type=None):
        """L1 / Charbonnier / SSIM loss into P['loss'], its gradient into the P['dE'] rows."""
        eng.pixel_loss(P, P["E"], H_img, P["dE"], P.get("dE_ld", 16), wr, eng.in_ch, P["H"] * eng.scale,
                       P["W"] * eng.scale, charb_eps=charb_eps, loss_type=loss_type)

    def scatter_grad(self, eng, P, gE, inv):
        """An upstream dL/dE (NCHW fp32) times inv into the P['dE'] rows."""
        H.image_to_nhwc(gE.contiguous(), P["dE"], P.get("dE_ld", 16), None, inv, P["B"], eng.in_ch, P["H"] * eng.scale,
                        P["W"] * eng.scale)


class PixelShuffleTail(_Tail):
    """Classical SR: conv_before_upsample + LeakyReLU 0.01, one conv + PixelShuffle per stage, conv_last."""
    MODS = ("conv_before_upsample", "upsample", "conv_last")

    def __init__(self, eng, net):
        self.cbu = _Conv(eng, net.conv_before_upsample[0], NF, eng.Cp, wr=eng.conv_wr)
        # split_act: a0 / the upsampled activations are stored as [hi | lo] pairs (128 channels), read by
        # the upsampling convs through weights tied over both halves (the halo kernel skips lo . lo)
        # (output channels sub-pixel-major, PSHUF_SPM)
        self.ups = [_Conv(eng, m, m.out_channels, NF, n_perm=m.out_channels // NF, tied_in=eng.split_act,
                          fwd_cip=2 * NF if eng.split_act else None, wr=eng.conv_wr)
                    for m in net.upsample if isinstance(m, torch.nn.Conv2d)]
        self.ups_r = [int(math.isqrt(c.Co // NF)) for c in self.ups]
        # conv_last 64 -> in_ch on the narrow-output kernels (bf16 engine; HR width a multiple of 16)
        # (per call: the HR width must be a multiple of 64, else the implicit-GEMM path runs)
        self.last_narrow = eng.tdt == torch.bfloat16 and eng.split_conv and eng.in_ch <= 4
        self.last = _Conv(eng, net.conv_last, 16, NF, narrow=self.last_narrow)
        # ... and their fp32x3 forms (csrc/tail.hip *_x3: fp16 pairs of the fp32 operands, as kair_gemm_nt_x3)
        self.last_narrow_x3 = eng.x3 and eng.in_ch <= 4

    def convs(self):
        return [self.cbu] + self.ups + [self.last]

    def plan_forward(self, eng, P, e):
        # split_act: [hi | lo] pair rows (ld 2 NF); the backward reads the hi half as its bf16 operand
        tl = P["tail_ld"] = 2 * NF if eng.split_act else NF
        P["a0"] = e(P["M"], tl, dt=eng.tdt)
        acts, hw = [], P["M"]
        for r in self.ups_r:
            hw *= r * r
            acts.append(e(hw, tl, dt=eng.tdt))
        P["ups_act"] = acts
        P["M_hr"] = hw
        if self.last_narrow_x3:
            P["narrow_fws"] = e(H.conv3x3_narrow_x3_ws())

    def plan_backward(self, eng, P, e):
        # the HR-image gradient rows: 4 fp32 slots when only the fp32x3 narrow kernels read them (conv_last at
        # an HR width % 64 == 0), else the 16 slots of the implicit-GEMM conv_last's K = 9 x 16
        P["dE_ld"] = 4 if self.last_narrow_x3 and (P["W"] * eng.scale) % 64 == 0 else 16
        P["dE"] = e(P["M_hr"], P["dE_ld"], dt=eng.tdt)
        if self.last.narrow or self.last_narrow_x3:
            P["narrow_ws"] = e(H.conv3x3_narrow_wgrad_ws(eng.in_ch))
            P["narrow_dws"] = e(H.conv3x3_narrow_x3_ws() if eng.x3 else H.conv3x3_narrow_dgrad_ws())
        dpre, hw = [], P["M"]
        for c in self.ups:
            dpre.append(e(hw, c.Co, dt=eng.tdt))
            hw *= c.Co // NF
        P["dpre"] = dpre
        P["da0"] = e(P["M"], NF, dt=eng.tdt)

    def wgrad_shapes(self, eng, M):
        out, hw = [(M, NF, 9 * eng.Cp)], M
        for c in self.ups:
            out.append((hw, c.Co, 9 * NF))
            hw *= c.Co // NF
        return out + [(hw, 16, 9 * NF)]

    def colsum_widths(self):
        return [16] + [c.Co for c in self.ups]

    def forward(self, eng, P):
        Cp, M, B, Hh, Ww = eng.Cp, P["M"], P["B"], P["H"], P["W"]
        sa, tl = eng.split_act, P["tail_ld"]
        lo = (lambda t: t[:, NF:]) if sa else (lambda t: None)   # the lo half of a pair buffer
        c = self.cbu
        if eng._wr_ok(c.wr_n64, 1, B, Hh, Ww, Cp, NF):
            H.conv3x3_wr(P["fb"], Cp, 0, c.Wc15, c.bp, None, P["a0"], B, Hh, Ww, Cp, NF, ldo=tl, split=True,
                         out_lo=lo(P["a0"]), act=H.ACT_LEAKY, slope=0.01)
        else:
            eng._nt(eng._ain(H.im2col(P["fb"], Hh, Ww, Cp)), c.fwd(),
                    H.epilogue(P["a0"], ldo=tl, bias=c.bp, act=H.ACT_LEAKY, slope=0.01, out_lo=lo(P["a0"])), M, NF,
                    9 * Cp)
        src, h, w = P["a0"], Hh, Ww
        for c, r, dst in zip(self.ups, self.ups_r, P["ups_act"]):
            if eng._wr_ok(c.wr_pair, 1, B, h, w, NF, c.Co):   # kair_conv3x3_wr, pair form
                H.conv3x3_wr(src, tl, 0, c.Wp15, c.bp, None, dst, B, h, w, NF, c.Co, ldo=tl, split=True,
                             out_lo=lo(dst), ps_r=r)
            else:
                A = H.asplit(H.im2col(src, h, w, c.fcip), pair=True) if sa else H.im2col(src, h, w, NF)
                eng._nt(A, c.fwd(), H.epilogue(dst, mode=H.OUT_PSHUF_SPM, ldo=tl, bias=c.bp, ps=(r, h, w), out_lo=lo(dst)),
                        B * h * w, c.Co, 9 * c.fcip)
            src, h, w = dst, h * r, w * r
        c = self.last
        if self.last_narrow_x3 and w % 64 == 0:
            H.conv3x3_narrow_fwd_x3(src, tl, eng.X3_AEXP, c.w.detach(), c.bp, eng.in_ch, P["narrow_fws"], eng.mean,
                                    eng.img_range, None, P["E"], B, h, w)
        elif c.narrow and w % 64 == 0:   # 64 -> in_ch: the narrow-output kernel (weights in VGPRs)
            H.conv3x3_narrow_fwd(src, tl, NF if sa else 0, c.Wn, c.bp, eng.in_ch, eng.mean, eng.img_range, None,
                                 P["E"], B, h, w)
        else:
            eng._nt(eng._ain(H.im2col(src, h, w, NF, ld=tl), lo(src)), c.fwd(),
                    H.epilogue(P["E"], mode=H.OUT_NCHW, ldo=0, bias=c.bp, img=(eng.mean, eng.img_range, eng.in_ch, h, w)),
                    B * h * w, c.Cop, 9 * NF)
        return P["E"]

    def backward(self, eng, P, grads):
        Cp, M, B, Hh, Ww = eng.Cp, P["M"], P["B"], P["H"], P["W"]
        g = lambda p: grads[p]
        h, w = Hh, Ww
        for r in self.ups_r:
            h, w = h * r, w * r
        c = self.last
        src = P["ups_act"][-1]
        tl = P["tail_ld"]   # the activations' row stride (a [hi | lo] pair under split_act: the hi half is read)
        # conv_last: dgrad into the pre-shuffle layout of the last upsampling conv
        r_last = self.ups_r[-1]
        if self.last_narrow_x3 and w % 64 == 0:
            H.conv3x3_narrow_dgrad_x3(P["dE"], P["dE_ld"], P["e_g"], c.w.detach(), eng.in_ch, P["narrow_dws"], P["dpre"][-1],
                                      self.ups[-1].Co, r_last, B, h, w)
            H.conv3x3_narrow_wgrad_x3(P["dE"], P["dE_ld"], P["e_g"], src, tl, eng.X3_AEXP, eng.in_ch, P["narrow_ws"], g(c.w),
                                      g(c.b), B, h, w)
        elif c.narrow and w % 64 == 0:   # the narrow-output kernels (rolling row window, fp32 master weight)
            H.conv3x3_narrow_dgrad(P["dE"], 16, c.w.detach(), eng.in_ch, P["narrow_dws"], P["dpre"][-1], self.ups[-1].Co,
                                   r_last, B, h, w)
            H.conv3x3_narrow_wgrad(P["dE"], 16, src, tl, eng.in_ch, P["narrow_ws"], g(c.w), g(c.b), B, h, w)
        else:
            eng._nt(H.im2col(P["dE"], h, w, 16, flip=True), H.rows(c.Wd),
                    H.epilogue(P["dpre"][-1], mode=H.OUT_PUNSHUF_SPM, ldo=self.ups[-1].Co,
                               ps=(r_last, h // r_last, w // r_last)),
                    B * h * w, NF, 9 * 16)
            eng._wgrad(P, H.rows(P["dE"]), H.im2col(src, h, w, NF, ld=tl), B * h * w, 16, 9 * NF, c.map, g(c.w))
            eng._bias_colsum(P, H.rows(P["dE"]), B * h * w, 16, c.mapb, g(c.b))
        # upsampling convs, last to first
        for i in range(len(self.ups) - 1, -1, -1):
            c, r = self.ups[i], self.ups_r[i]
            h, w = h // r, w // r
            dpre = P["dpre"][i]
            src = P["ups_act"][i - 1] if i > 0 else P["a0"]
            wr_d = eng._wr_ok(c.wr_pair, 0, B, h, w, c.Co, NF)
            if wr_d and i > 0:   # kair_conv3x3_wr: PixelUnshuffle store into the previous conv's pre-shuffle rows
                rp = self.ups_r[i - 1]
                H.conv3x3_wr(dpre, c.Co, 1, c.Wp16, None, None, P["dpre"][i - 1], B, h, w, c.Co, NF,
                             ldo=self.ups[i - 1].Co, split=False, ps_r=-rp)
            elif wr_d:           # ... or the LeakyReLU'(a0) gate of conv_before_upsample's output
                H.conv3x3_wr(dpre, c.Co, 1, c.Wp16, None, None, P["da0"], B, h, w, c.Co, NF, split=False,
                             gate=P["a0"], ldg=tl, slope=0.01)
            elif i > 0:
                rp = self.ups_r[i - 1]
                eng._nt(H.im2col(dpre, h, w, c.Co, flip=True), H.rows(c.Wd),
                        H.epilogue(P["dpre"][i - 1], mode=H.OUT_PUNSHUF_SPM, ldo=self.ups[i - 1].Co,
                                   ps=(rp, h // rp, w // rp)),
                        B * h * w, NF, 9 * c.Co)
            else:
                eng._nt(H.im2col(dpre, h, w, c.Co, flip=True), H.rows(c.Wd),
                        H.epilogue(P["da0"], gate=P["a0"], ldg=tl, gate_kind=2, slope=0.01), M, NF, 9 * c.Co)
            eng._wgrad(P, H.rows(dpre), H.im2col(src, h, w, NF, ld=tl), B * h * w, c.Co, 9 * NF, c.map, g(c.w))
            eng._bias_colsum(P, H.rows(dpre), B * h * w, c.Co, c.mapb, g(c.b))
        c = self.cbu
        if eng._wr_ok(c.wr_n64, 0, B, Hh, Ww, NF, Cp):
            H.conv3x3_wr(P["da0"], NF, 1, c.Wc16, None, None, P["dfb"], B, Hh, Ww, NF, Cp, split=False)
        else:
            eng._nt(H.im2col(P["da0"], Hh, Ww, NF, flip=True), H.rows(c.Wd), H.epilogue(P["dfb"]), M, Cp, 9 * NF)
        eng._wgrad(P, H.rows(P["da0"]), H.im2col(P["fb"], Hh, Ww, Cp, ones_col=eng.C), M, NF, 9 * Cp, c.map,
                   g(c.w), g(c.b), eng.C)


class NearestConvTail(_Tail):
    """Real-world SR x4 (network_swinir.py:824-830): conv_before_upsample + LeakyReLU 0.01, two conv(nearest x2) +
    LeakyReLU 0.2 stages, conv_hr + LeakyReLU 0.2, conv_last."""
    MODS = ("conv_before_upsample", "conv_up1", "conv_up2", "conv_hr", "conv_last")

    def __init__(self, eng, net):
        self.cbu = _Conv(eng, net.conv_before_upsample[0], NF, eng.Cp)
        self.nup = [_Conv(eng, net.conv_up1, NF, NF), _Conv(eng, net.conv_up2, NF, NF)]
        self.hrc = _Conv(eng, net.conv_hr, NF, NF)
        self.last = _Conv(eng, net.conv_last, 16, NF)

    def convs(self):
        return [self.cbu] + self.nup + [self.hrc, self.last]

    def plan_forward(self, eng, P, e):
        M, T = P["M"], eng.tdt
        P["a0"] = e(M, NF, dt=T)
        P["nup_act"] = [e(4 * M, NF, dt=T), e(16 * M, NF, dt=T)]
        P["nhr"] = e(16 * M, NF, dt=T)
        P["M_hr"] = 16 * M

    def plan_backward(self, eng, P, e):
        M, T = P["M"], eng.tdt
        P["dE"] = e(16 * M, 16, dt=T)
        P["dz_hr"], P["dz_u"] = e(16 * M, NF, dt=T), e(16 * M, NF, dt=T)
        P["G_hi"], P["G_lo"] = e(16 * M, NF), e(4 * M, NF)
        P["da0"] = e(M, NF, dt=T)

    def wgrad_shapes(self, eng, M):
        return [(M, NF, 9 * eng.Cp), (4 * M, NF, 9 * NF), (16 * M, NF, 9 * NF), (16 * M, NF, 9 * NF), (16 * M, 16, 9 * NF)]

    def colsum_widths(self):
        return [self.last.Cop, self.hrc.Cop, NF]

    def forward(self, eng, P):
        Cp, M, B, h, w = eng.Cp, P["M"], P["B"], P["H"], P["W"]
        c = self.cbu
        eng._nt(H.im2col(P["fb"], h, w, Cp), c.fwd(),
                H.epilogue(P["a0"], bias=c.bp, act=H.ACT_LEAKY, slope=0.01), M, NF, 9 * Cp)
        src = P["a0"]
        # lrelu(conv(nearest x2)) twice -- im2col reads through the upsample -- then lrelu(conv_hr)
        for c, up, dst in zip(self.nup + [self.hrc], (2, 2, 1), P["nup_act"] + [P["nhr"]]):
            h, w = up * h, up * w
            eng._nt(H.im2col(src, h, w, NF, up=up), c.fwd(), H.epilogue(dst, bias=c.bp, act=H.ACT_LEAKY, slope=0.2),
                    B * h * w, NF, 9 * NF)
            src = dst
        c = self.last
        eng._nt(H.im2col(P["nhr"], h, w, NF), c.fwd(),
                H.epilogue(P["E"], mode=H.OUT_NCHW, ldo=0, bias=c.bp, img=(eng.mean, eng.img_range, eng.in_ch, h, w)),
                B * h * w, c.Cop, 9 * NF)
        return P["E"]

    def backward(self, eng, P, grads):
        """Each input gradient gated by LeakyReLU' in the dgrad epilogue (conv_hr, conv_up2) or after the 2x2
        sum-pool that is nearest x2's adjoint (conv_up2 -> up1 -> cbu)."""
        B, Hh, Ww, M, Cp = P["B"], P["H"], P["W"], P["M"], eng.Cp
        g = lambda p: grads[p]
        h, w = 4 * Hh, 4 * Ww
        ML = B * h * w
        # conv_last (16 padded outputs) then conv_hr: dz = the conv's output gradient, src its input activation
        for c, dz, src, dst in ((self.last, P["dE"], P["nhr"], P["dz_hr"]), (self.hrc, P["dz_hr"], P["nup_act"][1], P["dz_u"])):
            eng._nt(H.im2col(dz, h, w, c.Cop, flip=True), H.rows(c.Wd), H.epilogue(dst, gate=src, gate_kind=2, slope=0.2),
                    ML, NF, 9 * c.Cop)
            eng._wgrad(P, H.rows(dz), H.im2col(src, h, w, NF), ML, c.Cop, 9 * NF, c.map, g(c.w))
            eng._bias_colsum(P, H.rows(dz), ML, c.Cop, c.mapb, g(c.b))
        dz = P["dz_u"]
        for i in (1, 0):   # conv_up2 then conv_up1: dz = dL/d(pre-activation) on the (h, w) grid
            c = self.nup[i]
            Mi = B * h * w
            src = P["nup_act"][0] if i == 1 else P["a0"]
            G_hi = P["G_hi"][:Mi]
            eng._nt(H.im2col(dz, h, w, NF, flip=True), H.rows(c.Wd), H.epilogue(G_hi), Mi, NF, 9 * NF)
            eng._wgrad(P, H.rows(dz), H.im2col(src, h, w, NF, up=2), Mi, NF, 9 * NF, c.map, g(c.w))
            eng._bias_colsum(P, H.rows(dz), Mi, NF, c.mapb, g(c.b))
            h, w = h // 2, w // 2
            Mo = B * h * w
            G_lo = P["G_lo"][:Mo]
            H.sumpool2x(G_hi, NF, G_lo, NF, B, h, w, NF)
            nxt = P["dz_hr"][:Mo] if i == 1 else P["da0"]      # dz_hr is free again after conv_hr's wgrad
            H.act_grad_cast(G_lo, NF, src, NF, nxt, NF, Mo, NF, 2, 0.2 if i == 1 else 0.01)
            dz = nxt
        c = self.cbu
        eng._nt(H.im2col(P["da0"], Hh, Ww, NF, flip=True), H.rows(c.Wd), H.epilogue(P["dfb"]), M, Cp, 9 * NF)
        eng._wgrad(P, H.rows(P["da0"]), H.im2col(P["fb"], Hh, Ww, Cp, ones_col=eng.C), M, NF, 9 * Cp, c.map,
                   g(c.w), g(c.b), eng.C)


class _OneConvTail(_Tail):
    """A tail of one conv `self.c` from P['fb'] to the image; the subclass gives its store epilogue."""

    def convs(self):
        return [self.c]

    def plan_backward(self, eng, P, e):
        P["dE"] = e(P["M"], self.c.Cop, dt=eng.tdt)

    def wgrad_shapes(self, eng, M):
        return [(M, self.c.Cop, 9 * eng.Cp)]

    def forward(self, eng, P):
        c, Cp, Hh, Ww = self.c, eng.Cp, P["H"], P["W"]
        eng._nt(eng._ain(H.im2col(P["fb"], Hh, Ww, Cp)), c.fwd(), self._epilogue(eng, P, Hh, Ww), P["M"], c.Cop, 9 * Cp)
        return P["E"]

    def backward(self, eng, P, grads):
        c, Cp, M, Hh, Ww = self.c, eng.Cp, P["M"], P["H"], P["W"]
        eng._nt(H.im2col(P["dE"], Hh, Ww, c.Cop, flip=True), H.rows(c.Wd), H.epilogue(P["dfb"]), M, Cp, 9 * c.Cop)
        eng._wgrad(P, H.rows(P["dE"]), H.im2col(P["fb"], Hh, Ww, Cp, ones_col=eng.C), M, c.Cop, 9 * Cp, c.map,
                   grads[c.w], grads[c.b], eng.C)


class DirectTail(_OneConvTail):
    """Lightweight SR (pixelshuffledirect): one conv whose store is the PixelShuffle; P['dE'] holds its pre-shuffle rows."""
    MODS = ("upsample",)

    def __init__(self, eng, net):
        conv = net.upsample[0]
        self.c = _Conv(eng, conv, _rup(conv.out_channels, 16), eng.Cp)

    def _epilogue(self, eng, P, Hh, Ww):
        return H.epilogue(P["E"], mode=H.OUT_PSHUF_NCHW, ldo=0, bias=self.c.bp, ps=(eng.scale, Hh, Ww),
                          img=(eng.mean, eng.img_range, eng.in_ch, Hh, Ww))

    def loss(self, eng, P, H_img, wr, charb_eps, loss_type=None):
        eng.pixel_loss(P, P["E"], H_img, P["dE"], self.c.Cop, wr, eng.in_ch, P["H"] * eng.scale, P["W"] * eng.scale,
                       ps_r=eng.scale, charb_eps=charb_eps, loss_type=loss_type)

    def scatter_grad(self, eng, P, gE, inv):
        tmp = torch.nn.functional.pixel_unshuffle(gE.contiguous(), eng.scale)   # [B, C*r*r, H, W]
        H.image_to_nhwc(tmp.contiguous(), P["dE"], self.c.Cop, None, inv, P["B"], tmp.shape[1], P["H"], P["W"])


class PlainTail(_OneConvTail):
    """Denoising / JPEG (upsampler None or ''): E = x + conv_last(res) / range."""
    MODS = ("conv_last",)

    def __init__(self, eng, net):
        self.c = _Conv(eng, net.conv_last, 16, eng.Cp)

    def _epilogue(self, eng, P, Hh, Ww):
        # x/range + mean with x = (x_in - mean) * range + conv_last(res)  ==  x_in + conv_last(res) / range
        return H.epilogue(P["E"], mode=H.OUT_NCHW, ldo=0, bias=self.c.bp, resid=P["x"],
                          img=(None, eng.img_range, eng.in_ch, Hh, Ww))


def make_tail(eng, net):
    kinds = {"pixelshuffle": PixelShuffleTail, "pixelshuffledirect": DirectTail, "nearest+conv": NearestConvTail,
             None: PlainTail, "": PlainTail}
    if net.upsampler not in kinds:
        raise NotImplementedError(net.upsampler)
    return kinds[net.upsampler](eng, net)
