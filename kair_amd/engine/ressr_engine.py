"""Residual SR step program for MI355X: MSRResNet0, the DPSR prior (MSRResNet_prior) and IMDN.

The networks (models/network_msrresnet.py, network_dpsr.py, network_imdn.py; restated from upstream cszn/KAIR, the
reference sources were not at hand) share one shape:

    head conv -> body blocks under a long skip (ShortcutBlock) -> upsampler -> tail

and the engine is built from a spec of their modules, as RRDBNetEngine is:
    {"head", "blocks": [("res", c1, c2) | ("imd", c1, c2, c3, c4, c1x1)], "body_tail", "up", "hr", "last", "ps", "act",
     "slope"}.

Layout: NHWC feature rows.  A block's output lives twice, as fp32 rows (the next skip's `resid`, added in fp32 in the
last conv's epilogue) and as compute-dtype rows (the next conv's im2col operand).

ResBlock:  a = relu(conv1(x));  y = x + conv2(a)                                  (resid = x in conv2's epilogue)

IMDBlock (d = nc / 4, r = nc - d): ONE compute-dtype buffer D [M, 4 nc] = [o1 | o2 | o3 | d4, 0] per block, so neither
split nor cat materialises.  conv_j (j = 1..3) writes its nc channels (bias + LeakyReLU 0.05) into slice j through
ldo; conv_{j+1} reads the last r channels of slice j, a channel-offset im2col view (pixel stride 4 nc, K = 9 r: 216 at
nc 32, 432 at nc 64 -- the im2col loaders take any K % 8 == 0).  conv4 writes its d channels at the head of slice 4;
the r columns behind them are zero-filled by one small launch per block and step (kair_row_copy of a zero row), so that the 1 x 1 conv is a plain row
GEMM over all 4 nc columns with a packed weight that is zero outside the four d-wide groups (kair_wmap k groups
(4, d, nc)): 2.25 nc^2 more multiply-adds per pixel than the gathered K = 4 d form, 9 % of the block's 25.2 nc^2,
against the 25 % of padding every conv's reads to nc channels.  Its epilogue adds the block input (resid) in fp32.
Backward mirrors it: the 1 x 1 input gradient fills one fp32 buffer Gd [M, 4 nc] (exact zeros on the r columns, the
packed weight's zero rows), conv_{j+1}'s input gradient lands on the last r columns of slice j, and slice j is gated by
LeakyReLU' read from the saved post-activation slice; conv4 and conv1x1 carry no gate.

Upsampler / tail:
  'upconv' (MSRResNet, x2 / x4): conv over a nearest x2 read (im2col up=2) + ReLU, adjoint kair_sumpool2x; then
      conv + ReLU and the bias-free last conv storing the NCHW image -- RRDBNet's tail.
  'pixelshuffle' (MSRResNet, x2 / x3 / x4): conv(nc -> r^2 nc) + PixelShuffle(r) + ReLU.  ReLU commutes with the
      shuffle, so it runs in the conv epilogue, which stores sub-pixel-major (KAIR_OUT_PSHUF_SPM, weights packed with
      n_perm = r^2).  Backward: the ReLU gate is read from that shuffled activation and the gated gradient is written
      as the conv's pre-shuffle rows [M, r^2 nc] in one launch (kair_act_grad_punshuf: act_grad_cast through the
      inverse shuffle; the GEMM's own PUNSHUF_SPM gate wants the activation in the pre-shuffle layout, which the
      forward never stores).
  'pixelshuffle' last conv (IMDN): _rup(out_nc r^2, 16) <= 48 columns stored straight into the NCHW image
      (KAIR_OUT_PSHUF_NCHW), as SRMDEngine's; the fused losses write the gradient as pre-shuffle rows (ps_r = r).
The last conv of MSRResNet has bias=False: no bias pack, no column sum, no gradient entry (_Conv with mod.bias None).

bf16 engine: every forward and input-gradient product reads its weights as hi/lo bf16 pairs (kair_wmap kinds 9 / 18,
17 / 19 for the 1 x 1 conv), i.e. to ~16 bits of the fp32 master weight: with plainly rounded packs the x4 MSRResNet's
mean gradient error against float64 (tests/test_ressr_gpu.py, autograd kind) measured 0.116, above the 0.105 bar that
a float64 run with bf16-rounded storage alone meets at 0.104; with the pairs it is 0.096 (worst 0.153, bar 0.2).
Carrying the fp32 gradient rows as hi/lo pairs as well changed that figure by 1e-4 and is not done.

Every launch goes through _nt / conv_wgrad / _wgrad / gate_cast or one of the kair_* elementwise calls: no torch
compute op between forward and the end of backward, so the fused trainer captures the step.
"""
import torch
import torch.nn as nn

from .. import _hip as H
from .base import ConvEngineBase, _Conv, _rup


class _ConvS(_Conv):
    """_Conv whose input-gradient form is, like its forward form, a hi/lo bf16 pair per weight on the bf16 engine
    (kair_wmap kind 18: the rows of kind 2 as 64-column chunks alternating hi / lo), so that neither product sees
    bf16-rounded weights.  fp32 engine: _Conv."""

    def __init__(self, eng, mod, Cop, Cip, need_dgrad=True, n_perm=0):
        super().__init__(eng, mod, Cop, Cip, need_dgrad=need_dgrad, n_perm=n_perm)
        self.dsplit = self.split and need_dgrad
        if self.dsplit:
            self.mapd = H.wmap(18, self.Co, self.Ci, (1, self.Co, Cop), (1, self.Ci, Cip), n_perm=n_perm)
            self.Wd = torch.empty(Cip, 2 * _rup(9 * Cop, 64), device=self.w.device, dtype=torch.bfloat16)

    def dgrad(self):
        """The input-gradient GEMM's B operand."""
        return H.rows(self.Wd, w_split=self.dsplit)


class _Lin1x1:
    """IMDBlock.conv1x1 over the block buffer: forward [nc][4 nc] (kair_wmap kind 0, k groups (4, d, nc): zero outside
    the d-wide groups), input-gradient form [4 nc][nc] (kind 3); on the bf16 engine both as hi/lo pairs (kinds 17 /
    19)."""

    def __init__(self, eng, mod, nc, d):
        self.w, self.b = mod.weight, mod.bias
        self.Cop, self.Kp = nc, 4 * nc
        dev, kg = self.w.device, (4, d, nc)
        self.split = bool(eng.split_conv) and eng.tdt == torch.bfloat16
        self.map = H.wmap(0, nc, 4 * d, (1, nc, nc), kg)
        self.mapf = H.wmap(17 if self.split else 0, nc, 4 * d, (1, nc, nc), kg)
        self.mapd = H.wmap(19 if self.split else 3, nc, 4 * d, (1, nc, nc), kg)
        self.mapb = H.wmap(4, nc, 0, (1, nc, nc), (1, 1, 1))
        self.Wf = torch.empty(nc, 2 * _rup(4 * nc, 64) if self.split else 4 * nc, device=dev, dtype=eng.tdt)
        self.Wd = torch.empty(4 * nc, 2 * _rup(nc, 64) if self.split else nc, device=dev, dtype=eng.tdt)
        self.bp = torch.empty(nc, device=dev)

    def fwd(self):
        return H.rows(self.Wf, w_split=self.split)

    def dgrad(self):
        return H.rows(self.Wd, w_split=self.split)

    def pack_jobs(self):
        w = self.w.detach()
        return [(w, self.Wf, self.mapf), (w, self.Wd, self.mapd), (self.b.detach(), self.bp, self.mapb)]


def _check_conv(m, k=3):
    if not isinstance(m, nn.Conv2d) or m.kernel_size != (k, k) or m.stride != (1, 1) or m.padding != (k // 2, k // 2) \
            or m.groups != 1 or m.dilation != (1, 1):
        raise NotImplementedError(f"kair_amd ResSR: {k}x{k} / stride 1 / pad {k // 2} convs only (got {m})")


class ResSREngine(ConvEngineBase):
    COMPUTE_DTYPES = ("bf16", "fp32")
    SPLIT_W = True    # bf16: hi/lo weight pairs in the forward and input-gradient products (below)

    def __init__(self, net, compute_dtype="bf16", spec=None):
        super().__init__(net, compute_dtype)
        self.split_conv = bool(self.SPLIT_W) and compute_dtype == "bf16"
        if spec is None:
            spec = net.engine_spec()
        head = spec["head"]
        self.device = head.weight.device
        self.nc = nc = head.out_channels
        self.act, self.slope = spec["act"], float(spec["slope"])
        self.act_epi = H.ACT_LEAKY if self.act == 2 else H.ACT_RELU
        self.in_ch = head.in_channels
        self.Cin_p = _rup(self.in_ch, 8)
        self.r = int(spec["ps"])
        kinds = {b[0] for b in spec["blocks"]}
        if not spec["blocks"] or len(kinds) != 1 or not kinds <= {"res", "imd"}:
            raise NotImplementedError(f"kair_amd ResSR: one body block kind of 'res' / 'imd' (got {sorted(kinds)})")
        self.kind = kinds.pop()
        if nc % 8 or (self.kind == "imd" and nc % 32):
            raise NotImplementedError(f"kair_amd ResSR: nc must be a multiple of {32 if self.kind == 'imd' else 8} (got {nc})")
        self.d, self.rn = nc // 4, nc - nc // 4
        for m in [head, spec["body_tail"], spec["last"]] + list(spec["up"]) + ([spec["hr"]] if spec["hr"] else []):
            _check_conv(m)
        self.head = _ConvS(self, head, nc, self.Cin_p, need_dgrad=False)
        self.blocks_c = []
        for b in spec["blocks"]:
            for m in b[1:5 if self.kind == "imd" else 3]:
                _check_conv(m)
            if self.kind == "res":
                self.blocks_c.append([_ConvS(self, b[1], nc, nc), _ConvS(self, b[2], nc, nc)])
            else:
                _check_conv(b[5], 1)
                want = [(nc, nc), (nc, self.rn), (nc, self.rn), (self.d, self.rn)]
                if [(m.out_channels, m.in_channels) for m in b[1:5]] != want or b[5].in_channels != 4 * self.d:
                    raise NotImplementedError("kair_amd ResSR: IMDBlock with d = nc / 4 distilled channels")
                self.blocks_c.append([_ConvS(self, b[1], nc, nc), _ConvS(self, b[2], nc, self.rn),
                                      _ConvS(self, b[3], nc, self.rn), _ConvS(self, b[4], self.d, self.rn),
                                      _Lin1x1(self, b[5], nc, self.d)])
        if self.kind == "imd":
            self.zero_row = torch.zeros(1, self.rn, device=self.device)
        self.body_tail = _ConvS(self, spec["body_tail"], nc, nc)
        # 'pixelshuffle' upsampling convs: r^2 nc output channels stored sub-pixel-major (n_perm); 'upconv': r = 2
        self.up_r = list(spec.get("up_r") or [])
        self.up_ps = bool(self.up_r)
        if self.up_ps:
            if len(self.up_r) != len(spec["up"]) or any(m.out_channels != nc * r * r for m, r in zip(spec["up"], self.up_r)):
                raise NotImplementedError("kair_amd ResSR: a 'pixelshuffle' upsampling conv writes r^2 nc channels")
            self.up = [_ConvS(self, m, nc * r * r, nc, n_perm=r * r) for m, r in zip(spec["up"], self.up_r)]
        else:
            self.up_r = [2] * len(spec["up"])
            self.up = [_ConvS(self, m, nc, nc) for m in spec["up"]]
        self.hr = _ConvS(self, spec["hr"], nc, nc) if spec["hr"] is not None else None
        last = spec["last"]
        if self.r:    # the last conv runs on the LR grid and stores through PixelShuffle(r)
            if self.up or self.hr is not None or last.out_channels % (self.r * self.r):
                raise NotImplementedError("kair_amd ResSR: a pixel-shuffle last conv follows the body directly")
            if last.out_channels > 48:
                raise NotImplementedError(f"kair_amd ResSR: out_nc * upscale^2 must be <= 48 (got {last.out_channels})")
            self.out_ch, self.Cout_p = last.out_channels // (self.r * self.r), _rup(last.out_channels, 16)
        else:
            if not self.up or self.hr is None or last.out_channels > 16:
                raise NotImplementedError("kair_amd ResSR: the 'upconv' tail is upsampling convs, conv + act, conv (out_nc <= 16)")
            self.out_ch, self.Cout_p = last.out_channels, 16
        self.scale = self.r
        if not self.r:
            self.scale = 1
            for r in self.up_r:
                self.scale *= r
        self.last = _ConvS(self, last, self.Cout_p, nc)

    def convs(self):
        return ([self.head] + [c for b in self.blocks_c for c in b] + [self.body_tail] + self.up +
                ([self.hr] if self.hr is not None else []) + [self.last])

    # ------------------------------------------------------------------------------------
    def _build_plan(self, key, infer):
        B, Hh, Ww = key
        T, e, nc = self.tdt, self._e, self.nc
        M = B * Hh * Ww
        nb = len(self.blocks_c)
        P = {"B": B, "H": Hh, "W": Ww, "M": M}
        P["xin"] = e(M, self.Cin_p, dt=T)
        P["fea"], P["feab"] = e(M, nc), e(M, nc, dt=T)
        P["y"] = [e(M, nc), e(M, nc)]                                  # fp32 block outputs, ping-pong
        P["xb"] = [e(M, nc, dt=T) for _ in range(nb)]                  # compute-dtype block outputs
        if self.kind == "res":
            P["a"] = [e(M, nc, dt=T) for _ in range(nb)]
        else:
            P["D"] = [e(M, 4 * nc, dt=T) for _ in range(nb)]
        P["fea2b"] = e(M, nc, dt=T)
        levels, h, w = [], Hh, Ww
        for r in self.up_r:
            h, w = r * h, r * w
            levels.append((h, w))
        P["levels"] = levels
        P["upa"] = [e(B * hh * ww, nc, dt=T) for hh, ww in levels]
        HL, WL = (levels[-1] if levels else (Hh, Ww))
        ML = B * HL * WL
        P["ML"] = ML
        P["E"] = e(B, self.out_ch, self.scale * Hh, self.scale * Ww)
        Co = self.Cout_p
        if self.r:
            P["dEf"], P["dn"] = e(M, Co), e(M, Co, dt=T)
        else:
            P["hr"] = e(ML, nc, dt=T)
            P["dE"] = e(ML, Co, dt=T)
            P["G_hr"], P["dz_hr"], P["G_hi"] = e(ML, nc), e(ML, nc, dt=T), e(ML, nc)
            P["G_lv"] = [e(B * hh * ww, nc) for hh, ww in levels[:-1]]
            if self.up_ps:   # the gated gradient as pre-shuffle rows [rows of the conv grid, r^2 nc] (+ fp32 for the bias)
                P["dpre"] = e(ML * nc, dt=T)
                P["dpre_f"] = e(ML * nc) if T != torch.float32 else None
        P["Gt"], P["dzt"], P["gy"], P["G"] = e(M, nc), e(M, nc, dt=T), e(M, nc), e(M, nc)
        P["dz"] = e(M, nc, dt=T)
        if self.kind == "imd":
            P["Gd"], P["dz4"] = e(M, 4 * nc), e(M, self.d, dt=T)
        P["dzf"] = e(ML, nc)   # fp32 gradient rows before the compute-dtype cast (bias gradients)
        P["loss"], P["loss_ws"] = e(1), e(1024)
        P["colsum_ws"] = e(H.colsum_ws(max(c.Cop for c in self.convs())))
        shapes = [(M, nc, 9 * self.Cin_p), (M, nc, 9 * nc), (ML, Co, 9 * nc), (ML, nc, 9 * nc), (M, nc, 4 * nc)]
        shapes += [(B * hh * ww // (r * r), c.Cop, 9 * nc) for (hh, ww), r, c in zip(levels, self.up_r, self.up)]
        P["wg_ws"] = e(self.wgrad_ws_size(shapes))
        return P

    # ------------------------------------------------------------------------------------
    def forward(self, x, *cond):
        B, Cx, Hh, Ww = x.shape
        if Cx != self.in_ch:
            raise ValueError(f"kair_amd ResSR: the input has {Cx} channels, the head conv reads {self.in_ch}")
        P = self.plan(B, Hh, Ww)
        self.pack()
        nc, M = self.nc, P["M"]
        x = x.contiguous()
        self.cur = P
        H.image_to_nhwc(x, P["xin"], self.Cin_p, None, 1.0, B, self.in_ch, Hh, Ww)
        c = self.head
        self._nt(H.im2col(P["xin"], Hh, Ww, self.Cin_p), c.fwd(), H.epilogue(P["fea"], bias=c.bp), M, nc, 9 * self.Cin_p)
        H.row_copy(P["fea"], nc, M, nc, H.copy_desc(P["feab"]))
        xf, xb = P["fea"], P["feab"]
        for i, cs in enumerate(self.blocks_c):
            y = P["y"][i % 2]
            if self.kind == "res":
                self._res_fwd(P, i, cs, xf, xb, y)
            else:
                self._imd_fwd(P, i, cs, xf, xb, y)
            H.row_copy(y, nc, M, nc, H.copy_desc(P["xb"][i]))
            xf, xb = y, P["xb"][i]
        c = self.body_tail                   # ShortcutBlock: fea + conv(body)
        self._nt(H.im2col(xb, Hh, Ww, nc), c.fwd(), H.epilogue(P["fea2b"], bias=c.bp, resid=P["fea"]), M, nc, 9 * nc)
        src = P["fea2b"]
        if self.r:
            c = self.last
            self._nt(H.im2col(src, Hh, Ww, nc), c.fwd(),
                     H.epilogue(P["E"], mode=H.OUT_PSHUF_NCHW, ldo=0, bias=c.bp, ps=(self.r, Hh, Ww),
                                img=(None, 1.0, self.out_ch, Hh, Ww)), M, c.Cop, 9 * nc)
            return P["E"]
        for c, r, (hh, ww), dst in zip(self.up, self.up_r, P["levels"], P["upa"]):
            if self.up_ps:   # act(shuffle(conv)) = shuffle(act(conv)): the activation in the epilogue, sub-pixel-major store
                h, w = hh // r, ww // r
                self._nt(H.im2col(src, h, w, nc), c.fwd(),
                         H.epilogue(dst, mode=H.OUT_PSHUF_SPM, ldo=nc, bias=c.bp, act=self.act_epi, slope=self.slope,
                                    ps=(r, h, w)), B * h * w, c.Cop, 9 * nc)
            else:            # act(conv(nearest x2))
                self._nt(H.im2col(src, hh, ww, nc, up=2), c.fwd(),
                         H.epilogue(dst, bias=c.bp, act=self.act_epi, slope=self.slope), B * hh * ww, nc, 9 * nc)
            src = dst
        HL, WL = P["levels"][-1]
        ML = P["ML"]
        c = self.hr
        self._nt(H.im2col(src, HL, WL, nc), c.fwd(), H.epilogue(P["hr"], bias=c.bp, act=self.act_epi, slope=self.slope),
                 ML, nc, 9 * nc)
        c = self.last
        self._nt(H.im2col(P["hr"], HL, WL, nc), c.fwd(),
                 H.epilogue(P["E"], mode=H.OUT_NCHW, ldo=0, bias=c.bp, img=(None, 1.0, self.out_ch, HL, WL)), ML, c.Cop,
                 9 * nc)
        return P["E"]

    def _res_fwd(self, P, i, cs, xf, xb, y):
        nc, M, Hh, Ww = self.nc, P["M"], P["H"], P["W"]
        a = P["a"][i]
        c = cs[0]
        self._nt(H.im2col(xb, Hh, Ww, nc), c.fwd(), H.epilogue(a, bias=c.bp, act=self.act_epi, slope=self.slope), M, nc,
                 9 * nc)
        c = cs[1]
        self._nt(H.im2col(a, Hh, Ww, nc), c.fwd(), H.epilogue(y, bias=c.bp, resid=xf), M, nc, 9 * nc)

    def _imd_fwd(self, P, i, cs, xf, xb, y):
        nc, d, rn, M, Hh, Ww = self.nc, self.d, self.rn, P["M"], P["H"], P["W"]
        D, W4 = P["D"][i], 4 * self.nc
        c = cs[0]
        self._nt(H.im2col(xb, Hh, Ww, nc), c.fwd(),
                 H.epilogue(D[:, :nc], ldo=W4, bias=c.bp, act=self.act_epi, slope=self.slope), M, nc, 9 * nc)
        for j in (1, 2):                     # o_{j+1} = lrelu(conv_{j+1}(last r channels of o_j))
            c = cs[j]
            self._nt(H.im2col(D[:, (j - 1) * nc + d:], Hh, Ww, rn, ld=W4), c.fwd(),
                     H.epilogue(D[:, j * nc:(j + 1) * nc], ldo=W4, bias=c.bp, act=self.act_epi, slope=self.slope), M, nc,
                     9 * rn)
        c = cs[3]                            # d4 = conv4(last r channels of o3), no activation
        self._nt(H.im2col(D[:, 2 * nc + d:], Hh, Ww, rn, ld=W4), c.fwd(),
                 H.epilogue(D[:, 3 * nc:3 * nc + d], ldo=W4, bias=c.bp), M, d, 9 * rn)
        # the r columns behind d4: zeros, read by the 1 x 1 GEMM under zero weights (a fill from the engine's own zero
        # row, source row stride 0: it depends on no other buffer's contents)
        H.row_copy(self.zero_row, 0, M, rn, H.copy_desc(D[:, 3 * nc + d:], ld=W4))
        c = cs[4]                            # y = x + conv1x1(cat(d1, d2, d3, d4))
        self._nt(H.rows(D, ld=W4), c.fwd(), H.epilogue(y, bias=c.bp, resid=xf), M, nc, W4)

    # ------------------------------------------------------------------------------------
    def backward_from_loss(self, H_img, grads, loss_weight=1.0, charb_eps=None, loss_type=None):
        P = self.cur
        s = self.scale
        if self.r:
            self.pixel_loss(P, P["E"], H_img, P["dEf"], self.Cout_p, loss_weight, self.out_ch, s * P["H"], s * P["W"],
                            ps_r=self.r, charb_eps=charb_eps, loss_type=loss_type)
        else:
            self.pixel_loss(P, P["E"], H_img, P["dE"], self.Cout_p, loss_weight, self.out_ch, s * P["H"], s * P["W"],
                            charb_eps=charb_eps, loss_type=loss_type)
        self.backward(grads, P)
        return P["loss"]

    def backward_from_grad(self, gE, grads):
        P = self.cur
        if self.r:   # an upstream autograd gradient as pre-shuffle rows: torch's pixel_unshuffle, as SRMDEngine._pack_grad
            # does -- the autograd path is never captured; the fused trainer's step (backward_from_loss) has no torch op
            rows = torch.nn.functional.pixel_unshuffle(gE.contiguous(), self.r).contiguous()
            H.image_to_nhwc(rows, P["dEf"], self.Cout_p, None, 1.0, P["B"], self.out_ch * self.r * self.r, P["H"], P["W"])
        else:
            HL, WL = P["levels"][-1]
            H.image_to_nhwc(gE.contiguous(), P["dE"], self.Cout_p, None, 1.0, P["B"], self.out_ch, HL, WL)
        self.backward(grads, P)

    def backward(self, grads, P):
        nc, Co = self.nc, self.Cout_p
        B, Hh, Ww, M, ML = P["B"], P["H"], P["W"], P["M"], P["ML"]
        Gt = P["Gt"]                         # dL/d(fea + body)
        if self.r:
            c = self.last
            H.act_grad_cast(P["dEf"], Co, None, 0, P["dn"], Co, M, Co, 0)
            self._nt(H.im2col(P["dn"], Hh, Ww, Co, flip=True), c.dgrad(), H.epilogue(Gt), M, nc, 9 * Co)
            self.conv_wgrad(P, c, P["dn"], Co, H.im2col(P["fea2b"], Hh, Ww, nc), M, grads, P["dEf"], Co)
        else:
            HL, WL = P["levels"][-1]
            c = self.last                    # no bias
            self._nt(H.im2col(P["dE"], HL, WL, Co, flip=True), c.dgrad(), H.epilogue(P["G_hr"]), ML, nc, 9 * Co)
            self.conv_wgrad(P, c, P["dE"], Co, H.im2col(P["hr"], HL, WL, nc), ML, grads)
            c = self.hr
            bs = self.gate_cast(P, P["G_hr"], nc, P["hr"], nc, P["dz_hr"], nc, ML, nc, self.act, self.slope)
            G = P["G_hr"]                    # (consumed by the gate: reused for dL/d(last upsampling activation))
            self._nt(H.im2col(P["dz_hr"], HL, WL, nc, flip=True), c.dgrad(), H.epilogue(G), ML, nc, 9 * nc)
            self.conv_wgrad(P, c, P["dz_hr"], nc, H.im2col(P["upa"][-1], HL, WL, nc), ML, grads, *bs)
            for i in range(len(self.up) - 1, -1, -1):   # G = dL/d(post-activation output of up[i])
                c, (hh, ww), a = self.up[i], P["levels"][i], P["upa"][i]
                Mi = B * hh * ww
                src = P["upa"][i - 1] if i > 0 else P["fea2b"]
                Gn = P["G_lv"][i - 1] if i > 0 else Gt
                if self.up_ps:   # gate on the shuffled grid, stored as the conv's pre-shuffle rows
                    r = self.up_r[i]
                    h, w, Cq = hh // r, ww // r, c.Cop
                    Ml = B * h * w
                    dpre = P["dpre"][:Ml * Cq].view(Ml, Cq)
                    dpf = P["dpre_f"][:Ml * Cq].view(Ml, Cq) if P["dpre_f"] is not None else None
                    H.act_grad_punshuf(G, a, dpre, dpf, B, h, w, nc, r, self.act, self.slope)
                    self._nt(H.im2col(dpre, h, w, Cq, flip=True), c.dgrad(), H.epilogue(Gn), Ml, nc, 9 * Cq)
                    self.conv_wgrad(P, c, dpre, Cq, H.im2col(src, h, w, nc), Ml, grads, dpf if dpf is not None else dpre, Cq)
                    G = Gn
                    continue
                dz = P["dz_hr"][:Mi]
                bs = self.gate_cast(P, G, nc, a, nc, dz, nc, Mi, nc, self.act, self.slope)
                Ghi = P["G_hi"][:Mi]
                self._nt(H.im2col(dz, hh, ww, nc, flip=True), c.dgrad(), H.epilogue(Ghi), Mi, nc, 9 * nc)
                self.conv_wgrad(P, c, dz, nc, H.im2col(src, hh, ww, nc, up=2), Mi, grads, *bs)
                H.sumpool2x(Ghi, nc, Gn, nc, B, hh // 2, ww // 2, nc)
                G = Gn
        # body tail conv: fea2 = fea + conv(x_nb)
        c = self.body_tail
        gy = P["gy"]
        H.act_grad_cast(Gt, nc, None, 0, P["dzt"], nc, M, nc, 0)
        self._nt(H.im2col(P["dzt"], Hh, Ww, nc, flip=True), c.dgrad(), H.epilogue(gy), M, nc, 9 * nc)
        self.conv_wgrad(P, c, P["dzt"], nc, H.im2col(P["xb"][-1], Hh, Ww, nc), M, grads, Gt, nc)
        for i in range(len(self.blocks_c) - 1, -1, -1):   # gy = dL/d(block output) -> dL/d(block input)
            xb = P["xb"][i - 1] if i > 0 else P["feab"]
            if self.kind == "res":
                self._res_bwd(P, i, xb, grads)
            else:
                self._imd_bwd(P, i, xb, grads)
        # head conv: dL/d fea = the long skip (Gt) + the body (gy), added in fp32
        H.axpby(gy, Gt, 1.0, 1.0)
        H.act_grad_cast(gy, nc, None, 0, P["dzt"], nc, M, nc, 0)
        self.conv_wgrad(P, self.head, P["dzt"], nc, H.im2col(P["xin"], Hh, Ww, self.Cin_p), M, grads, gy, nc)

    def _res_bwd(self, P, i, xb, grads):
        nc, M, Hh, Ww = self.nc, P["M"], P["H"], P["W"]
        c1, c2 = self.blocks_c[i]
        gy, G, dz, a = P["gy"], P["G"], P["dz"], P["a"][i]
        H.act_grad_cast(gy, nc, None, 0, dz, nc, M, nc, 0)
        self._nt(H.im2col(dz, Hh, Ww, nc, flip=True), c2.dgrad(), H.epilogue(G), M, nc, 9 * nc)
        self.conv_wgrad(P, c2, dz, nc, H.im2col(a, Hh, Ww, nc), M, grads, gy, nc)
        bs = self.gate_cast(P, G, nc, a, nc, dz, nc, M, nc, self.act, self.slope)
        self.conv_wgrad(P, c1, dz, nc, H.im2col(xb, Hh, Ww, nc), M, grads, *bs)
        # dL/dx = gy (the skip, fp32) + conv1's input gradient, in place
        self._nt(H.im2col(dz, Hh, Ww, nc, flip=True), c1.dgrad(), H.epilogue(gy, resid=gy), M, nc, 9 * nc)

    def _imd_bwd(self, P, i, xb, grads):
        nc, d, rn, M, Hh, Ww = self.nc, self.d, self.rn, P["M"], P["H"], P["W"]
        cs, D, Gd, gy, dz, W4 = self.blocks_c[i], P["D"][i], P["Gd"], P["gy"], P["dz"], 4 * self.nc
        c = cs[4]                            # conv1x1: Gd = dL/d[o1 | o2 | o3 | d4, 0] (zeros on the r columns)
        H.act_grad_cast(gy, nc, None, 0, dz, nc, M, nc, 0)
        self._nt(H.rows(dz), c.dgrad(), H.epilogue(Gd), M, W4, nc)
        self._wgrad(P, H.rows(dz), H.rows(D, ld=W4), M, nc, W4, c.map, grads[c.w])
        H.colsum(H.rows(gy), M, nc, c.mapb, grads[c.b], P["colsum_ws"])
        c = cs[3]                            # conv4 (no gate): its input gradient is dL/d r3
        dz4 = P["dz4"]
        bs = self.gate_cast(P, Gd[:, 3 * nc:], W4, None, 0, dz4, d, M, d, 0)
        self._nt(H.im2col(dz4, Hh, Ww, d, flip=True), c.dgrad(), H.epilogue(Gd[:, 2 * nc + d:3 * nc], ldo=W4), M, rn,
                 9 * d)
        self.conv_wgrad(P, c, dz4, d, H.im2col(D[:, 2 * nc + d:], Hh, Ww, rn, ld=W4), M, grads, *bs)
        for j in (2, 1):                     # conv_{j+1}: gate slice j+1, input gradient onto the r columns of slice j
            c = cs[j]
            bs = self.gate_cast(P, Gd[:, j * nc:], W4, D[:, j * nc:], W4, dz, nc, M, nc, self.act, self.slope)
            self._nt(H.im2col(dz, Hh, Ww, nc, flip=True), c.dgrad(),
                     H.epilogue(Gd[:, (j - 1) * nc + d:j * nc], ldo=W4), M, rn, 9 * nc)
            self.conv_wgrad(P, c, dz, nc, H.im2col(D[:, (j - 1) * nc + d:], Hh, Ww, rn, ld=W4), M, grads, *bs)
        c = cs[0]
        bs = self.gate_cast(P, Gd, W4, D, W4, dz, nc, M, nc, self.act, self.slope)
        self.conv_wgrad(P, c, dz, nc, H.im2col(xb, Hh, Ww, nc), M, grads, *bs)
        self._nt(H.im2col(dz, Hh, Ww, nc, flip=True), c.dgrad(), H.epilogue(gy, resid=gy), M, nc, 9 * nc)
