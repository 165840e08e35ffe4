"""The ResUNet step program shared by USRNet's prior (network_usrnet_v1.py:109-166) and DRUNet's UNetRes
(network_unet.py): m_head; three levels of nb bias-free C-R-C ResBlocks, each followed by a 2x2 stride-2 conv;
m_body; three 2x2 stride-2 transposed convs, each followed by nb ResBlocks, the skips added before each up stage;
m_tail.

Implicit-GEMM 3x3 convs (im2col address map), the 2x2/stride-2 conv as a space-to-depth operand (KAIR_LD_S2D), the
2x2/stride-2 transposed conv as a 1x1 GEMM with a pixel-shuffle store, ReLU fused into the first conv of each
ResBlock, the ResBlock residual and the U-Net skip fused into the second conv's epilogue (two residual operands).
Backward mirrors it: ReLU' gate in the dgrad epilogue, transposed-conv dgrad through the space-to-depth operand,
stride-conv dgrad through the pixel-shuffle store, skip gradients added by the first ResBlock of each level.

Maps are NHWC fp32 token rows (ReLU outputs and GEMM-only operands in the compute dtype).  The input is an
8-channel NHWC operand (the head pack pads Cip to 8), the output an NCHW image written by the tail conv's epilogue,
the output gradient 8-channel rows.  The grid (P["Hp"], P["Wp"]) is a multiple of 8 in both directions and
B*Hp*Wp < 2^24.  ResUNetProgram holds the packs, the buffers and the two passes for bf16, exact fp32 and fp32x3;
the engine on top of it owns the plan, whatever feeds the input rows and what becomes of the output.
"""
import torch
import torch.nn as nn

from .. import _hip as H
from .base import ConvEngineBase

C8 = 8   # channel stride of the ResUNet input rows and of the tail-output gradient rows


def _ks(k):
    """Row length of a split-pair pack of k columns: 64-column chunks alternating hi / lo."""
    return 2 * (-(-k // 64)) * 64


def _mods(m):
    return list(m) if isinstance(m, nn.Sequential) else [m]


class _Packs:
    """A bias-free conv's two packs of its weight `w`: Wf / mapf (forward) and Wd / mapd (input gradient)."""

    def pack_jobs(self):
        w = self.w.detach()
        return [(w, self.Wf, self.mapf), (w, self.Wd, self.mapd)]


class _Conv3(_Packs):
    """Bias-free 3x3 conv: forward [Cop][9 Cip] (kind 1) and input-gradient [Cip][9 Cop] (kind 2) packs."""

    def __init__(self, eng, mod, Cop=None, Cip=None):
        self.w = mod.weight
        self.Co, self.Ci = self.w.shape[:2]
        self.Cop, self.Cip = Cop or self.Co, Cip or self.Ci
        grp = ((1, self.Co, self.Cop), (1, self.Ci, self.Cip))
        self.map = H.wmap(1, self.Co, self.Ci, *grp)      # the weight gradient's layout (wgrad_finalize)
        if eng.x3:   # fp16 pairs of w 2^X3_WEXP: kinds 9 / 18
            self.mapf, self.mapd = H.wmap(9, self.Co, self.Ci, *grp), H.wmap(18, self.Co, self.Ci, *grp)
            self.Wf = eng._e(self.Cop, _ks(9 * self.Cip), dt=torch.float16)
            self.Wd = eng._e(self.Cip, _ks(9 * self.Cop), dt=torch.float16)
        else:
            self.mapf, self.mapd = self.map, H.wmap(2, self.Co, self.Ci, *grp)
            self.Wf = eng._e(self.Cop, 9 * self.Cip, dt=eng.tdt)
            self.Wd = eng._e(self.Cip, 9 * self.Cop, dt=eng.tdt)


class _Down(_Packs):
    """Conv2d(Ci, Co, 2, stride 2, bias=False) (basicblock.downsample_strideconv, basicblock.py:495-501):
    forward through the space-to-depth operand with the [Co][4 Ci] pack (kind 7); input gradient as a
    1x1 GEMM into a pixel-shuffle store with the [4 Ci][Co] pack (kind 8); weight gradient kind 7.
    fp32x3: the fp16-pair forms of both packs (kinds 20 / 21)."""

    def __init__(self, eng, mod):
        self.w = mod.weight
        self.Co, self.Ci = self.w.shape[:2]
        self.map = H.wmap(7, self.Co, self.Ci)
        if eng.x3:
            self.mapf, self.mapd = H.wmap(20, self.Co, self.Ci), H.wmap(21, self.Co, self.Ci)
            self.Wf = eng._e(self.Co, _ks(4 * self.Ci), dt=torch.float16)
            self.Wd = eng._e(4 * self.Ci, _ks(self.Co), dt=torch.float16)
        else:
            self.mapf, self.mapd = self.map, H.wmap(8, self.Co, self.Ci)
            self.Wf = eng._e(self.Co, 4 * self.Ci, dt=eng.tdt)
            self.Wd = eng._e(4 * self.Ci, self.Co, dt=eng.tdt)


class _Up(_Packs):
    """ConvTranspose2d(Ci, Co, 2, stride 2, bias=False) (basicblock.upsample_convtranspose,
    basicblock.py:471-477), weight [Ci][Co][2][2]: forward as a 1x1 GEMM into a pixel-shuffle store
    with the [4 Co][Ci] pack (kind 8 over (Ci, Co)); input gradient through the space-to-depth operand
    with the [Ci][4 Co] pack (kind 7 over (Ci, Co)); weight gradient kind 7 over (Ci, Co).
    fp32x3: the fp16-pair forms of both packs (kinds 21 / 20)."""

    def __init__(self, eng, mod):
        self.w = mod.weight
        self.Ci, self.Co = self.w.shape[:2]
        self.map = H.wmap(7, self.Ci, self.Co)
        if eng.x3:
            self.mapf, self.mapd = H.wmap(21, self.Ci, self.Co), H.wmap(20, self.Ci, self.Co)
            self.Wf = eng._e(4 * self.Co, _ks(self.Ci), dt=torch.float16)
            self.Wd = eng._e(self.Ci, _ks(4 * self.Co), dt=torch.float16)
        else:
            self.mapf, self.mapd = H.wmap(8, self.Ci, self.Co), self.map
            self.Wf = eng._e(4 * self.Co, self.Ci, dt=eng.tdt)
            self.Wd = eng._e(self.Ci, 4 * self.Co, dt=eng.tdt)


class _RB:
    def __init__(self, eng, rb):
        self.c1, self.c2 = _Conv3(eng, rb.res[0]), _Conv3(eng, rb.res[2])


class ResUNetProgram(ConvEngineBase):
    """ConvEngineBase + the ResUNet: init_resunet(p) builds the packs of the module tree p (m_head .. m_tail),
    unet_state / unet_grad_scratch / unet_wgrad_shapes size a plan's buffers, _unet_fwd / _unet_bwd issue the passes.
    A plan P carries "B", "Hp", "Wp", "M" (unet_levels), "G" (unet_grad_scratch) and "wg_ws"; fp32x3: "e_g"."""
    NAME = "ResUNet"   # the network the error messages name

    def init_resunet(self, p):
        self.device = p.m_head.weight.device
        self.in_nc, self.out_nc = p.m_head.in_channels, p.m_tail.out_channels
        self.head = _Conv3(self, p.m_head, Cip=C8)
        self.tail = _Conv3(self, p.m_tail, Cop=C8)
        self.down_rbs, self.downs = [], []
        for d in (p.m_down1, p.m_down2, p.m_down3):
            ms = _mods(d)
            self.down_rbs.append([_RB(self, m) for m in ms[:-1]])
            self.downs.append(_Down(self, ms[-1]))
        self.body_rbs = [_RB(self, m) for m in _mods(p.m_body)]
        self.ups, self.up_rbs = [], []                 # m_up3 (-> level 2), m_up2 (-> 1), m_up1 (-> 0)
        for u in (p.m_up3, p.m_up2, p.m_up1):
            ms = _mods(u)
            self.ups.append(_Up(self, ms[0]))
            self.up_rbs.append([_RB(self, m) for m in ms[1:]])
        self.nc = [self.head.Co] + [d.Co for d in self.downs]
        if any(c % 8 for c in self.nc):
            raise NotImplementedError(f"kair_amd {self.NAME}: ResUNet channel counts must be multiples of 8")

    def resunet_convs(self):
        cs = [self.head, self.tail] + self.downs + self.ups
        for rbs in self.down_rbs + [self.body_rbs] + self.up_rbs:
            for rb in rbs:
                cs += [rb.c1, rb.c2]
        return cs

    # ---- plan pieces ----------------------------------------------------------------------
    def unet_levels(self, B, Hp, Wp):
        """Pixel rows of the four levels of a B x Hp x Wp grid."""
        M = [B * (Hp >> l) * (Wp >> l) for l in range(4)]
        if M[0] >= 1 << 24:
            raise NotImplementedError(f"kair_amd {self.NAME}: B*Hp*Wp must be < 2^24")
        return M

    def _chain(self, M, c, n):
        return [{"h": self._e(M, c, dt=self.tdt), "out": self._e(M, c)} for _ in range(n)]

    def unet_state(self, M):
        """The activations one pass keeps for its backward."""
        e, nc = self._e, self.nc
        return {"X": [e(M[l], nc[l]) for l in range(4)],
                "down": [self._chain(M[l], nc[l], len(self.down_rbs[l])) for l in range(3)],
                "body": self._chain(M[3], nc[3], len(self.body_rbs)),
                "t": [e(M[l], nc[l]) for l in range(3)],
                "up": [self._chain(M[l], nc[l], len(self.up_rbs[2 - l])) for l in range(3)]}

    def unet_grad_scratch(self, M):
        e, nc = self._e, self.nc
        return [{"gS": e(M[l], nc[l]), "gc": e(M[l], nc[l]), "ga": e(M[l], nc[l]), "gb": e(M[l], nc[l]),
                 "gz": e(M[l], nc[l], dt=self.tdt)} for l in range(4)]

    def unet_wgrad_shapes(self, M):
        nc = self.nc
        shapes = [(M[0], nc[0], 9 * C8), (M[0], C8, 9 * nc[0])]
        shapes += [(M[l], nc[l], 9 * nc[l]) for l in range(4)]
        shapes += [(M[l + 1], nc[l + 1], 4 * nc[l]) for l in range(3)]
        return shapes

    def _grid(self, P, l):
        """The ResUNet's level-l grid."""
        return P["Hp"] >> l, P["Wp"] >> l

    # ---- forward --------------------------------------------------------------------------
    def _chain_fwd(self, rbs, bufs, x, Hl, Wl, M, c, skip=None):
        """ResBlocks x + conv2(relu(conv1(x))); the last adds `skip` (the U-Net skip) too."""
        cur = x
        for j, (rb, S) in enumerate(zip(rbs, bufs)):
            self._nt(H.im2col(cur, Hl, Wl, c), H.rows(rb.c1.Wf), H.epilogue(S["h"], act=H.ACT_RELU), M, c, 9 * c)
            last = j == len(rbs) - 1
            self._nt(H.im2col(S["h"], Hl, Wl, c), H.rows(rb.c2.Wf),
                     H.epilogue(S["out"], resid=cur, resid2=skip if last else None), M, c, 9 * c)
            cur = S["out"]
        return cur

    def _unet_fwd(self, P, S, xin, xo):
        """xin: [M0, 8] input rows (compute dtype), kept for the backward; xo: the NCHW output [B, out_nc, Hp, Wp]."""
        nc, M = self.nc, P["M"]
        H0, W0 = self._grid(P, 0)
        self._nt(H.im2col(xin, H0, W0, C8), H.rows(self.head.Wf), H.epilogue(S["X"][0]), M[0], nc[0], 9 * C8)
        cur = S["X"][0]
        for l in range(3):
            Hl, Wl = self._grid(P, l)
            a = self._chain_fwd(self.down_rbs[l], S["down"][l], cur, Hl, Wl, M[l], nc[l])
            Hn, Wn = self._grid(P, l + 1)
            self._nt(H.s2d(a, Hn, Wn, nc[l]), H.rows(self.downs[l].Wf), H.epilogue(S["X"][l + 1]), M[l + 1], nc[l + 1],
                     4 * nc[l])
            cur = S["X"][l + 1]
        H3, W3 = self._grid(P, 3)
        s = self._chain_fwd(self.body_rbs, S["body"], cur, H3, W3, M[3], nc[3], skip=S["X"][3])
        for u in range(3):
            l = 2 - u                              # output level of m_up(3-u)
            Hs, Ws = self._grid(P, l + 1)
            self._nt(H.rows(s), H.rows(self.ups[u].Wf), H.epilogue(S["t"][l], mode=H.OUT_PSHUF, ldo=nc[l], ps=(2, Hs, Ws)),
                     M[l + 1], 4 * nc[l], nc[l + 1])
            Hl, Wl = self._grid(P, l)
            s = self._chain_fwd(self.up_rbs[u], S["up"][l], S["t"][l], Hl, Wl, M[l], nc[l], skip=S["X"][l])
        self._nt(H.im2col(s, H0, W0, nc[0]), H.rows(self.tail.Wf),
                 H.epilogue(xo, mode=H.OUT_NCHW, ldo=0, img=(None, 1.0, self.out_nc, H0, W0)), M[0], C8,
                 9 * nc[0])

    # ---- backward -------------------------------------------------------------------------
    def _chain_bwd(self, P, rbs, bufs, x_in, g, Hl, Wl, M, c, G, grads, acc, skip_g=None):
        """g: fp32 dL/d(chain output) -> returns fp32 dL/d(chain input) (+ skip_g, the U-Net skip)."""
        cur = g
        for j in range(len(rbs) - 1, -1, -1):
            rb, S = rbs[j], bufs[j]
            r_in = bufs[j - 1]["out"] if j > 0 else x_in
            self._nt(H.im2col(cur, Hl, Wl, c, flip=True), H.rows(rb.c2.Wd), H.epilogue(G["gz"], gate=S["h"], gate_kind=3),
                     M, c, 9 * c)
            self._wgrad(P, H.rows(cur), H.im2col(S["h"], Hl, Wl, c), M, c, 9 * c, rb.c2.map, grads[rb.c2.w], acc=acc)
            out = G["ga"] if cur is not G["ga"] else G["gb"]
            self._nt(H.im2col(G["gz"], Hl, Wl, c, flip=True), H.rows(rb.c1.Wd),
                     H.epilogue(out, resid=cur, resid2=skip_g if j == 0 else None), M, c, 9 * c)
            self._wgrad(P, H.rows(G["gz"]), H.im2col(r_in, Hl, Wl, c), M, c, 9 * c, rb.c1.map, grads[rb.c1.w], acc=acc)
            cur = out
        return cur

    def _unet_bwd(self, P, S, xin, gE, gxin, grads, acc):
        """gE: [M0, 8] output-gradient rows (compute dtype) on the ResUNet's grid; gxin: [M0, 8] fp32 rows that
        receive the input gradient, or None when the input needs none (the head's dgrad is then not issued); acc: add
        the weight gradients to `grads` (weights shared by several passes)."""
        nc, M, Gs = self.nc, P["M"], P["G"]
        H0, W0 = self._grid(P, 0)
        self._nt(H.im2col(gE, H0, W0, C8, flip=True), H.rows(self.tail.Wd), H.epilogue(Gs[0]["gS"]), M[0], nc[0],
                 9 * C8)
        s1 = S["up"][0][-1]["out"]
        self._wgrad(P, H.rows(gE), H.im2col(s1, H0, W0, nc[0]), M[0], C8, 9 * nc[0], self.tail.map, grads[self.tail.w],
                    acc=acc)
        g = Gs[0]["gS"]
        for u in (2, 1, 0):                        # m_up1, m_up2, m_up3
            l = 2 - u
            Hl, Wl = self._grid(P, l)
            gt = self._chain_bwd(P, self.up_rbs[u], S["up"][l], S["t"][l], g, Hl, Wl, M[l], nc[l], Gs[l], grads, acc)
            up = self.ups[u]
            Hs, Ws = self._grid(P, l + 1)
            s_next = S["body"][-1]["out"] if l == 2 else S["up"][l + 1][-1]["out"]
            self._nt(H.s2d(gt, Hs, Ws, nc[l]), H.rows(up.Wd), H.epilogue(Gs[l + 1]["gS"]), M[l + 1], nc[l + 1],
                     4 * nc[l])
            self._wgrad(P, H.rows(s_next), H.s2d(gt, Hs, Ws, nc[l]), M[l + 1], nc[l + 1], 4 * nc[l], up.map,
                        grads[up.w], acc=acc, act_rows=True)
            g = Gs[l + 1]["gS"]
        H3, W3 = self._grid(P, 3)
        gx = self._chain_bwd(P, self.body_rbs, S["body"], S["X"][3], Gs[3]["gS"], H3, W3, M[3], nc[3], Gs[3], grads, acc,
                             skip_g=Gs[3]["gS"])
        for l in (2, 1, 0):
            d = self.downs[l]
            Hn, Wn = self._grid(P, l + 1)
            Hl, Wl = self._grid(P, l)
            a = S["down"][l][-1]["out"]
            self._nt(H.rows(gx), H.rows(d.Wd), H.epilogue(Gs[l]["gc"], mode=H.OUT_PSHUF, ldo=nc[l], ps=(2, Hn, Wn)),
                     M[l + 1], 4 * nc[l], nc[l + 1])
            self._wgrad(P, H.rows(gx), H.s2d(a, Hn, Wn, nc[l]), M[l + 1], nc[l + 1], 4 * nc[l], d.map, grads[d.w], acc=acc)
            gx = self._chain_bwd(P, self.down_rbs[l], S["down"][l], S["X"][l], Gs[l]["gc"], Hl, Wl, M[l], nc[l], Gs[l],
                                 grads, acc, skip_g=Gs[l]["gS"])
        if gxin is not None:
            self._nt(H.im2col(gx, H0, W0, nc[0], flip=True), H.rows(self.head.Wd), H.epilogue(gxin), M[0], C8,
                     9 * nc[0])
        self._wgrad(P, H.rows(gx), H.im2col(xin, H0, W0, C8), M[0], nc[0], 9 * C8, self.head.map,
                    grads[self.head.w], acc=acc)
