"""SCUNet (Swin-Conv-UNet) step program for MI355X: the residual U-Net skeleton of the ResUNet program (3x3 head / tail,
2x2 stride-2 convs as space-to-depth operands, 2x2 transposed convs as 1x1 GEMMs with a pixel-shuffle store, the U-Net
skips fused into the last block of each stage) with a ConvTransBlock in place of every ResBlock.

One ConvTransBlock over the level's [M, 2C] fp32 token rows X (C = conv_dim = trans_dim, nh = C / 32 heads):

  Y        = conv1_1(X)                                     rows GEMM + bias                     [M, 2C]
  Z[:, :C] = conv2(relu(conv1(Y[:, :C]))) + Y[:, :C]        im2col views with pixel stride 2C, residual in the epilogue
  ln1      = LN1(Y[:, C:])  (window order)  -> q/k/v (head-blocked) -> kair_window_attn_fwd_w (ws 8, head dim = head
             pad = 32, shift 4 for 'SW', the analytic Swin mask, the bias table packed as [(2ws-1)^2][nh])
  mid      = Y[:, C:] + linear(O)                           window -> token row map + residual in the epilogue
  Z[:, C:] = mid + fc2(gelu(fc1(LN2(mid))))
  out      = X + conv1_2(Z) (+ the U-Net skip on the last block of a stage)

The split and the cat never materialise: both halves address the columns of Y / Z through ldx / ldo / ldr.  The backward
mirrors it; the two halves' input gradients are finished in place in one [M, 2C] buffer.  At head dim 32 = head pad no
layout has a spare ones column (and LayerNorm's ldy <= 256 leaves none at C = 256), so at every width the Linear / 1x1
biases enter through kair_epilogue.bias and their gradients are column sums: kair_colsum for plain rows,
kair_qkvblk_colsum for the head-blocked dq/dk/dv.  The relative-position gradient leaves the attention backward as
[(2ws-1)^2][nh] and kair_table_transpose brings it into the parameter's [nh][2ws-1][2ws-1] layout (nh = 1: the same
memory, written directly).

The input is replication-padded bottom / right to multiples of 64 (kair_usr_pad, the ResUNet replicate-pad kernel
with its zero-pad, fold and crop forms) and the output cropped; the adjoint
(zero-padded output gradient, folded input gradient) gives the input gradient.  bf16 and exact-fp32 arithmetic; no
fp32x3 form.  Eval forwards of the bf16 engine run the transformer branch of the narrow levels (C = 32 / 64) as one
launch, kair_scu_block_fwd (fused_block; measured faster at both widths, profiles/scunet_bench.txt).  Launch-only: a whole training step captures into a HIP graph (FusedTrainer).
"""
import torch
import torch.nn as nn

from .. import _hip as H
from .base import ConvEngineBase, ConvNetFunction, lease_grads
from .resunet import C8, _Conv3, _Down, _Up

WS = 8          # window side
HD = 32         # head dim = head pad
PAD = 64        # the network pads H and W to multiples of this
NTAB = (2 * WS - 1) ** 2


class _Lin:
    """A Linear (or 1x1 conv) with bias: the [N][K] forward pack, the [K][N] input-gradient pack and the bias."""

    def __init__(self, eng, mod):
        self.w, self.b = mod.weight, mod.bias
        self.N, self.K = self.w.shape[:2]
        N, K = self.N, self.K
        self.map, self.mapT = H.wmap(0, N, K), H.wmap(3, N, K)
        self.mapb = H.wmap(4, N, 0, (1, N, N), (1, 1, 1))
        self.Wp, self.Wt, self.bp = eng._e(N, K, dt=eng.tdt), eng._e(K, N, dt=eng.tdt), eng._e(N)

    def pack_jobs(self):
        w = self.w.detach()
        return [(w, self.Wp, self.map), (w, self.Wt, self.mapT), (self.b.detach(), self.bp, self.mapb)]


class _CTB:
    """One ConvTransBlock's packs."""

    def __init__(self, eng, m):
        self.C = m.conv_dim
        if m.trans_dim != m.conv_dim or self.C % HD:
            raise NotImplementedError("kair_amd SCUNet: conv_dim == trans_dim, a multiple of the head dim 32")
        t = m.trans_block
        if t.msa.head_dim != HD or t.msa.window_size != WS:
            raise NotImplementedError("kair_amd SCUNet: head_dim 32 and window_size 8")
        self.nh = self.C // HD
        self.shift = WS // 2 if t.type == "SW" else 0
        self.scale = float(t.msa.scale)
        self.c11, self.c12 = _Lin(eng, m.conv1_1), _Lin(eng, m.conv1_2)
        self.c1, self.c2 = _Conv3(eng, m.conv_block[0]), _Conv3(eng, m.conv_block[2])
        self.ln1, self.ln2 = t.ln1, t.ln2
        self.qkv, self.proj = _Lin(eng, t.msa.embedding_layer), _Lin(eng, t.msa.linear)
        self.fc1, self.fc2 = _Lin(eng, t.mlp[0]), _Lin(eng, t.mlp[2])
        self.table = t.msa.relative_position_params          # [nh][2ws-1][2ws-1]
        self.tab = eng._e(NTAB, self.nh)                      # the kernels' [(2ws-1)^2][nh]
        self.map_tab = H.wmap(3, self.nh, NTAB)

    def layers(self):
        return (self.c11, self.c12, self.c1, self.c2, self.qkv, self.proj, self.fc1, self.fc2)

    def pack_jobs(self):
        return [j for c in self.layers() for j in c.pack_jobs()] + [(self.table.detach(), self.tab, self.map_tab)]


def _blocks_of(eng, mods):
    return [_CTB(eng, m) for m in mods if not isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]


class SCUNetEngine(ConvEngineBase):
    COMPUTE_DTYPES = ("bf16", "fp32")

    # trans_dim -> whether eval forwards of the bf16 engine run the Block as one launch (kair_scu_block_fwd) by default:
    # on where it measured faster than the unfused sequence on the same tensors (profiles/scunet_bench.txt)
    FUSED_BLOCK_DEFAULT = {32: True, 64: True}

    def __init__(self, net, compute_dtype="fp32", fused_block=None):
        """fused_block: None (FUSED_BLOCK_DEFAULT), a bool for both narrow widths, or {32: bool, 64: bool}.  The one-launch
        Block keeps nothing for a backward and is bf16: training plans and the fp32 engine run the unfused sequence."""
        super().__init__(net, compute_dtype)
        if fused_block is None:
            fused_block = self.FUSED_BLOCK_DEFAULT
        if isinstance(fused_block, bool):
            fused_block = {32: fused_block, 64: fused_block}
        self.fused_block = {c: bool(fused_block.get(c, False)) and compute_dtype == "bf16" for c in (32, 64)}
        self.device = net.m_head[0].weight.device
        self.in_nc = net.m_head[0].in_channels
        if self.in_nc > C8:
            raise NotImplementedError("kair_amd SCUNet: in_nc <= 8")
        self.head = _Conv3(self, net.m_head[0], Cip=C8)
        self.tail = _Conv3(self, net.m_tail[0], Cop=C8)
        self.down_blks, self.downs = [], []
        for d in (net.m_down1, net.m_down2, net.m_down3):
            self.down_blks.append(_blocks_of(self, d))
            self.downs.append(_Down(self, d[-1]))
        self.body_blks = _blocks_of(self, net.m_body)
        self.ups, self.up_blks = [], []                 # m_up3 (-> level 2), m_up2 (-> 1), m_up1 (-> 0)
        for u in (net.m_up3, net.m_up2, net.m_up1):
            self.ups.append(_Up(self, u[0]))
            self.up_blks.append(_blocks_of(self, u))
        self.nc = [self.head.Co] + [d.Co for d in self.downs]      # level widths 2C
        stages = self.down_blks + [self.body_blks] + self.up_blks
        if any(not s for s in stages):
            raise NotImplementedError("kair_amd SCUNet: every stage needs at least one block")
        for l, blks in zip((0, 1, 2, 3, 2, 1, 0), stages):
            if any(2 * b.C != self.nc[l] for b in blks):
                raise NotImplementedError("kair_amd SCUNet: a block's width differs from its level's")

    def convs(self):
        cs = [self.head, self.tail] + self.downs + self.ups
        for blks in self.down_blks + [self.body_blks] + self.up_blks:
            cs += blks
        return cs

    def grad_segments(self):
        """Parameter groups in the order backward() completes them (each contiguous in registration order)."""
        net = self.net_ref()
        ps = lambda *ms: [p for m in ms for p in m.parameters()]   # noqa: E731
        return [ps(net.m_up1, net.m_tail), ps(net.m_up2), ps(net.m_up3), ps(net.m_body), ps(net.m_down3),
                ps(net.m_down2), ps(net.m_head, net.m_down1)]

    # ---- plan -----------------------------------------------------------------------------
    def _block_state(self, M, C, infer=False):
        """infer: without "u", the GELU' the backward reads (the fc1 epilogue then stores no pre-activation copy)."""
        e, T = self._e, self.tdt
        nWin = M // (WS * WS)
        S = {"Y": e(M, 2 * C), "h": e(M, C, dt=T), "Z": e(M, 2 * C), "ln1": e(M, C, dt=T), "m1": e(M), "r1": e(M),
                "qkv": e(3 * M * C, dt=T), "O": e(M, C, dt=T), "lse": e(nWin * (C // HD) * WS * WS), "mid": e(M, C),
                "ln2": e(M, C, dt=T), "m2": e(M), "r2": e(M), "hh": e(M, 4 * C, dt=T), "out": e(M, 2 * C)}
        if not infer:
            S["u"] = e(M, 4 * C, dt=T)
        return S

    def _stage_state(self, M, C, n, infer):
        if not infer:
            return [self._block_state(M, C) for _ in range(n)]
        a = self._block_state(M, C, True)       # nothing is kept for a backward: two states that differ in "out"
        b = dict(a, out=self._e(M, 2 * C))
        return [(a, b)[j % 2] for j in range(n)]

    def _build_plan(self, key, infer):
        B, Hh, Ww = key
        Hp, Wp = -(-Hh // PAD) * PAD, -(-Ww // PAD) * PAD
        M = [B * (Hp >> l) * (Wp >> l) for l in range(4)]
        if M[0] >= 1 << 24:
            raise NotImplementedError("kair_amd SCUNet: B*Hp*Wp must be < 2^24")
        e, T, nc = self._e, self.tdt, self.nc
        Ch = [c // 2 for c in nc]
        Mu = B * Hh * Ww
        pad = (Hp, Wp) != (Hh, Ww)
        P = {"B": B, "H": Hh, "W": Ww, "Hp": Hp, "Wp": Wp, "M": M, "pad": pad, "infer": infer}
        P["xin"] = e(M[0], C8, dt=T)
        P["xin_u"] = e(Mu, C8, dt=T) if pad else P["xin"]
        P["E"] = e(B, self.in_nc, Hh, Ww)
        P["E_p"] = e(B, self.in_nc, Hp, Wp) if pad else P["E"]
        P["X"] = [e(M[l], nc[l]) for l in range(4)]
        P["t"] = [e(M[l], nc[l]) for l in range(3)]
        P["down"] = [self._stage_state(M[l], Ch[l], len(self.down_blks[l]), infer) for l in range(3)]
        P["body"] = self._stage_state(M[3], Ch[3], len(self.body_blks), infer)
        P["up"] = [self._stage_state(M[l], Ch[l], len(self.up_blks[2 - l]), infer) for l in range(3)]
        if infer:
            return P
        P["gE"] = torch.zeros(Mu, C8, device=self.device, dtype=T)
        P["gE_p"] = e(M[0], C8, dt=T) if pad else P["gE"]
        P["gxin"] = e(M[0], C8)
        P["gxin_u"] = e(Mu, C8) if pad else P["gxin"]
        G = []
        for l in range(4):
            m, c = M[l], Ch[l]
            nWin, nh = m // (WS * WS), c // HD
            G.append({"gS": e(m, 2 * c), "gc": e(m, 2 * c), "ga": e(m, 2 * c), "gb": e(m, 2 * c), "dZ": e(m, 2 * c),
                      "gz": e(m, c, dt=T), "dU": e(m, 4 * c, dt=T), "dxn": e(m, c), "Da": e(m, c, dt=T),
                      "dO": e(m, c, dt=T), "dqkv": e(3 * m * c, dt=T), "attn_ws": e(H.window_attn_bwd_ws(nWin, nh, WS)),
                      "tabg": e(NTAB * nh), "qcs_ws": e(H.qkvblk_colsum_ws(nh))})
        P["G"] = G
        P["ln_ws"] = e(2 * 2048 * Ch[3])
        P["colsum_ws"] = e(max(H.colsum_ws(w) for c in Ch for w in (c, 2 * c, 4 * c)))
        P["loss"], P["loss_ws"] = e(1), e(1024)
        shapes = [(M[0], nc[0], 9 * C8), (M[0], C8, 9 * nc[0])]
        for l in range(4):
            m, c = M[l], Ch[l]
            shapes += [(m, 2 * c, 2 * c), (m, c, 9 * c), (m, c, 4 * c), (m, 4 * c, c), (m, c, c), (m, 3 * c, c)]
        shapes += [(M[l + 1], nc[l + 1], 4 * nc[l]) for l in range(3)]
        P["wg_ws"] = e(self.wgrad_ws_size(shapes))
        return P

    def _grid(self, P, l):
        return P["Hp"] >> l, P["Wp"] >> l

    # ---- forward --------------------------------------------------------------------------
    def _ctb_fwd(self, b, P, S, X, l, skip=None):
        """One ConvTransBlock on the level-l rows X [M, 2C] -> S["out"] (+ skip)."""
        M, C = P["M"][l], b.C
        W2, nh = 2 * C, b.nh
        Hl, Wl = self._grid(P, l)
        win = (Hl, Wl, WS, b.shift)
        nt, ep, rows = self._nt, H.epilogue, H.rows
        Y, Z = S["Y"], S["Z"]
        Yt, Zt = Y[:, C:], Z[:, C:]                   # the trans_x columns (row stride 2C)
        nt(rows(X), rows(b.c11.Wp), ep(Y, bias=b.c11.bp), M, W2, W2)
        # conv branch on the first C channels (pixel stride 2C)
        nt(H.im2col(Y, Hl, Wl, C, ld=W2), rows(b.c1.Wf), ep(S["h"], act=H.ACT_RELU), M, C, 9 * C)
        nt(H.im2col(S["h"], Hl, Wl, C), rows(b.c2.Wf), ep(Z, ldo=W2, resid=Y, ldr=W2), M, C, 9 * C)
        # transformer branch on the last C channels
        if P["infer"] and self.fused_block.get(C):   # the whole Block in one launch, Y[:, C:] -> Z[:, C:]
            H.scu_block_fwd(Yt, W2, Zt, W2, b.ln1, b.ln2, b.qkv.Wp, b.qkv.bp, b.proj.Wp, b.proj.bp, b.fc1.Wp, b.fc1.bp,
                            b.fc2.Wp, b.fc2.bp, b.tab, b.scale, P["B"], Hl, Wl, C, b.shift)
            nt(rows(Z), rows(b.c12.Wp), ep(S["out"], bias=b.c12.bp, resid=X, resid2=skip), M, W2, W2)
            return S["out"]
        H.layernorm_fwd(Yt, W2, S["ln1"], C, b.ln1.weight, b.ln1.bias, S["m1"], S["r1"], M, C, b.ln1.eps, win)
        nt(rows(S["ln1"]), rows(b.qkv.Wp), ep(S["qkv"], mode=H.OUT_QKVBLK, ldo=0, bias=b.qkv.bp, qkv=(nh, HD, WS * WS)),
           M, 3 * C, C)
        H.window_attn_fwd(S["qkv"], b.tab, S["O"], C, S["lse"], M // (WS * WS), nh, HD, b.scale, Hl, Wl, b.shift,
                          ones_col=-1, head_pad=HD, ws=WS)
        nt(rows(S["O"]), rows(b.proj.Wp), ep(S["mid"], win=win, bias=b.proj.bp, resid=Yt, ldr=W2), M, C, C)
        H.layernorm_fwd(S["mid"], C, S["ln2"], C, b.ln2.weight, b.ln2.bias, S["m2"], S["r2"], M, C, b.ln2.eps)
        nt(rows(S["ln2"]), rows(b.fc1.Wp),
           ep(S["hh"], bias=b.fc1.bp, act=H.ACT_GELU, pre=S.get("u"), pre_grad="u" in S), M, 4 * C, C)
        nt(rows(S["hh"]), rows(b.fc2.Wp), ep(Zt, ldo=W2, bias=b.fc2.bp, resid=S["mid"]), M, C, 4 * C)
        nt(rows(Z), rows(b.c12.Wp), ep(S["out"], bias=b.c12.bp, resid=X, resid2=skip), M, W2, W2)
        return S["out"]

    def _stage_fwd(self, blks, states, P, x, l, skip=None):
        cur = x
        for j, (b, S) in enumerate(zip(blks, states)):
            cur = self._ctb_fwd(b, P, S, cur, l, skip if j == len(blks) - 1 else None)
        return cur

    def forward(self, x, drop_scales=None):
        """x [B, in_nc, H, W] fp32 NCHW (any H, W).  Returns the NCHW output buffer [B, in_nc, H, W]."""
        B, C, Hh, Ww = x.shape
        if C != self.in_nc:
            raise ValueError(f"kair_amd SCUNet: {C} input channels, network has {self.in_nc}")
        if drop_scales is not None:
            raise NotImplementedError("kair_amd SCUNet: no stochastic depth")
        P = self.plan(B, Hh, Ww)
        self.pack()
        self.cur = P
        nc, M = self.nc, P["M"]
        H0, W0 = self._grid(P, 0)
        H.image_to_nhwc(x.contiguous(), P["xin_u"], C8, None, 1.0, B, C, Hh, Ww)
        if P["pad"]:
            H.usr_pad(P["xin_u"], P["xin"], H.USR_PAD_REPLICATE, C8, B, Hh, Ww, H0, W0)
        self._nt(H.im2col(P["xin"], H0, W0, C8), H.rows(self.head.Wf), H.epilogue(P["X"][0]), M[0], nc[0], 9 * C8)
        cur = P["X"][0]
        for l in range(3):
            a = self._stage_fwd(self.down_blks[l], P["down"][l], P, cur, l)
            Hn, Wn = self._grid(P, l + 1)
            self._nt(H.s2d(a, Hn, Wn, nc[l]), H.rows(self.downs[l].Wf), H.epilogue(P["X"][l + 1]), M[l + 1], nc[l + 1],
                     4 * nc[l])
            cur = P["X"][l + 1]
        s = self._stage_fwd(self.body_blks, P["body"], P, cur, 3, skip=P["X"][3])
        for u in range(3):
            l = 2 - u
            Hs, Ws = self._grid(P, l + 1)
            self._nt(H.rows(s), H.rows(self.ups[u].Wf),
                     H.epilogue(P["t"][l], mode=H.OUT_PSHUF, ldo=nc[l], ps=(2, Hs, Ws)), M[l + 1], 4 * nc[l], nc[l + 1])
            s = self._stage_fwd(self.up_blks[u], P["up"][l], P, P["t"][l], l, skip=P["X"][l])
        self._nt(H.im2col(s, H0, W0, nc[0]), H.rows(self.tail.Wf),
                 H.epilogue(P["E_p"], mode=H.OUT_NCHW, ldo=0, img=(None, 1.0, self.in_nc, H0, W0)), M[0], C8, 9 * nc[0])
        if P["pad"]:
            H.usr_pad(P["E_p"], P["E"], H.USR_CROP_NCHW, 0, B * self.in_nc, Hh, Ww, H0, W0)
        return P["E"]

    # ---- backward -------------------------------------------------------------------------
    def _bias_grad(self, P, G, M, lin, grads):
        H.colsum(G, M, lin.N, lin.mapb, grads[lin.b], P["colsum_ws"])

    def _ctb_bwd(self, b, P, S, X, G, l, grads, out, skip_g=None):
        """G = dL/d(block output) [M, 2C] fp32 -> out = dL/dX (+ skip_g)."""
        M, C = P["M"][l], b.C
        W2, nh = 2 * C, b.nh
        Hl, Wl = self._grid(P, l)
        win = (Hl, Wl, WS, b.shift)
        nWin = M // (WS * WS)
        nt, ep, rows, wg = self._nt, H.epilogue, H.rows, self._wgrad
        g = lambda p: grads[p]   # noqa: E731
        Sc = P["G"][l]
        dZ, gz, dU, dxn, Da, dO, dqkv = Sc["dZ"], Sc["gz"], Sc["dU"], Sc["dxn"], Sc["Da"], Sc["dO"], Sc["dqkv"]
        Dt, Yt = dZ[:, C:], S["Y"][:, C:]
        # out = X + conv1_2(Z)
        wg(P, rows(G), rows(S["Z"]), M, W2, W2, b.c12.map, g(b.c12.w))
        self._bias_grad(P, rows(G), M, b.c12, grads)
        nt(rows(G), rows(b.c12.Wt), ep(dZ), M, W2, W2)
        # conv branch: Z[:, :C] = conv2(relu(conv1(Y[:, :C]))) + Y[:, :C]; dL/dY[:, :C] finished in place in dZ
        nt(H.im2col(dZ, Hl, Wl, C, flip=True, ld=W2), rows(b.c2.Wd), ep(gz, gate=S["h"], gate_kind=3), M, C, 9 * C)
        wg(P, rows(dZ, ld=W2), H.im2col(S["h"], Hl, Wl, C), M, C, 9 * C, b.c2.map, g(b.c2.w))
        wg(P, rows(gz), H.im2col(S["Y"], Hl, Wl, C, ld=W2), M, C, 9 * C, b.c1.map, g(b.c1.w))
        nt(H.im2col(gz, Hl, Wl, C, flip=True), rows(b.c1.Wd), ep(dZ, ldo=W2, resid=dZ, ldr=W2), M, C, 9 * C)
        # MLP: Z[:, C:] = mid + fc2(gelu(fc1(LN2(mid)))); Dt becomes dL/dmid
        wg(P, rows(Dt, ld=W2), rows(S["hh"]), M, C, 4 * C, b.fc2.map, g(b.fc2.w))
        self._bias_grad(P, rows(Dt, ld=W2), M, b.fc2, grads)
        nt(rows(Dt, ld=W2), rows(b.fc2.Wt), ep(dU, gate=S["u"], gate_kind=4), M, 4 * C, C)
        wg(P, rows(dU), rows(S["ln2"]), M, 4 * C, C, b.fc1.map, g(b.fc1.w))
        self._bias_grad(P, rows(dU), M, b.fc1, grads)
        nt(rows(dU), rows(b.fc1.Wt), ep(dxn), M, C, 4 * C)
        H.layernorm_bwd(S["mid"], C, dxn, C, b.ln2.weight, S["m2"], S["r2"], Dt, W2, True, g(b.ln2.weight), g(b.ln2.bias),
                        False, P["ln_ws"], M, C, copy=H.copy_desc(Da, win=win))
        # attention: mid = Y[:, C:] + linear(attn(LN1(Y[:, C:]))); Da = dL/dmid in window order
        wg(P, rows(Da), rows(S["O"]), M, C, C, b.proj.map, g(b.proj.w))
        self._bias_grad(P, rows(Da), M, b.proj, grads)
        nt(rows(Da), rows(b.proj.Wt), ep(dO), M, C, C)
        tabg = g(b.table) if nh == 1 else Sc["tabg"]     # one head: [225][1] is the parameter's layout
        H.window_attn_bwd(S["qkv"], S["O"], C, dO, C, b.tab, S["lse"], dqkv, tabg, False, Sc["attn_ws"], nWin, nh, HD,
                          b.scale, Hl, Wl, b.shift, head_pad=HD, win_ws=WS)
        if nh > 1:
            H.table_transpose(tabg, g(b.table), NTAB, nh)
        A = lambda: H.qkvblk(dqkv, nh, hdp=HD, ws=WS)   # noqa: E731
        wg(P, A(), rows(S["ln1"]), M, 3 * C, C, b.qkv.map, g(b.qkv.w))
        H.qkvblk_colsum(dqkv, nWin, nh, HD, Sc["qcs_ws"], g(b.qkv.b))
        nt(A(), rows(b.qkv.Wt), ep(dxn), M, C, 3 * C)
        H.layernorm_bwd(Yt, W2, dxn, C, b.ln1.weight, S["m1"], S["r1"], Dt, W2, True, g(b.ln1.weight), g(b.ln1.bias),
                        False, P["ln_ws"], M, C, win)
        # Y = conv1_1(X); dL/dX = G + dL/dY W11 (+ the U-Net skip gradient)
        wg(P, rows(dZ), rows(X), M, W2, W2, b.c11.map, g(b.c11.w))
        self._bias_grad(P, rows(dZ), M, b.c11, grads)
        nt(rows(dZ), rows(b.c11.Wt), ep(out, resid=G, resid2=skip_g), M, W2, W2)
        return out

    def _stage_bwd(self, blks, states, P, x_in, gr, l, grads, skip_g=None):
        Sc = P["G"][l]
        cur = gr
        for j in range(len(blks) - 1, -1, -1):
            X = states[j - 1]["out"] if j > 0 else x_in
            out = Sc["ga"] if cur is not Sc["ga"] else Sc["gb"]
            cur = self._ctb_bwd(blks[j], P, states[j], X, cur, l, grads, out, skip_g if j == 0 else None)
        return cur

    def backward_from_loss(self, H_img, grads, loss_weight=1.0, charb_eps=None, loss_type=None):
        P = self.cur
        self.pixel_loss(P, P["E"], H_img, P["gE"], C8, loss_weight, self.in_nc, P["H"], P["W"], charb_eps=charb_eps,
                        loss_type=loss_type)
        self.backward(grads, P, need_input_grad=False)
        return P["loss"]

    def backward_from_grad(self, gE, grads, need_input_grad=False):
        """gE: dL/dE [B, in_nc, H, W].  Returns dL/dx [B, in_nc, H, W] (a new tensor) when need_input_grad."""
        P = self.cur
        B, Hh, Ww = P["B"], P["H"], P["W"]
        H.image_to_nhwc(gE.contiguous(), P["gE"], C8, None, 1.0, B, self.in_nc, Hh, Ww)
        self.backward(grads, P, need_input_grad)
        if not need_input_grad:
            return None
        return P["gxin_u"].view(B, Hh, Ww, C8)[..., :self.in_nc].permute(0, 3, 1, 2).contiguous()

    def backward(self, grads, P, need_input_grad=False):
        if P["infer"]:
            raise RuntimeError("kair_amd SCUNet: backward through an inference plan")
        nc, M, Gs = self.nc, P["M"], P["G"]
        B, Hh, Ww = P["B"], P["H"], P["W"]
        H0, W0 = self._grid(P, 0)
        gE = P["gE"]
        if P["pad"]:   # adjoint of the crop: the output gradient on the padded grid, zeros outside
            H.usr_pad(gE, P["gE_p"], H.USR_PAD_ZERO, C8, B, Hh, Ww, H0, W0)
            gE = P["gE_p"]
        self._nt(H.im2col(gE, H0, W0, C8, flip=True), H.rows(self.tail.Wd), H.epilogue(Gs[0]["gS"]), M[0], nc[0], 9 * C8)
        s1 = P["up"][0][-1]["out"]
        self._wgrad(P, H.rows(gE), H.im2col(s1, H0, W0, nc[0]), M[0], C8, 9 * nc[0], self.tail.map, grads[self.tail.w])
        gr = Gs[0]["gS"]
        for u in (2, 1, 0):                        # m_up1, m_up2, m_up3
            l = 2 - u
            gt = self._stage_bwd(self.up_blks[u], P["up"][l], P, P["t"][l], gr, l, grads)
            up = self.ups[u]
            Hs, Ws = self._grid(P, l + 1)
            s_next = P["body"][-1]["out"] if l == 2 else P["up"][l + 1][-1]["out"]
            self._nt(H.s2d(gt, Hs, Ws, nc[l]), H.rows(up.Wd), H.epilogue(Gs[l + 1]["gS"]), M[l + 1], nc[l + 1], 4 * nc[l])
            self._wgrad(P, H.rows(s_next), H.s2d(gt, Hs, Ws, nc[l]), M[l + 1], nc[l + 1], 4 * nc[l], up.map, grads[up.w],
                        act_rows=True)
            gr = Gs[l + 1]["gS"]
            self._segment_done()
        gx = self._stage_bwd(self.body_blks, P["body"], P, P["X"][3], Gs[3]["gS"], 3, grads, skip_g=Gs[3]["gS"])
        self._segment_done()
        for l in (2, 1, 0):
            d = self.downs[l]
            Hn, Wn = self._grid(P, l + 1)
            a = P["down"][l][-1]["out"]
            self._nt(H.rows(gx), H.rows(d.Wd), H.epilogue(Gs[l]["gc"], mode=H.OUT_PSHUF, ldo=nc[l], ps=(2, Hn, Wn)),
                     M[l + 1], 4 * nc[l], nc[l + 1])
            self._wgrad(P, H.rows(gx), H.s2d(a, Hn, Wn, nc[l]), M[l + 1], nc[l + 1], 4 * nc[l], d.map, grads[d.w])
            gx = self._stage_bwd(self.down_blks[l], P["down"][l], P, P["X"][l], Gs[l]["gc"], l, grads, skip_g=Gs[l]["gS"])
            if l > 0:
                self._segment_done()
        if need_input_grad:
            self._nt(H.im2col(gx, H0, W0, nc[0], flip=True), H.rows(self.head.Wd), H.epilogue(P["gxin"]), M[0], C8,
                     9 * nc[0])
            if P["pad"]:   # adjoint of the replicate pad: pad pixels' gradients onto the edge they copied
                H.usr_pad(P["gxin"], P["gxin_u"], H.USR_PAD_FOLD, C8, B, Hh, Ww, H0, W0)
        self._wgrad(P, H.rows(gx), H.im2col(P["xin"], H0, W0, C8), M[0], nc[0], 9 * C8, self.head.map, grads[self.head.w])


class SCUNetFunction(ConvNetFunction):
    """ConvNetFunction with the input gradient (the head conv's dgrad, folded back over the replicate pad)."""

    @staticmethod
    def forward(ctx, engine, mode, n_cond, x, *rest):
        return ConvNetFunction.forward(ctx, engine, mode, n_cond, x, *rest)

    @staticmethod
    def backward(ctx, gE):
        _, grads = lease_grads(ctx, gE)
        gx = ctx.engine.backward_from_grad(gE.float(), grads, need_input_grad=ctx.needs_input_grad[3])
        ctx.lease.release()
        return (None, None, None, gx) + tuple(None for _ in range(ctx.n_cond)) + tuple(grads[p] for p in ctx.params)
