"""Plain float64 statements of the kair_gemm_nt / kair_gemm_tn forms that only the conv networks use, written from
include/kair_hip.h (kair_operand, kair_out_mode, kair_epilogue, kair_wmap) and pinned to torch's float64 functional
ops by tests/test_convnet_forms_cpu.py; tests/test_convnet_forms_gpu.py compares the kernels with them.

Operands    im2col3 (KAIR_LD_IM2COL3, with im_flip and the nearest x2 source of im_up = 2), s2d (KAIR_LD_S2D)
Packs       pack / unpack of kair_wmap kinds 1, 2, 7 and 8 as index formulas (one group per dimension, padded)
Stores      flat output offsets of the ROWS, PSHUF, PUNSHUF, NCHW and PSHUF_NCHW store modes
Epilogue    act (GELU, LeakyReLU, ReLU), gate_factor (kinds 1..4), nt_ref / img_tail / tn_ref
Bound       bound(), ratio(): the elementwise error bound every comparison uses

The bound.  With fp32 accumulation of K products of operands whose products are exact in fp32 (every test input is
bf16-exact: 8 + 8 significand bits), an output element obeys

    |got - ref| <= 2 (K + 4) 2^-24 S + r_out

S = (|A| |B|^T)[m, n] + |bias| + |resid| + |resid2| (the gate and the 1 / img_range factor applied to S as to the
value; + |mean| for the image stores), r_out = 2^-24 |ref| for an fp32 output, 2^-8 |ref| for a bf16 one.  (K + 4)
2^-24 S is the textbook gamma_K of a K-term sum plus the epilogue's additions and its division; the factor 2 covers
the matrix cores' undocumented summation order and internal rounding.  For the weight gradients K is the row count
M plus the number of splits.  ReLU and LeakyReLU are 1-Lipschitz, so S passes through them unchanged; GELU's
derivative reaches 1.13, and S takes that factor.
"""
import math

import torch

U24, U8 = 2.0 ** -24, 2.0 ** -8
ACT_NONE, ACT_GELU, ACT_LEAKY, ACT_RELU = 0, 1, 2, 3


def bf16_exact(t):
    return t.bfloat16().float()


# ---- operands ------------------------------------------------------------------------------------------------------
def im2col3(rows, B, H, W, C, flip=False, up=1):
    """rows: NHWC pixel rows [B * (H / up) * (W / up), ld >= C] of the SOURCE image; H x W is the conv grid.
    -> float64 [B H W, 9 C]: row m = (b, y, x), column k = tap C + c with tap = (dy + 1) 3 + (dx + 1) reads conv-grid
    pixel (y + dy, x + dx) -- (y - dy, x - dx) with flip -- or 0 outside the grid (pad 1); with up = 2 that pixel is
    source pixel ((y + dy) // 2, (x + dx) // 2) of the H/2 x W/2 image (nearest x2)."""
    src = rows.double().reshape(B, H // up, W // up, -1)[..., :C]
    out = torch.zeros(B, H, W, 9, C, dtype=torch.float64)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if flip:
            dy, dx = -dy, -dx
        for y in range(H):
            for x in range(W):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    out[:, y, x, tap] = src[:, yy // up, xx // up]
    return out.reshape(B * H * W, 9 * C)


def s2d(rows, B, Hn, Wn, C):
    """rows: NHWC pixel rows [B * 2 Hn * 2 Wn, ld >= C].  -> float64 [B Hn Wn, 4 C]: row m = (b, y, x) of the
    Hn x Wn OUTPUT grid, column k = (i 2 + j) C + c reads pixel (2 y + i, 2 x + j), channel c."""
    src = rows.double().reshape(B, 2 * Hn, 2 * Wn, -1)[..., :C]
    out = torch.zeros(B, Hn, Wn, 4, C, dtype=torch.float64)
    for y in range(Hn):
        for x in range(Wn):
            for i in range(2):
                for j in range(2):
                    out[:, y, x, i * 2 + j] = src[:, 2 * y + i, 2 * x + j]
    return out.reshape(B * Hn * Wn, 4 * C)


# ---- packed weight layouts -------------------------------------------------------------------------------------------
def pack_index(kind, N, K, Np=None, Kp=None):
    """(shape, src): the packed layout's shape and, per packed element, the flat index into the reference weight
    [N][K][taps] (taps 9: kinds 1 / 2, taps 4: kinds 7 / 8), -1 at pad entries.  N x K real, Np x Kp padded.
      1  [Np][9 Kp]   column tap Kp + kp                 <- w[np][kp][tap]
      2  [Kp][9 Np]   row kp, column tap Np + np         <- w[np][kp][tap]   (the taps' negation is the operand's im_flip)
      7  [Np][4 Kp]   column tap Kp + kp                 <- w[np][kp][tap]
      8  [4 Kp][Np]   row kp 4 + tap, column np          <- w[np][kp][tap]"""
    Np, Kp = Np or N, Kp or K
    taps = 9 if kind in (1, 2) else 4
    t = torch.arange(Np * Kp * taps)
    if kind in (1, 7):
        shape = (Np, taps * Kp)
        n, kk = t // (taps * Kp), t % (taps * Kp)
        tap, k = kk // Kp, kk % Kp
    elif kind == 2:
        shape = (Kp, 9 * Np)
        k, kk = t // (9 * Np), t % (9 * Np)
        tap, n = kk // Np, kk % Np
    elif kind == 8:
        shape = (4 * Kp, Np)
        row, n = t // Np, t % Np
        k, tap = row // 4, row % 4
    else:
        raise ValueError(kind)
    src = torch.where((n < N) & (k < K), (n * K + k) * taps + tap, torch.full_like(t, -1))
    return shape, src


def pack(w, kind, Np=None, Kp=None, dtype=torch.float64):
    """The packed form of the reference weight w [N][K][kh][kw]: a permutation, zero pads, one cast."""
    N, K = w.shape[:2]
    shape, src = pack_index(kind, N, K, Np, Kp)
    flat = w.reshape(-1)
    out = torch.zeros(src.numel(), dtype=w.dtype)
    ok = src >= 0
    out[ok] = flat[src[ok]]
    return out.reshape(shape).to(dtype)


def unpack(G, kind, N, K, Np=None, Kp=None):
    """The reference-layout gradient [N][K][kh][kw] of a packed-layout sum G (kair_wgrad_finalize, kinds 1 and 7)."""
    shape, src = pack_index(kind, N, K, Np, Kp)
    assert tuple(G.shape) == shape, (G.shape, shape)
    taps = 9 if kind in (1, 2) else 4
    out = torch.zeros(N * K * taps, dtype=G.dtype)
    ok = src >= 0
    out[src[ok]] = G.reshape(-1)[ok]
    s = 3 if taps == 9 else 2
    return out.reshape(N, K, s, s)


# ---- store maps: flat element offsets into `out` of GEMM element (m, n); valid = stored at all ------------------------
def _mn(M, N):
    return torch.arange(M).view(M, 1), torch.arange(N).view(1, N)


def rows_offsets(M, N, ldo):
    m, n = _mn(M, N)
    return m * ldo + n, torch.ones(M, N, dtype=torch.bool)


def pshuf_offsets(M, N, H, W, r, ldo):
    """KAIR_OUT_PSHUF: m = (b, y, x) of [H, W], n = c r^2 + i r + j -> NHWC [b, y r + i, x r + j, c], channel stride ldo."""
    m, n = _mn(M, N)
    b, p = m // (H * W), m % (H * W)
    y, x = p // W, p % W
    c, ij = n // (r * r), n % (r * r)
    i, j = ij // r, ij % r
    row = (b * H * r + y * r + i) * (W * r) + x * r + j
    return row * ldo + c, torch.ones(M, N, dtype=torch.bool)


def punshuf_offsets(M, N, H, W, r, ldo):
    """KAIR_OUT_PUNSHUF: m = pixel (b, Y, X) of the [H r, W r] image, n = c -> out[(b, Y // r, X // r) of H x W]
    [c r^2 + (Y % r) r + X % r], row stride ldo."""
    m, n = _mn(M, N)
    HW = H * r * W * r
    b, p = m // HW, m % HW
    Y, X = p // (W * r), p % (W * r)
    row = (b * H + Y // r) * W + X // r
    return row * ldo + n * r * r + (Y % r) * r + X % r, torch.ones(M, N, dtype=torch.bool)


def nchw_offsets(M, N, H, W, img_C):
    """KAIR_OUT_NCHW: image out[b][n][y][x] of [H, W] for n < img_C; the other columns are not stored."""
    m, n = _mn(M, N)
    b, p = m // (H * W), m % (H * W)
    return (b * img_C + n) * (H * W) + p, (n < img_C).expand(M, N)


def pshuf_nchw_offsets(M, N, H, W, r, img_C):
    """KAIR_OUT_PSHUF_NCHW: PixelShuffle(r) into the NCHW image [b][c][y r + i][x r + j] for c < img_C."""
    m, n = _mn(M, N)
    b, p = m // (H * W), m % (H * W)
    y, x = p // W, p % W
    c, ij = n // (r * r), n % (r * r)
    i, j = ij // r, ij % r
    off = ((b * img_C + c) * (H * r) + y * r + i) * (W * r) + x * r + j
    return off, (c < img_C).expand(M, N)


def scatter(V, off, valid, size):
    """A float64 buffer of `size` elements holding V at its offsets and NaN where nothing is stored."""
    out = torch.full((size,), float("nan"), dtype=torch.float64)
    out[off[valid]] = V.double()[valid]
    return out


# ---- epilogue -------------------------------------------------------------------------------------------------------
def act(v, kind, slope=0.0):
    """kair_act: 1 GELU (erf form), 2 LeakyReLU(slope), 3 ReLU."""
    if kind == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if kind == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    if kind == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def gate_factor(g, kind, slope=0.0):
    """kair_epilogue.gate_kind: 1 gelu'(gate), 2 leaky'(sign of gate), 3 relu', 4 the gate itself.  The derivative at a
    gate of 0 (either sign) is the negative side's: slope, or 0."""
    g = g.double()
    if kind == 1:
        return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    if kind == 2:
        return torch.where(g > 0, torch.ones_like(g), torch.full_like(g, slope))
    if kind == 3:
        return torch.where(g > 0, torch.ones_like(g), torch.zeros_like(g))
    if kind == 4:
        return g
    raise ValueError(kind)


def nt_ref(A, Bw, bias=None, act_kind=ACT_NONE, slope=0.0, gate=None, gate_kind=0, resid=None, resid2=None):
    """(value, S) [M, N] of kair_gemm_nt's ROWS epilogue over float64 operands A [M, K], Bw [N, K]:
    act(A Bw^T + bias) * gate' + resid + resid2, and the bound's magnitude sum S (module docstring)."""
    A, Bw = A.double(), Bw.double()
    v, S = A @ Bw.T, A.abs() @ Bw.abs().T
    if bias is not None:
        v, S = v + bias.double(), S + bias.double().abs()
    v = act(v, act_kind, slope)
    if act_kind == ACT_GELU:
        S = S * 1.13
    if gate is not None:
        f = gate_factor(gate, gate_kind, slope)
        v, S = v * f, S * f.abs()
    for r in (resid, resid2):
        if r is not None:
            v, S = v + r.double(), S + r.double().abs()
    return v, S


def img_tail(v, S, img_range=1.0, mean=None, resid=None):
    """The image stores' value v / img_range + mean[column] (+ resid, given per GEMM element) and its S."""
    v, S = v / img_range, S / img_range
    if mean is not None:
        v, S = v + mean.double(), S + mean.double().abs()
    if resid is not None:
        v, S = v + resid.double(), S + resid.double().abs()
    return v, S


def tn_ref(A, Bm, grad0=None):
    """(value, S) [N, K] of kair_gemm_tn + kair_wgrad_finalize in the packed layout: A^T Bm over the M rows
    (+ grad0, the gradient accumulated onto)."""
    A, Bm = A.double(), Bm.double()
    v, S = A.T @ Bm, A.abs().T @ Bm.abs()
    if grad0 is not None:
        v, S = v + grad0.double(), S + grad0.double().abs()
    return v, S


# ---- the bound ------------------------------------------------------------------------------------------------------
def bound(S, ref, K, out_bf16=False):
    return 2.0 * (K + 4) * U24 * S + (U8 if out_bf16 else U24) * ref.abs()


def ratio(got, ref, bnd):
    """(max |got - ref| / bound, flat argmax).  A zero bound admits only got == ref (else inf); a NaN in got is NaN."""
    d = (got.double() - ref).abs().reshape(-1)
    r = torch.where(d == 0, torch.zeros_like(d), d / bnd.reshape(-1))
    i = int(torch.argmax(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)))
    return r[i].item(), i


# ---- the shapes both test files use ------------------------------------------------------------------------------------
# two images, a non-square grid, an M that is no multiple of a tile and a pixel stride above im_C each occur at least once
UP2_CASES = [(2, 3, 5, 16, 24, 16), (1, 4, 4, 64, 64, 64), (2, 2, 6, 64, 32, 72)]     # (B, h, w, C, N, pixel stride)
S2D_CASES = [(2, 3, 5, 16, 32, 16), (1, 4, 4, 64, 128, 64), (2, 2, 3, 8, 24, 16)]     # (B, Hn, Wn, C, N, pixel stride)
RB_CASES = [(2, 5, 7, 16, 16), (1, 6, 6, 64, 64), (1, 4, 9, 24, 20)]                  # (B, H, W, Cin, N)
TAIL_GRID = (2, 3, 5)                                                                 # (B, H, W) of the image tails
TAIL_C = 16                                                                           # their input channels


def randn(g, *shape, scale=1.0):
    """bf16-exact normal data from generator g."""
    return bf16_exact(torch.randn(*shape, generator=g) * scale)


def relu_gate(g, M, ld):
    """A stored post-ReLU activation [M, ld], bf16-exact: about half exact zeros, every seventh zero negative."""
    t = torch.relu(randn(g, M, ld)).reshape(-1)
    z = (t == 0).nonzero().reshape(-1)
    t[z[::7]] = -0.0
    return t.reshape(M, ld)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def to_nchw(rows, B, H, W, C=None):
    """NHWC pixel rows [B H W, ld] -> NCHW float64 [B, C, H, W] (channels [0, C))."""
    t = rows.double().reshape(B, H, W, -1)
    return t[..., :C].permute(0, 3, 1, 2).contiguous()


def to_rows(img):
    B, C, H, W = img.shape
    return img.permute(0, 2, 3, 1).reshape(B * H * W, C)


# ---- the forms: inputs (seeded, bf16-exact) and their float64 (value, S) references ----------------------------------
# test_convnet_forms_cpu.py pins every entry to torch's functional ops; test_convnet_forms_gpu.py runs the kernels on
# the same inputs.  Each is computed once per case (cached) and never modified.
_CACHE = {}


def _cached(fn):
    def wrapped(case):
        key = (fn.__name__, case)
        if key not in _CACHE:
            _CACHE[key] = fn(case)
        return _CACHE[key]
    return wrapped


@_cached
def form_up2(case):
    """a / b: conv3x3(nearest x2 (src)) + bias, LeakyReLU 0.2; its weight gradient (also accumulated onto grad0) and
    bias gradient for an output gradient dy."""
    B, h, w, C, N, ld = case
    g = gen(1000 + N + ld)
    M, K = B * 4 * h * w, 9 * C
    d = dict(src=randn(g, B * h * w, ld), wt=randn(g, N, C, 3, 3, scale=0.1), bias=randn(g, N, scale=0.1),
             dy=randn(g, M, N), grad0=randn(g, N, C, 3, 3), M=M, K=K)
    d["A"] = im2col3(d["src"], B, 2 * h, 2 * w, C, up=2)
    d["fwd"] = nt_ref(d["A"], pack(d["wt"], 1), d["bias"], ACT_LEAKY, 0.2)
    Gp, Sp = tn_ref(d["dy"], d["A"])
    d["wgrad"] = unpack(Gp, 1, N, C), unpack(Sp, 1, N, C)
    d["wgrad_acc"] = d["wgrad"][0] + d["grad0"].double(), d["wgrad"][1] + d["grad0"].double().abs()
    d["bgrad"] = d["dy"].double().sum(0), d["dy"].double().abs().sum(0)
    return d


@_cached
def form_s2d(case):
    """c: the 2x2 / stride-2 forms over an image x of C channels on the 2 Hn x 2 Wn grid and rows t of N channels on
    the Hn x Wn grid, with one weight w [N][C][2][2] read as Conv2d(C, N, 2, 2)'s or as ConvTranspose2d(N, C, 2, 2)'s:
    fwd    s2d(x) pack7(w)^T                 = conv2d(x, w, stride 2)        = convT's input gradient of x
    wgrad  t^T s2d(x) unpacked (kind 7)      = both layers' weight gradient (conv: t = dL/dout; convT: t = its input)
    pshuf  t pack8(w)^T through OUT_PSHUF(2) = conv_transpose2d(t, w, stride 2) = the conv's input gradient of t"""
    B, Hn, Wn, C, N, ld = case
    g = gen(2000 + N + ld)
    M = B * Hn * Wn
    d = dict(x=randn(g, 4 * M, ld), t=randn(g, M, N), wt=randn(g, N, C, 2, 2, scale=0.2), M=M)
    d["A"] = s2d(d["x"], B, Hn, Wn, C)
    d["fwd"] = nt_ref(d["A"], pack(d["wt"], 7))
    Gp, Sp = tn_ref(d["t"], d["A"])
    d["wgrad"] = unpack(Gp, 7, N, C), unpack(Sp, 7, N, C)
    d["pshuf"] = nt_ref(d["t"], pack(d["wt"], 8))          # [M, 4 C] GEMM elements, stored through pshuf_offsets
    return d


@_cached
def form_rb(case):
    """d: the residual-block forms on a B x H x W grid: relu = ReLU(conv3x3(x, w) + bias) (Cin -> N); res = conv3x3(x,
    w) + resid + resid2; dgrad = (the input gradient of conv3x3(., wd) (N -> Cin) for the output gradient gy of Cin
    channels) * ReLU'(gate), gate a stored post-ReLU activation."""
    B, H, W, Cin, N = case
    g = gen(3000 + N + H)
    M = B * H * W
    d = dict(x=randn(g, M, Cin), wt=randn(g, N, Cin, 3, 3, scale=0.1), bias=randn(g, N, scale=0.1),
             resid=randn(g, M, N + 4), resid2=randn(g, M, N + 12), gy=randn(g, M, Cin),
             wd=randn(g, Cin, N, 3, 3, scale=0.1), gate=relu_gate(g, M, N + 8), M=M)
    A = im2col3(d["x"], B, H, W, Cin)
    d["relu"] = nt_ref(A, pack(d["wt"], 1), d["bias"], ACT_RELU)
    d["res"] = nt_ref(A, pack(d["wt"], 1), resid=d["resid"][:, :N], resid2=d["resid2"][:, :N])
    d["dgrad"] = nt_ref(im2col3(d["gy"], B, H, W, Cin, flip=True), pack(d["wd"], 2), gate=d["gate"][:, :N], gate_kind=3)
    return d


@_cached
def form_tail(case):
    """e: the image tails on TAIL_GRID over TAIL_C input channels.  case = (store, img_C, r, Np, with_mean, img_range,
    with_resid): conv3x3 to Np packed columns (every one non-zero, so a column the store must drop carries a value),
    + bias, then the NCHW store (r = 1) or PixelShuffle(r) into the NCHW image of img_C channels."""
    store, img_C, r, Np, with_mean, rng, with_resid = case
    B, H, W = TAIL_GRID
    g = gen(4000 + 10 * img_C + r + Np)
    M = B * H * W
    d = dict(x=randn(g, M, TAIL_C), wt=randn(g, Np, TAIL_C, 3, 3, scale=0.1), bias=randn(g, Np, scale=0.1),
             mean=randn(g, img_C) if with_mean else None, resid=randn(g, B, img_C, H, W) if with_resid else None, M=M)
    v, S = nt_ref(im2col3(d["x"], B, H, W, TAIL_C), pack(d["wt"], 1), d["bias"])
    if store == "nchw":
        off, ok = nchw_offsets(M, Np, H, W, img_C)
        col_c = torch.arange(Np).view(1, Np).expand(M, Np)
    else:
        off, ok = pshuf_nchw_offsets(M, Np, H, W, r, img_C)
        col_c = (torch.arange(Np) // (r * r)).view(1, Np).expand(M, Np)
    mean_mn = d["mean"][col_c.clamp(max=img_C - 1)] if with_mean else None
    resid_mn = d["resid"].reshape(-1)[off.clamp(max=d["resid"].numel() - 1)] if with_resid else None
    v, S = img_tail(v, S, rng, mean_mn, resid_mn)
    size = B * img_C * H * r * W * r
    d["img"] = scatter(v, off, ok, size), scatter(S, off, ok, size)
    return d


@_cached
def form_punshuf(case):
    """e: conv3x3 (TAIL_C -> N) over the [2 H, 2 W] image of TAIL_GRID's B, stored through OUT_PUNSHUF(2) into rows of
    stride ldo, optionally times LeakyReLU'(gate) (kind 2, slope 0.2), the gate [B H W, ldg] in the OUTPUT's layout."""
    N, ldo, ldg, gated = case
    B, H, W = TAIL_GRID
    g = gen(5000 + N + gated)
    M = B * 4 * H * W
    d = dict(x=randn(g, M, TAIL_C), wt=randn(g, N, TAIL_C, 3, 3, scale=0.1), gate=randn(g, B * H * W, ldg), M=M)
    d["gate"][::3, ::5] = 0.0
    off, ok = punshuf_offsets(M, N, H, W, 2, ldo)
    gate_mn = None
    if gated:
        goff, _ = punshuf_offsets(M, N, H, W, 2, ldg)
        gate_mn = d["gate"].reshape(-1)[goff]
    v, S = nt_ref(im2col3(d["x"], B, 2 * H, 2 * W, TAIL_C), pack(d["wt"], 1), slope=0.2, gate=gate_mn, gate_kind=2)
    d["v_mn"] = v
    d["out"] = scatter(v, off, ok, B * H * W * ldo), scatter(S, off, ok, B * H * W * ldo)
    return d


TAIL_CASES = [("nchw", 1, 1, 16, False, 255.0, False), ("nchw", 3, 1, 16, True, 255.0, True),
              ("nchw", 3, 1, 16, False, 255.0, True), ("pshuf_nchw", 3, 2, 16, False, 1.0, False),
              ("pshuf_nchw", 3, 3, 32, True, 255.0, False)]
PUNSHUF_CASES = [(12, 56, 64, False), (12, 56, 64, True)]     # (N, ldo, ldg, gated)
