"""PixelShuffle(3): the 576-column, 9-sub-pixel forms of SwinIR classical SR x3 (network_swinir.py:584 Upsample with
scale 3: one conv 64 -> 9 * 64, then PixelShuffle(3)), each against a float64 reference.

The bias gradient's column sum (kair_colsum) to its workspace contract kair_colsum_ws(Np) -- the workspace is the
middle third of a buffer whose outer thirds must come back bit-identical, so a kernel that wrote past it fails an
assertion -- the weight packs and the weight-gradient finalize at kair_wmap.n_perm = 9, the forward conv's three-tile
PSHUF_SPM store, the input gradient's PUNSHUF_SPM store into 576-wide rows, and the x3 engine in its three
arithmetics against the CPU oracle at the small-network bars of test_swinir_gpu.py / test_x3_gpu.py.  (The narrow
conv_last kernels at ps_r = 3: tests/test_tail_gpu.py; the plain column-sum shapes: tests/test_kernels_gpu.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.swinir_engine import _Resi3  # noqa: E402
from kair_amd.models.network_swinir import SwinIR  # noqa: E402
from oracle import swinir as osw  # noqa: E402

dev = torch.device("cuda")
F = torch.nn.functional
R, NF, CO = 3, 64, 576
PAT = 0x5A5AA5A5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def spm_index(N=CO, r2=R * R):
    """packed (sub-pixel-major) row p = s * (N / r2) + c  ->  reference row c * r2 + s"""
    p = torch.arange(N)
    nf = N // r2
    return (p % nf) * r2 + p // nf


# ---- a. kair_colsum to its workspace contract ------------------------------------------------------------------
def guarded_ws(Np):
    n = H.colsum_ws(Np)
    buf = torch.full((3 * n,), PAT, dtype=torch.int32, device=dev)
    return buf, buf[n:2 * n].view(torch.float32)


def guards_intact(buf):
    n = buf.numel() // 3
    return bool((buf[:n] == PAT).all()) and bool((buf[2 * n:] == PAT).all())


def colsum_timed(*args, **kw):
    """H.colsum inside a kernel timing window: the symbols of the kernels it launched."""
    torch.cuda.synchronize()
    H.ktime_begin(8)
    try:
        H.colsum(*args, **kw)
    finally:
        nk = H.ktime_end()
    torch.cuda.synchronize()
    return [H.ktime_read(i)[1] for i in range(nk)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_colsum_unaligned_rows_take_scalar_kernel(dt):
    """Np = 64, ld = 64 would take the vector kernel, but the rows start 4 bytes past a 16-byte boundary."""
    M, Np = 1000, 64
    g = torch.Generator().manual_seed(64)
    off = 4 // torch.empty(0, dtype=dt).element_size()
    flat = torch.randn(M * Np + 8, generator=g).to(dt).to(dev)
    assert flat.data_ptr() % 16 == 0
    x = flat[off:off + M * Np].view(M, Np)
    assert x.data_ptr() % 16 == 4
    ref = x.double().cpu().sum(0)
    buf, ws = guarded_ws(Np)
    out = torch.full((Np,), float("nan"), device=dev)
    names = colsum_timed(H.rows(x), M, Np, H.wmap(0, Np, 0), out, ws)
    assert len(names) == 2 and "colsum_partial" in names[0] and "colsum_partial_v" not in names[0], names
    assert guards_intact(buf)
    assert (out.double().cpu() - ref).abs().max().item() < 1e-3 * (1 + ref.abs().max().item())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["nperm9", "nperm9_acc", "pad", "pad_groups"])
def test_colsum_maps(dt, case):
    """Bias maps (kind 4): the sub-pixel-major permutation of the x3 upsampling conv (output n receives packed
    column (n % 9) * 64 + n / 9), also accumulated onto a non-zero bias gradient; padded output channels."""
    g = torch.Generator().manual_seed(len(case))
    if case.startswith("nperm9"):
        M, N, Np = 1500, CO, CO
        m = H.wmap(4, N, 0, (1, N, Np), (1, 1, 1), n_perm=R * R)
        n = torch.arange(N)
        col = (n % 9) * 64 + n // 9
    elif case == "pad":
        M, N, Np = 1500, 180, 192
        m = H.wmap(4, N, 0, (1, N, Np), (1, 1, 1))
        col = torch.arange(N)
    else:
        M, N, Np = 1500, 180, 192
        m = H.wmap(4, N, 0, (3, 60, 64), (1, 1, 1))
        n = torch.arange(N)
        col = (n // 60) * 64 + n % 60
    x = torch.randn(M, Np, generator=g).to(dt)   # (pad columns hold data too: they must not be read)
    ref = x.double().sum(0)[col]
    acc = case.endswith("_acc")
    out0 = torch.randn(N, generator=g) * 10 if acc else torch.full((N,), float("nan"))
    if acc:
        ref = ref + out0.double()
    outs = []
    buf, ws = guarded_ws(Np)
    for _ in range(2):
        out = out0.clone().to(dev)
        H.colsum(H.rows(x.to(dev)), M, Np, m, out, ws, accumulate=acc)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert guards_intact(buf)
    assert torch.equal(outs[0], outs[1])
    assert (outs[0].double() - ref).abs().max().item() < 1e-3 * (1 + ref.abs().max().item())


def test_colsum_undersized_ws_raises():
    """One float short of kair_colsum_ws(576): ValueError, and nothing is launched."""
    M, Np = 64, CO
    x = torch.ones(M, Np, device=dev)
    out = torch.full((Np,), -7.0, device=dev)
    ws = torch.empty(H.colsum_ws(Np) - 1, device=dev)
    torch.cuda.synchronize()
    H.ktime_begin(8)
    try:
        with pytest.raises(ValueError):
            H.colsum(H.rows(x), M, Np, H.wmap(0, Np, 0), out, ws)
    finally:
        nk = H.ktime_end()
    torch.cuda.synchronize()
    assert nk == 0
    assert bool((out == -7.0).all())
    assert H.colsum_ws(Np) == 512 * Np and H.colsum_ws(16) == 512 * 16


# ---- b. packs at n_perm = 9 ---------------------------------------------------------------------------------------
def _weights(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(CO, NF, 3, 3, generator=g) * 0.05, torch.randn(CO, generator=g) * 0.1


def _pack(w, shape, dt, m):
    dst = torch.full(shape, float("nan"), device=dev, dtype=dt)
    H.pack_weight(w.to(dev), dst, m)
    torch.cuda.synchronize()
    return dst.cpu()


def test_pack_kinds_nperm9():
    """pack_weight of the [576, 64, 3, 3] upsampling weight and its bias with n_perm = 9 against an index-exact
    torch permutation: kinds 1 / 2 / 4 exactly (fp32) and to the rounded reference (bf16); the pair forms 9 (bf16
    and fp16) and 18 (fp16): hi plane = the rounded reference, hi + lo back to fp32 (bf16 pairs 2^-16, fp16 pairs of
    w 2^KAIR_X3_WEXP 1e-6, the bar of test_x3_gpu.py::test_split_pack_kinds)."""
    w, b = _weights()
    idx = spm_index()
    grp = ((1, CO, CO), (1, NF, NF))
    fwd = w.permute(0, 2, 3, 1).reshape(CO, 9 * NF)[idx]                 # [p][tap * 64 + ci]
    dgr = w[idx].permute(1, 2, 3, 0).reshape(NF, 9 * CO)                 # [ci][tap * 576 + p]
    for dt in (torch.float32, torch.bfloat16):
        assert torch.equal(_pack(w, (CO, 9 * NF), dt, H.wmap(1, CO, NF, *grp, n_perm=9)), fwd.to(dt))
        assert torch.equal(_pack(w, (NF, 9 * CO), dt, H.wmap(2, CO, NF, *grp, n_perm=9)), dgr.to(dt))
    assert torch.equal(_pack(b, (CO,), torch.float32, H.wmap(4, CO, 0, (1, CO, CO), (1, 1, 1), n_perm=9)), b[idx])
    # pair forms: 64-column chunks alternate hi / lo
    for kind, plain, dt, e in ((9, fwd, torch.bfloat16, 0), (9, fwd, torch.float16, H.X3_WEXP),
                               (18, dgr, torch.float16, H.X3_WEXP)):
        rows, rowlen = plain.shape
        assert rowlen % 64 == 0
        got = _pack(w, (rows, 2 * rowlen), dt, H.wmap(kind, CO, NF, *grp, n_perm=9)).view(rows, rowlen // 64, 2, 64)
        hi, lo = got[:, :, 0].reshape(rows, rowlen), got[:, :, 1].reshape(rows, rowlen)
        sc = plain * 2.0 ** e
        assert torch.equal(hi, sc.to(dt)), (kind, dt)
        recon = (hi.double() + lo.double()) * 2.0 ** -e
        assert rel(recon, plain) < (2.0 ** -16 if dt == torch.bfloat16 else 1e-6), (kind, dt)
    # tied over a [hi | lo] pair image (kG = 2): both halves repeat the 64 input channels
    tied = w.permute(0, 2, 3, 1)[idx].repeat(1, 1, 1, 2).reshape(CO, 9 * 128)
    got = _pack(w, (CO, 2 * 9 * 128), torch.bfloat16, H.wmap(9, CO, NF, (1, CO, CO), (2, NF, NF), n_perm=9))
    assert torch.equal(got.view(CO, 18, 2, 64)[:, :, 0].reshape(CO, 9 * 128), tied.bfloat16())


def test_wgrad_finalize_nperm9():
    """Split planes [S][576][9 * 64] in the packed (sub-pixel-major) layout, built on the host, summed back into the
    reference layout [576, 64, 3, 3]; accumulate adds onto the gradient."""
    g = torch.Generator().manual_seed(23)
    S = 5
    part = torch.randn(S, CO, 9 * NF, generator=g)
    tot = part.double().sum(0)                                            # [p][tap * 64 + ci]
    ref = torch.empty(CO, NF, 3, 3, dtype=torch.float64)
    ref[spm_index()] = tot.view(CO, 9, NF).permute(0, 2, 1).reshape(CO, NF, 3, 3)
    m = H.wmap(1, CO, NF, (1, CO, CO), (1, NF, NF), n_perm=9)
    grad = torch.full((CO, NF, 3, 3), float("nan"), device=dev)
    H.wgrad_finalize(part.to(dev), S, m, grad)
    torch.cuda.synchronize()
    assert rel(grad, ref) < 1e-6
    H.wgrad_finalize(part.to(dev), S, m, grad, accumulate=True)
    torch.cuda.synchronize()
    assert rel(grad, 2 * ref) < 1e-6


# ---- c. forward upsampling conv 64 -> 576, PSHUF_SPM store -------------------------------------------------------
def _rows(t):
    B, C, Hh, Ww = t.shape
    return t.permute(0, 2, 3, 1).reshape(-1, C).contiguous()


def _pair(r):
    hi = r.bfloat16()
    return torch.cat([hi, (r - hi.float()).bfloat16()], 1).contiguous()


def _shuffled(out, B, Hh, Ww):
    """[B * 3H * 3W, 64] NHWC rows of the shuffled image -> NCHW"""
    return out.double().cpu().view(B, R * Hh, R * Ww, NF).permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", [(2, 12, 16), (1, 10, 14)])
def test_upsampling_conv_pshuf_r3(shape):
    """conv 64 -> 576 stored through PixelShuffle(3) (three column tiles; (1, 10, 14): M = 140 rows, no multiple of
    an M tile) vs float64 pixel_shuffle(conv2d).  Bars of the r = 2 siblings: fp32 2e-5 (test_kernels_gpu.py TOL);
    bf16 with hi/lo weights over bf16-exact activations 3e-5 and plain bf16 weights > 8x worse
    (test_conv3x3_split_weights); split activations with a [hi | lo] pair output 3e-5 and a pair input through tied
    weights 5e-5 (test_conv_asplit_hilo_pairs); fp32x3 2e-6 (test_gemm_nt_x3_ring_epilogues)."""
    B, Hh, Ww = shape
    M = B * Hh * Ww
    g = torch.Generator().manual_seed(Hh * Ww)
    w, b = _weights(7)
    x = torch.randn(B, NF, Hh, Ww, generator=g)
    xb = x.bfloat16().float()
    ref = F.pixel_shuffle(F.conv2d(x.double(), w.double(), b.double(), padding=1), R)
    refb = F.pixel_shuffle(F.conv2d(xb.double(), w.double(), b.double(), padding=1), R)
    wd, grp = w.to(dev), ((1, CO, CO), (1, NF, NF))
    bp = torch.empty(CO, device=dev)
    H.pack_weight(b.to(dev), bp, H.wmap(4, CO, 0, (1, CO, CO), (1, 1, 1), n_perm=9))
    ep = lambda out, **kw: H.epilogue(out, mode=H.OUT_PSHUF_SPM, ldo=out.shape[1], bias=bp, ps=(R, Hh, Ww), **kw)
    new = lambda ld=NF, dt=torch.float32: torch.full((M * R * R, ld), float("nan"), device=dev, dtype=dt)

    # fp32
    W1 = torch.empty(CO, 9 * NF, device=dev)
    H.pack_weight(wd, W1, H.wmap(1, CO, NF, *grp, n_perm=9))
    out = new()
    H.gemm_nt(H.im2col(_rows(x).to(dev), Hh, Ww, NF), H.rows(W1), ep(out), M, CO, 9 * NF, H.F32)
    torch.cuda.synchronize()
    assert rel(_shuffled(out, B, Hh, Ww), ref) < 2e-5

    # bf16: hi/lo weights and plain weights over bf16-exact activations
    W9 = torch.empty(CO, 2 * 9 * NF, device=dev, dtype=torch.bfloat16)
    H.pack_weight(wd, W9, H.wmap(9, CO, NF, *grp, n_perm=9))
    W1b = torch.empty(CO, 9 * NF, device=dev, dtype=torch.bfloat16)
    H.pack_weight(wd, W1b, H.wmap(1, CO, NF, *grp, n_perm=9))
    xin = _rows(xb).to(dev, torch.bfloat16)
    errs = []
    for Wb, split in ((W9, True), (W1b, False)):
        out = new()
        H.gemm_nt(H.im2col(xin, Hh, Ww, NF), H.rows(Wb, w_split=split), ep(out), M, CO, 9 * NF, H.BF16)
        torch.cuda.synchronize()
        errs.append(rel(_shuffled(out, B, Hh, Ww), refb))
    assert errs[0] < 3e-5 and errs[1] > 8 * errs[0] and errs[1] < 1e-2, errs

    # bf16, split activations of the fp32 image, the output as a [hi | lo] pair
    pair = new(2 * NF, torch.bfloat16)
    H.gemm_nt(H.asplit(H.im2col(_rows(x).to(dev), Hh, Ww, NF)), H.rows(W9, w_split=True), ep(pair, out_lo=pair[:, NF:]),
              M, CO, 9 * NF, H.BF16)
    torch.cuda.synchronize()
    assert rel(_shuffled(pair[:, :NF].double() + pair[:, NF:].double(), B, Hh, Ww), ref) < 3e-5

    # bf16, a [hi | lo] pair image read through weights tied over both halves (the engine's split_act form)
    W9t = torch.empty(CO, 2 * 9 * 2 * NF, device=dev, dtype=torch.bfloat16)
    H.pack_weight(wd, W9t, H.wmap(9, CO, NF, (1, CO, CO), (2, NF, NF), n_perm=9))
    out = new()
    H.gemm_nt(H.asplit(H.im2col(_pair(_rows(x)).to(dev), Hh, Ww, 2 * NF), pair=True), H.rows(W9t, w_split=True), ep(out),
              M, CO, 9 * 2 * NF, H.BF16)
    torch.cuda.synchronize()
    assert rel(_shuffled(out, B, Hh, Ww), ref) < 5e-5

    # fp32x3: fp16 pairs of w 2^KAIR_X3_WEXP
    W9h = torch.empty(CO, 2 * 9 * NF, device=dev, dtype=torch.float16)
    H.pack_weight(wd, W9h, H.wmap(9, CO, NF, *grp, n_perm=9))
    A, Bw = H.im2col(_rows(x).to(dev), Hh, Ww, NF), H.rows(W9h, w_split=True)
    A.x3_exp, Bw.x3_exp = 4, H.X3_WEXP
    out = new()
    H.gemm_nt(A, Bw, ep(out), M, CO, 9 * NF, H.X3)
    torch.cuda.synchronize()
    assert rel(_shuffled(out, B, Hh, Ww), ref) < 2e-6


# ---- d. input gradient 576 -> 64, PUNSHUF_SPM store ----------------------------------------------------------------
@pytest.mark.parametrize("compute", [H.BF16, H.X3])
@pytest.mark.parametrize("mode", ["punshuf", "gate"])
def test_input_gradient_c576_punshuf_r3(mode, compute):
    """test_tail_gpu.py::test_halo_channel_groups at C = 576 (the x3 pre-shuffle gradient, nine 64-channel groups):
    into the PixelUnshuffle(3) sub-pixel-major rows of a previous stage (ldo = 9 * 64, ps 4 x 6) and into plain
    gated rows, vs float64 conv_transpose2d.  bf16 (bf16-exact operands): that test's 1e-5; fp32x3 (fp32 operands):
    2e-6, the bar of test_x3_gpu.py's flipped im2col forms.  `out` starts as NaN: an unwritten element fails."""
    B, Hh, Ww, C, N, r = 2, 12, 18, CO, NF, R
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, C, Hh, Ww, generator=g)
    w = torch.randn(C, N, 3, 3, generator=g) * 0.03   # forward conv N -> C
    M = B * Hh * Ww
    if compute == H.BF16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
        xin = _rows(x).to(dev, torch.bfloat16)
        Wd = torch.empty(N, 9 * C, device=dev, dtype=torch.bfloat16)
        H.pack_weight(w.to(dev), Wd, H.wmap(2, C, N, (1, C, C), (1, N, N)))
        gate = torch.randn(M, 128, generator=g).bfloat16()
        bar = 1e-5
    else:
        xin = _rows(x).to(dev)
        Wd = torch.empty(N, 2 * 9 * C, device=dev, dtype=torch.float16)
        H.pack_weight(w.to(dev), Wd, H.wmap(18, C, N, (1, C, C), (1, N, N)))
        gate = torch.randn(M, 128, generator=g)
        bar = 2e-6
    ref = F.conv_transpose2d(x.double(), w.double(), padding=1)   # [B, N, H, W]
    A, Bw = H.im2col(xin, Hh, Ww, C, flip=True), H.rows(Wd)
    if compute == H.X3:
        A.x3_exp, Bw.x3_exp = 4, H.X3_WEXP
    if mode == "punshuf":
        out = torch.full((M // (r * r), r * r * N), float("nan"), device=dev)
        H.gemm_nt(A, Bw, H.epilogue(out, mode=H.OUT_PUNSHUF_SPM, ldo=r * r * N, ps=(r, Hh // r, Ww // r)), M, N, 9 * C,
                  compute)
        torch.cuda.synchronize()
        got = out.cpu().view(B, Hh // r, Ww // r, r, r, N).permute(0, 5, 1, 3, 2, 4).reshape(B, N, Hh, Ww)
    else:
        out = torch.full((M, N), float("nan"), device=dev)
        H.gemm_nt(A, Bw, H.epilogue(out, gate=gate.to(dev), ldg=128, gate_kind=2, slope=0.01), M, N, 9 * C, compute)
        torch.cuda.synchronize()
        got = out.cpu().view(B, Hh, Ww, N).permute(0, 3, 1, 2)
        gs = torch.where(gate[:, :N].float() > 0, 1.0, 0.01).view(B, Hh, Ww, N).permute(0, 3, 1, 2)
        ref = ref * gs.double()
    assert bool(torch.isfinite(got).all())
    assert rel(got, ref) < bar


# ---- f. the engine ------------------------------------------------------------------------------------------------
OUT_BAR = {"fp32": 1e-4, "bf16": 2e-2, "fp32x3": 1e-4}
GRAD_BAR = {"fp32": 2e-3, "bf16": 8e-2, "fp32x3": 2e-3}
_ORACLE = {}


def _net(dt, embed=60, lr=16, seed=11):
    torch.manual_seed(seed)
    return SwinIR(upscale=3, in_chans=3, img_size=lr, window_size=8, img_range=1.0, depths=[2, 2], embed_dim=embed,
                  num_heads=[6, 6], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv", drop_path_rate=0.0,
                  compute_dtype=dt)


def _oracle(embed, h, w, img=16):
    """The CPU oracle's output, loss and gradients for the (embed, LR h x w) case: computed once, shared by the
    compute dtypes and both backward entries (same seed -> same weights and batch), never modified."""
    key = (embed, h, w)
    if key not in _ORACLE:
        net = _net("fp32", embed, img)
        ref = osw.SwinIR(3, 3, img, 8, 1.0, [2, 2], embed, [6, 6], 2, "pixelshuffle")
        ref.load_state_dict(net.state_dict(), strict=True)
        g = torch.Generator().manual_seed(12)
        L, Hh = torch.rand(2, 3, h, w, generator=g), torch.rand(2, 3, R * h, R * w, generator=g)
        Er = ref(L)
        loss = F.l1_loss(Er, Hh)
        loss.backward()
        _ORACLE[key] = (L, Hh, Er.detach(), loss.item(), {k: p.grad.detach() for k, p in ref.named_parameters()})
    return _ORACLE[key]


def _check(dt, E, loss, grads, oracle):
    L, Hh, Er, lr_, gref = oracle
    tol = OUT_BAR[dt]
    e_rel = rel(E, Er)
    errs = sorted(((rel(g, gref[k]), k) for k, g in grads.items()), reverse=True)
    print(f"x3 {dt}: E rel {e_rel:.3e}, loss {loss:.6f} vs {lr_:.6f}, upsample.0.bias {dict((k, e) for e, k in errs)['upsample.0.bias']:.3e}, "
          f"worst {errs[0]}")
    assert e_rel < tol
    assert abs(loss - lr_) < 10 * tol * lr_
    assert set(grads) == set(gref)
    assert errs[0][0] < GRAD_BAR[dt], errs[:3]


@pytest.mark.parametrize("entry", ["loss", "grad"])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp32x3"])
def test_engine_x3_vs_oracle(dt, entry):
    """pixelshuffle x3, embed 60, depths [2, 2], LR 16 x 16, B = 2 against oracle.swinir.SwinIR(3, ...) on the same
    state dict: output, loss and every parameter gradient (the 576-wide bias gradient upsample.0.bias among them),
    through backward_from_loss and, through autograd, backward_from_grad."""
    oracle = _oracle(60, 16, 16)
    L, Hh = oracle[0].to(dev), oracle[1].to(dev)
    net = _net(dt).to(dev).train()
    if entry == "grad":
        E = net(L)
        loss = F.l1_loss(E, Hh)
        loss.backward()
        grads = {k: p.grad for k, p in net.named_parameters()}
        loss = loss.item()
    else:
        eng = net.engine()
        named = list(net.named_parameters())
        flat = torch.full((sum(p.numel() for _, p in named),), float("nan"), device=dev)   # every element is written
        grads, off = {}, 0
        for k, p in named:
            grads[k] = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        E = eng.forward(L)
        loss = eng.backward_from_loss(Hh, {p: grads[k] for k, p in named}).item()
    torch.cuda.synchronize()
    _check(dt, E, loss, grads, oracle)


@pytest.mark.parametrize("dt", ["bf16", "fp32x3"])
def test_engine_x3_narrow_conv_last(dt):
    """LR 8 x 64 (HR width 192, a multiple of 64): conv_last runs on the narrow-output kernels with the
    PixelUnshuffle(3) store (r_last = 3) -- asserted from the plan."""
    oracle = _oracle(60, 8, 64)
    L, Hh = oracle[0].to(dev), oracle[1].to(dev)
    net = _net(dt).to(dev).train()   # (img_size 16: the 8 x 64 input takes the blocks' shifted windows as any size does)
    E = net(L)
    loss = F.l1_loss(E, Hh)
    loss.backward()
    torch.cuda.synchronize()
    eng = net.engine()
    P = eng.cur
    assert eng.tail.ups_r == [3] and (P["W"] * eng.scale) % 64 == 0
    if dt == "fp32x3":
        assert eng.tail.last_narrow_x3 and P["dE_ld"] == 4
    else:
        assert eng.tail.last.narrow and "narrow_ws" in P
    _check(dt, E, loss.item(), {k: p.grad for k, p in net.named_parameters()}, oracle)


@pytest.mark.parametrize("dt", ["bf16", "fp32x3"])
def test_engine_x3_embed180_falls_back_to_gemm(dt):
    """embed 180, LR 24: the 64 -> 576 upsampling conv is no kair_conv3x3_wr pair form (that needs Cop == 256); it
    must run on the implicit-GEMM path without error, at the same bars."""
    oracle = _oracle(180, 24, 24, img=24)
    L, Hh = oracle[0].to(dev), oracle[1].to(dev)
    net = _net(dt, 180, 24).to(dev).train()
    E = net(L)
    loss = F.l1_loss(E, Hh)
    loss.backward()
    torch.cuda.synchronize()
    eng = net.engine()
    assert [c.Co for c in eng.tail.ups] == [CO] and not any(c.wr_pair for c in eng.tail.ups)
    _check(dt, E, loss.item(), {k: p.grad for k, p in net.named_parameters()}, oracle)


# ---- g. every engine's column-sum workspace covers the widest launch it issues -----------------------------------
def _swinir_engine(ups, sc, resi="1conv", ch=3):
    net = SwinIR(upscale=sc, in_chans=ch, img_size=16, window_size=8, img_range=1.0, depths=[2], embed_dim=60,
                 num_heads=[6], mlp_ratio=2, upsampler=ups, resi_connection=resi, drop_path_rate=0.0,
                 compute_dtype="fp32").to(dev).train()
    return net, net.engine()


def _swinir_widths(eng):
    """Np of every kair_colsum the SwinIR step can issue, read from the layer objects: the tail convs' packed and
    real output widths, and a '3conv' residual's Cp and bottleneck width."""
    w = [c.Cop for c in eng.tail.convs()] + [c.Co for c in eng.tail.convs()]
    for r in eng._resis():
        if isinstance(r, _Resi3):
            w += [eng.Cp, r.Cq]
    return w


@pytest.mark.parametrize("case", ["swinir_x3", "swinir_x4", "swinir_nearest", "swinir_3conv", "rrdbnet", "dncnn"])
def test_colsum_workspace_covers_plan(case):
    if case.startswith("swinir"):
        ups, sc, resi = {"swinir_x3": ("pixelshuffle", 3, "1conv"), "swinir_x4": ("pixelshuffle", 4, "1conv"),
                         "swinir_nearest": ("nearest+conv", 4, "1conv"), "swinir_3conv": ("", 1, "3conv")}[case]
        net, eng = _swinir_engine(ups, sc, resi)
        widths = _swinir_widths(eng)
        if case == "swinir_x3":
            assert CO in widths
    elif case == "rrdbnet":
        from kair_amd.models.network_rrdbnet import RRDBNet
        net = RRDBNet(3, 3, 32, 1, 16, 4, compute_dtype="fp32").to(dev).train()
        eng = net.engine()
        widths = [c.Cop for c in eng.convs()]
    else:
        from kair_amd.models.network_dncnn import DnCNN
        net = DnCNN(1, 1, 64, 5, "BR", compute_dtype="fp32").to(dev).train()
        eng = net.engine()
        widths = [c.Cop for c in eng.convs()]
    P = eng.plan(2, 16, 16)
    need = max(H.colsum_ws(n) for n in widths)
    assert P["colsum_ws"].dtype == torch.float32 and P["colsum_ws"].numel() >= need, (P["colsum_ws"].numel(), need)
