"""The small kernels that only whole networks used to exercise, each against a float64 torch restatement on the CPU:
BatchNorm forward / backward (csrc/batchnorm.hip), act_grad_cast / sumpool2x / axpby / axpby_rows / image_to_nhwc
(csrc/elementwise.hip), and the USRNet helpers usr_pad / usr_upsample_nearest / usr_pack_input / usr_chan_sum /
hypanet_fwd / hypanet_bwd (csrc/fft.hip).

Rows are wider than C and the padding holds a sentinel that must survive (usr_pack_input and image_to_nhwc define
their pad as 0 instead).  Bounds: a kernel that only moves values matches torch bit for bit; fp32 arithmetic is held
to 2e-5 relative (TOL[F32] of test_kernels_gpu.py, norm-relative as there); a bf16 output to one bf16 rounding of
the float64 result, 2^-8 relative per element, on top of that fp32 bound (which is what a value next to zero, formed
by cancellation, can be off by before it is rounded)."""
import pytest
import torch
import torch.nn.functional as F

from kair_amd import _hip as H

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
SENT = 7.0
F32_TOL = 2e-5                      # TOL[H.F32][0] of test_kernels_gpu.py
DTS = [torch.float32, torch.bfloat16]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def assert_close(got, ref, what=""):
    """fp32 result: norm-relative 2e-5.  bf16 result: every element within 2^-8 |ref| + 2e-5 max|ref|."""
    ref = ref.double().cpu()
    if got.dtype == torch.bfloat16:
        d = (got.double().cpu() - ref).abs()
        lim = 2.0 ** -8 * ref.abs() + F32_TOL * ref.abs().max()
        assert (d <= lim).all(), (what, (d - lim).max().item())
    else:
        assert rel_err(got, ref) < F32_TOL, (what, rel_err(got, ref))


def padded(v, ld, dtype=torch.float32):
    """rows of v [M, C] in a sentinel-filled [M, ld] device tensor"""
    t = torch.full((v.shape[0], ld), SENT, dtype=dtype)
    t[:, :v.shape[1]] = v.to(dtype)
    return t.to(dev)


def gate64(pos, neg):
    """1 where pos, else neg, in float64"""
    return torch.where(pos, torch.tensor(1.0, dtype=torch.float64), torch.tensor(float(neg), dtype=torch.float64))


def pad_intact(t, C):
    return bool((t[:, C:] == SENT).all().item())


# ------------------------------------------------------------------------------------------------------------
# BatchNorm (momentum 0.9, eps 1e-4: basicblock.py:69)
# ------------------------------------------------------------------------------------------------------------
MOM, EPS, SLOPE = 0.9, 1e-4, 0.2
BN_SHAPES = [(1000, 64), (300, 40), (2049, 65), (1, 8)]


def _act(y, act):
    return y if act == 0 else (F.relu(y) if act == 1 else F.leaky_relu(y, SLOPE))


def _bn_train_ref(z, gamma, beta, rm, rv):
    """float64 F.batch_norm in train mode (updates rm / rv in place).  F.batch_norm refuses one value per channel;
    there the same formula is written out: batch variance 0, and the running variance takes the biased one."""
    if z.shape[0] > 1:
        return F.batch_norm(z, rm, rv, gamma, beta, True, MOM, EPS)
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    rm.mul_(1 - MOM).add_(MOM * mu.detach())
    rv.mul_(1 - MOM).add_(MOM * var.detach())
    return (z - mu) / torch.sqrt(var + EPS) * gamma + beta


def _bn_inputs(M, C, seed=0):
    g = torch.Generator().manual_seed(100 * C + M + seed)
    z = torch.randn(M, C, generator=g) * 1.7 + 0.4
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return g, z, gamma, beta, rm, rv


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_fwd(M, C, act, dt):
    g, z, gamma, beta, rm, rv = _bn_inputs(M, C)
    ldz, ldo = C + 3, C + 5
    zd, gd, bd = padded(z, ldz), gamma.to(dev), beta.to(dev)
    rmd, rvd = rm.to(dev), rv.to(dev)
    out = torch.full((M, ldo), SENT, device=dev, dtype=dt)
    mean, rstd = torch.full((C,), SENT, device=dev), torch.full((C,), SENT, device=dev)
    ws = torch.empty(H.bn_ws(C), device=dev)
    H.bn_fwd(zd, ldz, out, ldo, M, C, gd, bd, rmd, rvd, MOM, EPS, True, mean, rstd, act, SLOPE, ws)
    torch.cuda.synchronize()
    z64, rm64, rv64 = z.double(), rm.double(), rv.double()
    ref = _act(_bn_train_ref(z64, gamma.double(), beta.double(), rm64, rv64), act)
    assert_close(out[:, :C], ref, "out")
    assert pad_intact(out, C)
    assert rel_err(mean, z64.mean(0)) < F32_TOL
    assert rel_err(rstd, 1 / torch.sqrt(z64.var(0, unbiased=False) + EPS)) < F32_TOL
    assert rel_err(rmd, rm64) < F32_TOL and rel_err(rvd, rv64) < F32_TOL          # rv64: unbiased variance
    assert not torch.equal(rv64, rv.double())

    # eval mode: from the running statistics, which it leaves alone
    out2 = torch.full((M, ldo), SENT, device=dev, dtype=dt)
    rm2, rv2 = rm.to(dev), rv.to(dev)
    H.bn_fwd(zd, ldz, out2, ldo, M, C, gd, bd, rm2, rv2, MOM, EPS, False, None, None, act, SLOPE, None)
    torch.cuda.synchronize()
    ref2 = _act(F.batch_norm(z64, rm.double(), rv.double(), gamma.double(), beta.double(), False, MOM, EPS), act)
    assert_close(out2[:, :C], ref2, "eval")
    assert pad_intact(out2, C)
    assert torch.equal(rm2.cpu(), rm) and torch.equal(rv2.cpu(), rv)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_bwd(M, C, act, dt):
    """dz / dgamma / dbeta against autograd through the float64 BatchNorm, the activation gated by the kernel's own
    stored output a (so a sign disagreement at a == 0 cannot arise); accumulate off, then on."""
    g, z, gamma, beta, rm, rv = _bn_inputs(M, C, seed=1)
    da = torch.randn(M, C, generator=g)
    ldz, lda, ldda, lddz = C + 3, C + 5, C + 1, C + 2
    zd, gd, bd = padded(z, ldz), gamma.to(dev), beta.to(dev)
    a = torch.full((M, lda), SENT, device=dev, dtype=dt)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(H.bn_ws(C), device=dev)
    H.bn_fwd(zd, ldz, a, lda, M, C, gd, bd, rm.to(dev), rv.to(dev), MOM, EPS, True, mean, rstd, act, SLOPE, ws)
    dad = padded(da, ldda)
    dz = torch.full((M, lddz), SENT, device=dev, dtype=dt)
    dgam, dbet = torch.full((C,), SENT, device=dev), torch.full((C,), SENT, device=dev)
    H.bn_bwd(zd, ldz, a, lda, dad, ldda, dz, lddz, M, C, gd, mean, rstd, act, SLOPE, dgam, dbet, False, ws)
    torch.cuda.synchronize()

    zr, gr, br = (t.double().requires_grad_(True) for t in (z, gamma, beta))
    y = _bn_train_ref(zr, gr, br, rm.double(), rv.double())
    pos = a[:, :C].float().cpu() > 0
    gate = torch.ones(M, C, dtype=torch.float64) if act == 0 else gate64(pos, SLOPE if act == 2 else 0.0)
    y.backward(da.double() * gate)
    assert_close(dz[:, :C], zr.grad, "dz")
    assert pad_intact(dz, C)
    assert rel_err(dgam, gr.grad) < F32_TOL and rel_err(dbet, br.grad) < F32_TOL  # the pre-fill is overwritten

    pre_g, pre_b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dgam, dbet = pre_g.to(dev), pre_b.to(dev)
    H.bn_bwd(zd, ldz, a, lda, dad, ldda, dz, lddz, M, C, gd, mean, rstd, act, SLOPE, dgam, dbet, True, ws)
    torch.cuda.synchronize()
    assert rel_err(dgam, pre_g.double() + gr.grad) < F32_TOL and rel_err(dbet, pre_b.double() + br.grad) < F32_TOL


def test_bn_rstd_conditioning():
    """z = 100 + 0.1 randn: the variance is 1e-6 of the mean square.  A float32 two-pass computation in torch on the
    CPU (mean, then the mean of squared deviations, 1 / sqrt) of this same z is off from float64 by 1.10e-7 relative
    at worst over the 64 channels (1.22e-7 with another CPU's summation order; the smaller figure is the one used);
    the kernel gets 4x that, and measures 1.22e-7.  One pass (E[z^2] - E[z]^2) in float32 is off by 0.31."""
    M, C = 4096, 64
    g = torch.Generator().manual_seed(41)
    z = 100 + 0.1 * torch.randn(M, C, generator=g)
    ldz = C + 3
    out = torch.empty(M, C, device=dev)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    H.bn_fwd(padded(z, ldz), ldz, out, C, M, C, torch.ones(C, device=dev), torch.zeros(C, device=dev), None, None, MOM,
             EPS, True, mean, rstd, 0, 0.0, torch.empty(H.bn_ws(C), device=dev))
    torch.cuda.synchronize()
    r64 = 1 / torch.sqrt(z.double().var(0, unbiased=False) + EPS)
    m32 = z.mean(0)
    r32 = 1 / torch.sqrt(((z - m32) ** 2).mean(0) + EPS)
    emu = ((r32.double() - r64).abs() / r64).max().item()
    err = ((rstd.cpu().double() - r64).abs() / r64).max().item()
    print(f"rstd: kernel {err:.3e}, float32 two-pass emulation {emu:.3e}")
    assert err < 4 * 1.10e-7, (err, emu)                                          # measured 1.10e-7, margin 4x


# ------------------------------------------------------------------------------------------------------------
# elementwise.hip
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", DTS)
@pytest.mark.parametrize("xdt", DTS)
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_act_grad_cast(kind, xdt, odt):
    """out = scale * G * act'(X): X the post-activation for ReLU / LeakyReLU (gate xv > 0, so ReLU'(0) = 0 and
    leaky'(0) = slope), the pre-activation for the exact-erf GELU' (kind 3)."""
    M, C, slope, scale = 37, 45, 0.2, 1.7                                         # M C = 1665: not a multiple of 256
    g = torch.Generator().manual_seed(50 + kind)
    G = torch.randn(M, C, generator=g)
    X = (torch.randn(M, C, generator=g) * 1.5).to(xdt)
    X[::3, ::4] = 0
    ldg, ldx, ldo = C + 1, C + 2, C + 3
    out = torch.full((M, ldo), SENT, device=dev, dtype=odt)
    H.act_grad_cast(padded(G, ldg), ldg, padded(X, ldx, xdt), ldx, out, ldo, M, C, kind, slope, scale)
    torch.cuda.synchronize()
    x64 = X.double()
    if kind == 0:
        d = torch.ones_like(x64)
    elif kind == 3:
        d = 0.5 * (1 + torch.erf(x64 / 2 ** 0.5)) + x64 * torch.exp(-0.5 * x64 * x64) / (2 * torch.pi) ** 0.5
    else:
        d = gate64(x64 > 0, slope if kind == 2 else 0.0)
    assert_close(out[:, :C], scale * G.double() * d)
    assert pad_intact(out, C)
    if kind in (1, 2):
        z = out[:, :C].float().cpu()[::3, ::4]
        want = (scale * G.double() * (slope if kind == 2 else 0.0))[::3, ::4]
        assert (z == 0).all() if kind == 1 else (z != 0).all()
        assert_close(out[:, :C][::3, ::4], want)


@pytest.mark.parametrize("accumulate", [False, True])
def test_sumpool2x(accumulate):
    B, Hh, Ww, C, lds, ldd = 2, 3, 5, 7, 9, 12
    g = torch.Generator().manual_seed(60)
    src = torch.randn(B, 2 * Hh, 2 * Ww, C, generator=g) + 1.5
    pre = torch.randn(B * Hh * Ww, C, generator=g)
    dst = padded(pre, ldd)
    H.sumpool2x(padded(src.view(-1, C), lds), lds, dst, ldd, B, Hh, Ww, C, accumulate)
    torch.cuda.synchronize()
    ref = 4 * F.avg_pool2d(src.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, C)
    assert rel_err(dst[:, :C], ref + pre.double() if accumulate else ref) < F32_TOL
    assert pad_intact(dst, C)
    if not accumulate:   # the adjoint of nearest x2 upsampling: <up(a), b> = <a, pool(b)>
        a = torch.rand(B, C, Hh, Ww, generator=g, dtype=torch.float64) + 0.5   # both mostly positive: no cancellation
        up = F.interpolate(a, scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
        lhs = (up * src.double()).sum().item()
        rhs = (a.permute(0, 2, 3, 1).reshape(-1, C) * dst[:, :C].double().cpu()).sum().item()
        assert abs(lhs - rhs) < 1e-6 * abs(lhs)


@pytest.mark.parametrize("n", [5, 8192 * 256 + 5])
def test_axpby(n):
    """y = a x + b y; the larger n is one element past 8192 blocks of 256, so the grid-stride loop runs a second
    time.  The kernel multiplies whatever y holds: b = 0 does NOT clean a NaN or Inf left in y (0 * NaN = NaN), so
    a caller that wants y = a x passes an initialised y."""
    g = torch.Generator().manual_seed(61)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    yd = torch.full((n + 3,), SENT, device=dev)
    yd[:n] = y.to(dev)
    H.axpby(yd, x.to(dev), 0.75, -1.5, n)
    torch.cuda.synchronize()
    assert rel_err(yd[:n], 0.75 * x.double() - 1.5 * y.double()) < F32_TOL
    assert (yd[n:] == SENT).all()


def test_axpby_rows():
    M, C, ldy, ldx = 37, 45, 48, 51
    g = torch.Generator().manual_seed(62)
    x, y = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    yd = padded(y, ldy)
    H.axpby_rows(yd, ldy, padded(x, ldx), ldx, M, C, 0.75, -1.5)
    torch.cuda.synchronize()
    assert rel_err(yd[:, :C], 0.75 * x.double() - 1.5 * y.double()) < F32_TOL
    assert pad_intact(yd, C)


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("dt", DTS)
def test_image_to_nhwc(dt, with_mean):
    B, C, Hh, Ww, ldc, rng = 2, 3, 5, 9, 32, 255.0
    g = torch.Generator().manual_seed(63)
    img = torch.rand(B, C, Hh, Ww, generator=g)
    mean = torch.tensor([0.4488, 0.4371, 0.4040]) if with_mean else None
    out = torch.full((B * Hh * Ww, ldc), SENT, device=dev, dtype=dt)
    H.image_to_nhwc(img.to(dev), out, ldc, mean.to(dev) if with_mean else None, rng, B, C, Hh, Ww)
    torch.cuda.synchronize()
    v = img.double() - (mean.double().view(1, C, 1, 1) if with_mean else 0.0)
    assert_close(out[:, :C], (v * rng).permute(0, 2, 3, 1).reshape(-1, C))
    assert (out[:, C:] == 0).all()


# ------------------------------------------------------------------------------------------------------------
# USRNet helpers (fft.hip)
# ------------------------------------------------------------------------------------------------------------
PAD_GEOM = [(13, 10, 16, 16), (8, 8, 8, 8)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["replicate", "zero"])
@pytest.mark.parametrize("Hh,Ww,Hp,Wp", PAD_GEOM)
def test_usr_pad_replicate_zero(Hh, Ww, Hp, Wp, mode, dt):
    nb, ldc = 2, 5
    g = torch.Generator().manual_seed(70)
    src = torch.randn(nb, Hh, Ww, ldc, generator=g).to(dt)
    dst = torch.full((nb, Hp, Wp, ldc), SENT, device=dev, dtype=dt)
    H.usr_pad(src.to(dev), dst, H.USR_PAD_REPLICATE if mode == "replicate" else H.USR_PAD_ZERO, ldc, nb, Hh, Ww, Hp, Wp)
    torch.cuda.synchronize()
    ref = F.pad(src.float().permute(0, 3, 1, 2), (0, Wp - Ww, 0, Hp - Hh), mode="replicate" if mode == "replicate" else "constant")
    assert torch.equal(dst.cpu(), ref.permute(0, 2, 3, 1).to(dt))


@pytest.mark.parametrize("Hh,Ww,Hp,Wp", PAD_GEOM)
def test_usr_pad_fold_crop(Hh, Ww, Hp, Wp):
    nb, ldc = 2, 5
    g = torch.Generator().manual_seed(71)
    b = torch.randn(nb, Hp, Wp, ldc, generator=g)
    dst = torch.full((nb, Hh, Ww, ldc), SENT, device=dev)
    H.usr_pad(b.to(dev), dst, H.USR_PAD_FOLD, ldc, nb, Hh, Ww, Hp, Wp)
    torch.cuda.synchronize()
    a = torch.randn(nb, ldc, Hh, Ww, generator=g, dtype=torch.float64).requires_grad_(True)
    pa = F.pad(a, (0, Wp - Ww, 0, Hp - Hh), mode="replicate")
    pa.backward(b.double().permute(0, 3, 1, 2))                                    # the replicate pad's adjoint
    fold = dst.cpu().double().permute(0, 3, 1, 2)
    assert rel_err(fold, a.grad) < F32_TOL
    lhs, rhs = (pa.detach() * b.double().permute(0, 3, 1, 2)).sum().item(), (a.detach() * fold).sum().item()
    assert abs(lhs - rhs) < F32_TOL * (pa.detach() * b.double().permute(0, 3, 1, 2)).abs().sum().item()
    # crop of NCHW planes
    planes = torch.randn(nb * 3, Hp, Wp, generator=g)
    crop = torch.full((nb * 3, Hh, Ww), SENT, device=dev)
    H.usr_pad(planes.to(dev), crop, H.USR_CROP_NCHW, 0, nb * 3, Hh, Ww, Hp, Wp)
    torch.cuda.synchronize()
    assert torch.equal(crop.cpu(), planes[:, :Hh, :Ww])


def test_usr_pad_rejects():
    src = torch.zeros(2, 13, 10, 5, device=dev)
    dst = torch.full((2, 16, 16, 5), SENT, device=dev)
    H.ktime_begin(8)
    try:
        with pytest.raises(RuntimeError):   # bf16 fold
            H.usr_pad(dst.bfloat16(), src.bfloat16(), H.USR_PAD_FOLD, 5, 2, 13, 10, 16, 16)
        with pytest.raises(RuntimeError):   # in place
            H.usr_pad(dst, dst, H.USR_PAD_REPLICATE, 5, 2, 13, 10, 16, 16)
        with pytest.raises(RuntimeError):   # Hp < H
            H.usr_pad(src, dst, H.USR_PAD_REPLICATE, 5, 2, 13, 10, 12, 16)
    finally:
        n = H.ktime_end()
    assert n == 0 and (dst == SENT).all()


@pytest.mark.parametrize("sf", [2, 3, 4])
def test_usr_upsample_nearest(sf):
    planes, h, w = 3, 5, 7
    L = torch.randn(planes, h, w, generator=torch.Generator().manual_seed(72))
    out = torch.full((planes * h * sf * w * sf + 4,), SENT, device=dev)
    H.usr_upsample_nearest(L.to(dev), out, planes, h, w, sf)
    torch.cuda.synchronize()
    ref = F.interpolate(L[None], scale_factor=sf, mode="nearest")[0]
    assert torch.equal(out[:-4].cpu().view(planes, h * sf, w * sf), ref)
    assert (out[-4:] == SENT).all()


@pytest.mark.parametrize("dt", DTS)
def test_usr_pack_input(dt):
    B, C, HW, ld, bs = 2, 3, 35, 8, 2
    g = torch.Generator().manual_seed(73)
    x, beta = torch.randn(B, C, HW, generator=g), torch.randn(B * bs, generator=g)
    out = torch.full((B * HW, ld), SENT, device=dev, dtype=dt)
    H.usr_pack_input(x.to(dev), beta.to(dev), bs, out, ld, B, C, HW)
    torch.cuda.synchronize()
    ref = torch.zeros(B, HW, ld)
    ref[:, :, :C] = x.permute(0, 2, 1)
    ref[:, :, C] = beta[::bs][:, None]
    assert torch.equal(out.cpu(), ref.view(-1, ld).to(dt))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("HW", [35, 4096])
def test_usr_chan_sum(HW, accumulate):
    B, ld, c, ostride = 3, 6, 2, 2
    g = torch.Generator().manual_seed(74)
    x = torch.randn(B * HW, ld, generator=g)
    pre = torch.randn(B * ostride, generator=g)
    out = pre.to(dev)
    ws = torch.empty(B * H.USR_CHAN_CHUNKS, device=dev)
    H.usr_chan_sum(x.to(dev), ld, c, HW, B, ws, out, ostride, accumulate)
    torch.cuda.synchronize()
    col = x[:, c].double().view(B, HW)
    ref = pre.double().clone()
    ref[::ostride] = col.sum(1) + (pre.double()[::ostride] if accumulate else 0.0)
    got = out.cpu().double()
    assert ((got - ref)[::ostride].abs() <= F32_TOL * col.abs().sum(1)).all()
    assert torch.equal(out.cpu()[1::ostride], pre[1::ostride])                     # between the strided outputs


def _hypa_params(hc, no, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    W1, b1 = r(hc, 2) * 0.5, r(hc) * 0.3
    W2, b2 = r(hc, hc) / hc ** 0.5, r(hc) * 0.3
    W3, b3 = r(no, hc) / hc ** 0.5, r(no) * 0.3
    b3[1] = 25.0      # softplus's x > 20 branch
    b1[2] = -50.0     # a dead ReLU in layer 1
    return g, [W1, b1, W2, b2, W3, b3]


def _hypa_ref(sigma, sf, P):
    W1, b1, W2, b2, W3, b3 = P
    inp = torch.stack([sigma, torch.full_like(sigma, sf)], 1)
    z3 = F.relu(F.relu(inp @ W1.t() + b1) @ W2.t() + b2) @ W3.t() + b3
    return F.softplus(z3) + 1e-6, z3


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("hc", [32, 64])
def test_hypanet_fwd_bwd(hc, accumulate):
    """HyPaNet (network_usrnet_v1.py:204-216) and its gradients for all six parameter tensors against autograd
    through the float64 MLP."""
    no, B, sf = 16, 3, 3.0
    g, P = _hypa_params(hc, no, 80 + hc)
    sigma = torch.rand(B, generator=g) * 0.2
    gab = torch.randn(B, no, generator=g)
    Pd = [p.to(dev) for p in P]
    ab = torch.full((B * no + 4,), SENT, device=dev)
    H.hypanet_fwd(sigma.to(dev), sf, *Pd, hc, no, B, ab)
    P64 = [p.double().requires_grad_(True) for p in P]
    ref, z3 = _hypa_ref(sigma.double(), sf, P64)
    assert (z3[:, 1] > 20).all() and (sigma.double()[:, None] * P64[0][2, 0] + sf * P64[0][2, 1] + P64[1][2] < 0).all()
    ref.backward(gab.double())
    pre = [torch.randn(p.shape, generator=g) for p in P]
    G = [p.to(dev) for p in pre]
    H.hypanet_bwd(sigma.to(dev), sf, *Pd, hc, no, B, gab.to(dev), *G, accumulate=accumulate)
    torch.cuda.synchronize()
    abg = ab[:B * no].view(B, no).cpu().double()          # per element: the b3 = 25 output would carry a norm
    assert ((abg - ref.detach()).abs() <= F32_TOL * ref.detach().abs()).all()
    assert (ab[B * no:] == SENT).all()
    for name, got, p0, p in zip(("W1", "b1", "W2", "b2", "W3", "b3"), G, pre, P64):
        want = p.grad + p0.double() if accumulate else p.grad
        assert rel_err(got, want) < F32_TOL, name
    dead_W1, dead_b1 = G[0][2].cpu(), G[1][2].cpu()         # the dead unit gets no gradient at all
    assert torch.equal(dead_W1, pre[0][2] if accumulate else torch.zeros(2))
    assert torch.equal(dead_b1, pre[1][2] if accumulate else torch.zeros(()))


def test_hypanet_rejects_batch_beyond_lds():
    """B (4 hc + 2 no) floats of LDS for the backward: 58 x 288 x 4 bytes > 64 KiB is refused, not launched."""
    hc, no, B = 64, 16, 58
    g, P = _hypa_params(hc, no, 90)
    Pd = [p.to(dev) for p in P]
    G = [torch.full(p.shape, SENT, device=dev) for p in P]
    sigma, gab = torch.rand(B, device=dev), torch.randn(B, no, device=dev)
    H.ktime_begin(8)
    try:
        with pytest.raises(RuntimeError, match="hypanet_bwd"):
            H.hypanet_bwd(sigma, 3.0, *Pd, hc, no, B, gab, *G)
    finally:
        n = H.ktime_end()
    assert n == 0 and all((t == SENT).all() for t in G)
