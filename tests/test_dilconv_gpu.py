"""Dilated 3x3 convs on the device against the float64 statements of tests/dilconv_ref.py, elementwise, at the bound of
tests/convnet_forms_ref.py:  |got - ref| <= 2 (K + 4) 2^-24 S + r_out  (K = 9 C; M + splits for weight gradients).

Generic path: kair_gemm_nt forward and flipped, kair_gemm_tn weight gradient, over kair_operand.im_dil (H.im2col(dil=)),
in the modes f32 / bf16 / bf16_f32A for d = 1..4.  The second case (C = 64, M = 2 * 144, aligned pointers) is one the
+-1-tap fast paths (halo conv, tap-per-tile rings) accept without dilation: a missed guard gives wrong numbers here.
kair_conv3x3_dil: forward (bias + ReLU) and flipped input gradient, d = 2..4, C = N = 64, bf16 rows in, bf16 and fp32
rows out into a wider, pattern-filled buffer.

Every input is bf16-exact; outputs live in guarded allocations filled with a bit pattern, so an element that must not be
written (a pad column of the wider rows, anything past the buffer) has to keep the pattern."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import convnet_forms_ref as R  # noqa: E402
import dilconv_ref as D  # noqa: E402
from kair_amd import _hip as H  # noqa: E402

dev = torch.device("cuda")
F32, BF = torch.float32, torch.bfloat16
MODES = {"f32": (H.F32, F32, F32), "bf16": (H.BF16, BF, BF), "bf16_f32A": (H.BF16, F32, F32)}   # compute, operands, out
PAT = {F32: (torch.int32, 0x5A5AA5A5), BF: (torch.int16, 0x5A5A)}
GUARD = 64


def wdt(mode):
    return F32 if MODES[mode][0] == H.F32 else BF


def poisoned(n, dt):
    """n elements of dtype dt between two guards, the whole allocation filled with a bit pattern."""
    it, pat = PAT[dt]
    buf = torch.full((n + 2 * GUARD,), pat, dtype=it, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dt)


def timed(fn):
    """Run fn inside a kernel timing window: the symbols of the kernels it launched."""
    torch.cuda.synchronize()
    H.ktime_begin(16)
    try:
        fn()
    finally:
        nk = H.ktime_end()
    torch.cuda.synchronize()
    return [H.ktime_read(i)[1].split("(")[0][-90:] for i in range(nk)]


def check(form, mode, case, buf, view, ref, S, K, names=()):
    """The buffer against the dense float64 reference (NaN: not stored) at the bound; guards and unstored elements
    must still hold the pattern."""
    torch.cuda.synchronize()
    dt = view.dtype
    raw = buf.cpu()
    pat = PAT[dt][1]
    assert bool((raw[:GUARD] == pat).all()) and bool((raw[-GUARD:] == pat).all()), f"{form}: wrote outside the buffer"
    ref, S = ref.reshape(-1), S.reshape(-1)
    live = ~torch.isnan(ref)
    assert bool((raw[GUARD:-GUARD][~live] == pat).all()), f"{form}: wrote an element the store mode does not own"
    got = view.cpu().double()[live]
    r, i = R.ratio(got, ref[live], R.bound(S[live], ref[live], K, out_bf16=dt == BF))
    print(f"RATIO {form:24s} {mode:10s} {str(case):34s} {r:.4f} (live index {i}) {' | '.join(names)}")
    assert r <= 1.0, (form, mode, case, r, i)


def gpack(w, kind, N, K, dt):
    m = H.wmap(kind, N, K, (1, N, N), (1, K, K))
    shape, _ = R.pack_index(kind, N, K)
    dst = torch.full(shape, float("nan"), device=dev, dtype=dt)
    H.pack_weight(w.to(dev), dst, m)
    return dst


# ---- the generic path: kair_operand.im_dil --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", D.DILS)
@pytest.mark.parametrize("case", D.GEMM_CASES)
def test_gemm_nt_forward(case, d, mode):
    B, Hh, Ww, C, N = case
    comp, adt, odt = MODES[mode]
    f = D.form(case, d)
    M, K = f["M"], 9 * C
    Wp = gpack(f["w"], 1, N, C, wdt(mode))
    x, bias = f["x"].to(dev, adt), f["bias"].to(dev)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(x, Hh, Ww, C, dil=d), H.rows(Wp),
                                    H.epilogue(out.view(M, N), bias=bias, act=H.ACT_RELU), M, N, K, comp))
    check("dil_nt_forward", mode, (case, d), buf, out, *f["relu"], K, names)
    if d == 1:   # dil = 1 is the call without the argument, bit for bit
        buf2, out2 = poisoned(M * N, odt)
        H.gemm_nt(H.im2col(x, Hh, Ww, C), H.rows(Wp), H.epilogue(out2.view(M, N), bias=bias, act=H.ACT_RELU), M, N, K, comp)
        torch.cuda.synchronize()
        assert torch.equal(buf, buf2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", D.DILS)
@pytest.mark.parametrize("case", D.GEMM_CASES)
def test_gemm_nt_flipped(case, d, mode):
    """The input gradient: the output-gradient rows gy (C channels) through im_flip and the kind-2 pack of wd (N -> C)."""
    B, Hh, Ww, C, N = case
    comp, adt, odt = MODES[mode]
    f = D.form(case, d)
    M, K = f["M"], 9 * C
    Wd = gpack(f["wd"], 2, C, N, wdt(mode))     # [N][9 C]: rows = the conv's input channels
    gy = f["gy"].to(dev, adt)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(gy, Hh, Ww, C, flip=True, dil=d), H.rows(Wd), H.epilogue(out.view(M, N)),
                                    M, N, K, comp))
    check("dil_nt_flipped", mode, (case, d), buf, out, *f["dgrad"], K, names)
    if d == 1:
        buf2, out2 = poisoned(M * N, odt)
        H.gemm_nt(H.im2col(gy, Hh, Ww, C, flip=True), H.rows(Wd), H.epilogue(out2.view(M, N)), M, N, K, comp)
        torch.cuda.synchronize()
        assert torch.equal(buf, buf2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", D.DILS)
@pytest.mark.parametrize("case", D.GEMM_CASES)
def test_gemm_tn_wgrad(case, d, mode):
    """conv_wgrad's roles: A = the output-gradient rows, B = the im2col of the layer's input; finalize kind 1."""
    B, Hh, Ww, C, N = case
    comp, adt, _ = MODES[mode]
    f = D.form(case, d)
    M, K = f["M"], 9 * C
    dy, x = f["dy"].to(dev, adt), f["x"].to(dev, adt)
    splits = H.wgrad_splits(M, N, K)

    def run(op):
        ws = torch.full((splits * N * K,), float("nan"), device=dev)
        names = timed(lambda: H.gemm_tn(H.rows(dy), op, ws, splits, M, N, K, comp))
        buf, grad = poisoned(N * K, F32)
        H.wgrad_finalize(ws, splits, H.wmap(1, N, C), grad.view(N, C, 3, 3))
        return buf, grad, names
    buf, grad, names = run(H.im2col(x, Hh, Ww, C, dil=d))
    check("dil_tn_wgrad", mode, (case, d), buf, grad, *f["wgrad"], M + splits, names)
    if d == 1:
        buf2, _, _ = run(H.im2col(x, Hh, Ww, C))
        torch.cuda.synchronize()
        assert torch.equal(buf, buf2)


# ---- kair_conv3x3_dil -------------------------------------------------------------------------------------------------
# (B, H, W): an image smaller than one 8 x 16 tile plus halo (d = 4 taps leave both edges; a batch-neighbour leak would
# show); ragged in both directions; 3 x 3 tiles per image, two images
DIL_SHAPES = [(2, 8, 8), (1, 13, 19), (2, 17, 33)]
LDX, LDO = 72, 80


def fpack(w, kind):
    """Pack kind 15 (forward, hi / lo halves) or 16 (input-gradient form) of a 64 -> 64 conv weight, bf16."""
    dst = torch.full((64 * 9 * 64 * (2 if kind == 15 else 1),), float("nan"), device=dev, dtype=BF)
    H.pack_weight(w.to(dev), dst, H.wmap(kind, 64, 64, (1, 64, 64), (1, 64, 64)))
    return dst


def wide(rows, ld):
    """bf16 rows [M, 64] inside rows of stride ld, the pad columns NaN (never read)."""
    out = torch.full((rows.shape[0], ld), float("nan"), dtype=BF)
    out[:, :64] = rows.to(BF)
    return out.to(dev)


def scattered(v, S, M):
    off, ok = R.rows_offsets(M, 64, LDO)
    return R.scatter(v, off, ok, M * LDO), R.scatter(S, off, ok, M * LDO)


@pytest.mark.parametrize("odt", [BF, F32], ids=["bf16out", "f32out"])
@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("shape", DIL_SHAPES)
def test_conv3x3_dil_forward(shape, d, odt):
    """Bias + ReLU, rows of stride 72 in, stride 80 out: the 16 pad columns keep the pattern.  The grid is one workgroup
    per tile (not persistent), so no workgroup runs a second tile; the third shape spans 3 x 3 tiles per image."""
    B, Hh, Ww = shape
    f = D.form((B, Hh, Ww, 64, 64), d)
    M = f["M"]
    x, bias, Wf = wide(f["x"], LDX), f["bias"].to(dev), fpack(f["w"], 15)
    buf, out = poisoned(M * LDO, odt)
    names = timed(lambda: H.conv3x3_dil(x, LDX, d, False, Wf, 15, bias, out, B, Hh, Ww, 64, 64, ldo=LDO, act=H.ACT_RELU))
    assert len(names) == 1 and "conv3x3_dil_kernel" in names[0], names
    check("conv3x3_dil_fwd", str(odt)[6:], (shape, d), buf, out, *scattered(*f["relu"], M), 9 * 64, names)


@pytest.mark.parametrize("odt", [BF, F32], ids=["bf16out", "f32out"])
@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("shape", DIL_SHAPES)
def test_conv3x3_dil_dgrad(shape, d, odt):
    """The input gradient: flipped taps over the output-gradient rows, pack kind 16, no bias, no activation."""
    B, Hh, Ww = shape
    f = D.form((B, Hh, Ww, 64, 64), d)
    M = f["M"]
    gy, Wd = wide(f["gy"], LDX), fpack(f["wd"], 16)
    buf, out = poisoned(M * LDO, odt)
    names = timed(lambda: H.conv3x3_dil(gy, LDX, d, True, Wd, 16, None, out, B, Hh, Ww, 64, 64, ldo=LDO))
    assert len(names) == 1 and "conv3x3_dil_kernel" in names[0], names
    check("conv3x3_dil_dgrad", str(odt)[6:], (shape, d), buf, out, *scattered(*f["dgrad"], M), 9 * 64, names)


@pytest.mark.parametrize("geom", [(2, 32, 64), (2, 64, 48), (1, 64, 64), (5, 64, 64)], ids=str)
def test_conv3x3_dil_outside_the_contract(geom):
    """C = 32, N = 48, dilation 1 or 5: KAIR_ERR_ARG naming the geometry, nothing written.  (The engine routes such a
    layer to the generic path: tests/test_ircnn_gpu.py runs nc = 32.)"""
    d, C, N = geom
    x, w = torch.zeros(64, 64, device=dev, dtype=BF), torch.zeros(64 * 18 * 64, device=dev, dtype=BF)
    buf, out = poisoned(64 * 64, F32)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        H.conv3x3_dil(x, 64, d, False, w, 15, None, out, 1, 8, 8, C, N, ldo=64)
    torch.cuda.synchronize()
    assert bool((buf == PAT[F32][1]).all())
