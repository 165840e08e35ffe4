"""The kair_gemm_nt / kair_gemm_tn forms that only the conv networks reach (DnCNN, FDnCNN, FFDNet, RRDBNet, DRUNet,
USRNet and SwinIR's conv tails), each kernel against the float64 statements of tests/convnet_forms_ref.py
(pinned to torch's functional ops by tests/test_convnet_forms_cpu.py), elementwise, at that module's derived bound

    |got - ref| <= 2 (K + 4) 2^-24 S + r_out        (K -> M + splits for the weight gradients)

Every input is bf16-exact, so one reference serves fp32 compute ("f32"), bf16 compute with bf16 operands and outputs
("bf16") and bf16 compute with fp32 operands and outputs ("bf16_f32A").  Each check prints max |got - ref| / bound
and asserts it <= 1; outputs live inside pattern-filled allocations, so an element the form must not write -- a pad
channel, a column at or above img_C, a float past the image -- has to keep its pattern, and one it must write fails
the bound if it kept it.  (g): kair_gemm_nt rejects every optional epilogue field its store mode does not read."""
import ctypes
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import convnet_forms_ref as R  # noqa: E402
from kair_amd import _hip as H  # noqa: E402

dev = torch.device("cuda")
F32, BF = torch.float32, torch.bfloat16
MODES = {"f32": (H.F32, F32, F32), "bf16": (H.BF16, BF, BF), "bf16_f32A": (H.BF16, F32, F32)}   # compute, operands, out
PAT = {F32: (torch.int32, 0x5A5AA5A5), BF: (torch.int16, 0x5A5A)}
GUARD = 64
WORST = {}


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
    WORST[(form, mode)] = max(WORST.get((form, mode), 0.0), r if r == r else float("inf"))
    print(f"RATIO {form:24s} {mode:10s} {str(case):34s} {r:.4f} (live index {i}) {' | '.join(names)}")
    assert r <= 1.0, (form, mode, case, r, i)


def gpack(w, kind, N, K, dt, Np=None, Kp=None):
    m = H.wmap(kind, N, K, (1, N, Np or N), (1, K, Kp or K))
    shape, _ = R.pack_index(kind, N, K, Np, Kp)
    dst = torch.full(shape, float("nan"), device=dev, dtype=dt)
    H.pack_weight(w.to(dev), dst, m)
    return dst


def dense(v, S):
    return v.reshape(-1), S.reshape(-1)


# ---- a. nearest-x2 conv forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.UP2_CASES)
def test_up2_forward(case, mode):
    B, h, w, C, N, ld = case
    comp, adt, odt = MODES[mode]
    d = R.form_up2(case)
    M, K = d["M"], d["K"]
    Wp = gpack(d["wt"], 1, N, C, wdt(mode))
    src, bias = d["src"].to(dev, adt), d["bias"].to(dev)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(src, 2 * h, 2 * w, C, ld=ld, up=2), H.rows(Wp),
                                    H.epilogue(out.view(M, N), bias=bias, act=H.ACT_LEAKY, slope=0.2), M, N, K, comp))
    check("up2_forward", mode, case, buf, out, *dense(*d["fwd"]), K, names)


# ---- b. its weight gradient ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.UP2_CASES)
def test_up2_wgrad(case, mode):
    """N = 24 / 64 / 32 against K = 144 / 576 / 576: the 32 x 160, 64 x 128 and 32 x 256 tiles.  Case 0 accumulates
    onto a non-zero gradient, case 2 takes the bias gradient through kair_colsum; 3 splits leave the last one empty."""
    B, h, w, C, N, ld = case
    comp, adt, _ = MODES[mode]
    d = R.form_up2(case)
    M, K = d["M"], d["K"]
    acc = case == R.UP2_CASES[0]
    dy, src = d["dy"].to(dev, adt), d["src"].to(dev, adt)
    for splits in (H.wgrad_splits(M, N, K), 3):
        ws = torch.full((splits * N * K,), float("nan"), device=dev)
        names = timed(lambda: H.gemm_tn(H.rows(dy), H.im2col(src, 2 * h, 2 * w, C, ld=ld, up=2), ws, splits, M, N, K, comp))
        buf, grad = poisoned(N * K, F32)
        if acc:
            grad.copy_(d["grad0"].reshape(-1))
        H.wgrad_finalize(ws, splits, H.wmap(1, N, C), grad.view(N, C, 3, 3), accumulate=acc)
        check("up2_wgrad", mode, (case, splits), buf, grad, *dense(*d["wgrad_acc" if acc else "wgrad"]), M + splits, names)
    if case == R.UP2_CASES[2]:
        nws = H.colsum_ws(N)
        wbuf, cws = poisoned(nws, F32)
        buf, bg = poisoned(N, F32)
        H.colsum(H.rows(dy), M, N, H.wmap(4, N, 0, (1, N, N), (1, 1, 1)), bg, cws)
        check("up2_bias_colsum", mode, case, buf, bg, *d["bgrad"], M + nws // N)
        raw = wbuf.cpu()
        assert bool((raw[:GUARD] == PAT[F32][1]).all()) and bool((raw[-GUARD:] == PAT[F32][1]).all())


# ---- c. space-to-depth --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.S2D_CASES)
def test_s2d_forward(case, mode):
    """The stride-2 conv forward (= the transposed conv's input gradient): NT, A = S2D, kind 7 weights."""
    B, Hn, Wn, C, N, ld = case
    comp, adt, odt = MODES[mode]
    d = R.form_s2d(case)
    M = d["M"]
    Wf = gpack(d["wt"], 7, N, C, wdt(mode))
    x = d["x"].to(dev, adt)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.s2d(x, Hn, Wn, C, ld=ld), H.rows(Wf), H.epilogue(out.view(M, N)), M, N, 4 * C, comp))
    check("s2d_forward", mode, case, buf, out, *dense(*d["fwd"]), 4 * C, names)


@pytest.mark.parametrize("role", ["conv", "convT"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.S2D_CASES)
def test_s2d_wgrad(case, mode, role):
    """Both weight gradients: TN with B = S2D, finalize kind 7.  conv: A is the output gradient; convT: A is the layer's
    input and B its output gradient -- one GEMM form (test_convnet_forms_cpu.py pins the reference to both layers'
    autograd), run here at the default split count and at 2 splits."""
    B, Hn, Wn, C, N, ld = case
    comp, adt, _ = MODES[mode]
    d = R.form_s2d(case)
    M, K = d["M"], 4 * C
    t, x = d["t"].to(dev, adt), d["x"].to(dev, adt)
    splits = H.wgrad_splits(M, N, K) if role == "conv" else 2
    ws = torch.full((splits * N * K,), float("nan"), device=dev)
    names = timed(lambda: H.gemm_tn(H.rows(t), H.s2d(x, Hn, Wn, C, ld=ld), ws, splits, M, N, K, comp))
    buf, grad = poisoned(N * K, F32)
    H.wgrad_finalize(ws, splits, H.wmap(7, N, C), grad.view(N, C, 2, 2))
    check("s2d_wgrad_" + role, mode, case, buf, grad, *dense(*d["wgrad"]), M + splits, names)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.S2D_CASES)
def test_s2d_pixelshuffle(case, mode):
    """The transposed conv's forward (= the stride-2 conv's input gradient): ROWS A, kind 8 weights, OUT_PSHUF r = 2
    into pixel rows of stride ld; the channels at and above C keep the pattern."""
    B, Hn, Wn, C, N, ld = case
    comp, adt, odt = MODES[mode]
    d = R.form_s2d(case)
    M = d["M"]
    Wd = gpack(d["wt"], 8, N, C, wdt(mode))
    t = d["t"].to(dev, adt)
    buf, out = poisoned(4 * M * ld, odt)
    names = timed(lambda: H.gemm_nt(H.rows(t), H.rows(Wd),
                                    H.epilogue(out.view(4 * M, ld), mode=H.OUT_PSHUF, ldo=ld, ps=(2, Hn, Wn)), M, 4 * C, N, comp))
    off, ok = R.pshuf_offsets(M, 4 * C, Hn, Wn, 2, ld)
    v, S = d["pshuf"]
    check("s2d_pixelshuffle", mode, case, buf, out, R.scatter(v, off, ok, 4 * M * ld), R.scatter(S, off, ok, 4 * M * ld), N, names)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("kind", [1, 2, 7, 8])
def test_packs_bit_for_bit(kind, dt):
    """A pack is a permutation plus a cast: bit for bit the index formula, pad entries exactly +0, and the single
    kair_pack_weight call and the PackTable launch agree.  Unpadded (an S2D / RB case) and padded (24 x 8 in 32 x 16)."""
    g = R.gen(50 + kind)
    s = 3 if kind in (1, 2) else 2
    for N, K, Np, Kp in ((32, 16, 32, 16), (24, 8, 32, 16), (20, 24, 20, 24)):
        w = torch.randn(N, K, s, s, generator=g)
        exp = R.pack(w, kind, Np, Kp, dtype=dt)
        assert int((exp != 0).sum()) <= w.numel()
        one = gpack(w, kind, N, K, dt, Np, Kp)
        tab = torch.full_like(one, float("nan"))
        wd = w.to(dev)
        H.PackTable([(wd, tab, H.wmap(kind, N, K, (1, N, Np), (1, K, Kp)))]).run()
        torch.cuda.synchronize()
        assert torch.equal(_bits(one.cpu()), _bits(exp)), (kind, dt, N, K, Np, Kp)
        assert torch.equal(_bits(tab.cpu()), _bits(exp)), (kind, dt, N, K, Np, Kp)


# ---- d. residual-block forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.RB_CASES)
def test_rb_relu_conv(case, mode):
    B, Hh, Ww, Cin, N = case
    comp, adt, odt = MODES[mode]
    d = R.form_rb(case)
    M, K = d["M"], 9 * Cin
    Wp = gpack(d["wt"], 1, N, Cin, wdt(mode))
    x, bias = d["x"].to(dev, adt), d["bias"].to(dev)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(x, Hh, Ww, Cin), H.rows(Wp), H.epilogue(out.view(M, N), bias=bias, act=H.ACT_RELU),
                                    M, N, K, comp))
    check("rb_relu_conv", mode, case, buf, out, *dense(*d["relu"]), K, names)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.RB_CASES)
def test_rb_two_residuals(case, mode):
    """out (row stride N) = conv + resid (row stride N + 4) + resid2 (row stride N + 12)."""
    B, Hh, Ww, Cin, N = case
    comp, adt, odt = MODES[mode]
    d = R.form_rb(case)
    M, K = d["M"], 9 * Cin
    Wp = gpack(d["wt"], 1, N, Cin, wdt(mode))
    x, r1, r2 = d["x"].to(dev, adt), d["resid"].to(dev), d["resid2"].to(dev)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(x, Hh, Ww, Cin), H.rows(Wp),
                                    H.epilogue(out.view(M, N), resid=r1, ldr=N + 4, resid2=r2, ldr2=N + 12), M, N, K, comp))
    check("rb_two_residuals", mode, case, buf, out, *dense(*d["res"]), K, names)


@pytest.mark.parametrize("gdt", [BF, F32])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.RB_CASES)
def test_rb_gated_dgrad(case, mode, gdt):
    """The flipped-tap input gradient times ReLU'(gate), gate_kind 3: the gate is a stored post-ReLU activation (row
    stride N + 8) with exact zeros of both signs, where the derivative is 0."""
    B, Hh, Ww, Cin, N = case
    comp, adt, odt = MODES[mode]
    d = R.form_rb(case)
    M, K = d["M"], 9 * Cin
    Wd = gpack(d["wd"], 2, Cin, N, wdt(mode))
    gy, gate = d["gy"].to(dev, adt), d["gate"].to(dev, gdt)
    buf, out = poisoned(M * N, odt)
    names = timed(lambda: H.gemm_nt(H.im2col(gy, Hh, Ww, Cin, flip=True), H.rows(Wd),
                                    H.epilogue(out.view(M, N), gate=gate, ldg=N + 8, gate_kind=3), M, N, K, comp))
    check("rb_gated_dgrad", mode, (case, str(gdt)[6:]), buf, out, *dense(*d["dgrad"]), K, names)


# ---- e. image tails -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.TAIL_CASES)
def test_image_tails(case, mode):
    """OUT_NCHW (img_C 1 and 3 inside 16 packed columns, mean set and null, img_range 255, the NCHW resid image) and
    OUT_PSHUF_NCHW (r = 2: 12 of 16 columns; r = 3: 27 of 32 columns, mean and range): the columns at and above img_C
    carry non-zero values and must not be stored, nor anything past the image."""
    store, img_C, r, Np, with_mean, rng, with_resid = case
    B, Hh, Ww = R.TAIL_GRID
    comp, adt, _ = MODES[mode]
    d = R.form_tail(case)
    M, K = d["M"], 9 * R.TAIL_C
    Wp = gpack(d["wt"], 1, Np, R.TAIL_C, wdt(mode))
    x, bias = d["x"].to(dev, adt), d["bias"].to(dev)
    mean = d["mean"].to(dev) if with_mean else None
    resid = d["resid"].to(dev) if with_resid else None
    n = B * img_C * Hh * r * Ww * r
    buf, out = poisoned(n, F32)
    if store == "nchw":
        E = H.epilogue(out, mode=H.OUT_NCHW, ldo=0, bias=bias, resid=resid, img=(mean, rng, img_C, Hh, Ww))
    else:
        E = H.epilogue(out, mode=H.OUT_PSHUF_NCHW, ldo=0, bias=bias, ps=(r, Hh, Ww), img=(mean, rng, img_C, Hh, Ww))
    names = timed(lambda: H.gemm_nt(H.im2col(x, Hh, Ww, R.TAIL_C), H.rows(Wp), E, M, Np, K, comp))
    check("tail_" + store, mode, case, buf, out, *d["img"], K, names)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.PUNSHUF_CASES)
def test_plain_punshuf(case, mode):
    """OUT_PUNSHUF r = 2 (N = 12: a partial chunk; 48 of 56 row elements stored), plain and times LeakyReLU'(gate)."""
    N, ldo, ldg, gated = case
    B, Hh, Ww = R.TAIL_GRID
    comp, adt, odt = MODES[mode]
    d = R.form_punshuf(case)
    M, K = d["M"], 9 * R.TAIL_C
    Wp = gpack(d["wt"], 1, N, R.TAIL_C, wdt(mode))
    x = d["x"].to(dev, adt)
    gate = d["gate"].to(dev, odt) if gated else None
    rows = B * Hh * Ww
    buf, out = poisoned(rows * ldo, odt)
    E = H.epilogue(out.view(rows, ldo), mode=H.OUT_PUNSHUF, ldo=ldo, ps=(2, Hh, Ww), gate=gate, ldg=ldg,
                   gate_kind=2 if gated else 0, slope=0.2)
    names = timed(lambda: H.gemm_nt(H.im2col(x, 2 * Hh, 2 * Ww, R.TAIL_C), H.rows(Wp), E, M, N, K, comp))
    check("punshuf" + ("_gate" if gated else ""), mode, case, buf, out, *d["out"], K, names)


# ---- f. the fp32-A cast in bf16 compute --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "im2col"])
def test_f32_a_cast(form):
    """An fp32 A that is NOT bf16-exact: the kernel's cast is round-to-nearest-even -- elementwise the reference over
    A.bfloat16() at the bound; a truncating cast is hundreds of bounds away (test_convnet_forms_cpu.py::test_cast_fault)."""
    g = R.gen(13)
    if form == "rows":
        M, K, N = 120, 64, 24
        A = torch.randn(M, K, generator=g)
        Bw = R.randn(g, N, K, scale=0.2)
        op, A64 = H.rows(A.to(dev)), A.bfloat16()
    else:
        B, Hh, Ww, C, N = R.RB_CASES[0]
        M, K = B * Hh * Ww, 9 * C
        A = torch.randn(M, C, generator=g)
        Bw = R.pack(R.randn(g, N, C, 3, 3, scale=0.1), 1, dtype=F32)
        op, A64 = H.im2col(A.to(dev), Hh, Ww, C), R.im2col3(A.bfloat16(), B, Hh, Ww, C)
    assert bool((A.bfloat16().float() != A).any())
    Bd = Bw.to(dev, BF)
    buf, out = poisoned(M * N, F32)
    names = timed(lambda: H.gemm_nt(op, H.rows(Bd), H.epilogue(out.view(M, N)), M, N, K, H.BF16))
    check("f32_a_cast_" + form, "bf16_f32A", (M, N, K), buf, out, *dense(*R.nt_ref(A64, Bw)), K, names)


# ---- g. the epilogue contract ------------------------------------------------------------------------------------------
OUT_MODES = {"ROWS": H.OUT_ROWS, "QKVBLK": H.OUT_QKVBLK, "PSHUF": H.OUT_PSHUF, "PUNSHUF": H.OUT_PUNSHUF, "NCHW": H.OUT_NCHW,
             "PSHUF_NCHW": H.OUT_PSHUF_NCHW, "PSHUF_SPM": H.OUT_PSHUF_SPM, "PUNSHUF_SPM": H.OUT_PUNSHUF_SPM}
NOT_ROWS = [m for m in OUT_MODES if m != "ROWS"]
# (store mode, field, the word kair_last_error() must carry): the (mode, field) pairs epi_chunk does not read --
# the list of the kair_epilogue comment in kair_hip.h and of the checks in kair_gemm_nt
CONTRACT = ([(m, "gate", "gate") for m in ("QKVBLK", "PSHUF", "NCHW", "PSHUF_NCHW", "PSHUF_SPM")] +
            [(m, f"gate_kind{k}", "gate_kind") for m in ("ROWS", "PUNSHUF", "PUNSHUF_SPM") for k in (0, 5)] +
            [(m, "gate_kind1", "gate_kind") for m in ("PUNSHUF", "PUNSHUF_SPM")] +
            [(m, f, f) for m in NOT_ROWS for f in ("resid2", "rowscale", "out_ones_col_p1")] +
            [(m, "window", "win_ws") for m in NOT_ROWS] +
            [(m, "resid", "resid") for m in ("QKVBLK", "PSHUF", "PUNSHUF", "PSHUF_NCHW", "PSHUF_SPM", "PUNSHUF_SPM")] +
            [(m, "out_pre", "out_pre") for m in ("QKVBLK", "PUNSHUF", "NCHW", "PSHUF_NCHW", "PUNSHUF_SPM")])
CM, CN, CK = 32, 16, 16


def _contract_epilogue(mode, out):
    """A valid epilogue of store mode `mode` for a 32 x 16 product (grids of 32 pixels, r = 2)."""
    kw = {"ROWS": dict(ldo=CN), "QKVBLK": dict(ldo=0, qkv=(1, 16, 32)), "PSHUF": dict(ldo=4, ps=(2, 4, 8)),
          "PUNSHUF": dict(ldo=64, ps=(2, 2, 4)), "NCHW": dict(ldo=0, img=(None, 1.0, 3, 4, 8)),
          "PSHUF_NCHW": dict(ldo=0, ps=(2, 4, 8), img=(None, 1.0, 3, 4, 8)), "PSHUF_SPM": dict(ldo=4, ps=(2, 4, 8)),
          "PUNSHUF_SPM": dict(ldo=64, ps=(2, 2, 4))}[mode]
    return H.epilogue(out, mode=OUT_MODES[mode], **kw)


@pytest.mark.parametrize("mode,field,word", CONTRACT, ids=[f"{m}-{f}" for m, f, _ in CONTRACT])
def test_epilogue_contract(mode, field, word):
    """The field set where the store mode does not read it: KAIR_ERR_ARG in every compute mode, the message names the
    field, nothing is launched and the pattern-filled output is bit-identical; the same call without the field runs."""
    g = R.gen(3)
    A, Bw = R.randn(g, CM, CK).to(dev), R.randn(g, CN, CK).to(dev)
    side = torch.ones(4096, device=dev)
    buf, out = poisoned(2048, F32)
    before = buf.clone()
    E = _contract_epilogue(mode, out)
    if mode != "ROWS":   # the control: the mode's own fields alone are accepted and the kernel runs
        H.gemm_nt(H.rows(A), H.rows(Bw), E, CM, CN, CK, H.F32)
        torch.cuda.synchronize()
        assert not torch.equal(buf, before)
        buf.copy_(before)
    if field == "gate" or field.startswith("gate_kind"):
        E.gate, E.gate_dtype, E.ldg = side.data_ptr(), H.F32, 64
        E.gate_kind = int(field[9:]) if field.startswith("gate_kind") else 2
    elif field == "resid2":
        E.resid2, E.ldr2 = side.data_ptr(), 64
    elif field == "rowscale":
        E.rowscale, E.rows_per_scale = side.data_ptr(), 8
    elif field == "out_ones_col_p1":
        E.out_ones_col_p1 = 1
    elif field == "window":
        E.win_H, E.win_W, E.win_ws, E.win_shift = 8, 8, 8, 0
    elif field == "resid":
        E.resid, E.ldr = side.data_ptr(), 64
    elif field == "out_pre":
        E.out_pre, E.pre_dtype, E.ldp = side.data_ptr(), H.F32, 64
    lib = H.lib()
    for comp in (H.F32, H.BF16, H.X3):
        torch.cuda.synchronize()
        H.ktime_begin(4)
        try:
            rc = lib.kair_gemm_nt(ctypes.byref(H.rows(A)), ctypes.byref(H.rows(Bw)), ctypes.byref(E), CM, CN, CK, comp,
                                  H.stream_ptr())
        finally:
            nk = H.ktime_end()
        torch.cuda.synchronize()
        msg = lib.kair_last_error().decode()
        assert rc == -1 and nk == 0, (comp, rc, nk, msg)
        assert re.search(rf"\b{word}\b", msg), (comp, msg)
        assert torch.equal(buf, before) and bool((side == 1).all())


def test_zz_worst_ratios():
    """The worst ratio per form and compute mode of this session's run (printed for the record; asserted above)."""
    for (form, mode), r in sorted(WORST.items()):
        print(f"WORST {form:24s} {mode:10s} {r:.4f}")
    assert all(r <= 1.0 for r in WORST.values())
