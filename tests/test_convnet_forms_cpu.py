"""tests/convnet_forms_ref.py against torch's float64 functional ops, on the shapes of tests/test_convnet_forms_gpu.py:
the reference the kernels are compared with is shown right here, without a GPU, before any kernel meets it.

Every form is pinned (PIN: relative 1e-12 in float64) to F.interpolate(nearest) + F.conv2d, F.conv2d(stride=2),
F.conv_transpose2d(stride=2), F.pixel_shuffle, F.pixel_unshuffle and to autograd for every gradient.  Then one seeded
fault per form is applied to the REFERENCE (no kernel is touched): the ratio max |faulted - ref| / bound must leave 1
by a wide margin (FAULT_MARGIN) and its argmax must be a faulted element -- the derived bound has teeth."""
import pytest
import torch

import convnet_forms_ref as R

F = torch.nn.functional
PIN = 1e-12
FAULT_MARGIN = 16.0


def close(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item() < PIN


def fault(name, faulted, ref, S, K, mask):
    """The faulted reference against the true one at the bound of an fp32 output: far outside, worst at the fault."""
    bnd = R.bound(S, ref, K)
    assert R.ratio(ref, ref, bnd)[0] == 0.0
    r, i = R.ratio(faulted, ref, bnd)
    print(f"fault {name}: ratio {r:.3g} at flat index {i}")
    assert r > FAULT_MARGIN, (name, r)
    assert bool(mask.reshape(-1)[i]), (name, i)


# ---- a / b. nearest x2 conv and its gradients ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.UP2_CASES)
def test_up2_forms(case):
    B, h, w, C, N, ld = case
    d = R.form_up2(case)
    M, K = d["M"], d["K"]
    x = R.to_nchw(d["src"], B, h, w, C).requires_grad_(True)
    wt = d["wt"].double().requires_grad_(True)
    bias = d["bias"].double().requires_grad_(True)
    pre = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1)
    out = F.leaky_relu(pre, 0.2)
    assert close(d["fwd"][0], R.to_rows(out))
    pre.backward(R.to_nchw(d["dy"], B, 2 * h, 2 * w))
    assert close(d["wgrad"][0], wt.grad) and close(d["bgrad"][0], bias.grad)
    assert close(d["wgrad_acc"][0], wt.grad + d["grad0"].double())

    ref, S = d["fwd"]
    Hc, Wc = 2 * h, 2 * w
    # one border tap shifted: pixel (0, Wc - 1) of the LAST image reads tap (0, +1) from the next row's first pixel
    A = d["A"].clone()
    m = (B - 1) * Hc * Wc + Wc - 1
    A[m, 5 * C:6 * C] = d["src"].double()[(B - 1) * h * w + (1 // 2) * w + 0, :C] + 1.0
    bad = R.nt_ref(A, R.pack(d["wt"], 1), d["bias"], R.ACT_LEAKY, 0.2)[0]
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[m] = True
    fault("up2 border tap", bad, ref, S, K, mask)
    if B > 1:   # the second image's base offset taken from the upsampled size (4 h w, wrapped into the buffer)
        A2 = R.im2col3(torch.roll(d["src"], -(3 * h * w) % (B * h * w), 0), B, Hc, Wc, C, up=2)
        A = d["A"].clone()
        A[Hc * Wc:] = A2[Hc * Wc:]
        bad = R.nt_ref(A, R.pack(d["wt"], 1), d["bias"], R.ACT_LEAKY, 0.2)[0]
        mask = torch.zeros(M, N, dtype=torch.bool)
        mask[Hc * Wc:] = True
        fault("up2 second image base", bad, ref, S, K, mask)
    # weight gradient: the last row of the last split left out
    ref, S = d["wgrad"]
    Gp = R.tn_ref(d["dy"][:-1], d["A"][:-1])[0]
    fault("up2 wgrad last row", R.unpack(Gp, 1, N, C), ref, S, M + 1, torch.ones_like(ref, dtype=torch.bool))
    # bias gradient: the first row of the second 64-row block left out
    ref, S = d["bgrad"]
    bad = ref - d["dy"].double()[min(64, M - 1)]
    fault("up2 bias gradient row", bad, ref, S, M + 1, torch.ones(N, dtype=torch.bool))


# ---- c. space-to-depth forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.S2D_CASES)
def test_s2d_forms(case):
    B, Hn, Wn, C, N, ld = case
    d = R.form_s2d(case)
    M = d["M"]
    wt = d["wt"].double()
    x = R.to_nchw(d["x"], B, 2 * Hn, 2 * Wn, C)
    t = R.to_nchw(d["t"], B, Hn, Wn)
    off, ok = R.pshuf_offsets(M, 4 * C, Hn, Wn, 2, C)
    up = R.scatter(d["pshuf"][0], off, ok, 4 * M * C).reshape(4 * M, C)

    # read as Conv2d(C, N, 2, stride 2): forward, weight gradient and input gradient
    xc, wc = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xc, wc, stride=2)
    assert close(d["fwd"][0], R.to_rows(y))
    y.backward(t)
    assert close(d["wgrad"][0], wc.grad)
    assert close(up, R.to_rows(xc.grad))
    # read as ConvTranspose2d(N, C, 2, stride 2): forward, weight gradient and input gradient
    tc, wc = t.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    z = F.conv_transpose2d(tc, wc, stride=2)
    assert close(up, R.to_rows(z))
    assert close(up, R.to_rows(F.pixel_shuffle(R.to_nchw(d["pshuf"][0], B, Hn, Wn), 2)))
    z.backward(x)
    assert close(d["wgrad"][0], wc.grad)
    assert close(d["fwd"][0], R.to_rows(tc.grad))

    # forward: the last row of the last image reads sub-pixel (j, i) for (i, j)
    ref, S = d["fwd"]
    A = d["A"].clone()
    A[M - 1, C:2 * C], A[M - 1, 2 * C:3 * C] = d["A"][M - 1, 2 * C:3 * C], d["A"][M - 1, C:2 * C]
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[M - 1] = True
    fault("s2d sub-pixel order", R.nt_ref(A, R.pack(d["wt"], 7))[0], ref, S, 4 * C, mask)
    # weight gradient: taps (0, 1) and (1, 0) of one input channel exchanged by the finalize
    ref, S = d["wgrad"]
    bad = ref.clone()
    bad[:, C - 1, 0, 1], bad[:, C - 1, 1, 0] = ref[:, C - 1, 1, 0], ref[:, C - 1, 0, 1]
    mask = torch.zeros_like(ref, dtype=torch.bool)
    mask[:, C - 1] = True
    fault("s2d wgrad tap order", bad, ref, S, M + 1, mask)
    # pixel shuffle: the first pixel of the last image stores sub-pixel (1, 0) where (0, 1) belongs, channel 0
    ref, S = d["pshuf"]
    m = (B - 1) * Hn * Wn
    bad = ref.clone()
    bad[m, 1], bad[m, 2] = ref[m, 2], ref[m, 1]
    mask = torch.zeros_like(ref, dtype=torch.bool)
    mask[m, 1:3] = True
    fault("pshuf sub-pixel order", bad, ref, S, N, mask)


# ---- packs: the index formulas ---------------------------------------------------------------------------------------------
def test_pack_formulas():
    """The four packs with pads against a second, loop-written statement of the header's text; unpack inverts pack."""
    g = R.gen(7)
    N, K, Np, Kp = 5, 3, 8, 4
    for kind, taps in ((1, 9), (2, 9), (7, 4), (8, 4)):
        s = 3 if taps == 9 else 2
        w = torch.randn(N, K, s, s, generator=g, dtype=torch.float64)
        got = R.pack(w, kind, Np, Kp)
        exp = torch.zeros_like(got)
        for n in range(N):
            for k in range(K):
                for tap in range(taps):
                    v = w[n, k, tap // s, tap % s]
                    if kind in (1, 7):
                        exp[n, tap * Kp + k] = v
                    elif kind == 2:
                        exp[k, tap * Np + n] = v
                    else:
                        exp[k * 4 + tap, n] = v
        assert torch.equal(got, exp), kind
        assert int((got != 0).sum()) == w.numel()
        if kind in (1, 7):
            assert torch.equal(R.unpack(got, kind, N, K, Np, Kp), w)


# ---- d. residual-block forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RB_CASES)
def test_rb_forms(case):
    B, H, W, Cin, N = case
    d = R.form_rb(case)
    M, K = d["M"], 9 * Cin
    x = R.to_nchw(d["x"], B, H, W)
    conv = F.conv2d(x, d["wt"].double(), None, padding=1)
    assert close(d["relu"][0], R.to_rows(F.relu(conv + d["bias"].double().view(1, N, 1, 1))))
    assert close(d["res"][0], R.to_rows(conv) + d["resid"].double()[:, :N] + d["resid2"].double()[:, :N])
    # the gated input gradient through autograd: h = ReLU(u) stored; dL/du = conv(h, wd)'s input gradient * ReLU'(u)
    gate = d["gate"].double()[:, :N]
    u = torch.where(gate > 0, gate, -torch.ones_like(gate))          # any pre-activation with ReLU(u) = the gate
    u = R.to_nchw(u, B, H, W).requires_grad_(True)
    hgate = F.relu(u)
    assert torch.equal(R.to_rows(hgate.detach()), gate.abs())          # (|.|: the stored -0.0 equals 0)
    F.conv2d(hgate, d["wd"].double(), None, padding=1).backward(R.to_nchw(d["gy"], B, H, W))
    assert close(d["dgrad"][0], R.to_rows(u.grad))
    assert bool((gate == 0).any()) and bool(torch.signbit(d["gate"][:, :N][gate == 0]).any())

    # the tail chunk's bias dropped in the last row (columns from the last multiple of 8 on)
    ref, S = d["relu"]
    n0 = (N - 1) // 8 * 8
    bias = d["bias"].clone()
    bias[n0:] = 0
    A = R.im2col3(d["x"], B, H, W, Cin)
    bad = ref.clone()
    bad[M - 1] = R.nt_ref(A[M - 1:], R.pack(d["wt"], 1), bias, R.ACT_RELU)[0][0]
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[M - 1, n0:] = True
    fault("relu tail-chunk bias", bad, ref, S, K, mask)
    # resid2 left off the last row
    ref, S = d["res"]
    bad = ref.clone()
    bad[M - 1] -= d["resid2"].double()[M - 1, :N]
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[M - 1] = True
    fault("resid2 last row", bad, ref, S, K, mask)
    # resid2 read with resid's row stride
    r2 = d["resid2"].reshape(-1)[:M * (N + 4)].reshape(M, N + 4)
    bad = R.nt_ref(A, R.pack(d["wt"], 1), resid=d["resid"][:, :N], resid2=r2[:, :N])[0]
    mask = torch.ones(M, N, dtype=torch.bool)
    mask[0] = False
    fault("resid2 row stride", bad, ref, S, K, mask)
    # ReLU' taken as 1 at a gate of exactly 0
    ref, S = d["dgrad"]
    Ag = R.im2col3(d["gy"], B, H, W, Cin, flip=True)
    bad = R.nt_ref(Ag, R.pack(d["wd"], 2), gate=(gate >= 0).double(), gate_kind=4)[0]
    fault("relu' at gate 0", bad, ref, S, 9 * Cin, gate == 0)
    # the taps not negated (im_flip dropped)
    bad = R.nt_ref(R.im2col3(d["gy"], B, H, W, Cin), R.pack(d["wd"], 2), gate=gate, gate_kind=3)[0]
    fault("dgrad tap flip", bad, ref, S, 9 * Cin, gate > 0)


# ---- e. image tails ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TAIL_CASES)
def test_tail_forms(case):
    store, img_C, r, Np, with_mean, rng, with_resid = case
    B, H, W = R.TAIL_GRID
    d = R.form_tail(case)
    conv = F.conv2d(R.to_nchw(d["x"], B, H, W), d["wt"].double(), d["bias"].double(), padding=1)
    raw = conv[:, :img_C] if store == "nchw" else F.pixel_shuffle(conv[:, :img_C * r * r], r)
    rest = torch.zeros_like(raw)
    if with_mean:
        rest = rest + d["mean"].double().view(1, img_C, 1, 1)
    if with_resid:
        rest = rest + d["resid"].double()
    img = raw / rng + rest
    ref, S = d["img"]
    assert not bool(torch.isnan(ref).any()) and ref.numel() == img.numel()
    assert close(ref, img.reshape(-1))

    # the second image's base offset taken from the packed column count: its first pixel lands elsewhere
    M = d["M"]
    off, ok = (R.nchw_offsets(M, Np, H, W, img_C) if store == "nchw" else R.pshuf_nchw_offsets(M, Np, H, W, r, img_C))
    v = ref[off.clamp(max=ref.numel() - 1)]
    m = H * W                                    # first pixel of the second image
    bad = ref.clone()
    shift = (Np - img_C) * H * W * r * r         # (b Np + c) instead of (b img_C + c), taken modulo the image
    mask = torch.zeros_like(ref, dtype=torch.bool)
    for n in range(Np):
        if ok[m, n]:
            o = (int(off[m, n]) + shift) % ref.numel()
            bad[o] = v[m, n] + 1.0
            mask[o] = True
    fault(f"{store} second image base", bad, ref, S, 9 * R.TAIL_C, mask)
    # 1 / img_range not applied
    if rng != 1.0:
        bad = (raw + rest).reshape(-1)
        fault(f"{store} range order", bad, ref, S, 9 * R.TAIL_C, torch.ones_like(ref, dtype=torch.bool))


@pytest.mark.parametrize("case", R.PUNSHUF_CASES)
def test_punshuf_forms(case):
    N, ldo, ldg, gated = case
    B, H, W = R.TAIL_GRID
    d = R.form_punshuf(case)
    conv = F.conv2d(R.to_nchw(d["x"], B, 2 * H, 2 * W), d["wt"].double(), None, padding=1)
    un = F.pixel_unshuffle(conv, 2)                              # [B, 4 N, H, W]
    if gated:
        gimg = R.to_nchw(d["gate"], B, H, W, 4 * N)
        un = un * torch.where(gimg > 0, torch.ones_like(gimg), torch.full_like(gimg, 0.2))
    ref, S = d["out"]
    rows = ref.reshape(B * H * W, ldo)
    assert close(rows[:, :4 * N], R.to_rows(un)) and bool(torch.isnan(rows[:, 4 * N:]).all())
    # the gate addressed with the output's row stride
    if gated:
        M = d["M"]
        goff, _ = R.punshuf_offsets(M, N, H, W, 2, ldo)
        f = R.gate_factor(d["gate"].reshape(-1)[goff], 2, 0.2)
        v = R.nt_ref(R.im2col3(d["x"], B, 2 * H, 2 * W, R.TAIL_C), R.pack(d["wt"], 1))[0] * f
        off, ok = R.punshuf_offsets(M, N, H, W, 2, ldo)
        bad = R.scatter(v, off, ok, ref.numel())
        live = ~torch.isnan(ref)
        fault("punshuf gate stride", bad[live], ref[live], S[live], 9 * R.TAIL_C, torch.ones(int(live.sum()), dtype=torch.bool))
    else:   # sub-pixel (i, j) stored as (j, i) for the last pixel row of the image
        bad = rows.clone()
        bad[-1, 1:4 * N:4], bad[-1, 2:4 * N:4] = rows[-1, 2:4 * N:4], rows[-1, 1:4 * N:4]
        live = ~torch.isnan(ref)
        mask = torch.zeros_like(rows, dtype=torch.bool)
        mask[-1, :4 * N] = True
        fault("punshuf sub-pixel order", bad.reshape(-1)[live], ref[live], S[live], 9 * R.TAIL_C, mask.reshape(-1)[live])


# ---- gates and activations ----------------------------------------------------------------------------------------------
def test_gates_and_activations():
    g = R.gen(11)
    x = torch.randn(4000, generator=g, dtype=torch.float64)
    x[::9] = 0.0
    x[::18] = -0.0
    for kind, fn in ((R.ACT_GELU, F.gelu), (R.ACT_LEAKY, lambda t: F.leaky_relu(t, 0.2)), (R.ACT_RELU, F.relu)):
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        assert close(R.act(x, kind, 0.2), y)
        y.sum().backward()
        assert close(R.gate_factor(x, {R.ACT_GELU: 1, R.ACT_LEAKY: 2, R.ACT_RELU: 3}[kind], 0.2), xr.grad), kind
    assert torch.equal(R.gate_factor(x, 4), x)
    # the two derivative gates read the STORED activation: its sign is the pre-activation's
    for kind, fn in ((2, lambda t: F.leaky_relu(t, 0.2)), (3, F.relu)):
        assert torch.equal(R.gate_factor(fn(x), kind, 0.2), R.gate_factor(x, kind, 0.2))
    assert float(R.gate_factor(torch.tensor([0.0, -0.0]), 3).abs().sum()) == 0.0
    assert torch.equal(R.gate_factor(torch.tensor([0.0, -0.0]), 2, 0.2), torch.tensor([0.2, 0.2], dtype=torch.float64))


# ---- f. the fp32-A cast ----------------------------------------------------------------------------------------------------
def test_cast_fault():
    """An fp32 A that is not bf16-exact enters bf16 compute rounded to nearest-even; a truncating cast is far outside
    the bound (the check test_convnet_forms_gpu.py::test_f32_a_cast relies on)."""
    g = R.gen(13)
    M, K, N = 120, 64, 24
    A = torch.randn(M, K, generator=g)
    Bw = R.randn(g, N, K, scale=0.2)
    ref, S = R.nt_ref(A.bfloat16(), Bw)
    trunc = (A.view(torch.int32) & -65536).view(torch.float32)
    assert bool((trunc != A.bfloat16().float()).any())
    fault("truncating cast", R.nt_ref(trunc, Bw)[0], ref, S, K, torch.ones(M, N, dtype=torch.bool))


def test_bound_and_ratio():
    ref, S = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64), torch.tensor([4.0, 4.0, 0.0], dtype=torch.float64)
    b32, b16 = R.bound(S, ref, 60), R.bound(S, ref, 60, out_bf16=True)
    assert b32[0].item() == 2 * 64 * 2.0 ** -24 * 4 + 2.0 ** -24 and b16[1].item() == 2 * 64 * 2.0 ** -24 * 4 + 2.0 ** -7
    assert b32[2].item() == 0.0
    assert R.ratio(ref.float(), ref, b32) == (0.0, 0)
    r, i = R.ratio(ref + torch.tensor([0.0, 0.0, 1e-30]), ref, b32)
    assert r == float("inf") and i == 2                       # a zero bound admits only the exact value
    r, i = R.ratio(torch.tensor([1.0, float("nan"), 0.0]), ref, b32)
    assert r != r and i == 1                                  # an unwritten (NaN) element can not pass
    r, i = R.ratio(ref + 0.5 * b32, ref, b32)
    assert 0.49 < r < 0.51
