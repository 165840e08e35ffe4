"""Window size 7 (49-token windows; the reference's options/swinir/train_swinir_car_jpeg.json and every published
SwinIR JPEG-artifact-reduction checkpoint) on the fp32, fp32x3 and bf16 paths.

The kernels keep their 64-slot tile: the 15 pad slots are zero-filled, take probability exactly 0 and are never
stored, so the padding adds no arithmetic and every bar below is the one the project holds for the same kernel at
window size 8 (tests/test_kernels_gpu.py::test_window_attention_fwd_bwd, tests/test_x3_gpu.py::
test_window_attention_x3, tests/test_swinir_variants_gpu.py, tests/test_inference_gpu.py).  References: float64
autograd of a window-size-general window attention written here, and the CPU oracle (oracle/swinir.py,
oracle/train.py).  The shapes: a non-square 14 x 21 grid (2 x 3 windows, so all 9 shift regions occur), 2 images.

bf16 at window 7 runs the generic attention pair (attn_fwd_kernel<true, 7> / attn_bwd_kernel<true, 7>, head pad 32);
its bars are the bf16 ones of the same tests.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from conftest import state_rel_excluding_kbias  # noqa: E402
from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.network_swinir import SwinIR  # noqa: E402
from kair_amd.utils import utils_model  # noqa: E402
from oracle import swinir as osw  # noqa: E402
from oracle.train import OracleTrainer  # noqa: E402

dev = torch.device("cuda")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def hilo(x, e=0):
    """The fp16 pair planes of x * 2^e: [2, *x.shape]."""
    w = x * 2.0 ** e
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.stack([hi, lo])


def _relidx(ws):
    """relative_position_index of network_swinir.py:94-105 for a ws x ws window: [ws^2, ws^2]."""
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    r = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return r[..., 0] * (2 * ws - 1) + r[..., 1]


def _shift_mask(Hh, Ww, ws, shift):
    """calculate_mask of network_swinir.py:216-237: [nW, ws^2, ws^2], 0 / -100."""
    img = torch.zeros(Hh, Ww)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    mw = img.view(Hh // ws, ws, Ww // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = mw[:, None, :] - mw[:, :, None]
    return torch.where(d != 0, torch.tensor(-100.0), torch.tensor(0.0)).double()


def attn_ref(q, k, v, table, nh, ws, shift, Hh, Ww, scale):
    """q, k, v [nWin, nh, T, hd] float64 -> O [nWin, nh, T, hd] (WindowAttention.forward, network_swinir.py:114-145)."""
    T = ws * ws
    bias = table[_relidx(ws).view(-1)].view(T, T, nh).permute(2, 0, 1)
    s = (q * scale) @ k.transpose(-2, -1) + bias
    if shift:
        mask = _shift_mask(Hh, Ww, ws, shift)
        nW = mask.shape[0]
        s = (s.view(-1, nW, nh, T, T) + mask[None, :, None]).view(-1, nh, T, T)
    return torch.softmax(s, -1) @ v


# the attention cases' shape: B = 2, 14 x 21 tokens (12 windows), 6 heads of dim 30
B_, HH, WW, NH, HD, WS7, T7 = 2, 14, 21, 6, 30, 7, 49
NWIN = B_ * (HH // WS7) * (WW // WS7)
_REF = {}


def _case(shift, bf=False):
    """Inputs and the float64 reference (computed once per case, never modified).  bf: q, k, v and dO rounded to
    bf16 first, so the comparison is on the values the bf16 kernels read (test_window_attention_fwd_bwd)."""
    if (shift, bf) not in _REF:
        g = torch.Generator().manual_seed(19)
        q, k, v = (torch.randn(NWIN, NH, T7, HD, generator=g) for _ in range(3))
        table = torch.randn(169, NH, generator=g) * 0.5
        if bf:
            q, k, v = (t.bfloat16().float() for t in (q, k, v))
        qr, kr, vr, tr = (t.double().clone().requires_grad_(True) for t in (q, k, v, table))
        o = attn_ref(qr, kr, vr, tr, NH, WS7, shift, HH, WW, HD ** -0.5)
        go = torch.randn(o.shape, generator=g, dtype=torch.float64)
        if bf:
            go = go.bfloat16().double()
        o.backward(go)
        qkv = torch.zeros(3, NWIN, NH, T7, 32)
        qkv[0, ..., :HD], qkv[1, ..., :HD], qkv[2, ..., :HD] = q, k, v
        _REF[(shift, bf)] = dict(qkv=qkv, table=table, o=o.detach(), go=go, dq=qr.grad, dk=kr.grad, dv=vr.grad, dt=tr.grad)
    return _REF[(shift, bf)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shift", [0, 3])
def test_window7_attention_fp32_bf16(shift, dtype):
    """kair_window_attn_fwd_w / _bwd_w at ws = 7 in fp32 and bf16: the bars of test_window_attention_fwd_bwd (fp32:
    forward 2e-5, backward 5e-5; bf16: 1.5e-2 / 3e-2 on the bf16-rounded inputs); pad columns of O exactly 0; every
    output pre-filled with NaN and finite after."""
    bf = dtype == "bf16"
    tdt = torch.bfloat16 if bf else torch.float32
    tol_f, tol_b = (1.5e-2, 3e-2) if bf else (2e-5, 5e-5)
    c = _case(shift, bf)
    scale = HD ** -0.5
    qkv_d = c["qkv"].to(dev, tdt).contiguous()
    nan = float("nan")
    O = torch.full((NWIN * T7, NH * 32), nan, device=dev, dtype=tdt)
    lse = torch.full((NWIN, NH, T7), nan, device=dev)
    H.window_attn_fwd(qkv_d, c["table"].to(dev), O, NH * 32, lse, NWIN, NH, HD, scale, HH, WW, shift, ws=7)
    torch.cuda.synchronize()
    Ov = O.float().cpu().view(NWIN, T7, NH, 32)
    assert torch.isfinite(Ov).all() and torch.isfinite(lse).all()
    e_f = rel(Ov[..., :HD].permute(0, 2, 1, 3), c["o"])
    print(dtype, "ws7 fwd rel", e_f)
    assert e_f < tol_f
    assert Ov[..., HD:].abs().max() == 0
    dO = torch.zeros(NWIN, T7, NH, 32)
    dO[..., :HD] = c["go"].float().permute(0, 2, 1, 3)
    dqkv = torch.full_like(qkv_d, nan)
    dtab = torch.full((169, NH), nan, device=dev)
    ws = torch.empty(H.window_attn_bwd_ws(NWIN, NH, ws=7), device=dev)
    H.window_attn_bwd(qkv_d, O, NH * 32, dO.view(NWIN * T7, NH * 32).to(dev, tdt), NH * 32, c["table"].to(dev), lse, dqkv,
                      dtab, False, ws, NWIN, NH, HD, scale, HH, WW, shift, win_ws=7)
    torch.cuda.synchronize()
    d = dqkv.float().cpu()
    assert torch.isfinite(d).all() and torch.isfinite(dtab).all()
    errs = [rel(d[0, ..., :HD], c["dq"]), rel(d[1, ..., :HD], c["dk"]), rel(d[2, ..., :HD], c["dv"]), rel(dtab, c["dt"])]
    print(dtype, "ws7 bwd rel dq dk dv dtable", errs)
    assert max(errs) < tol_b
    assert d[..., HD:].abs().max() == 0


@pytest.mark.parametrize("f32_out", [False, True])
@pytest.mark.parametrize("shift", [0, 3])
def test_window7_attention_x3(shift, f32_out):
    """kair_window_attn_fwd_x3_w / _bwd_x3_w at ws = 7: test_window_attention_x3's bars (forward 2e-6; dq, dk, dv,
    dtable 5e-6), the fp16-pair and the fp32 output forms."""
    c = _case(shift)
    scale = HD ** -0.5
    e_act, e_grad = 4, 26
    nan = float("nan")
    qkv_p = hilo(c["qkv"].view(-1).to(dev), e_act)
    if f32_out:
        O = torch.full((NWIN * T7, NH * 32), nan, device=dev)
    else:
        O = torch.full((2, NWIN * T7, NH * 32), nan, device=dev, dtype=torch.float16)
    lse = torch.full((NWIN, NH, T7), nan, device=dev)
    H.window_attn_fwd_x3(qkv_p, c["table"].to(dev), O, NH * 32, lse, NWIN, NH, HD, scale, HH, WW, shift, e_in=e_act,
                         e_out=e_act, ws=7)
    torch.cuda.synchronize()
    assert torch.isfinite(O).all() and torch.isfinite(lse).all()
    if f32_out:
        Of = O.double().cpu().view(NWIN, T7, NH, 32)
    else:
        Of = (O[0].double() + O[1].double()).cpu().view(NWIN, T7, NH, 32) * 2.0 ** -e_act
    e_f = rel(Of[..., :HD].permute(0, 2, 1, 3), c["o"])
    print("x3 ws7 fwd rel", e_f)
    assert e_f < 2e-6
    assert Of[..., HD:].abs().max() == 0
    dO = torch.zeros(NWIN, T7, NH, 32)
    dO[..., :HD] = c["go"].float().permute(0, 2, 1, 3) * 1e-7
    dO_p = hilo(dO.view(NWIN * T7, NH * 32).to(dev), e_grad)
    if f32_out:
        dqkv = torch.full((NWIN * T7, 3 * NH * 32), nan, device=dev)
    else:
        dqkv = torch.full((2, NWIN * T7, 3 * NH * 32), nan, device=dev, dtype=torch.float16)
    dtab = torch.full((169, NH), nan, device=dev)
    ws = torch.empty(H.window_attn_bwd_ws(NWIN, NH, ws=7), device=dev)
    H.window_attn_bwd_x3(qkv_p, O, NH * 32, dO_p, NH * 32, c["table"].to(dev), lse, dqkv, dtab, False, ws, NWIN, NH, HD,
                         scale, HH, WW, shift, e_act=e_act, e_grad=e_grad, win_ws=7)
    torch.cuda.synchronize()
    assert torch.isfinite(dqkv).all() and torch.isfinite(dtab).all()
    if f32_out:
        d = dqkv.double().cpu().view(NWIN, T7, 3, NH, 32)[..., :HD].permute(2, 0, 3, 1, 4) * 1e7
    else:
        d = (dqkv[0].double() + dqkv[1].double()).cpu().view(NWIN, T7, 3, NH, 32)[..., :HD].permute(2, 0, 3, 1, 4)
        d = d * 2.0 ** -e_grad * 1e7
    errs = [rel(d[0], c["dq"]), rel(d[1], c["dk"]), rel(d[2], c["dv"]), rel(dtab * 1e7, c["dt"])]
    print("x3 ws7 bwd rel dq dk dv dtable", errs)
    assert max(errs) < 5e-6


def test_window8_identity_fp32():
    """The window-size-taking entry points at ws = 8 give the bits of the existing ones (O, lse, dqkv, dtable) on
    test_window_attention_fwd_bwd's shape."""
    Bn, Hh, Ww, nh, hd, shift = 2, 16, 24, 6, 30, 4
    nWin = Bn * (Hh // 8) * (Ww // 8)
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(19)
    qkv = torch.zeros(3, nWin, nh, 64, 32)
    qkv[..., :hd] = torch.randn(3, nWin, nh, 64, hd, generator=g)
    table = (torch.randn(225, nh, generator=g) * 0.5).to(dev)
    dO = torch.zeros(nWin * 64, nh, 32)
    dO[..., :hd] = torch.randn(nWin * 64, nh, hd, generator=g)
    qkv_d, dO_d = qkv.to(dev), dO.view(nWin * 64, nh * 32).to(dev)
    L = H.lib()
    out = []
    for new in (False, True):
        O = torch.empty(nWin * 64, nh * 32, device=dev)
        lse = torch.empty(nWin, nh, 64, device=dev)
        dqkv = torch.empty_like(qkv_d)
        dtab = torch.empty(225, nh, device=dev)
        ws = torch.empty(H.window_attn_bwd_ws(nWin, nh), device=dev)
        p, sp = H.ptr, H.stream_ptr()
        if new:
            assert H.window_attn_bwd_ws(nWin, nh, ws=8) == H.window_attn_bwd_ws(nWin, nh)
            H.window_attn_fwd(qkv_d, table, O, nh * 32, lse, nWin, nh, hd, scale, Hh, Ww, shift, ws=8)
            H.window_attn_bwd(qkv_d, O, nh * 32, dO_d, nh * 32, table, lse, dqkv, dtab, False, ws, nWin, nh, hd, scale,
                              Hh, Ww, shift, win_ws=8)
        else:
            H.check(L.kair_window_attn_fwd(p(qkv_d), H.F32, p(table), p(O), nh * 32, p(lse), nWin, nh, hd, scale, Hh, Ww,
                                           shift, -1, None, 0, sp), "fwd")
            H.check(L.kair_window_attn_bwd(p(qkv_d), p(O), nh * 32, p(dO_d), nh * 32, H.F32, p(table), p(lse), p(dqkv),
                                           p(dtab), 0, p(ws), nWin, nh, hd, scale, Hh, Ww, shift, None, 0, sp), "bwd")
        torch.cuda.synchronize()
        out.append((O.cpu(), lse.cpu(), dqkv.cpu(), dtab.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("f32_out", [False, True])
def test_window8_identity_x3(f32_out):
    """The same for the fp32x3 pair on test_window_attention_x3's shape."""
    Bn, Hh, Ww, nh, hd, shift = 2, 16, 24, 6, 30, 4
    nWin = Bn * (Hh // 8) * (Ww // 8)
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(19)
    qkv = torch.zeros(3, nWin, nh, 64, 32)
    qkv[..., :hd] = torch.randn(3, nWin, nh, 64, hd, generator=g)
    table = (torch.randn(225, nh, generator=g) * 0.5).to(dev)
    dO = torch.zeros(nWin * 64, nh, 32)
    dO[..., :hd] = torch.randn(nWin * 64, nh, hd, generator=g) * 1e-7
    e_act, e_grad = 4, 26
    qkv_p = hilo(qkv.view(-1).to(dev), e_act)
    dO_p = hilo(dO.view(nWin * 64, nh * 32).to(dev), e_grad)
    L = H.lib()
    out = []
    for new in (False, True):
        if f32_out:
            O = torch.empty(nWin * 64, nh * 32, device=dev)
            dqkv = torch.empty(nWin * 64, 3 * nh * 32, device=dev)
        else:
            O = torch.empty(2, nWin * 64, nh * 32, device=dev, dtype=torch.float16)
            dqkv = torch.empty(2, nWin * 64, 3 * nh * 32, device=dev, dtype=torch.float16)
        lse = torch.empty(nWin, nh, 64, device=dev)
        dtab = torch.empty(225, nh, device=dev)
        ws = torch.empty(H.window_attn_bwd_ws(nWin, nh), device=dev)
        if new:
            H.window_attn_fwd_x3(qkv_p, table, O, nh * 32, lse, nWin, nh, hd, scale, Hh, Ww, shift, e_in=e_act,
                                 e_out=e_act, ws=8)
            H.window_attn_bwd_x3(qkv_p, O, nh * 32, dO_p, nh * 32, table, lse, dqkv, dtab, False, ws, nWin, nh, hd, scale,
                                 Hh, Ww, shift, e_act=e_act, e_grad=e_grad, win_ws=8)
        else:
            p, sp = H.ptr, H.stream_ptr()
            (o, ol), (dq, dql) = H._planes(O), H._planes(dqkv)
            H.check(L.kair_window_attn_fwd_x3(p(qkv_p[0]), p(qkv_p[1]), p(table), o, ol, nh * 32, p(lse), nWin, nh, hd,
                                              scale, Hh, Ww, shift, -1, e_act, e_act, sp), "fwd_x3")
            H.check(L.kair_window_attn_bwd_x3(p(qkv_p[0]), p(qkv_p[1]), o, ol, nh * 32, p(dO_p[0]), p(dO_p[1]), nh * 32,
                                              p(table), p(lse), dq, dql, p(dtab), 0, p(ws), nWin, nh, hd, scale, Hh, Ww,
                                              shift, e_act, e_grad, sp), "bwd_x3")
        torch.cuda.synchronize()
        out.append((O.cpu(), lse.cpu(), dqkv.cpu(), dtab.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# network vs oracle
# ---------------------------------------------------------------------------------------------------------------
def _net_pair(dt, embed=60, depths=(2, 2), in_chans=1, seed=3):
    torch.manual_seed(seed)
    depths = list(depths)
    net = SwinIR(img_size=14, window_size=7, depths=depths, embed_dim=embed, num_heads=[6] * len(depths), mlp_ratio=2,
                 upscale=1, in_chans=in_chans, img_range=255.0, upsampler=None, resi_connection="1conv",
                 drop_path_rate=0.0, compute_dtype=dt)
    ref = osw.SwinIR(1, in_chans, 14, 7, 255.0, depths, embed, [6] * len(depths), 2, None, "1conv")
    with torch.no_grad():   # non-trivial biases / LayerNorm affine so every gradient is exercised
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    ref.load_state_dict(net.state_dict(), strict=True)
    return net.to(dev), ref


def _fwd_bwd_vs_oracle(net, ref, L, Hh, tol, gtol, med_tol=None):
    net.train()
    E = net(L.to(dev))
    torch.nn.functional.l1_loss(E, Hh.to(dev)).backward()
    Er = ref(L)
    torch.nn.functional.l1_loss(Er, Hh).backward()
    e = rel(E, Er)
    gref = dict(ref.named_parameters())
    worst = {k: rel(p.grad, gref[k].grad) for k, p in net.named_parameters()}
    k = max(worst, key=worst.get)
    med = sorted(worst.values())[len(worst) // 2]
    print("ws7 network: output rel", e, "worst gradient", k, worst[k], "median", med)
    assert e < tol
    assert worst[k] < gtol, (k, worst[k])
    assert med_tol is None or med < med_tol, med


@pytest.mark.parametrize("dt", ["fp32", "fp32x3", "bf16"])
def test_window7_small_network_vs_oracle(dt):
    """The JPEG head at small size (gray, img_range 255, no upsampler), 2 x 1 x 14 x 21, L1 loss: output < 1e-4,
    every gradient < 2e-3; bf16: test_swinir_variant_vs_golden's bf16 bars with '1conv' (output 2e-2, worst
    gradient 0.12, median gradient 2e-2)."""
    net, ref = _net_pair(dt)
    g = torch.Generator().manual_seed(4)
    L, Hh = torch.rand(2, 1, 14, 21, generator=g), torch.rand(2, 1, 14, 21, generator=g)
    if dt == "bf16":
        _fwd_bwd_vs_oracle(net, ref, L, Hh, 2e-2, 0.12, 2e-2)
    else:
        _fwd_bwd_vs_oracle(net, ref, L, Hh, 1e-4, 2e-3)


@pytest.mark.parametrize("dt", ["fp32x3", "bf16"])
def test_window7_width180_vs_oracle(dt):
    """embed_dim 180 (Cp = 192, where the 8 x 8-only specialised paths would otherwise engage), colour, 21 x 14:
    test_swinir_variant_width180_vs_oracle's bars for the dtype (fp32x3 1e-4 / 2e-3, bf16 2e-2 / 8e-2)."""
    net, ref = _net_pair(dt, embed=180, depths=(2,), in_chans=3)
    if dt == "bf16":
        e = net.engine()
        assert not (e.fused_attn or e.fused_mlp or e.fused_mlp_bwd or e.rowgemm) and e.hp == 32
    g = torch.Generator().manual_seed(4)
    L, Hh = torch.rand(2, 3, 21, 14, generator=g), torch.rand(2, 3, 21, 14, generator=g)
    tol, gtol = (2e-2, 8e-2) if dt == "bf16" else (1e-4, 2e-3)
    _fwd_bwd_vs_oracle(net, ref, L, Hh, tol, gtol)


def test_window7_reflect_pad_vs_oracle():
    """A 12 x 17 input reflect-pads to 14 x 21 (network_swinir.py:783-788) and is cropped back."""
    net, ref = _net_pair("fp32x3")
    net.eval()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 1, 12, 17, generator=g)
    with torch.no_grad():
        e, r = net(x.to(dev)), ref(x)
    assert e.shape == r.shape == (2, 1, 12, 17)
    assert rel(e, r) < 1e-4


def test_window7_tiled_inference_vs_oracle():
    """utils_model.test_tiled at window_size 7, tile 14, on a 21 x 28 image against the oracle under the same tiling
    (tests/test_inference_gpu.py::test_tiled_inference_vs_oracle's bar)."""
    net, ref = _net_pair("fp32x3")
    net.eval()
    g = torch.Generator().manual_seed(6)
    x = torch.rand(1, 1, 21, 28, generator=g)
    with torch.no_grad():
        e = utils_model.test_tiled(net, x.to(dev), tile=14, tile_overlap=7, sf=1, window_size=7)
        r = utils_model.test_tiled(ref, x, tile=14, tile_overlap=7, sf=1, window_size=7)
    assert e.shape == r.shape == (1, 1, 21, 28)
    assert rel(e, r) < 1e-5


@pytest.mark.parametrize("use_graph", [False, True])
def test_window7_trainer_x3_vs_oracle_trainer(use_graph):
    """3 FusedTrainer steps (Adam + EMA, the MultiStepLR halving at step 2) at window size 7 on the fp32x3 engine
    against OracleTrainer: test_trainer_x3_matches_reference_trajectory's network and bars (losses and every state
    entry < 1e-4) on 14 x 21 inputs.  The key third of each qkv bias has a zero gradient in exact arithmetic; it is
    compared as every OracleTrainer comparison here does (conftest.state_rel_excluding_kbias: <= 2 lr per step)."""
    torch.manual_seed(11)
    mk = lambda: SwinIR(upscale=4, in_chans=3, img_size=14, window_size=7, img_range=1.0, depths=[2, 2], embed_dim=60,
                        num_heads=[6, 6], mlp_ratio=2, upsampler="pixelshuffle", drop_path_rate=0.0,
                        compute_dtype="fp32x3")
    net, ema = mk(), mk()
    ema.load_state_dict(net.state_dict())
    mko = lambda: osw.SwinIR(4, 3, 14, 7, 1.0, [2, 2], 60, [6, 6], 2, "pixelshuffle")
    ref, ref_e = mko(), mko()
    ref.load_state_dict(net.state_dict(), strict=True)
    ref_e.load_state_dict(net.state_dict(), strict=True)
    net, ema = net.to(dev).train(), ema.to(dev).eval()
    tr = FusedTrainer(net, ema, lr=2e-4, E_decay=0.999, use_graph=use_graph)
    otr = OracleTrainer(ref, ref_e, lr=2e-4, milestones=[2, 100], gamma=0.5, E_decay=0.999)
    g = torch.Generator().manual_seed(12)
    for s in range(1, 4):
        L = torch.rand(2, 3, 14, 21, generator=g)
        Hh = torch.rand(2, 3, 56, 84, generator=g)
        tr.lr = 2e-4 * 0.5 ** sum(1 for m in (2, 100) if m <= s)
        loss = tr.step(L.to(dev), Hh.to(dev)).item()
        otr.update_learning_rate()
        _, lo = otr.optimize_parameters(L, Hh)
        lo = float(lo)
        assert abs(loss - lo) < 1e-4 * abs(lo), (s, loss, lo)
    for mine, theirs in ((net, ref), (ema, ref_e)):
        r, kmax = state_rel_excluding_kbias(mine.state_dict(), theirs.state_dict(), 60)
        worst = max((v, k) for k, v in r.items())
        assert worst[0] < 1e-4, worst
        assert kmax <= 2 * 2e-4 * 3, kmax
