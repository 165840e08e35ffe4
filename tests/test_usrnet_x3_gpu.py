"""USRNet on the fp32x3 engine (the fp32 reference's precision class on the 16-bit matrix cores: every ResUNet
product as hi.hi + hi.lo + lo.hi of power-of-2-scaled fp16 pairs; the FFT / DataNet / HyPaNet passes are the fp32
engine's own).

  * the fp16-pair packs of the 2x2 / stride-2 layouts (kair_wmap kinds 20 / 21, the pairs of kinds 7 / 8);
  * the space-to-depth operand (KAIR_LD_S2D) of kair_gemm_nt (A) and kair_gemm_tn (B) under KAIR_COMPUTE_X3, against
    float64 at tests/test_x3_gpu.py's bar for the generic kernels (2e-6 relative L2), and its argument errors;
  * the whole network against the CPU oracle at exactly the exact-fp32 engine's bars (tests/test_usrnet_gpu.py
    TOL["fp32"]: output 1e-4, worst gradient 5e-3, mean gradient 1e-3), the fused trainer against the oracle trainer,
    the range guard, and a define_Model('plain4') step.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from conftest import load_golden, sub_grads, sub_state  # noqa: E402
from kair_amd import _hip as H  # noqa: E402
from kair_amd.models.network_usrnet import USRNet  # noqa: E402
from oracle import convnets as ocv  # noqa: E402

dev = torch.device("cuda")
TOL_FP32 = (1e-4, 5e-3, 1e-3)   # out, worst grad, mean grad: TOL["fp32"] of tests/test_usrnet_gpu.py
NT_BAR = TN_BAR = 2e-6          # tests/test_x3_gpu.py: the generic x3 NT / TN kernels against float64
WIDTHS = dict(h_nc=32, in_nc=4, out_nc=3, nc=[16, 32, 64, 64], nb=2)   # options/train_usrnet.json


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rand_kernel(B, n, g):
    k = torch.rand(B, 1, n, n, generator=g, dtype=torch.float64)
    return k / k.sum((-2, -1), keepdim=True)


def ks(k):
    return 2 * (-(-k // 64)) * 64


def wsplit(w):
    """kind-17 pair pack of a [N][K] weight and its operand (as tests/test_x3_gpu.py)."""
    N, K = w.shape
    Wp = torch.empty(N, ks(K), device=dev, dtype=torch.float16)
    H.pack_weight(w.to(dev), Wp, H.wmap(17, N, K))
    o = H.rows(Wp)
    o.x3_exp = H.X3_WEXP
    return o, Wp


# ------------------------------------------------------------------------------------------
# packs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Co,Ci", [(32, 16), (24, 8)])
@pytest.mark.parametrize("kind", [20, 21])
def test_split_pack_2x2(kind, Co, Ci):
    """Kinds 20 / 21: fp16 pairs of w 2^KAIR_X3_WEXP in the 64-column alternating hi / lo rows of kind 7 ([Co][4 Ci],
    k = tap Ci + ci) and kind 8 ([4 Ci][Co], row = ci 4 + tap).  The hi plane is f16(w 2^WEXP) exactly and every
    element has |(hi + lo) 2^-WEXP - w| <= 2^-21 |w|: hi leaves a residual <= 2^-11 |w| that fp32 holds exactly, and
    lo rounds it to 2^-11 relative, as long as lo is a normal fp16 or its subnormal half-ulp 2^-25 (2^-37 in w's
    units) is under the bound, i.e. |w| >= 2^-16; the random weight's magnitudes are kept above 2^-12 (weights
    nearer zero than that meet an absolute bound instead, which this test does not ask for).  The single launch
    (kair_pack_weight) and the batched one (kair_pack_weights) give the same bits; pad columns are zero."""
    g = torch.Generator().manual_seed(7 + kind + Co)
    w = torch.randn(Co, Ci, 2, 2, generator=g) * 0.2
    w = torch.where(w.abs() < 2.0 ** -12, torch.full_like(w, 2.0 ** -12), w)
    if kind == 20:
        plain = w.permute(0, 2, 3, 1).reshape(Co, 4 * Ci)                    # [n][tap * Ci + k]
    else:
        plain = w.reshape(Co, Ci, 4).permute(1, 2, 0).reshape(4 * Ci, Co)     # [k * 4 + tap][n]
    rows, rowlen = plain.shape
    KS = ks(rowlen)
    wd = w.to(dev)
    sp = torch.full((rows, KS), float("nan"), device=dev, dtype=torch.float16)
    H.pack_weight(wd, sp, H.wmap(kind, Co, Ci))
    sp2 = torch.full((rows, KS), float("nan"), device=dev, dtype=torch.float16)
    H.PackTable([(wd, sp2, H.wmap(kind, Co, Ci))]).run()
    torch.cuda.synchronize()
    assert torch.isfinite(sp).all()
    assert torch.equal(sp.view(torch.int16), sp2.view(torch.int16))
    s = sp.cpu().view(rows, KS // 128, 2, 64)
    hi, lo = s[:, :, 0].reshape(rows, -1), s[:, :, 1].reshape(rows, -1)
    assert (hi[:, rowlen:] == 0).all() and (lo[:, rowlen:] == 0).all()
    hi, lo = hi[:, :rowlen], lo[:, :rowlen]
    assert torch.equal(hi, (plain * 2.0 ** H.X3_WEXP).to(torch.float16))
    err = ((hi.double() + lo.double()) * 2.0 ** -H.X3_WEXP - plain.double()).abs()
    worst = (err / plain.double().abs()).max().item()
    print(f"pack kind {kind} ({Co}, {Ci}): worst relative error {worst:.3e} (bar {2.0 ** -21:.3e})")
    assert (err <= 2.0 ** -21 * plain.double().abs()).all()


# ------------------------------------------------------------------------------------------
# the space-to-depth operand
# ------------------------------------------------------------------------------------------
S2D_SHAPES = [(1, 4, 4, 8, 16), (3, 6, 10, 24, 40)]   # B, Hn, Wn, C, N: M = 16 / 180, K = 32 / 96


def s2d_cols(x, B, Hn, Wn, C):
    """[M][4 C] float64: row (b, y, x), column (i 2 + j) C + c = pixel (2y + i, 2x + j), channel c."""
    return x.double().view(B, Hn, 2, Wn, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * Hn * Wn, 4 * C)


@pytest.mark.parametrize("pshuf", [False, True])
@pytest.mark.parametrize("B,Hn,Wn,C,N", S2D_SHAPES)
def test_gemm_nt_x3_s2d(B, Hn, Wn, C, N, pshuf):
    """kair_gemm_nt, KAIR_COMPUTE_X3, A the space-to-depth view of an fp32 [B, 2Hn, 2Wn, C] map, against float64;
    a plain ROWS store and the OUT_PSHUF r = 2 store (n = c 4 + i 2 + j -> pixel (2y + i, 2x + j), channel c).  The
    second shape has M = 180 (no multiple of a row tile), K = 96 (a multiple of the 32-deep k-step, not of the pack's
    64-column chunk) and N = 40 (no multiple of 32)."""
    g = torch.Generator().manual_seed(11 + C)
    M, K = B * Hn * Wn, 4 * C
    x = torch.randn(B, 2 * Hn, 2 * Wn, C, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    Wo, keep = wsplit(w)
    A = H.s2d(x.to(dev), Hn, Wn, C)
    A.x3_exp = 4
    ref = s2d_cols(x, B, Hn, Wn, C) @ w.double().T
    if pshuf:
        c = N // 4
        out = torch.full((4 * M, c), float("nan"), device=dev)
        E = H.epilogue(out, mode=H.OUT_PSHUF, ldo=c, ps=(2, Hn, Wn))
        ref = ref.view(B, Hn, Wn, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(4 * M, c)
    else:
        out = torch.full((M, N), float("nan"), device=dev)
        E = H.epilogue(out)
    H.gemm_nt(A, Wo, E, M, N, K, H.X3)
    torch.cuda.synchronize()
    r = rel(out, ref)
    print(f"nt s2d {(B, Hn, Wn, C, N)} pshuf={pshuf}: rel {r:.3e} (bar {NT_BAR:.0e})")
    assert torch.isfinite(out).all() and r < NT_BAR


@pytest.mark.parametrize("B,Hn,Wn,C,N", S2D_SHAPES)
def test_gemm_tn_x3_s2d(B, Hn, Wn, C, N):
    """kair_gemm_tn, KAIR_COMPUTE_X3, B the space-to-depth view (the 2x2 convs' weight gradients): a gradient-sized A
    at exponent 24, three row splits (M = 180: 64 + 64 + 52 rows; M = 16: one 32-row range, the other planes zero),
    against float64."""
    g = torch.Generator().manual_seed(13 + C)
    M, K, S = B * Hn * Wn, 4 * C, 3
    x = torch.randn(B, 2 * Hn, 2 * Wn, C, generator=g)
    dy = torch.randn(M, N, generator=g) * 1e-6
    ws = torch.full((S, N, K), float("nan"), device=dev)
    A = H.rows(dy.to(dev))
    A.x3_exp = 24
    Bop = H.s2d(x.to(dev), Hn, Wn, C)
    Bop.x3_exp = 4
    H.gemm_tn(A, Bop, ws, S, M, N, K, H.X3)
    torch.cuda.synchronize()
    r = rel(ws.sum(0), dy.double().T @ s2d_cols(x, B, Hn, Wn, C))
    print(f"tn s2d {(B, Hn, Wn, C, N)}: rel {r:.3e} (bar {TN_BAR:.0e})")
    assert torch.isfinite(ws).all() and r < TN_BAR


def test_s2d_x3_argument_errors():
    """K != 4 im_C and im_C % 8 != 0 are argument errors of both entry points, and nothing is launched: the
    outputs keep their fill."""
    g = torch.Generator().manual_seed(17)
    B, Hn, Wn, N = 1, 4, 4, 16
    M = B * Hn * Wn
    for C, K in ((8, 40), (8, 24), (12, 48)):
        x = torch.randn(B, 2 * Hn, 2 * Wn, C, generator=g).to(dev)
        Wo, keep = wsplit(torch.randn(N, K, generator=g))
        out = torch.full((M, N), 7.0, device=dev)
        A = H.s2d(x, Hn, Wn, C)
        A.x3_exp = 4
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            H.gemm_nt(A, Wo, H.epilogue(out), M, N, K, H.X3)
        ws = torch.full((1, N, K), 7.0, device=dev)
        dy = H.rows(torch.randn(M, N, generator=g).to(dev))
        dy.x3_exp = 4
        Bop = H.s2d(x, Hn, Wn, C)
        Bop.x3_exp = 4
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            H.gemm_tn(dy, Bop, ws, 1, M, N, K, H.X3)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (ws == 7.0).all()


# ------------------------------------------------------------------------------------------
# the network
# ------------------------------------------------------------------------------------------
def _fwd_bwd_check(net, x, k, sf, sigma, out_ref, gout, grads_ref, tag):
    """_usrnet_fwd_bwd_check of tests/test_usrnet_gpu.py at TOL["fp32"], printing the figures first."""
    out = net(x.to(dev), k.to(dev), sf, sigma.to(dev))
    e_out = rel(out, out_ref)
    out.backward(gout.to(dev))
    errs = {name: rel(p.grad, grads_ref[name]) for name, p in net.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    mean = sum(errs.values()) / len(errs)
    print(f"usrnet fp32x3 {tag}: out {e_out:.3e} (bar {TOL_FP32[0]:.0e}), worst grad {worst[1]:.3e} {worst[0]} "
          f"(bar {TOL_FP32[1]:.0e}), mean grad {mean:.3e} (bar {TOL_FP32[2]:.0e})")
    assert net.engine().x3 and net.engine().x3_backoffs == 0
    assert e_out < TOL_FP32[0]
    bad = {k: e for k, e in errs.items() if e > TOL_FP32[1]}
    assert not bad, bad
    assert mean < TOL_FP32[2], sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def test_usrnet_x3_vs_golden():
    """The golden case of test_usrnet_vs_golden (n_iter 2, HR 64x64, sf 4) on the fp32x3 engine at TOL["fp32"]."""
    z = load_golden("usrnet")
    net = USRNet(n_iter=2, compute_dtype="fp32x3", **WIDTHS)
    net.load_state_dict(sub_state(z, ""), strict=True)
    _fwd_bwd_check(net.to(dev).train(), torch.from_numpy(z["x"]), torch.from_numpy(z["k"]), int(z["sf"]),
                   torch.from_numpy(z["sigma"]), torch.from_numpy(z["out"]), torch.from_numpy(z["gout"]),
                   sub_grads(z, ""), "golden")


@pytest.mark.parametrize("lq,sf,n_iter,B", [(16, 4, 2, 2), (16, 4, 6, 2), (24, 2, 3, 2), (27, 4, 2, 1), (18, 3, 2, 2)])
def test_usrnet_x3_vs_oracle(lq, sf, n_iter, B):
    """Output and every parameter gradient against oracle.convnets.USRNet at TOL["fp32"]; (16, 4, 6): one gradient
    exponent across six shared-weight stages; (27, 4) and (18, 3): the replicate pad / crop and their adjoints."""
    torch.manual_seed(21 + sf)
    net = USRNet(n_iter=n_iter, compute_dtype="fp32x3", **WIDTHS)
    ref = ocv.USRNet(n_iter=n_iter, **WIDTHS)
    ref.load_state_dict(net.state_dict(), strict=True)
    g = torch.Generator().manual_seed(22 + sf)
    x = torch.rand(B, 3, lq, lq, generator=g)
    k = rand_kernel(B, 25, g).float()
    sigma = torch.rand(B, 1, 1, 1, generator=g) * (25.0 / 255)
    out_ref = ref(x, k, sf, sigma)
    gout = torch.randn(out_ref.shape, generator=g)
    out_ref.backward(gout)
    grads = {n: p.grad for n, p in ref.named_parameters()}
    _fwd_bwd_check(net.to(dev).train(), x, k, sf, sigma, out_ref, gout, grads, str((lq, sf, n_iter, B)))


def test_usrnet_x3_fused_trainer_vs_oracle_trainer():
    """Four graph-captured FusedTrainer steps on the fp32x3 engine against the oracle trainer, at
    test_usrnet_fused_trainer_vs_oracle_trainer's bars (loss 1e-4 relative; parameters 1e-4, one-dimensional ones
    1e-3); the range guard is armed and never fires."""
    from kair_amd.engine.trainer import FusedTrainer
    from oracle.train import OracleTrainer
    torch.manual_seed(31)
    mk = lambda: USRNet(n_iter=2, compute_dtype="fp32x3", **WIDTHS)   # noqa: E731
    net, ema = mk(), mk()
    ema.load_state_dict(net.state_dict())
    ref, ref_e = ocv.USRNet(n_iter=2, **WIDTHS), ocv.USRNet(n_iter=2, **WIDTHS)
    ref.load_state_dict(net.state_dict(), strict=True)
    ref_e.load_state_dict(net.state_dict(), strict=True)
    net, ema = net.to(dev).train(), ema.to(dev).eval()
    tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
    otr = OracleTrainer(ref, ref_e, lr=1e-4, E_decay=0.999)
    g = torch.Generator().manual_seed(32)
    B, sf = 2, 4
    for _ in range(4):
        L = torch.rand(B, 3, 16, 16, generator=g)
        Hh = torch.rand(B, 3, 64, 64, generator=g)
        k = rand_kernel(B, 25, g).float()
        sigma = torch.rand(B, 1, 1, 1, generator=g) * (25.0 / 255)
        loss = tr.step(L.to(dev), Hh.to(dev), k.to(dev), sf, sigma.to(dev)).item()
        _, lo = otr.optimize_parameters(L, Hh, forward=lambda x: ref(x, k, sf, sigma))
        print(f"trainer fp32x3: loss {loss:.8f} oracle {lo:.8f} rel {abs(loss - lo) / abs(lo):.3e}")
        assert abs(loss - lo) < 1e-4 * abs(lo), (loss, lo)
    tr.check_range()
    assert tr.graph is not None
    assert tr.range_guard is True
    assert tr.engine.x3_backoffs == 0 and not tr.range_events
    sd, sdr = net.state_dict(), ref.state_dict()
    worst = {1: 0.0, 2: 0.0}
    for key in sdr:
        r = rel(sd[key], sdr[key])
        worst[1 if sdr[key].dim() == 1 else 2] = max(worst[1 if sdr[key].dim() == 1 else 2], r)
        assert r < (1e-3 if sdr[key].dim() == 1 else 1e-4), (key, r)
    print(f"trainer fp32x3: worst parameter rel {worst[2]:.3e} (bar 1e-4), one-dimensional {worst[1]:.3e} (bar 1e-3)")


def test_usrnet_x3_range_guard():
    """The pattern of tests/test_x3_range_gpu.py's test_guard_activations_near_1e4, with that file's scale factor
    (patches x 1e4: the ResUNet's head operand z ~ 1e4, 2^4 x 1e4 > 65504, which trips the guard here too).  The
    first step's loss is not finite: its Adam update is skipped (parameters and moments bit-identical), x3_backoff
    lowers the activation exponent only, the step is re-run finite, and three more steps (graph-captured at the
    lowered exponent) leave finite parameters."""
    from kair_amd.engine.trainer import FusedTrainer
    torch.manual_seed(41)
    net = USRNet(n_iter=2, compute_dtype="fp32x3", **WIDTHS).to(dev).train()
    tr = FusedTrainer(net, None, lr=1e-4, E_decay=0.0, use_graph=True)
    g = torch.Generator().manual_seed(42)
    B, sf, scale = 2, 4, 1e4
    p0 = tr.flat_p.clone()
    for step in range(4):
        L = (torch.rand(B, 3, 16, 16, generator=g) * scale).to(dev)
        Hh = (torch.rand(B, 3, 64, 64, generator=g) * scale).to(dev)
        k = rand_kernel(B, 25, g).float().to(dev)
        sigma = (torch.rand(B, 1, 1, 1, generator=g) * (25.0 / 255)).to(dev)
        loss = tr.step(L, Hh, k, sf, sigma)
        if step == 0:   # flagged: nothing was updated
            torch.cuda.synchronize()
            assert int(tr.rflag) != 0 and not torch.isfinite(loss).all()
            assert torch.equal(tr.flat_p, p0) and not tr.m.any() and not tr.v.any()
        tr.check_range()
        assert torch.isfinite(loss).all(), (step, loss)
        if step == 0:   # re-run at the lowered exponent: now the update happened
            assert tr.range_events and tr.range_events[0][0] == 1
            assert not torch.equal(tr.flat_p, p0)
    eng = tr.engine
    assert eng.x3_backoffs >= 1 and eng.X3_AEXP < 4 and eng.x3_gexp_off == 4   # only the activation class backed off
    assert tr.graph is not None
    assert torch.isfinite(tr.flat_p).all()


def test_usrnet_x3_modelplain4_step():
    """define_Model('plain4') with netG.compute_dtype 'fp32x3' (as test_usrnet_modelplain4_step): the fused path, a
    captured graph, finite losses, parameters that move."""
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = {"model": "plain4", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 4, "path": {"models": "/tmp/k"},
           "netG": {"net_type": "usrnet", "n_iter": 2, "h_nc": 32, "in_nc": 4, "out_nc": 3, "nc": [16, 32, 64, 64],
                    "nb": 2, "act_mode": "R", "downsample_mode": "strideconv", "upsample_mode": "convtranspose",
                    "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 0.2, "compute_dtype": "fp32x3"},
           "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                     "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                     "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                     "G_scheduler_gamma": 0.5, "E_decay": 0, "G_param_strict": True, "E_param_strict": True}}
    model = define_Model(dict_to_nonedict(opt))
    model.init_train()
    g = torch.Generator().manual_seed(3)
    B = 2
    data = {"L": torch.rand(B, 3, 16, 16, generator=g), "H": torch.rand(B, 3, 64, 64, generator=g),
            "k": rand_kernel(B, 25, g).float(), "sf": torch.full((B, 1), 4), "sigma": torch.full((B, 1, 1, 1), 0.02)}
    before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    losses = []
    for step in range(3):
        model.feed_data(data)
        model.optimize_parameters(step)
        losses.append(model.log_dict["G_loss"])
    after = model.netG.state_dict()
    assert model.trainer is not None and model.trainer.graph is not None   # fused path, captured at step 3
    assert model.trainer.engine.x3 and model.trainer.range_guard and model.trainer.engine.x3_backoffs == 0
    assert all(torch.isfinite(torch.tensor(losses)))
    assert any((after[k] - before[k]).abs().max() > 0 for k in before)
