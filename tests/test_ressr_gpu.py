"""MSRResNet0, the DPSR prior and IMDN on the MI355X: ResSREngine against the float64 functional reference of
tests/test_ressr_cpu.py (written from the state_dict alone, not kair_amd's module), ModelPlain on the fused trainer
against a float64 Adam + EMA on that reference, eval forwards at odd sizes, and the checkpoint round trip.

Engine bars (tests/test_srmd_gpu.py's fp32 / bf16 pair, unchanged): fp32 output within 1e-4 relative (L2) of float64,
every parameter gradient within max(2e-3, 3 x the error of the same network in torch fp32), the fused loss within 1e-4;
bf16 output 2e-2, worst gradient 0.2, mean gradient 1.05e-1.  test_bf16_rounded_float64_reference_is_inside_the_bars
keeps a float64 forward / backward whose stored activations are rounded to bf16 under the same bars.  The fused-loss
tests put H at least 0.04 away from the float64 output, so that no |E - H| sits at L1's kink.  Each test prints its
figures (pytest -s).

Shapes: B 2, LR 12 x 10 (non-square, no tile multiple), nb 2; IMDN at nc 32 (d 8, r 24, K = 9 r = 216) and nc 64
(d 16, r 48, K 432): the channel-offset im2col reads whose K is no multiple of the K tile.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from test_ressr_cpu import ref_forward, sd_of  # noqa: E402

from kair_amd.models.network_dpsr import MSRResNet_prior  # noqa: E402
from kair_amd.models.network_imdn import IMDN  # noqa: E402
from kair_amd.models.network_msrresnet import MSRResNet0  # noqa: E402

dev = torch.device("cuda")
BF16_TOL = (2e-2, 0.2, 1.05e-1)   # output, worst gradient, mean gradient (tests/test_srmd_gpu.py)
F64 = torch.float64
B0, LH, LW = 2, 12, 10

CASES = {
    "msr_up2": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=2)),
    "msr_up4": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=4)),
    "msr_ps2": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=2, upsample_mode="pixelshuffle")),
    "msr_ps3": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=3, upsample_mode="pixelshuffle")),
    "msr_ps4": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=4, upsample_mode="pixelshuffle")),
    "msr_c1": (MSRResNet0, dict(in_nc=1, out_nc=1, nc=32, nb=2, upscale=2)),
    "dpsr": (MSRResNet_prior, dict(in_nc=4, out_nc=3, nc=96, nb=2, upscale=4)),
    "imdn32x2": (IMDN, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=2)),
    "imdn32x3": (IMDN, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=3)),
    "imdn32x4": (IMDN, dict(in_nc=3, out_nc=3, nc=32, nb=2, upscale=4)),
    "imdn64x4": (IMDN, dict(in_nc=3, out_nc=3, nc=64, nb=1, upscale=4)),
}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def build(name, **kw):
    cls, args = CASES[name]
    return cls(**args, **kw)


def grad_errs(grads, gref):
    return {k: ((a.detach().double().cpu() - gref[k].double()).norm() / gref[k].double().norm()).item()
            for k, a in grads.items()}


def _ref_run(net, sd, x, R=None, Himg=None, loss=None, dtype=F64, rnd=lambda t: t):
    """The functional reference in `dtype` -> (output, {key: gradient})."""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    out = ref_forward(net, p, x.to(dtype), rnd)
    if loss is None:
        (out * R.to(dtype)).sum().backward()
    elif loss == "l1":
        (out - Himg.to(dtype)).abs().mean().backward()
    else:
        ((out - Himg.to(dtype)) ** 2).mean().backward()
    return out.detach(), {k: v.grad.clone() for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(state_dict, x, R, Himg, float64 and torch-fp32 outputs / gradients for the three backward kinds): once."""
    torch.manual_seed(40 + len(name))
    net = build(name)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(41 + len(name))
    x = torch.rand(B0, net.in_nc, LH, LW, generator=g)
    if isinstance(net, MSRResNet_prior):
        x[:, -1:] = x[:, -1:, :1, :1] * (50 / 255)               # the level channel: constant per sample
    sf = net.upscale
    R = torch.randn(B0, net.out_nc, sf * LH, sf * LW, generator=g)
    with torch.no_grad():
        out64 = ref_forward(net, sd_of(net), x.double())
    off = torch.rand(out64.shape, generator=g, dtype=F64) * 0.45 + 0.05
    Himg = (out64 + off * torch.where(torch.rand(out64.shape, generator=g) < 0.5, -1.0, 1.0)).float()
    assert ((out64 - Himg.double()).abs() > 0.04).all()
    refs = {kind: (_ref_run(net, sd, x, R, Himg, kind), _ref_run(net, sd, x, R, Himg, kind, torch.float32))
            for kind in (None, "l1", "l2")}
    return sd, x, R, Himg, refs


def _engine_run(name, dt, kind):
    sd, x, R, Himg, refs = case_ref(name)
    (out64, g64), (_, g32) = refs[kind]
    net = build(name, compute_dtype=dt)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    if kind is None:   # autograd through net(x): backward_from_grad
        out = net(x.to(dev))
        (out * R.to(dev)).sum().backward()
        grads = {n: p.grad for n, p in net.named_parameters()}
    else:              # the fused pixel loss on the HR grid: backward_from_loss
        eng = net.engine()
        grads = {p: torch.zeros_like(p) for p in net.parameters()}
        out = eng.forward(x.to(dev), None).clone()
        loss = eng.backward_from_loss(Himg.to(dev), grads, 1.0, loss_type=kind)
        want = (out64 - Himg.double()).abs().mean() if kind == "l1" else ((out64 - Himg.double()) ** 2).mean()
        print(f"ressr {name} {dt} {kind}: loss {loss.item():.7e} float64 {want.item():.7e}")
        assert abs(loss.item() - want.item()) < (1e-4 if dt == "fp32" else 2e-2) * want.item()
        grads = {n: grads[p] for n, p in net.named_parameters()}
    assert out.shape == out64.shape and set(grads) == set(g64)
    e_out, errs, floor = rel(out, out64), grad_errs(grads, g64), grad_errs(g32, g64)
    print(f"ressr {name} {dt} {kind or 'autograd'}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad "
          f"{sum(errs.values()) / len(errs):.3e} (torch fp32 worst {max(floor.values()):.3e})")
    return e_out, errs, floor


@pytest.mark.parametrize("kind", [None, "l1", "l2"])
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_forward_and_gradients_vs_float64(name, kind):
    e_out, errs, floor = _engine_run(name, "fp32", kind)
    assert e_out < 1e-4
    bad = {k: (errs[k], floor[k]) for k in errs if errs[k] > max(2e-3, 3.0 * floor[k])}
    assert not bad, bad


@pytest.mark.parametrize("kind", [None, "l1", "l2"])
@pytest.mark.parametrize("name", list(CASES))
def test_bf16_forward_and_gradients_vs_float64(name, kind):
    """Measured on the MI355X: outputs 1.9e-3 .. 5.1e-3, worst gradients <= 0.153, mean gradients <= 9.6e-2; the
    tightest case is [msr_up4-None] (MSRResNet x4, the autograd kind: a unit-normal upstream gradient through two
    upsampling stages) at 4.1e-3 / 0.153 / 0.0959.  The float64 reference with bf16-rounded storage
    (test_bf16_rounded_float64_reference_is_inside_the_bars) lands at 4.05e-3 / 0.164 / 0.1038 for that case.  With
    plainly bf16-rounded weight packs the engine measured 5.3e-3 / 0.1995 / 0.1159 there, outside the mean bar: the
    reason the bf16 engine reads its weights as hi/lo pairs in the forward and input-gradient products."""
    e_out, errs, _ = _engine_run(name, "bf16", kind)
    assert e_out < BF16_TOL[0]
    bad = {k: e for k, e in errs.items() if e > BF16_TOL[1]}
    assert not bad, bad
    assert sum(errs.values()) / len(errs) < BF16_TOL[2]


class _RoundBF16(torch.autograd.Function):
    """bf16 storage of a float64 tensor: rounded on the way forward, its gradient rounded on the way back."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


@pytest.mark.parametrize("name", ["msr_up4", "msr_ps3", "msr_ps4", "dpsr", "imdn32x3", "imdn64x4"])
def test_bf16_rounded_float64_reference_is_inside_the_bars(name):
    sd, x, R, _, refs = case_ref(name)
    (out64, g64), _ = refs[None]
    out, grads = _ref_run(build(name), sd, x, R.double().bfloat16().double(), rnd=_RoundBF16.apply)
    errs, e_out = grad_errs(grads, g64), rel(out, out64)
    print(f"bf16-rounded float64 {name}: out {e_out:.3e} worst {max(errs.values()):.3e} mean {sum(errs.values()) / len(errs):.3e}")
    assert e_out < BF16_TOL[0] and max(errs.values()) < BF16_TOL[1] and sum(errs.values()) / len(errs) < BF16_TOL[2]


@pytest.mark.parametrize("name", ["msr_up2", "imdn32x2"])
def test_input_gets_no_gradient(name):
    net = build(name).to(dev).train()
    x = torch.rand(1, net.in_nc, 6, 6, device=dev, requires_grad=True)
    net(x).sum().backward()
    assert x.grad is None and all(p.grad is not None for p in net.parameters())


def _plan_tensors(P):
    for key, v in P.items():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if torch.is_tensor(t) and t.is_floating_point():
                yield t


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["msr_c1", "msr_ps3", "imdn32x3", "imdn64x4"])
@pytest.mark.parametrize("kind", ["grad", "l1"])
def test_padding_columns_survive_nan_filled_workspaces(name, dt, kind):
    """Rows of 1 / 3 channels in 8, 27 output columns in 32, the r columns behind d4 in the IMD block buffer, the r
    columns of the 1 x 1 input gradient: whatever a plan buffer held before, the forward and the backward write every
    column they later read."""
    sd, x, R, Himg, _ = case_ref(name)
    net = build(name, compute_dtype=dt)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    eng = net.engine()

    def run():
        grads = {p: torch.zeros_like(p) for p in net.parameters()}
        out = eng.forward(x.to(dev), None).clone()
        if kind == "grad":
            eng.backward_from_grad(R.to(dev), grads)
        else:
            eng.backward_from_loss(Himg.to(dev), grads, 1.0, loss_type="l1")
        return out, [grads[p].clone() for p in net.parameters()]

    out0, g0 = run()
    for t in _plan_tensors(eng.cur):
        t.fill_(float("nan"))
    out1, g1 = run()
    assert torch.isfinite(out1).all() and all(torch.isfinite(g).all() for g in g1)
    assert torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_engine_refuses_a_wrong_channel_count():
    net = build("imdn32x2").to(dev)
    with pytest.raises(ValueError, match="channels"):
        net.engine().forward(torch.rand(1, 4, 8, 8, device=dev), None)


# ---------------------------------------------------------------------------------------------------------------------
# inference helper, checkpoint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["msr_up2", "msr_up4", "msr_ps3", "msr_ps4", "dpsr", "imdn32x2", "imdn32x3", "imdn32x4",
                                  "imdn64x4"])
def test_eval_forward_odd_size_through_test_mode(name):
    from kair_amd.utils.utils_model import test_mode
    torch.manual_seed(31 + len(name))
    net = build(name)
    sd64 = sd_of(net)
    ref = lambda t: ref_forward(net, sd64, t)
    net = net.to(dev).eval()
    sf = net.upscale
    L = torch.rand(1, net.in_nc, 13, 11, generator=torch.Generator().manual_seed(32))
    with torch.no_grad():
        for mode in (0, 1, 2, 3):
            E = test_mode(net, L.to(dev), mode=mode, sf=sf, refield=4, min_size=8)
            want = test_mode(ref, L.double(), mode=mode, sf=sf, refield=4, min_size=8)
            assert E.shape == (1, net.out_nc, 13 * sf, 11 * sf) == want.shape
            assert rel(E, want) < 1e-4, (mode, rel(E, want))


@pytest.mark.parametrize("name", ["msr_up4", "imdn32x3"])
def test_checkpoint_round_trip(name, tmp_path):
    """A state_dict written by the CPU torch path loads strictly; ModelPlain.save / load returns the same network."""
    torch.manual_seed(33)
    net = build(name)
    sd64 = sd_of(net)
    torch.save(net.state_dict(), tmp_path / "net.pth")
    fresh = build(name)
    fresh.load_state_dict(torch.load(tmp_path / "net.pth"), strict=True)
    x = torch.rand(2, net.in_nc, 11, 14, device=dev)
    with torch.no_grad():
        a, b = net.to(dev).eval()(x), fresh.to(dev).eval()(x)
        want = ref_forward(net, sd64, x.double().cpu())
    assert a.shape == (2, net.out_nc, 11 * net.upscale, 14 * net.upscale) and torch.equal(a, b) and rel(a, want) < 1e-4
    model = _model(False, name=name, path=str(tmp_path))
    model.save(7)
    other = _model(False, name=name, path=str(tmp_path), seed=99)
    assert not torch.equal(other.netG.state_dict()["model.0.weight"], model.netG.state_dict()["model.0.weight"])
    other.load_network(str(tmp_path / "7_G.pth"), other.netG, strict=True)
    for k, v in model.netG.state_dict().items():
        assert torch.equal(other.netG.state_dict()[k], v), k


# ---------------------------------------------------------------------------------------------------------------------
# fused trainer
# ---------------------------------------------------------------------------------------------------------------------
def _opt(use_graph, clip, name, path):
    cls, a = CASES[name]
    t = {MSRResNet0: "msrresnet0", MSRResNet_prior: "dpsr", IMDN: "imdn"}[cls]
    return {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": a["upscale"], "path": {"models": path},
            "netG": {"net_type": t, "in_nc": a["in_nc"], "out_nc": a["out_nc"], "nc": a["nc"], "nb": a["nb"], "scale": a["upscale"],
                     "act_mode": "L" if cls is IMDN else "R",
                     "upsample_mode": "pixelshuffle" if cls is IMDN else a.get("upsample_mode", "upconv"),
                     "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 1.0},
            "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": clip,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                      "use_hip_graph": use_graph}}


def _model(use_graph, clip=None, name="imdn32x3", path="/tmp/k", seed=51):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(seed)
    model = define_Model(dict_to_nonedict(_opt(use_graph, clip, name, path)))
    model.init_train()
    return model


@pytest.mark.parametrize("use_graph,clip", [(True, None), (False, None), (True, 0.05)])
@pytest.mark.parametrize("name", ["imdn32x3", "msr_up2", "msr_ps3"])
def test_define_model_plain_step_vs_float64_adam(name, use_graph, clip):
    """define_Model('plain') trains on FusedTrainer: three steps (L1, Adam, EMA 0.999; one run clipped to a gradient
    norm the first steps exceed) against the float64 functional reference under torch.optim.Adam with the same EMA.
    Tolerances of tests/test_srmd_gpu.py::test_define_model_plain_step_vs_float64_adam."""
    from kair_amd.engine.ressr_engine import ResSREngine
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.models.model_plain import ModelPlain
    model = _model(use_graph, clip, name)
    assert type(model) is ModelPlain and isinstance(model.trainer, FusedTrainer)
    assert type(model.trainer.engine) is ResSREngine and model.trainer.engine.tdt == torch.float32
    net = model.netG
    keys = list(net.state_dict())
    p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    pe = {k: v.detach().clone() for k, v in p.items()}
    adam = torch.optim.Adam(list(p.values()), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(52)
    sf, norms = net.upscale, []
    for step in range(3):
        L, Hh = torch.rand(2, net.in_nc, 8, 6, generator=g), torch.rand(2, net.out_nc, 8 * sf, 6 * sf, generator=g)
        model.feed_data({"L": L, "H": Hh})
        model.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref_forward(net, p, L.double()) - Hh.double()).abs().mean()
        lo.backward()
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(p.values()), max_norm=clip, norm_type=2)))
        adam.step()
        with torch.no_grad():
            for k in keys:
                pe[k].mul_(0.999).add_(p[k], alpha=1 - 0.999)
        loss = model.log_dict["G_loss"]
        print(f"{name} graph {use_graph} clip {clip} step {step}: loss {loss:.7e} float64 {lo.item():.7e}")
        assert abs(loss - lo.item()) < 1e-4 * abs(lo.item()), (step, loss, lo.item())
    if clip:
        assert min(norms) > clip, norms                        # the clip was active
        assert abs(float(model.trainer.gnorm) - norms[-1]) < 1e-3 * norms[-1]
    assert (model.trainer.graph is not None) == use_graph
    for mine, theirs in ((model.netG, p), (model.netE, pe)):
        sd = mine.state_dict()
        assert list(sd) == keys
        for key in keys:
            assert rel(sd[key], theirs[key]) < (1e-3 if theirs[key].dim() == 1 else 1e-4), key


# ---------------------------------------------------------------------------------------------------------------------
# kair_synth_dpsr / PatchSynth(task="dpsr")
# ---------------------------------------------------------------------------------------------------------------------
def _pool(C=3):
    return torch.rand(4, C, 61, 54, generator=torch.Generator().manual_seed(91)).to(dev)


@pytest.mark.parametrize("sf,C", [(2, 3), (3, 3), (4, 3), (4, 1)])
def test_synth_dpsr_without_noise_is_task_sr(sf, C):
    from kair_amd.data.gpu_synth import PatchSynth
    pool = _pool(C)
    a = PatchSynth(pool, task="dpsr", scale=sf, H_size=24, sigma=(0, 0), seed=3)
    b = PatchSynth(pool, task="sr", scale=sf, H_size=24, seed=3)
    for _ in range(2):
        L = torch.full((9, C + 1, 24 // sf, 24 // sf), float("nan"), device=dev)
        Hh = torch.full((9, C, 24, 24), float("nan"), device=dev)
        a.next(9, out=(L, Hh))
        Ls, Hs = b.next(9)
        assert torch.equal(a.last_params[:, :4], b.last_params)
        assert torch.equal(L[:, :C], Ls) and torch.equal(Hh, Hs) and (L[:, C] == 0).all()


def test_synth_dpsr_levels_noise_statistics_and_determinism():
    from kair_amd.data.gpu_synth import PatchSynth
    pool = _pool()
    mk = lambda sigma, seed=3: PatchSynth(pool, task="dpsr", scale=2, H_size=48, sigma=sigma, seed=seed)
    B, ls = 12, 24
    s = mk((0, 50))
    L, Hh = s.next(B)
    L0, H0 = mk((0, 0)).next(B)
    lev = s.last_params[:, 4:5].view(torch.float32).flatten()
    assert L.shape == (B, 4, ls, ls) and torch.equal(Hh, H0)
    assert torch.equal(L[:, 3], lev.view(B, 1, 1).expand(B, ls, ls))          # constant per sample, the drawn level / 255
    assert ((lev >= 0) & (lev <= 50 / 255 + 1e-7)).all() and len(set(lev.tolist())) == B
    N = 3 * ls * ls
    big = [b for b in range(B) if lev[b] >= 5 / 255]
    assert len(big) >= 6
    for b in big:                                                             # bars from N alone: 5 sigma of the estimators
        n = ((L[b, :3] - L0[b, :3]).double() / lev[b].double()).flatten()
        print(f"dpsr noise sample {b}: level {lev[b].item() * 255:.2f} mean {n.mean().item():+.4f} std {n.std().item():.4f}")
        assert abs(n.mean().item()) < 5 / N ** 0.5 and abs(n.std().item() - 1) < 5 / (2 * N) ** 0.5
    L2, _ = mk((0, 50)).next(B)                                               # the same (seed, step): the same bytes
    assert torch.equal(L2, L)
    L3, _ = s.next(B)                                                         # another step: other noise
    t = mk((0, 50))
    t.step = 1
    L4, _ = t.next(B)                                                         # step 1 on the first batch's draws
    assert torch.equal(L4[:, 3], L[:, 3]) and not torch.equal(L4[:, :3], L[:, :3])
    assert ((L4[:, :3] - L0[:, :3]).abs().amax((1, 2, 3)) > 0).all()


def test_synth_dpsr_argument_errors():
    from kair_amd import _hip as H
    from kair_amd.utils import utils_image as util
    pool = torch.rand(2, 3, 32, 32, device=dev)
    par = torch.zeros(4, 8, dtype=torch.int32, device=dev)
    taps = lambda n, sf: tuple(t.to(dev) for t in util.bicubic_taps(n, n // sf, 1.0 / sf))
    th = taps(32, 2)
    Hp, Lp = torch.empty(4, 3, 24, 24, device=dev), torch.empty(4, 4, 12, 12, device=dev)
    H.synth_dpsr(pool, par, 4, 24, 2, th, th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="scale"):
        H.synth_dpsr(pool, par, 4, 24, 5, th, th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="scale"):
        H.synth_dpsr(pool, par, 4, 25, 2, th, th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="output"):
        H.synth_dpsr(pool, par, 4, 24, 2, th, th, 0, 0, Hp, Lp[:, :3].contiguous())
    with pytest.raises(ValueError, match="output"):
        H.synth_dpsr(pool, par, 4, 24, 2, th, th, 0, 0, Hp.double(), Lp)
    with pytest.raises(ValueError, match="params"):
        H.synth_dpsr(pool, par[:, :4].contiguous(), 4, 24, 2, th, th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="params"):
        H.synth_dpsr(pool, par.float(), 4, 24, 2, th, th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="taps"):
        H.synth_dpsr(pool, par, 4, 24, 2, taps(32, 4), th, 0, 0, Hp, Lp)
    with pytest.raises(ValueError, match="cropped to the scale"):
        H.synth_dpsr(pool[..., :31, :].contiguous(), par, 4, 24, 2, th, th, 0, 0, Hp, Lp)
    with pytest.raises(RuntimeError):
        H.synth_dpsr(pool.cpu(), par, 4, 24, 2, th, th, 0, 0, Hp, Lp)


def test_patch_synth_dpsr_feeds_the_fused_trainer():
    from kair_amd.data.gpu_synth import PatchSynth
    from kair_amd.engine.trainer import FusedTrainer
    import math
    synth = PatchSynth(_pool(), task="dpsr", scale=4, H_size=32, sigma=(0, 50), seed=0)
    model = _model(True, name="dpsr")
    for step in range(4):   # two eager steps, the capture, one replay
        d = synth.next_dict(4)
        assert set(d) == {"L", "H"} and d["L"].shape == (4, 4, 8, 8) and d["H"].shape == (4, 3, 32, 32)
        model.feed_data(d)
        model.optimize_parameters(step)
        assert math.isfinite(model.log_dict["G_loss"]) and 0 < model.log_dict["G_loss"] < 2.0
    assert isinstance(model.trainer, FusedTrainer) and model.trainer.graph is not None
    assert all(torch.isfinite(p).all() for p in model.netG.parameters())
