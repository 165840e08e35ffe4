"""Gradient-norm clipping inside the fused step (G_optimizer_clipgrad) and the l2 / l2sum losses on the trainer, on the
MI355X: kair_grad_norm against the float64 norm, kair_adam_ema_clip against kair_adam_ema_ex, and FusedTrainer /
ModelPlain steps.

Bars.
  kair_grad_norm: (c + 2) * 2^-24 relative, c the longest fp32 addition chain of the kernel at that n, from the
  exported geometry (chain()): the worst case of a sum of non-negative terms is one 2^-24 per addition on the path
  plus one for the squares; the square root halves the relative error and adds one rounding, the last sum is in
  double.  c <= 64 at the sizes here is a condition on the kernel (a fixed grid of many short chains), not a measurement.
  kair_adam_ema_clip, clipping: against kair_adam_ema_ex fed g * coef (coef by torch in fp32 on the device): g within
  2 ulp, m within 4 * 2^-24 and v within 8 * 2^-24 relative, p and ema within one fp32 ulp.
  Fused steps: m = (1 - beta1) coef g and v = (1 - beta2) (coef g)^2 of the first step, with the betas the fp32 numbers
  the kernel receives, at the same Adam bars; l2 value at the kernel test's value bar (tests/test_l2_loss_gpu.py
  value_bar, scaled by |weight| and numel).
  Fused against the autograd path: 2 x what the same comparison shows with Charbonnier and no clipping in the same
  test, never below one rounding of dE in the engine's row dtype (2^-20 fp32 / fp32x3, 2^-8 bf16).
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from test_l2_loss_gpu import value_bar  # noqa: E402
from test_ssim_loss_gpu import _batch, _dncnn, _swinir  # noqa: E402

dev = torch.device("cuda")
U = 2.0 ** -24
B1, B2 = 0.9, 0.999
B1F, B2F = float(np.float32(B1)), float(np.float32(B2))   # the betas as the kernels receive them


def chain(n):
    """The longest fp32 addition chain of kair_grad_norm over n values (16-byte aligned): 2 inside a float4, one per
    float4 of the thread, one tail element, the tree over the workgroup."""
    grid, block, _ = H.grad_norm_geometry()
    per_thread = -(-(n // 4) // (grid * block))
    return 2 + per_thread + 1 + int(math.log2(block))


def ulp(x):
    """The spacing of fp32 at |x| (elementwise)."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def norm_of(g, ws=None):
    out = torch.full((1,), float("nan"), device=dev)
    ws = torch.empty(H.grad_norm_geometry()[2], device=dev) if ws is None else ws
    H.grad_norm(g, ws, out)
    torch.cuda.synchronize()
    return out.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# kair_grad_norm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4099, 1_000_003])
def test_grad_norm(n):
    """Measured on the MI355X (|norm - float64| / float64 in units of 2^-24, without / with the 1e3 element; the bar
    c + 2 is 13 / 14 / 14): n 1: 0 / 0; n 4099: 0.22 / 0.03; n 1,000,003: 0.25 / 0.20."""
    c = chain(n)
    assert c <= 64, c
    gen = torch.Generator().manual_seed(n)
    g = (torch.randn(n, generator=gen) * 1e-3).to(dev)
    for spike in (False, True):
        if spike:
            g[n // 2] = 1e3
        ref = g.double().cpu().norm().item()
        a, b = norm_of(g), norm_of(g)
        err = abs(a.item() - ref) / ref
        print(f"grad_norm n {n} spike {spike}: {a.item():.9g} vs {ref:.9g}, err {err / U:.3g} x 2^-24 (bar {c + 2})")
        assert err <= (c + 2) * U
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert norm_of(torch.zeros(n, device=dev)).item() == 0.0
    # a misaligned view (element by element): the same bar with its own chain, n / (grid * block) per thread
    if n == 4099:
        grid, block, _ = H.grad_norm_geometry()
        v = g[1:]
        cv = -(-(n - 1) // (grid * block)) + int(math.log2(block))
        ref = v.double().cpu().norm().item()
        assert abs(norm_of(v).item() - ref) <= (cv + 2) * U * ref


def test_grad_norm_workspace_is_what_the_query_says():
    grid, block, nws = H.grad_norm_geometry()
    assert nws == grid
    buf = torch.full((nws + 1024,), 1234.5, device=dev)
    g = torch.randn(100_003, device=dev)
    out = norm_of(g, buf[:nws])
    assert (buf[nws:] == 1234.5).all()
    assert abs(out.item() - g.double().norm().item()) <= (chain(g.numel()) + 2) * U * out.item()
    with pytest.raises(ValueError):
        H.grad_norm(g, buf[:nws - 1], torch.empty(1, device=dev))


# ---------------------------------------------------------------------------------------------------------------------
# kair_adam_ema_clip
# ---------------------------------------------------------------------------------------------------------------------
def _adam_state(n=4099):
    gen = torch.Generator().manual_seed(77)
    r = lambda s: (torch.randn(n, generator=gen) * s).to(dev)
    return {"p": r(0.1), "g": r(1e-2), "m": r(1e-3), "v": r(1e-3).abs() * 1e-2, "ema": r(0.1)}


def _adam(st, lr_t, gnorm=None, max_norm=None, skip=None, wd=0.0):
    s = {k: v.clone() for k, v in st.items()}
    n = s["p"].numel()
    if gnorm is None:
        H.adam_ema(s["p"], s["g"], s["m"], s["v"], s["ema"], n, lr_t, B1, B2, 1e-8, wd, 0.999,
                   skip=torch.zeros(1, dtype=torch.int32, device=dev) if skip is None else skip)   # kair_adam_ema_ex
    else:
        H.adam_ema_clip(s["p"], s["g"], s["m"], s["v"], s["ema"], n, lr_t, B1, B2, 1e-8, wd, 0.999, gnorm, max_norm,
                        skip=skip)
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_ema_clip_against_adam_ema_ex(wd):
    st = _adam_state()
    lr_t = torch.tensor([2e-4 / (1 - B1 ** 3), math.sqrt(1 - B2 ** 3)], device=dev)
    max_norm = 0.25
    # no clipping: bit-equal to kair_adam_ema_ex, g untouched
    ref = _adam(st, lr_t, wd=wd)
    for flag in (None, torch.zeros(1, dtype=torch.int32, device=dev)):
        got = _adam(st, lr_t, torch.tensor([0.5 * max_norm], device=dev), max_norm, skip=flag, wd=wd)
        for k in st:
            assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), k
        assert torch.equal(got["g"], st["g"])
    # clipping
    gnorm = torch.tensor([4 * max_norm], device=dev)
    coef = (torch.tensor([max_norm], device=dev) / (gnorm + 1e-6)).clamp(max=1.0)
    assert 0.24 < coef.item() < 0.26
    fed = dict(st, g=st["g"] * coef)
    ref = _adam(fed, lr_t, wd=wd)
    got = _adam(st, lr_t, gnorm, max_norm, wd=wd)
    d = lambda k: (got[k].double() - ref[k].double()).abs()
    print("adam_ema_clip vs adam_ema_ex(g coef): worst differences g %.3g ulp, m %.3g, v %.3g x 2^-24 rel, p %.3g, ema %.3g ulp"
          % ((d("g") / ulp(ref["g"])).max().item(), (d("m") / ref["m"].double().abs()).max().item() / U,
             (d("v") / ref["v"].double().abs()).max().item() / U, (d("p") / ulp(ref["p"])).max().item(),
             (d("ema") / ulp(ref["ema"])).max().item()))
    assert (d("g") <= 2 * ulp(ref["g"])).all()
    assert not torch.equal(got["g"], st["g"])
    assert (d("m") <= 4 * U * ref["m"].double().abs()).all()
    assert (d("v") <= 8 * U * ref["v"].double().abs()).all()
    assert (d("p") <= ulp(ref["p"])).all()
    assert (d("ema") <= ulp(ref["ema"])).all()
    # a flagged step: nothing changes, g included
    got = _adam(st, lr_t, gnorm, max_norm, skip=torch.ones(1, dtype=torch.int32, device=dev), wd=wd)
    for k in st:
        assert torch.equal(got[k].view(torch.int32), st[k].view(torch.int32)), k
    with pytest.raises(RuntimeError, match="adam_ema_clip"):
        _adam(st, lr_t, gnorm, 0.0)
    with pytest.raises(RuntimeError, match="adam_ema_clip"):
        H.adam_ema_clip(st["p"], st["g"], st["m"], st["v"], st["ema"], 8, lr_t, B1, B2, 1e-8, 0.0, 0.999, None, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the fused step
# ---------------------------------------------------------------------------------------------------------------------
NETS = [("dncnn", "fp32"), ("dncnn", "bf16"), ("swinir", "fp32x3")]


def _mk(kind, dt):
    return functools.partial(_dncnn if kind == "dncnn" else _swinir, dt)


@functools.lru_cache(maxsize=None)
def _state(kind, dt):
    torch.manual_seed(21)
    return copy.deepcopy(_mk(kind, dt)().state_dict())


def _trainer(kind, dt, use_graph=False, **kw):
    net = _mk(kind, dt)()
    net.load_state_dict(_state(kind, dt))
    return FusedTrainer(net.to(dev).train(), None, lr=1e-4, E_decay=0, betas=(B1, B2), use_graph=use_graph, **kw)


def _steps(tr, L, Ht, n):
    losses = [tr.step(L, Ht).clone() for _ in range(n)]
    tr.check_range()
    torch.cuda.synchronize()
    assert not tr.range_events
    return torch.cat(losses).cpu()


@functools.lru_cache(maxsize=None)
def _twin_first_step(kind, dt, loss_type=None):
    """The unclipped trainer's first step: (flat gradient on the CPU, its float64 norm, loss).  Computed once."""
    tr = _trainer(kind, dt, loss_type=loss_type)
    loss = _steps(tr, *_batch(kind), 1)
    g = tr.flat_g.detach().cpu().clone()
    return g, g.double().norm().item(), loss.item()


@pytest.mark.parametrize("kind,dt", NETS)
def test_max_norm_1e30_is_the_trainer_without_clipping(kind, dt):
    L, Ht = _batch(kind)
    for use_graph in (False, True):
        a = _trainer(kind, dt, use_graph=use_graph)
        b = _trainer(kind, dt, use_graph=use_graph, clip_grad=1e30)
        la, lb = _steps(a, L, Ht, 3), _steps(b, L, Ht, 3)
        assert (b.graph is not None) == use_graph
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
        assert torch.equal(a.flat_p.view(torch.int32), b.flat_p.view(torch.int32))
        assert torch.equal(a.m.view(torch.int32), b.m.view(torch.int32))
        assert a.gnorm is None and b.gnorm.shape == (1,) and b.gnorm.item() > 0


@pytest.mark.parametrize("kind,dt", NETS)
def test_clipped_first_step(kind, dt):
    """max_norm = half the first step's norm (from the twin run without clipping): the norm, the written-back gradient
    and Adam's moments show the clip (m and v; the first parameter update is all but invariant to the gradient's scale).
    Measured on the MI355X (gnorm error in 2^-24 relative, bar 14; g in ulp, bar 2; m, v in 2^-24 relative, bars 4, 8):
        dncnn fp32 (75,073 parameters)     0.01 / 0 / 0.95 / 1.92
        dncnn bf16                         0.73 / 0 / 0.95 / 1.94
        swinir fp32x3 (134,952)            0.24 / 0 / 0.95 / 1.94"""
    g0, n64, _ = _twin_first_step(kind, dt)
    max_norm = 0.5 * n64
    tr = _trainer(kind, dt, clip_grad=max_norm)
    _steps(tr, *_batch(kind), 1)
    n = g0.numel()
    gn = tr.gnorm.cpu()
    assert tr.gnorm.shape == (1,) and tr.gnorm.device.type == "cuda"
    e_n = abs(gn.item() - n64) / n64
    assert e_n <= (chain(n) + 2) * U, (gn.item(), n64)
    coef = (torch.tensor([max_norm], dtype=torch.float32) / (gn + 1e-6)).clamp(max=1.0)   # fp32, as the kernel
    assert 0.49 < coef.item() < 0.51
    want = (g0 * coef).double()
    got = tr.flat_g.cpu().double()
    e_g = ((got - want).abs() / ulp(want)).max().item()
    m_ref, v_ref = (1 - B1F) * want, (1 - B2F) * want * want
    nz = want != 0
    e_m = ((tr.m.cpu().double() - m_ref).abs()[nz] / m_ref.abs()[nz]).max().item() / U
    e_v = ((tr.v.cpu().double() - v_ref).abs()[nz] / v_ref.abs()[nz]).max().item() / U
    print(f"clipped first step {kind} {dt}: n {n} gnorm err {e_n / U:.3g} (bar {chain(n) + 2}) g {e_g:.3g} ulp, "
          f"m {e_m:.3g} v {e_v:.3g} x 2^-24")
    assert e_g <= 2
    assert ((tr.m.cpu().double() - m_ref).abs() <= 4 * U * m_ref.abs()).all()
    assert ((tr.v.cpu().double() - v_ref).abs() <= 8 * U * v_ref.abs()).all()


@pytest.mark.parametrize("kind,dt", NETS)
def test_clipped_steps_eager_equal_graph(kind, dt):
    _, n64, _ = _twin_first_step(kind, dt)
    L, Ht = _batch(kind)
    runs = []
    for use_graph in (False, True):
        tr = _trainer(kind, dt, use_graph=use_graph, clip_grad=0.5 * n64)
        losses = _steps(tr, L, Ht, 3)
        assert (tr.graph is not None) == use_graph
        runs.append((losses, tr.flat_p.cpu().clone(), tr.gnorm.cpu().clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert torch.equal(runs[0][2], runs[1][2]) and math.isfinite(runs[0][2].item())


@pytest.mark.parametrize("kind,dt", NETS)
def test_l2_and_l2sum_first_step(kind, dt):
    """l2: the loss is weight * mean((E - H)^2) of the engine's own forward output.  l2sum: numel x the l2 loss of the
    same forward, and numel x its flat gradient: 8 * 2^-24 in the relative 2-norm on the fp32 engine (the two runs
    round dE against different constants, every sum after that is the same), one dE rounding of the row dtype on the
    others (2^-20 fp32x3, 2^-8 bf16).
    Measured on the MI355X (weight 0.5: |l2 - float64| (bar 1.05e-8); |l2sum - numel x float64| (bar numel x that:
    1.2e-5 dncnn, 6.5e-5 swinir); gradient, relative 2-norm (bar)):
        dncnn fp32      2.1e-10 / 1.2e-7 / 4.28e-7 (4.77e-7)
        dncnn bf16      3.7e-10 / 1.3e-7 / 1.5e-3 (3.9e-3)
        swinir fp32x3   4.2e-9  / 2.6e-5 / 3.1e-7 (9.5e-7)"""
    L, Ht = _batch(kind)
    w = 0.5
    out = {}
    for lt in ("l2", "l2sum"):
        tr = _trainer(kind, dt, loss_type=lt, loss_weight=w)
        loss = _steps(tr, L, Ht, 1).item()
        E = tr.engine.cur["E"].detach().double().cpu().view(Ht.shape)
        out[lt] = (loss, tr.flat_g.cpu().double().clone(), E)
    numel = Ht.numel()
    assert torch.equal(out["l2"][2], out["l2sum"][2])
    mean64 = ((out["l2"][2] - Ht.double().cpu()) ** 2).mean().item()
    e1 = abs(out["l2"][0] - w * mean64)
    e2 = abs(out["l2sum"][0] - numel * w * mean64)
    e3 = abs(out["l2sum"][0] - numel * out["l2"][0])
    bar = value_bar() * w
    gs, gm = out["l2sum"][1], numel * out["l2"][1]
    eg = ((gs - gm).norm() / gs.norm()).item()
    gbar = {"fp32": 8 * U, "fp32x3": 2.0 ** -20, "bf16": 2.0 ** -8}[dt]
    print(f"l2 / l2sum first step {kind} {dt}: l2 {out['l2'][0]:.8g} err {e1:.3g} (bar {bar:.3g}); l2sum err {e2:.3g}, "
          f"vs numel x l2 {e3:.3g} (bar {numel * bar:.3g}); gradient {eg:.3g} (bar {gbar:.3g})")
    assert gs.abs().max() > 0 and torch.isfinite(gs).all()
    assert e1 <= bar
    assert e2 <= numel * bar and e3 <= numel * bar
    assert eg <= gbar


# ---------------------------------------------------------------------------------------------------------------------
# ModelPlain: fused against use_fused_trainer false
# ---------------------------------------------------------------------------------------------------------------------
def _opt(kind, dt, train):
    if kind == "dncnn":
        netG = {"net_type": "dncnn", "in_nc": 1, "out_nc": 1, "nc": 64, "nb": 4, "act_mode": "R",
                "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 0.2, "compute_dtype": dt}
    else:
        netG = {"net_type": "swinir", "upscale": 2, "in_chans": 3, "img_size": 16, "window_size": 8, "img_range": 1.0,
                "depths": [2], "embed_dim": 60, "num_heads": [6], "mlp_ratio": 2, "upsampler": "pixelshuffledirect",
                "resi_connection": "1conv", "init_type": "default", "compute_dtype": dt}
    return {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1 if kind == "dncnn" else 2,
            "path": {"models": "/tmp/k"}, "netG": netG,
            "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                      "use_hip_graph": False, **train}}


def _model_step(kind, dt, state, train):
    """One optimize_parameters of a define_Model model from `state` -> (model, loss, flat gradient)."""
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    model = define_Model(dict_to_nonedict(_opt(kind, dt, train)))
    model.init_train()
    if state is not None:
        model.get_bare_model(model.netG).load_state_dict(state)
    sd = copy.deepcopy(model.get_bare_model(model.netG).state_dict())
    L, Ht = _batch(kind)
    model.feed_data({"L": L, "H": Ht})
    model.optimize_parameters(1)
    if model.trainer is not None:
        g = model.trainer.flat_g.detach().clone()
    else:
        g = torch.cat([p.grad.reshape(-1) for p in model.netG.parameters()])
    torch.cuda.synchronize()
    assert sorted(model.log_dict) == ["G_loss"]   # the reference's keys: no norm is logged
    return model, sd, model.log_dict["G_loss"], g.double().cpu()


def _fused_vs_autograd(kind, dt, train):
    mf, sd, lf, gf = _model_step(kind, dt, None, train)
    ma, _, la, ga = _model_step(kind, dt, sd, {**train, "use_fused_trainer": False})
    return mf, ma, abs(lf - la) / abs(la), ((gf - ga).norm() / ga.norm()).item()


@pytest.mark.parametrize("kind,dt", NETS)
def test_model_plain_fused_l2_clip_against_the_autograd_path(kind, dt):
    """G_lossfn_type 'l2' with G_optimizer_clipgrad at half the first gradient norm, through define_Model: the fused
    trainer (loss kernel rows, clip inside the step, clipped gradient written back) against use_fused_trainer false
    (nn.MSELoss, autograd, clip_grad_norm_).  The two paths round dE in different kernels.
    Measured on the MI355X (relative loss difference / relative 2-norm of the gradient difference; Charbonnier without
    clipping -> l2 with clipping; bars):
        dncnn fp32      0 / 9.3e-7 -> 0 / 9.2e-8    (9.5e-7 / 1.9e-6)
        dncnn bf16      0 / 0      -> 0 / 0         (3.9e-3 / 3.9e-3)
        swinir fp32x3   0 / 6.9e-8 -> 0 / 6.7e-8    (9.5e-7 / 9.5e-7)"""
    torch.manual_seed(33)
    mf, ma, cl, cg = _fused_vs_autograd(kind, dt, {"G_lossfn_type": "charbonnier", "G_charbonnier_eps": 1e-6})
    assert isinstance(mf.trainer, FusedTrainer) and mf.trainer.clip_grad is None and ma.trainer is None
    torch.manual_seed(33)
    m0, _, _, g0 = _model_step(kind, dt, None, {"G_lossfn_type": "l2"})
    assert isinstance(m0.trainer, FusedTrainer) and m0.trainer.loss_type == "l2"
    clip = 0.5 * g0.norm().item()
    torch.manual_seed(33)
    mf, ma, ll, lg = _fused_vs_autograd(kind, dt, {"G_lossfn_type": "l2", "G_optimizer_clipgrad": clip})
    assert isinstance(mf.trainer, FusedTrainer) and mf.trainer.clip_grad == clip and mf.trainer.loss_type == "l2"
    assert ma.trainer is None
    assert mf.trainer.gnorm.item() > clip   # it clipped
    floor = 2.0 ** -8 if dt == "bf16" else 2.0 ** -20
    bl, bg = max(2 * cl, floor), max(2 * cg, floor)
    print(f"fused vs autograd {kind} {dt}: charbonnier loss {cl:.3g} grad {cg:.3g}; l2 + clip loss {ll:.3g} grad {lg:.3g} "
          f"(bars {bl:.3g} / {bg:.3g})")
    assert ll <= bl
    assert lg <= bg
    # the written-back gradient has the clipped norm max_norm * gnorm / (gnorm + 1e-6)
    gn = mf.trainer.gnorm.item()
    assert abs(mf.trainer.flat_g.double().norm().item() - clip * gn / (gn + 1e-6)) <= 1e-5 * clip


# ---------------------------------------------------------------------------------------------------------------------
# fp32x3 range guard with clipping
# ---------------------------------------------------------------------------------------------------------------------
def test_x3_range_guard_with_clipping():
    """tests/test_x3_range_gpu.py's scaled-input case (patches x 1e4: 2^4 x 1e4 > 65504 in conv_first's split operand)
    with clip_grad set: the flagged step is skipped (its norm is not finite, nothing is read from it), the exponents
    drop, the step is re-run; parameters stay finite and the steps after the re-run have a finite norm."""
    from test_x3_range_gpu import _pair
    net, ema, _, _ = _pair()
    tr = FusedTrainer(net, ema, lr=2e-4, E_decay=0.999, use_graph=True, clip_grad=1.0)
    p0 = tr.flat_p.clone()
    g = torch.Generator().manual_seed(22)
    norms = []
    for _ in range(4):   # 2 eager warm-up steps, then graph capture + replay
        L = torch.rand(2, 3, 16, 16, generator=g) * 1e4
        Hh = torch.rand(2, 3, 32, 32, generator=g) * 1e4
        loss = tr.step(L.to(dev), Hh.to(dev))
        tr.check_range()
        norms.append(tr.gnorm.item())
        assert math.isfinite(loss.item())
    assert tr.range_events and tr.range_events[0][0] == 1, tr.range_events
    assert tr.graph is not None
    assert all(math.isfinite(v) and v > 0 for v in norms), norms
    assert torch.isfinite(tr.flat_p).all() and torch.isfinite(tr.flat_e).all()
    assert not torch.equal(tr.flat_p, p0)
    assert torch.isfinite(tr.m).all() and torch.isfinite(tr.v).all()
