"""SRMD on the MI355X: SRMDEngine (DnCNN's step program with a 24-channel head and a 16 / 32 / 48-column PixelShuffle
tail) against a float64 plain-torch nn.Sequential loaded from the module's state_dict, ModelPlain on the fused trainer
against float64 Adam + EMA, the kernel / code launch (kair_srmd_kernels) and the batch launch (kair_synth_srmd) against
the float64 host maths of utils_sisr, and PatchSynth(task="srmd").

Engine bars (tests/test_ffdnet_gpu.py's fp32 / bf16 pair): fp32 output within 1e-4 relative (L2) of float64, every
parameter gradient within max(2e-3, 3 x the error of torch's own fp32 run); bf16 output 2e-2, worst gradient 0.2, mean
gradient 1.05e-1.  test_bf16_rounded_float64_reference_is_inside_the_bars keeps a float64 forward / backward whose
input, activations and output gradient are rounded to bf16 -- the storage the bf16 engine has -- under the same bars.
The fused-loss tests put H at least 0.05 away from the float64 output, so that no |E - H| sits at L1's kink, where a
float64 reference of the gradient's sign means nothing.

Synthesis bar: TOL of tests/test_usrnet_data_gpu.py (4e-5, the circular blur against float64) plus the bicubic bar of
tests/test_data_gpu.py (2e-6), summed: 4.2e-5.  Measured on the MI355X: at most 3.5e-7 over the cases of
test_synth_noise_off_vs_float64; the delta-kernel L is within 1.8e-7 of task "sr"'s (bit-equal at augment mode 0);
kair_srmd_kernels 2.6e-8 on the kernels and 4.5e-8 on the codes; engine fp32 outputs <= 3e-7, bf16 outputs <= 2.6e-3
with worst / mean gradient errors <= 0.17 / 0.077.  Each test prints its figures (pytest -s).
"""
import functools
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, _table  # noqa: E402
from kair_amd.models.network_srmd import SRMD  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_sisr as sisr  # noqa: E402

dev = torch.device("cuda")
BF16_TOL = (2e-2, 0.2, 1.05e-1)   # output, worst gradient, mean gradient (tests/test_ffdnet_gpu.py)
SYNTH_TOL = 4e-5 + 2e-6
F64 = torch.float64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def ref_net(in_nc, out_nc, nc, nb, sf):
    mods = [nn.Conv2d(in_nc, nc, 3, 1, 1), nn.ReLU()]
    for _ in range(nb - 2):
        mods += [nn.Conv2d(nc, nc, 3, 1, 1), nn.ReLU()]
    return nn.Sequential(*mods, nn.Conv2d(nc, out_nc * sf * sf, 3, 1, 1), nn.PixelShuffle(sf))


def twin(net, dtype=F64):
    ref = ref_net(net.in_nc, net.out_nc, net.model[0].out_channels, (len(net.model) - 1) // 2 + 1, net.upscale).to(dtype)
    ref.load_state_dict({k[len("model."):]: v.detach().to(dtype).cpu() for k, v in net.state_dict().items()}, strict=True)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the engine against float64
# ---------------------------------------------------------------------------------------------------------------------
# (C, sf, noise channel): Cop 16 / 32 / 48, the r = 3 padding columns (27 of 32, 9 of 16), and one C + 15 input
CASES = {"c3x2": (3, 2, True), "c3x3": (3, 3, True), "c3x4": (3, 4, True), "c1x3": (1, 3, True), "c3x4nf": (3, 4, False)}
NC, NB, B0, LH, LW = 32, 4, 2, 12, 10


def grad_errs(grads, gref):
    return {k: ((a.detach().double().cpu() - gref[k].double()).norm() / gref[k].double().norm()).item()
            for k, a in grads.items()}


def _ref_run(ref, x, R=None, Himg=None, loss=None):
    dt = next(ref.parameters()).dtype
    for p in ref.parameters():
        p.grad = None
    out = ref(x.to(dt))
    if loss is None:
        (out * R.to(dt)).sum().backward()
    elif loss == "l1":
        (out - Himg.to(dt)).abs().mean().backward()
    else:
        ((out - Himg.to(dt)) ** 2).mean().backward()
    return out.detach(), {"model." + n: p.grad.clone() for n, p in ref.named_parameters()}


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(state_dict, x, R, Himg, float64 and torch-fp32 outputs / gradients for the three backward kinds): once."""
    C, sf, noise = CASES[name]
    in_nc = C + 15 + int(noise)
    torch.manual_seed(40 + len(name) + sf)
    net = SRMD(in_nc, C, NC, NB, sf)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(41 + sf)
    x = torch.rand(B0, in_nc, LH, LW, generator=g)
    x[:, C:] = x[:, C:, :1, :1]                                 # map channels: constant per sample
    R = torch.randn(B0, C, sf * LH, sf * LW, generator=g)
    r64, r32 = twin(net), twin(net, torch.float32)
    out64 = r64(x.double()).detach()
    off = torch.rand(out64.shape, generator=g, dtype=F64) * 0.45 + 0.05
    Himg = (out64 + off * torch.where(torch.rand(out64.shape, generator=g) < 0.5, -1.0, 1.0)).float()
    assert ((out64 - Himg.double()).abs() > 0.04).all()
    refs = {kind: (_ref_run(r64, x, R, Himg, kind), _ref_run(r32, x, R, Himg, kind)) for kind in (None, "l1", "l2")}
    return sd, x, R, Himg, refs


def _engine_run(name, dt, kind):
    C, sf, noise = CASES[name]
    sd, x, R, Himg, refs = case_ref(name)
    (out64, g64), (_, g32) = refs[kind]
    net = SRMD(C + 15 + int(noise), C, NC, NB, sf, compute_dtype=dt)
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
        assert abs(loss.item() - want.item()) < (1e-4 if dt == "fp32" else 2e-2) * want.item()
        grads = {n: grads[p] for n, p in net.named_parameters()}
    assert out.shape == out64.shape
    e_out, errs, floor = rel(out, out64), grad_errs(grads, g64), grad_errs(g32, g64)
    print(f"srmd {name} {dt} {kind or 'autograd'}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad "
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


@pytest.mark.parametrize("name", ["c3x3", "c3x4"])
def test_bf16_rounded_float64_reference_is_inside_the_bars(name):
    sd, x, R, _, refs = case_ref(name)
    (out64, g64), _ = refs[None]
    C, sf, noise = CASES[name]
    ref = twin(SRMD(C + 15 + int(noise), C, NC, NB, sf))
    ref.load_state_dict({k[len("model."):]: v.double() for k, v in sd.items()}, strict=True)
    h = _RoundBF16.apply(x.double())
    for m in ref:
        h = m(h)
        if isinstance(m, nn.ReLU):
            h = _RoundBF16.apply(h)
    (h * R.double().bfloat16().double()).sum().backward()
    errs = grad_errs({"model." + n: p.grad for n, p in ref.named_parameters()}, g64)
    e_out = rel(h, out64)
    print(f"bf16-rounded float64 {name}: out {e_out:.3e} worst {max(errs.values()):.3e} mean {sum(errs.values()) / len(errs):.3e}")
    assert e_out < BF16_TOL[0] and max(errs.values()) < BF16_TOL[1] and sum(errs.values()) / len(errs) < BF16_TOL[2]


def test_input_gets_no_gradient():
    net = SRMD(19, 3, 16, 3, 2).to(dev).train()
    x = torch.rand(1, 19, 6, 6, device=dev, requires_grad=True)
    net(x).sum().backward()
    assert x.grad is None and all(p.grad is not None for p in net.parameters())


def _plan_tensors(P):
    for key, v in P.items():
        if key == "x":   # the caller's input, not a workspace
            continue
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if torch.is_tensor(t) and t.is_floating_point():
                yield t


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["c3x3", "c1x3", "c3x4"])
@pytest.mark.parametrize("kind", ["grad", "l1"])
def test_padding_columns_survive_nan_filled_workspaces(name, dt, kind):
    """Rows of 19 channels in 24, 27 output columns in 32 (9 in 16): whatever a plan buffer held before, the forward and
    the backward write every column they later read."""
    C, sf, noise = CASES[name]
    sd, x, R, Himg, _ = case_ref(name)
    net = SRMD(C + 16, C, NC, NB, sf, compute_dtype=dt)
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


# ---------------------------------------------------------------------------------------------------------------------
# inference helper, checkpoint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", [2, 3, 4])
def test_eval_forward_odd_size_through_test_mode(sf):
    from kair_amd.utils.utils_model import test_mode
    torch.manual_seed(31 + sf)
    net = SRMD(19, 3, 16, 4, sf)
    ref = twin(net).eval()
    net = net.to(dev).eval()
    L = torch.rand(1, 19, 13, 9, generator=torch.Generator().manual_seed(32))
    L[:, 3:] = L[:, 3:, :1, :1]
    with torch.no_grad():
        for mode in (0, 3):
            E = test_mode(net, L.to(dev), mode=mode, sf=sf)
            want = test_mode(ref, L.double(), mode=mode, sf=sf)
            assert E.shape == (1, 3, 13 * sf, 9 * sf) == want.shape
            assert rel(E, want) < 1e-4, (mode, rel(E, want))


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(33)
    net = SRMD(19, 3, 16, 3, 3)
    assert list(net.state_dict()) == [f"model.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    torch.save(net.state_dict(), tmp_path / "srmd.pth")
    fresh = SRMD(19, 3, 16, 3, 3)
    fresh.load_state_dict(torch.load(tmp_path / "srmd.pth"), strict=True)
    x = torch.rand(2, 19, 11, 14, device=dev)
    with torch.no_grad():
        a, b = net.to(dev).eval()(x), fresh.to(dev).eval()(x)
    assert a.shape == (2, 3, 33, 42) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# fused trainer
# ---------------------------------------------------------------------------------------------------------------------
def _opt(use_graph, clip=None, sf=3, **netg):
    o = {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": sf, "path": {"models": "/tmp/k"},
         "netG": {"net_type": "srmd", "in_nc": 19, "out_nc": 3, "nc": 16, "nb": 4, "scale": sf, "act_mode": "R",
                  "upsample_mode": "pixelshuffle", "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 1.0},
         "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                   "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": clip,
                   "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                   "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                   "use_hip_graph": use_graph}}
    o["netG"].update(netg)
    return o


def _model(use_graph, clip=None, **netg):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(51)
    model = define_Model(dict_to_nonedict(_opt(use_graph, clip, **netg)))
    model.init_train()
    return model


@pytest.mark.parametrize("use_graph,clip", [(True, None), (False, None), (True, 0.05)])
def test_define_model_plain_step_vs_float64_adam(use_graph, clip):
    """define_Model('plain') trains SRMD on FusedTrainer: three steps (L1, Adam, EMA 0.999; one run clipped to a
    gradient norm the first steps exceed) against the float64 reference under torch.optim.Adam with the same EMA.
    Tolerances of tests/test_ffdnet_gpu.py::test_define_model_plain2_step_vs_float64_adam."""
    from kair_amd.engine.dncnn_engine import SRMDEngine
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.models.model_plain import ModelPlain
    model = _model(use_graph, clip)
    assert type(model) is ModelPlain and isinstance(model.trainer, FusedTrainer)
    assert type(model.trainer.engine) is SRMDEngine and model.trainer.engine.tdt == torch.float32
    assert model.trainer.segment_buckets() == [(0, sum(p.numel() for p in model.netG.parameters()))]
    ref, ref_e = twin(model.netG), twin(model.netG)
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(52)
    norms = []
    for step in range(3):
        L, Hh = torch.rand(2, 19, 8, 6, generator=g), torch.rand(2, 3, 24, 18, generator=g)
        model.feed_data({"L": L, "H": Hh})
        model.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref(L.double()) - Hh.double()).abs().mean()
        lo.backward()
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=clip, norm_type=2)))
        adam.step()
        with torch.no_grad():
            for pe, pg in zip(ref_e.parameters(), ref.parameters()):
                pe.mul_(0.999).add_(pg, alpha=1 - 0.999)
        loss = model.log_dict["G_loss"]
        assert abs(loss - lo.item()) < 1e-4 * abs(lo.item()), (step, loss, lo.item())
    if clip:
        assert min(norms) > clip, norms                        # the clip was active
        assert abs(float(model.trainer.gnorm) - norms[-1]) < 1e-3 * norms[-1]
    assert (model.trainer.graph is not None) == use_graph
    for mine, theirs in ((model.netG, ref), (model.netE, ref_e)):
        sd, sdr = mine.state_dict(), theirs.state_dict()
        assert [k[len("model."):] for k in sd] == list(sdr)
        for key in sdr:
            assert rel(sd["model." + key], sdr[key]) < (1e-3 if sdr[key].dim() == 1 else 1e-4), key


# ---------------------------------------------------------------------------------------------------------------------
# kair_srmd_kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_srmd_kernels_and_codes():
    g = torch.Generator().manual_seed(61)
    rows = [[0.0, 4.0, 1.0], [1.0, 3.0, 3.0], [0.3, 10.1, 0.1], [math.pi / 2, 0.1, 0.1], [3.1, 10.1, 10.1]]
    while len(rows) < 17:
        th, l1 = float(torch.rand(1, generator=g)) * math.pi, 0.1 + float(torch.rand(1, generator=g)) * 10
        rows.append([th, l1, 0.1 + float(torch.rand(1, generator=g)) * (l1 - 0.1)])
    kpar = torch.tensor(rows, dtype=torch.float32)
    P = sisr.cal_pca_matrix().float()
    outs = []
    for _ in range(2):
        k, code = torch.full((17, 1, 15, 15), float("nan"), device=dev), torch.full((17, 15), float("nan"), device=dev)
        H.srmd_kernels(kpar.to(dev), P.to(dev), k, code)
        outs.append((k.cpu(), code.cpu()))
    (k, code), (k2, code2) = outs
    assert torch.equal(k, k2) and torch.equal(code, code2)
    want = torch.stack([sisr.anisotropic_gaussian(15, *[float(v) for v in r]) for r in kpar])
    ek = (k[:, 0].double() - want).abs().max().item()
    es = (k.double().sum((1, 2, 3)) - 1).abs().max().item()
    ec = (code.double() - sisr.vec_f(k[:, 0].double()) @ P.double().T).abs().max().item()
    print(f"srmd_kernels: kernel {ek:.2e} sum {es:.2e} code {ec:.2e}")
    assert ek < 1e-6 and es < 1e-6 and ec < 1e-5
    # a table with a row stride (the float columns of PatchSynth's table), and the argument checks
    wide = torch.zeros(17, 4)
    wide[:, :3] = kpar
    k3, c3 = torch.empty(17, 1, 15, 15, device=dev), torch.empty(17, 15, device=dev)
    H.srmd_kernels(wide.to(dev), P.to(dev), k3, c3)
    assert torch.equal(k3.cpu(), k) and torch.equal(c3.cpu(), code)
    with pytest.raises(ValueError):
        H.srmd_kernels(kpar.to(dev), P[:, :224].contiguous().to(dev), k3, c3)
    with pytest.raises(ValueError):
        H.srmd_kernels(kpar[:5].to(dev), P.to(dev), k3, c3)
    with pytest.raises(RuntimeError):
        H.srmd_kernels(kpar, P.to(dev), k3, c3)


# ---------------------------------------------------------------------------------------------------------------------
# kair_synth_srmd
# ---------------------------------------------------------------------------------------------------------------------
def _taps(PS, sf):
    return tuple(t.to(dev) for t in util.bicubic_taps(PS, PS // sf, 1.0 / sf))


def _params(N, Hs, Ws, PS, B, g, sigma=None, align=1):
    ints, flts = [], []
    for b in range(B):
        rh = int(torch.randint(0, (Hs - PS) // align + 1, (1,), generator=g)) * align
        rw = int(torch.randint(0, (Ws - PS) // align + 1, (1,), generator=g)) * align
        ints.append([int(torch.randint(0, N, (1,), generator=g)), rh, rw, b % 8])
        th, l1 = float(torch.rand(1, generator=g)) * math.pi, 0.1 + float(torch.rand(1, generator=g)) * 10
        flts.append([th, l1, 0.1 + float(torch.rand(1, generator=g)) * (l1 - 0.1), 0.0 if sigma is None else float(sigma[b])])
    return _table(ints, flts)


def _crops(pool, par, PS):
    return torch.cat([util.augment_img_tensor4(pool[i:i + 1, :, rh:rh + PS, rw:rw + PS], m)
                      for i, rh, rw, m in par[:, :4].tolist()])


def _run_synth(pool, par, PS, sf, k=None, noise_channel=True, seed=0, step=0):
    B, C = par.shape[0], pool.shape[1]
    pd = par.to(dev)
    P = sisr.cal_pca_matrix().float().to(dev)
    kd, code = torch.empty(B, 1, 15, 15, device=dev), torch.empty(B, 15, device=dev)
    H.srmd_kernels(pd[:, 4:].view(torch.float32), P, kd, code)
    if k is not None:
        kd = k.to(dev).contiguous()
    Hp = torch.full((B, C, PS, PS), float("nan"), device=dev)
    Lp = torch.full((B, C + 15 + int(noise_channel), PS // sf, PS // sf), float("nan"), device=dev)
    H.synth_srmd(pool.to(dev), pd, B, PS, sf, kd, code, noise_channel, _taps(PS, sf), seed, step, Hp, Lp, sigma_col=7)
    torch.cuda.synchronize()
    return Lp.cpu(), Hp.cpu(), kd.cpu(), code.cpu()


# (pool shape, H_size, sf, B): 24-px patches over all 8 modes (the blur wraps, the bicubic edge taps reflect), every
# band one L row; 96-px patches, 1 and 3 channels; 192 (sample, channel) pairs, so that a band holds 5 L rows
SYNTH_CASES = [((3, 3, 40, 37), 24, 2, 8), ((3, 3, 40, 37), 24, 3, 8), ((3, 3, 40, 37), 24, 4, 8),
               ((2, 1, 100, 120), 96, 4, 3), ((2, 3, 100, 120), 96, 3, 2), ((4, 3, 60, 50), 48, 2, 64)]


@pytest.mark.parametrize("shape,PS,sf,B", SYNTH_CASES)
def test_synth_noise_off_vs_float64(shape, PS, sf, B):
    """Measured maximum |L - float64| over these cases: 3.5e-7 (B 64, 48-px patches, sf 2); bar 4.2e-5."""
    g = torch.Generator().manual_seed(70 + PS + sf)
    pool = torch.rand(shape, generator=g)
    par = _params(shape[0], shape[2], shape[3], PS, B, g)
    L, Hh, k, code = _run_synth(pool, par, PS, sf)
    C, LS = shape[1], PS // sf
    want_H = _crops(pool, par, PS)
    assert torch.equal(Hh, want_H)
    want = sisr.srmd_degrade(want_H.double(), k.double(), sf)
    err = (L[:, :C].double() - want).abs().max().item()
    print(f"synth_srmd {shape} PS {PS} sf {sf} B {B}: max |L - float64| {err:.3e}")
    assert L.shape == (B, C + 16, LS, LS) and err < SYNTH_TOL
    # the map: the codes and the level, exactly, constant over the LR grid
    assert torch.equal(L[:, C:C + 15], code.view(B, 15, 1, 1).expand(B, 15, LS, LS))
    assert torch.equal(L[:, C + 15], torch.zeros(B, LS, LS))
    # SRMDNF: 15 map channels, the same image
    Lnf, _, _, _ = _run_synth(pool, par, PS, sf, noise_channel=False)
    assert Lnf.shape == (B, C + 15, LS, LS) and torch.equal(Lnf, L[:, :C + 15])


@pytest.mark.parametrize("sf", [2, 3, 4])
def test_synth_delta_kernel_is_the_sr_task(sf):
    """A delta kernel leaves the bicubic downscale of the patch: task "sr"'s L when the pool images are the patch (its L
    is cut from the whole image's downscale).  The resize pass is this kernel's own, so the bar is the bicubic one; H is
    the same gather and equal bit for bit, also for crops of larger images at corners the scale divides."""
    PS, B = 24, 8
    g = torch.Generator().manual_seed(80 + sf)
    pool = torch.rand(3, 3, PS, PS, generator=g)
    par = _params(3, PS, PS, PS, B, g)
    delta = torch.zeros(B, 1, 15, 15)
    delta[:, 0, 7, 7] = 1.0
    L, Hh, _, _ = _run_synth(pool, par, PS, sf, k=delta)
    head = par[:, :4].contiguous().to(dev)
    Hs, Ls = torch.empty(B, 3, PS, PS, device=dev), torch.empty(B, 3, PS // sf, PS // sf, device=dev)
    H.synth_sr(pool.to(dev), head, B, PS, sf, _taps(PS, sf), _taps(PS, sf), Hs, Ls)
    err = (L[:, :3] - Ls.cpu()).abs().max().item()
    print(f"delta kernel vs task sr, sf {sf}: max |dL| {err:.3e}, mode 0 bit-equal {torch.equal(L[0, :3], Ls[0].cpu())}")
    assert err < 2e-6 and torch.equal(Hh, Hs.cpu())
    big = torch.rand(3, 3, 40, 52, generator=g)
    par2 = _params(3, 40, 52, PS, B, g, align=sf)
    _, H2, _, _ = _run_synth(big, par2, PS, sf)
    head2 = par2[:, :4].clone()
    head2[:, 1:3] //= sf                                        # task "sr" counts the corner in L pixels
    bigc = big[..., :40 - 40 % sf, :52 - 52 % sf].contiguous()
    th = tuple(t.to(dev) for t in util.bicubic_taps(bigc.shape[2], bigc.shape[2] // sf, 1.0 / sf))
    tw = tuple(t.to(dev) for t in util.bicubic_taps(bigc.shape[3], bigc.shape[3] // sf, 1.0 / sf))
    H.synth_sr(bigc.to(dev), head2.to(dev), B, PS, sf, th, tw, Hs, Ls)
    assert torch.equal(H2, Hs.cpu())


def test_noise_statistics_and_determinism():
    """tests/test_usrnet_data_gpu.py::test_noise_statistics_and_determinism's thresholds on as many samples."""
    g = torch.Generator().manual_seed(110)
    B = 20
    pool = torch.rand(3, 3, 100, 120, generator=g)
    sigma = torch.tensor([0.0 if b % 5 == 2 else (1 + b) / 255.0 for b in range(B)], dtype=torch.float32)
    par = _params(3, 100, 120, 96, B, g, sigma=sigma)
    par0 = par.clone()
    par0[:, 7] = 0
    L0, _, _, _ = _run_synth(pool, par0, 96, 2)
    L, _, _, _ = _run_synth(pool, par, 96, 2, seed=5, step=7)
    zero = sigma == 0
    assert int(zero.sum()) == 4 and torch.equal(L[zero][:, :3], L0[zero][:, :3])
    assert torch.equal(L[:, 18], sigma.view(B, 1, 1).expand(B, 48, 48)) and torch.equal(L[:, 3:18], L0[:, 3:18])
    n = ((L[~zero][:, :3] - L0[~zero][:, :3]).double() / sigma[~zero].double().view(-1, 1, 1, 1)).flatten()
    assert n.numel() >= 100000
    mean, std, m4 = n.mean().item(), n.std().item(), (n ** 4).mean().item()
    print(f"noise: mean {mean:.4f} std {std:.4f} m4 {m4:.4f} max {n.abs().max().item():.2f}")
    assert abs(mean) < 0.01 and abs(std - 1.0) < 0.01 and abs(m4 - 3.0) < 0.1
    L2, _, _, _ = _run_synth(pool, par, 96, 2, seed=5, step=7)
    assert torch.equal(L2, L)
    L3, _, _, _ = _run_synth(pool, par, 96, 2, seed=5, step=8)
    assert not torch.equal(L3[~zero], L[~zero]) and torch.equal(L3[zero][:, :3], L0[zero][:, :3])


def test_synth_argument_errors():
    pool = torch.rand(2, 3, 32, 32, device=dev)
    par = _params(2, 32, 32, 24, 4, torch.Generator().manual_seed(1)).to(dev)
    k, code = torch.zeros(4, 1, 15, 15, device=dev), torch.zeros(4, 15, device=dev)
    Hp, Lp = torch.empty(4, 3, 24, 24, device=dev), torch.empty(4, 19, 12, 12, device=dev)
    with pytest.raises(ValueError, match="divisible"):
        H.synth_srmd(pool, par, 4, 24, 5, k, code, True, _taps(24, 2), 0, 0, Hp, Lp, sigma_col=7)
    with pytest.raises(ValueError, match="taps"):
        H.synth_srmd(pool, par, 4, 24, 2, k, code, True, _taps(24, 3), 0, 0, Hp, Lp, sigma_col=7)
    with pytest.raises(ValueError, match="output"):
        H.synth_srmd(pool, par, 4, 24, 2, k, code, False, _taps(24, 2), 0, 0, Hp, Lp, sigma_col=7)
    with pytest.raises(RuntimeError, match="level column"):
        H.synth_srmd(pool, par[:, :7].contiguous(), 4, 24, 2, k, code, True, _taps(24, 2), 0, 0, Hp, Lp, sigma_col=3)
    with pytest.raises(RuntimeError, match="smaller than the patch"):
        H.synth_srmd(pool[..., :20, :].contiguous(), par, 4, 24, 2, k, code, True, _taps(24, 2), 0, 0, Hp, Lp, sigma_col=7)


# ---------------------------------------------------------------------------------------------------------------------
# PatchSynth
# ---------------------------------------------------------------------------------------------------------------------
def test_patch_synth_srmd_batches_and_model_steps():
    pool = torch.rand(3, 3, 40, 44, generator=torch.Generator().manual_seed(91)).to(dev)
    synth = PatchSynth(pool, task="srmd", H_size=24, scale=3, sigma=(5, 50), seed=0)
    L, Hh = synth.next(8)
    assert L.shape == (8, 19, 8, 8) and Hh.shape == (8, 3, 24, 24)
    fl = synth.last_params[:, 4:].view(torch.float32).cpu()
    k, code = synth.last_kernels.cpu(), synth.last_codes.cpu()
    want_k = torch.stack([sisr.anisotropic_gaussian(15, *[float(v) for v in r[:3]]) for r in fl])
    assert (k[:, 0].double() - want_k).abs().max() < 1e-6
    assert torch.equal(L[:, 3:18].cpu(), code.view(8, 15, 1, 1).expand(8, 15, 8, 8))
    assert torch.equal(L[:, 18].cpu(), fl[:, 3].view(8, 1, 1).expand(8, 8, 8))
    assert ((fl[:, 3] * 255 >= 5 - 1e-4) & (fl[:, 3] * 255 <= 50 + 1e-4)).all()
    assert torch.equal(Hh.cpu(), _crops(pool.cpu(), synth.last_params.cpu(), 24))
    clean = sisr.srmd_degrade(Hh.cpu().double(), k.double(), 3)
    resid = (L[:, :3].cpu().double() - clean) / fl[:, 3].double().view(8, 1, 1, 1)
    assert 0.9 < resid.std() < 1.1                              # (1536 samples: a sanity check, not the noise test)
    # the same seed draws the same batch; next(B, out=) fills the caller's tensors
    again = PatchSynth(pool, task="srmd", H_size=24, scale=3, sigma=(5, 50), seed=0)
    out = (torch.empty_like(L), torch.empty_like(Hh))
    L2, H2 = again.next(8, out=out)
    assert L2 is out[0] and torch.equal(L2, L) and torch.equal(H2, Hh)
    nf = PatchSynth(pool, task="srmd", H_size=24, scale=3, noise_channel=False, seed=0).next(4)[0]
    assert nf.shape == (4, 18, 8, 8)
    # two training steps of ModelPlain on next_dict batches
    model = _model(False)
    for step in range(2):
        d = synth.next_dict(8)
        assert set(d) == {"L", "H"}
        model.feed_data(d)
        model.optimize_parameters(step)
        assert math.isfinite(model.log_dict["G_loss"]) and 0 < model.log_dict["G_loss"] < 2.0
    assert all(torch.isfinite(p).all() for p in model.netG.parameters())


def test_patch_synth_srmd_errors():
    pool = torch.rand(2, 3, 40, 40, device=dev)
    with pytest.raises(ValueError, match="scale 2, 3 or 4"):
        PatchSynth(pool, task="srmd", H_size=24, scale=5)
    with pytest.raises(ValueError, match="not divisible by the scale"):
        PatchSynth(pool, task="srmd", H_size=26, scale=4)
    with pytest.raises(ValueError, match="pca must be"):
        PatchSynth(pool, task="srmd", H_size=24, scale=4, pca=torch.zeros(15, 15))
    with pytest.raises(ValueError, match="larger than the pool"):
        PatchSynth(pool, task="srmd", H_size=48, scale=4)
