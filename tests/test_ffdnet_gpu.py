"""FFDNet on the MI355X: the PixelUnshuffle head kernel (kair_ffd_pack) exactly, FFDNetEngine (DnCNN's step program over
the half grid) against a float64 plain-torch FFDNet written here (nn.Conv2d / nn.BatchNorm2d / nn.ReLU, F.pad replicate,
F.pixel_unshuffle, F.pixel_shuffle) loaded with load_state_dict(strict=True) from the kair_amd module's state_dict(),
ModelPlain2 on the fused trainer against float64 Adam + EMA, and PatchSynth(task="ffdnet") against task "fdncnn".

fp32 bars (tests/test_full_configs_gpu.py::test_c1_dncnn_full): output within 1e-4 relative (L2) of float64, every
parameter gradient within max(2e-3, 3 x the error of torch's own fp32 run against float64).
bf16 bars: tests/test_drunet_gpu.py's for bf16 conv programs are 2e-2 output, 0.2 worst gradient, 5e-2 mean gradient.
The existing bf16 program itself must stay inside them at these shapes: FDnCNN bf16 of the same nc and nb on the "gray"
case's same-sized input, against its float64 twin, measures output 9.99e-3, worst gradient 8.16e-2 and mean gradient
5.26e-2.  Its mean gradient error exceeds the 5e-2 bar (six of the eight parameters of this 4-layer, 16-channel net sit
at 6-8e-2: there are no deep, well-averaged layers to pull the mean down), so the mean bar here is 2 x that measured
reference error, 1.05e-1; the output and worst-gradient bars stay 2e-2 and 0.2.  FFDNet bf16 on the same case measures
2.8e-3 / 7.3e-2 / 5.0e-2.  test_bf16_reference_is_inside_the_bars keeps the reference under the bars used.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.models.network_dncnn import FDnCNN  # noqa: E402
from kair_amd.models.network_ffdnet import FFDNet  # noqa: E402

dev = torch.device("cuda")
BF16_TOL = (2e-2, 0.2, 1.05e-1)   # output, worst gradient, mean gradient (2 x the reference's 5.26e-2: docstring)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _stack(cin, cout, nc, nb, bn):
    mods = [nn.Conv2d(cin, nc, 3, 1, 1), nn.ReLU()]
    for _ in range(nb - 2):
        mods.append(nn.Conv2d(nc, nc, 3, 1, 1))
        if bn:
            mods.append(nn.BatchNorm2d(nc, momentum=0.9, eps=1e-4))
        mods.append(nn.ReLU())
    mods.append(nn.Conv2d(nc, cout, 3, 1, 1))
    return nn.Sequential(*mods)


class RefFFDNet(nn.Module):
    """The restated reference forward ('R' / 'BR')."""

    def __init__(self, in_nc, out_nc, nc, nb, bn=False):
        super().__init__()
        self.model = _stack(in_nc * 4 + 1, out_nc * 4, nc, nb, bn)

    def forward(self, x, sigma):
        h, w = x.shape[-2:]
        x = F.pad(x, (0, -w % 2, 0, -h % 2), mode="replicate")
        x = F.pixel_unshuffle(x, 2)
        x = torch.cat((x, sigma.repeat(1, 1, x.shape[2], x.shape[3])), 1)
        return F.pixel_shuffle(self.model(x), 2)[..., :h, :w]


class RefFDnCNN(nn.Module):
    def __init__(self, in_nc, out_nc, nc, nb):
        super().__init__()
        self.model = _stack(in_nc, out_nc, nc, nb, False)

    def forward(self, x, sigma=None):
        return self.model(x)


def twin(net, ref, dtype=torch.float64):
    ref = ref.to(dtype)
    ref.load_state_dict({k: v.detach().to(dtype).cpu() for k, v in net.state_dict().items()}, strict=True)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# kair_ffd_pack
# ---------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [((2, 1, 5, 7), 8), ((2, 3, 6, 4), 16), ((1, 3, 1, 1), 16)]


def _unshuffled(x, mode):
    """[B, 4C, Hh, Wh] of x padded to even sizes (replicate for the input, zeros for a gradient)."""
    h, w = x.shape[-2:]
    pad = (0, -w % 2, 0, -h % 2)
    x = F.pad(x, pad, mode="replicate") if mode == "replicate" else F.pad(x, pad)
    return F.pixel_unshuffle(x, 2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape, ldc", PACK_SHAPES)
def test_ffd_pack_input_mode_exact(shape, ldc, dt):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(3)
    x = torch.rand(shape, generator=g)
    sigma = torch.tensor([5.0, 50.0])[:B] / 255
    u = _unshuffled(x, "replicate")
    Hh, Wh = u.shape[-2:]
    want = torch.zeros(B, Hh, Wh, ldc)
    want[..., :4 * C] = u.permute(0, 2, 3, 1)
    want[..., 4 * C] = sigma.view(B, 1, 1)
    out = torch.full((B * Hh * Wh, ldc), float("nan"), device=dev, dtype=dt)
    H.ffd_pack(x.to(dev), sigma.to(dev), out, ldc, B, C, h, w)
    assert torch.equal(out.cpu().view(B, Hh, Wh, ldc), want.to(dt))


@pytest.mark.parametrize("shape", [s for s, _ in PACK_SHAPES])
def test_ffd_pack_gradient_mode_exact(shape):
    B, C, h, w = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    u = _unshuffled(x, "zeros")
    Hh, Wh = u.shape[-2:]
    want = torch.zeros(B, Hh, Wh, 16)
    want[..., :4 * C] = u.permute(0, 2, 3, 1)
    out = torch.full((B * Hh * Wh, 16), float("nan"), device=dev)
    H.ffd_pack(x.to(dev), None, out, 16, B, C, h, w)
    out = out.cpu().view(B, Hh, Wh, 16)
    assert torch.equal(out, want)
    assert (out[..., 4 * C:] == 0).all()
    if h % 2:   # the cropped row: sub-pixels i = 1 of the last grid row
        assert (out[:, -1, :, :4 * C].reshape(B, Wh, C, 2, 2)[..., 1, :] == 0).all()
    if w % 2:
        assert (out[:, :, -1, :4 * C].reshape(B, Hh, C, 2, 2)[..., :, 1] == 0).all()


def test_ffd_pack_argument_errors():
    x = torch.rand(1, 1, 4, 4, device=dev)
    s = torch.rand(1, device=dev)
    with pytest.raises(RuntimeError, match="ffd_pack"):
        H.ffd_pack(x, s, torch.empty(4, 4, device=dev), 4, 1, 1, 4, 4)              # ldc % 8
    with pytest.raises(RuntimeError, match="ffd_pack"):
        H.ffd_pack(x.expand(1, 2, 4, 4).contiguous(), s, torch.empty(4, 8, device=dev), 8, 1, 2, 4, 4)   # 4C + 1 > ldc
    with pytest.raises(RuntimeError):
        H.ffd_pack(x.cpu(), s, torch.empty(4, 8, device=dev), 8, 1, 1, 4, 4)


# ---------------------------------------------------------------------------------------------------------------------
# forward and gradients against float64
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    # the half grid is 6 x 10: non-square, with an interior and a border
    "gray": dict(in_nc=1, nc=16, nb=4, act="R", shape=(2, 1, 12, 20)),
    # odd sizes: replicate pad at the head, crop at the tail, the gradient pack's zeros
    "odd": dict(in_nc=3, nc=16, nb=3, act="R", shape=(2, 3, 9, 11)),
    # BatchNorm with batch statistics
    "bn": dict(in_nc=1, nc=16, nb=4, act="BR", shape=(2, 1, 16, 16)),
}


def grad_errs(grads, gref):
    """Relative error per parameter; a conv bias feeding a train-mode BatchNorm has an analytically zero gradient
    and is judged against 1e-4 x the largest gradient norm (tests/test_full_configs_gpu.py grad_errs)."""
    scale = max(v.double().norm().item() for v in gref.values())
    out = {}
    for k, a in grads.items():
        a, b = a.detach().double().cpu(), gref[k].detach().double()
        out[k] = (a.norm().item() / (1e-4 * scale) * 1e-3 if b.norm().item() < 1e-4 * scale
                  else ((a - b).norm() / b.norm()).item())
    return out


def _run_ref(ref, x, sigma, R):
    ref.train()
    dt = next(ref.parameters()).dtype
    out = ref(x.to(dt), sigma.to(dt))
    (out * R.to(dt)).sum().backward()
    return out.detach(), {n: p.grad.clone() for n, p in ref.named_parameters()}


@functools.lru_cache(maxsize=None)
def case_ref(name, kind="ffdnet"):
    """(state_dict, x, sigma, R, float64 output and gradients, torch-fp32 gradients) of a case: computed once."""
    c = CASES[name]
    C = c["in_nc"]
    torch.manual_seed(20 + len(name))
    bn = "B" in c["act"]
    if kind == "ffdnet":
        net, mk = FFDNet(C, C, c["nc"], c["nb"], c["act"]), lambda: RefFFDNet(C, C, c["nc"], c["nb"], bn)
    else:   # the bf16 reference program on a same-sized input
        net, mk = FDnCNN(C + 1, C, c["nc"], c["nb"], "R"), lambda: RefFDnCNN(C + 1, C, c["nc"], c["nb"])
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.0)
            m.bias.data.uniform_(-0.1, 0.1)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(21 + len(name))
    B, _, h, w = c["shape"]
    x = torch.rand(B, C if kind == "ffdnet" else C + 1, h, w, generator=g)
    sigma = (torch.tensor([5.0, 50.0]) / 255).view(2, 1, 1, 1)
    R = torch.randn(B, C, h, w, generator=g)
    out64, g64 = _run_ref(twin(net, mk()), x, sigma, R)
    _, g32 = _run_ref(twin(net, mk(), torch.float32), x, sigma, R)
    return sd, x, sigma, R, out64, g64, g32


def _run_engine(name, dt, kind="ffdnet"):
    c = CASES[name]
    C = c["in_nc"]
    sd, x, sigma, R, out64, g64, g32 = case_ref(name, kind)
    net = (FFDNet(C, C, c["nc"], c["nb"], c["act"], compute_dtype=dt) if kind == "ffdnet"
           else FDnCNN(C + 1, C, c["nc"], c["nb"], "R", compute_dtype=dt))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    out = net(x.to(dev), sigma.to(dev)) if kind == "ffdnet" else net(x.to(dev))
    assert out.shape == R.shape
    (out * R.to(dev)).sum().backward()
    e_out = rel(out, out64)
    errs = grad_errs({n: p.grad for n, p in net.named_parameters()}, g64)
    floor = grad_errs(g32, g64)
    print(f"{kind} {name} {dt}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad "
          f"{sum(errs.values()) / len(errs):.3e} (torch fp32 worst {max(floor.values()):.3e})")
    return e_out, errs, floor


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_forward_and_gradients_vs_float64(name):
    e_out, errs, floor = _run_engine(name, "fp32")
    assert e_out < 1e-4
    bad = {k: (errs[k], floor[k]) for k in errs if errs[k] > max(2e-3, 3.0 * floor[k])}
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_forward_and_gradients_vs_float64(name):
    e_out, errs, _ = _run_engine(name, "bf16")
    assert e_out < BF16_TOL[0]
    bad = {k: e for k, e in errs.items() if e > BF16_TOL[1]}
    assert not bad, bad
    assert sum(errs.values()) / len(errs) < BF16_TOL[2]


@pytest.mark.parametrize("name", ["gray", "odd"])
def test_bf16_reference_is_inside_the_bars(name):
    """FDnCNN(in_nc + 1, out_nc, same nc, same nb) bf16 on a same-sized input against its float64 twin: the bf16 bars
    above are ones the existing bf16 conv program meets."""
    e_out, errs, _ = _run_engine(name, "bf16", kind="fdncnn")
    assert e_out < BF16_TOL[0] and max(errs.values()) < BF16_TOL[1] and sum(errs.values()) / len(errs) < BF16_TOL[2]


def test_neither_input_gets_a_gradient():
    net = FFDNet(1, 1, 16, 3, "R").to(dev).train()
    x = torch.rand(1, 1, 8, 8, device=dev, requires_grad=True)
    s = torch.full((1, 1, 1, 1), 0.1, device=dev, requires_grad=True)
    net(x, s).sum().backward()
    assert x.grad is None and s.grad is None and all(p.grad is not None for p in net.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# inference helper, broadcasting, checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_forward_odd_size_through_test_mode():
    from kair_amd.utils.utils_model import test_mode
    torch.manual_seed(31)
    net = FFDNet(1, 1, 16, 4, "R")
    ref = twin(net, RefFFDNet(1, 1, 16, 4)).eval()
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(32)
    L = torch.rand(1, 1, 19, 21, generator=g)
    sigma = torch.full((1, 1, 1, 1), 25 / 255.0)
    with torch.no_grad():
        E = test_mode(lambda t: net(t, sigma.to(dev)), L.to(dev), mode=0)
        want = ref(L.double(), sigma.double())
    assert E.shape == (1, 1, 19, 21)
    assert rel(E, want) < 1e-4
    # a one-element sigma broadcasts over B = 2, in each accepted form
    L2 = torch.rand(2, 1, 10, 12, generator=g)
    with torch.no_grad():
        want2 = ref(L2.double(), sigma.double().expand(2, 1, 1, 1))
        for s in (sigma.to(dev), sigma.view(1).to(dev), sigma.expand(2, 1, 1, 1).to(dev), sigma.view(1).expand(2).to(dev)):
            assert rel(net(L2.to(dev), s), want2) < 1e-4


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(33)
    net = FFDNet(3, 3, 16, 3, "R")
    assert list(net.state_dict()) == [f"model.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    torch.save(net.state_dict(), tmp_path / "ffdnet.pth")
    fresh = FFDNet(3, 3, 16, 3, "R")
    fresh.load_state_dict(torch.load(tmp_path / "ffdnet.pth"), strict=True)
    x = torch.rand(2, 3, 11, 14, device=dev)
    s = torch.tensor([0.05, 0.2], device=dev).view(2, 1, 1, 1)
    with torch.no_grad():
        a, b = net.to(dev).eval()(x, s), fresh.to(dev).eval()(x, s)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# fused trainer
# ---------------------------------------------------------------------------------------------------------------------
def _opt(use_graph, **netg):
    o = {"model": "plain2", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
         "netG": {"net_type": "ffdnet", "in_nc": 1, "out_nc": 1, "nc": 16, "nb": 4, "act_mode": "R",
                  # (gain 1: at the option files' 0.2 the level moves this 4-layer net's loss by < 1e-5 relative)
                  "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 1.0},
         "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                   "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                   "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                   "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                   "use_hip_graph": use_graph}}
    o["netG"].update(netg)
    return o


def _model(use_graph, **netg):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(51)
    model = define_Model(dict_to_nonedict(_opt(use_graph, **netg)))
    model.init_train()
    return model


@pytest.mark.parametrize("use_graph", [True, False])
def test_define_model_plain2_step_vs_float64_adam(use_graph):
    """define_Model('plain2') trains FFDNet on FusedTrainer: three steps (L1, Adam, EMA 0.999) with fresh per-step
    levels against the float64 reference under torch.optim.Adam with the same EMA; then a fourth step (a graph replay
    when use_graph) whose result must follow its own C, not the previous step's."""
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.models.model_plain2 import ModelPlain2
    model, other = _model(use_graph), _model(use_graph)
    assert type(model) is ModelPlain2 and isinstance(model.trainer, FusedTrainer)
    assert model.trainer.engine.tdt == torch.float32
    ref, ref_e = (twin(model.netG, RefFFDNet(1, 1, 16, 4)) for _ in range(2))
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(52)
    levels = torch.tensor([[5.0, 50.0], [30.0, 10.0], [5.0, 10.0], [75.0, 60.0]]) / 255
    batches = [(torch.rand(2, 1, 16, 16, generator=g), torch.rand(2, 1, 16, 16, generator=g), levels[i].view(2, 1, 1, 1))
               for i in range(4)]
    for step, (L, Hh, C) in enumerate(batches[:3]):
        for m in (model, other):
            m.feed_data({"L": L, "H": Hh, "C": C})
            m.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref(L.double(), C.double()) - Hh.double()).abs().mean()
        lo.backward()
        adam.step()
        with torch.no_grad():
            for pe, pg in zip(ref_e.parameters(), ref.parameters()):
                pe.mul_(0.999).add_(pg, alpha=1 - 0.999)
        loss = model.log_dict["G_loss"]
        assert abs(loss - lo.item()) < 1e-4 * abs(lo.item()), (step, loss, lo.item())
    assert (model.trainer.graph is not None) == use_graph
    for mine, theirs in ((model.netG, ref), (model.netE, ref_e)):
        sd, sdr = mine.state_dict(), theirs.state_dict()
        assert list(sd) == list(sdr)
        for key in sdr:
            assert rel(sd[key], sdr[key]) < (1e-3 if sdr[key].dim() == 1 else 1e-4), key
    # step 4 on the same (L, H): `model` with its own C, `other` with step 3's C
    L, Hh, C = batches[3]
    model.feed_data({"L": L, "H": Hh, "C": C})
    model.optimize_parameters(3)
    other.feed_data({"L": L, "H": Hh, "C": batches[2][2]})
    other.optimize_parameters(3)
    lo = (ref(L.double(), C.double()) - Hh.double()).abs().mean().item()
    stale = (ref(L.double(), batches[2][2].double()) - Hh.double()).abs().mean().item()
    assert abs(lo - stale) > 1e-3 * lo                          # the level matters for this batch ...
    assert abs(model.log_dict["G_loss"] - lo) < 1e-4 * lo       # ... and each step read its own
    assert abs(other.log_dict["G_loss"] - stale) < 1e-4 * stale
    assert model.log_dict["G_loss"] != other.log_dict["G_loss"]


# ---------------------------------------------------------------------------------------------------------------------
# on-device data
# ---------------------------------------------------------------------------------------------------------------------
def test_patch_synth_ffdnet_equals_fdncnn_and_feeds_plain2():
    from kair_amd.data.gpu_synth import PatchSynth
    pool = torch.rand(3, 3, 24, 24, generator=torch.Generator().manual_seed(61)).to(dev)
    B, C = 4, 3
    kw = dict(H_size=16, sigma=(5, 60), seed=0)
    ffd, fdn = PatchSynth(pool, task="ffdnet", **kw), PatchSynth(pool, task="fdncnn", **kw)
    for _ in range(2):   # two steps: the Philox step counter moves alike
        L, Hh, lev = ffd.next(B)
        L_fd, H_fd = fdn.next(B)
        assert L.shape == (B, C, 16, 16) and Hh.shape == (B, C, 16, 16) and lev.shape == (B, 1, 1, 1)
        assert torch.equal(L, L_fd[:, :C]) and torch.equal(Hh, H_fd)
        assert torch.equal(lev.view(B), L_fd[:, C, 0, 0])
        assert torch.equal(ffd.last_params, fdn.last_params)
    assert ((lev >= 5 / 255.0 - 1e-7) & (lev <= 60 / 255.0 + 1e-7)).all() and lev.unique().numel() == B
    model = _model(False, in_nc=3, out_nc=3, nb=3)
    d = ffd.next_dict(2)
    assert set(d) == {"L", "H", "C"} and d["C"].shape == (2, 1, 1, 1)
    model.feed_data(d)
    model.optimize_parameters(0)
    ref = twin(model.netG, RefFFDNet(3, 3, 16, 3))   # (the parameters after the step: only the loss scale is checked)
    assert 0 < model.log_dict["G_loss"] < 2.0 and torch.isfinite(torch.tensor(model.log_dict["G_loss"]))
    assert all(torch.isfinite(p).all() for p in ref.parameters())
    with pytest.raises(ValueError):
        PatchSynth(pool, task="ffdnet", H_size=16, sigma=(60, 5))


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    from kair_amd.engine.trainer import FusedTrainer
    net = FFDNet(1, 1, 16, 3, "R").to(dev)
    with pytest.raises(RuntimeError):
        net(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 1, 1))
    for kw in (dict(nc=12), dict(out_nc=5), dict(act_mode="IR")):
        with pytest.raises(NotImplementedError):
            FFDNet(**kw)
    with pytest.raises(ValueError, match="sigma"):
        net(torch.rand(2, 1, 8, 8, device=dev), torch.rand(3, 1, 1, 1, device=dev))
    tr = FusedTrainer(net.train(), None, E_decay=0, use_graph=False)
    with pytest.raises(ValueError, match="even"):
        tr.step(torch.rand(2, 1, 9, 8, device=dev), torch.rand(2, 1, 9, 8, device=dev), torch.rand(2, 1, 1, 1, device=dev))
