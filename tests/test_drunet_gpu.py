"""DRUNet (UNetRes on the shared ResUNet step program, kair_amd/engine/resunet.py) on the MI355X vs a float64 plain-torch
UNetRes written here (nn.Conv2d / nn.ConvTranspose2d, x = m_up3(x + x4) ...), loaded with load_state_dict(strict=True)
from the kair_amd module's state_dict() -- which also pins the key names and shapes.

Tolerances are the ones tests/test_usrnet_gpu.py holds for the same program (its TOL): fp32 and fp32x3 -- output within
1e-4 relative (L2), every parameter gradient within 5e-3 and their mean within 1e-3; bf16 -- 2e-2 / 0.2 / 5e-2.  The
fused ModelPlain step is held to test_usrnet_fused_trainer_vs_oracle_trainer's bars: loss within 1e-4 relative per
step, parameters (netG and netE) within 1e-4 relative.
"""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd.models.network_unet import UNetRes  # noqa: E402
from kair_amd.models.select_network import compute_dtype_of, define_G  # noqa: E402

dev = torch.device("cuda")
TOL = {"fp32": (1e-4, 5e-3, 1e-3), "fp32x3": (1e-4, 5e-3, 1e-3), "bf16": (2e-2, 0.2, 5e-2)}   # out, worst grad, mean grad


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class RefResBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.res = nn.Sequential(nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.ReLU(), nn.Conv2d(c, c, 3, 1, 1, bias=False))

    def forward(self, x):
        return x + self.res(x)


class RefUNetRes(nn.Module):
    """The reference's UNetRes (strideconv / convtranspose, act 'R', no bias)."""

    def __init__(self, in_nc, out_nc, nc, nb):
        super().__init__()
        seq = lambda *m: m[0] if len(m) == 1 else nn.Sequential(*m)   # noqa: E731  (basicblock.sequential)
        rb = lambda c: [RefResBlock(c) for _ in range(nb)]             # noqa: E731
        self.m_head = nn.Conv2d(in_nc, nc[0], 3, 1, 1, bias=False)
        self.m_down1 = seq(*rb(nc[0]), nn.Conv2d(nc[0], nc[1], 2, 2, 0, bias=False))
        self.m_down2 = seq(*rb(nc[1]), nn.Conv2d(nc[1], nc[2], 2, 2, 0, bias=False))
        self.m_down3 = seq(*rb(nc[2]), nn.Conv2d(nc[2], nc[3], 2, 2, 0, bias=False))
        self.m_body = seq(*rb(nc[3]))
        self.m_up3 = seq(nn.ConvTranspose2d(nc[3], nc[2], 2, 2, 0, bias=False), *rb(nc[2]))
        self.m_up2 = seq(nn.ConvTranspose2d(nc[2], nc[1], 2, 2, 0, bias=False), *rb(nc[1]))
        self.m_up1 = seq(nn.ConvTranspose2d(nc[1], nc[0], 2, 2, 0, bias=False), *rb(nc[0]))
        self.m_tail = nn.Conv2d(nc[0], out_nc, 3, 1, 1, bias=False)

    def forward(self, x0):
        x1 = self.m_head(x0)
        x2 = self.m_down1(x1)
        x3 = self.m_down2(x2)
        x4 = self.m_down3(x3)
        x = self.m_body(x4)
        x = self.m_up3(x + x4)
        x = self.m_up2(x + x3)
        x = self.m_up1(x + x2)
        return self.m_tail(x + x1)


def ref_of(net, in_nc, out_nc, nc, nb):
    ref = RefUNetRes(in_nc, out_nc, nc, nb).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in net.state_dict().items()}, strict=True)
    return ref


CASES = {
    # non-square; the level-3 grid is 2 x 3: the smallest at which a 3x3 halo has an interior and a border
    "2x3": dict(B=2, in_nc=2, out_nc=1, nc=(16, 32, 48, 64), nb=2, hw=(16, 24)),
    # the level-3 grid is 1 x 1 (every tap but the centre outside), m_body a bare ResBlock
    "1x1": dict(B=2, in_nc=4, out_nc=3, nc=(16, 32, 48, 64), nb=1, hw=(8, 8)),
}


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(state_dict, x, R, float64 output, float64 gradients) of a case: computed once, shared by the three engines."""
    c = CASES[name]
    torch.manual_seed(40 + len(name) + c["nb"])
    net = UNetRes(c["in_nc"], c["out_nc"], c["nc"], c["nb"])
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(41 + c["nb"])
    x = torch.rand(c["B"], c["in_nc"], *c["hw"], generator=g)
    ref = ref_of(net, c["in_nc"], c["out_nc"], c["nc"], c["nb"])
    out = ref(x.double())
    R = torch.randn(out.shape, generator=g)
    (out * R.double()).sum().backward()
    return sd, x, R, out.detach(), {n: p.grad.clone() for n, p in ref.named_parameters()}


@pytest.mark.parametrize("dt", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_vs_float64(name, dt):
    c = CASES[name]
    sd, x, R, out_ref, grads_ref = case_ref(name)
    net = UNetRes(c["in_nc"], c["out_nc"], c["nc"], c["nb"], compute_dtype=dt)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    out = net(x.to(dev))                         # ConvNetFunction on the DRUNet engine
    e_out = rel(out, out_ref)
    (out * R.to(dev)).sum().backward()
    errs = {n: rel(p.grad, grads_ref[n]) for n, p in net.named_parameters()}
    print(f"{name} {dt}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad {sum(errs.values()) / len(errs):.3e}")
    assert e_out < TOL[dt][0]
    bad = {k: e for k, e in errs.items() if e > TOL[dt][1]}
    assert not bad, bad
    assert sum(errs.values()) / len(errs) < TOL[dt][2], sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def _opt(use_graph, **netg):
    o = {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
         "netG": {"net_type": "drunet", "in_nc": 2, "out_nc": 1, "nc": [16, 32, 48, 64], "nb": 2, "act_mode": "R",
                  "downsample_mode": "strideconv", "upsample_mode": "convtranspose", "init_type": "orthogonal",
                  "init_bn_type": "uniform", "init_gain": 0.2},
         "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                   "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                   "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                   "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                   "use_hip_graph": use_graph}}
    o["netG"].update(netg)
    return o


@pytest.mark.parametrize("use_graph", [True, False])
def test_define_g_modelplain_step_vs_float64_adam(use_graph):
    """define_Model('plain') trains DRUNet on FusedTrainer: three steps (L1, Adam, EMA 0.999) against the float64
    reference under torch.optim.Adam with the same EMA."""
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(51)
    model = define_Model(dict_to_nonedict(_opt(use_graph)))
    model.init_train()
    assert isinstance(model.trainer, FusedTrainer)
    assert model.trainer.engine.tdt == torch.float32 and not model.trainer.engine.x3   # the plain option file: fp32
    ref, ref_e = (ref_of(model.netG, 2, 1, (16, 32, 48, 64), 2) for _ in range(2))
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(52)
    for step in range(3):
        L, Hh = torch.rand(2, 2, 16, 16, generator=g), torch.rand(2, 1, 16, 16, generator=g)
        model.feed_data({"L": L, "H": Hh})
        model.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref(L.double()) - Hh.double()).abs().mean()
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


def test_compute_dtype_selection():
    o = _opt(True)
    assert compute_dtype_of(o) == "fp32"
    o["train"]["amp_enabled"] = True
    assert compute_dtype_of(o) == "bf16"
    assert compute_dtype_of(_opt(True, compute_dtype="fp32x3")) == "fp32x3"
    net = define_G({**_opt(True, compute_dtype="fp32x3"), "is_train": False})
    assert isinstance(net, UNetRes) and net.compute_dtype == "fp32x3"


def test_errors():
    net = UNetRes(2, 1, (16, 32, 48, 64), 1).to(dev)
    with pytest.raises(ValueError, match="8"):
        net(torch.rand(1, 2, 20, 16, device=dev))
    with pytest.raises(NotImplementedError, match="8"):
        UNetRes(in_nc=9)
    with pytest.raises(NotImplementedError, match="8"):
        UNetRes(nc=(12, 32, 48, 64))
    with pytest.raises(NotImplementedError):
        UNetRes(act_mode="L")
    with pytest.raises(NotImplementedError):
        UNetRes(nb=0)
    with pytest.raises(RuntimeError):
        net(torch.rand(1, 2, 16, 16))


def test_inference_test_mode_pad_and_noise_map():
    from kair_amd.utils import utils_image as util
    from kair_amd.utils.utils_model import test_mode
    torch.manual_seed(61)
    net = UNetRes(2, 1, (16, 32, 48, 64), 2)
    ref = ref_of(net, 2, 1, (16, 32, 48, 64), 2)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(62)
    img = torch.rand(1, 1, 19, 21, generator=g)
    L = util.add_noise_map(img, 25)
    assert torch.equal(L, torch.cat((img, torch.full((1, 1, 19, 21), 25 / 255.0)), 1))
    Ld = util.add_noise_map(img.to(dev), 25)
    assert Ld.is_cuda and torch.equal(Ld.cpu(), L)
    two = util.add_noise_map(torch.cat((img, img)), torch.tensor([25.0, 50.0]))          # one level per image
    assert torch.equal(two, torch.cat((torch.cat((img, img)), torch.tensor([25.0, 50.0]).view(2, 1, 1, 1).div(255.0)
                                       .expand(2, 1, 19, 21)), 1))
    with torch.no_grad():
        E = test_mode(net, L.to(dev), mode=1, modulo=8)
        want = ref(torch.nn.functional.pad(L.double(), (0, 3, 0, 5), mode="replicate"))[..., :19, :21]
    assert E.shape == (1, 1, 19, 21)
    assert rel(E, want) < TOL["fp32"][0]


def test_checkpoint_keys_and_roundtrip(tmp_path):
    nb = 4
    rb = lambda p: [f"{p}.res.{j}.weight" for j in (0, 2)]   # noqa: E731
    keys = ["m_head.weight"]
    for l in (1, 2, 3):
        keys += [k for i in range(nb) for k in rb(f"m_down{l}.{i}")] + [f"m_down{l}.{nb}.weight"]
    keys += [k for i in range(nb) for k in rb(f"m_body.{i}")]
    for l in (3, 2, 1):
        keys += [f"m_up{l}.0.weight"] + [k for i in range(1, nb + 1) for k in rb(f"m_up{l}.{i}")]
    keys += ["m_tail.weight"]
    nc = (16, 32, 48, 64)
    torch.manual_seed(71)
    net = UNetRes(2, 1, nc, nb)
    sd = net.state_dict()
    assert list(sd) == keys
    for l in (1, 2, 3):
        assert tuple(sd[f"m_down{l}.{nb}.weight"].shape) == (nc[l], nc[l - 1], 2, 2)
        assert tuple(sd[f"m_up{l}.0.weight"].shape) == (nc[l], nc[l - 1], 2, 2)      # ConvTranspose2d: [C_in, C_out, 2, 2]
    assert tuple(sd["m_head.weight"].shape) == (16, 2, 3, 3) and tuple(sd["m_tail.weight"].shape) == (1, 16, 3, 3)
    assert list(UNetRes(2, 1, nc, 1).state_dict())[1:4] == ["m_down1.0.res.0.weight", "m_down1.0.res.2.weight",
                                                             "m_down1.1.weight"]
    assert "m_body.res.0.weight" in UNetRes(2, 1, nc, 1).state_dict()               # nb = 1: a bare ResBlock
    torch.save(sd, tmp_path / "drunet.pth")
    fresh = UNetRes(2, 1, nc, nb)
    fresh.load_state_dict(torch.load(tmp_path / "drunet.pth"), strict=True)
    x = torch.rand(1, 2, 16, 16, device=dev)
    with torch.no_grad():
        a, b = net.to(dev).eval()(x), fresh.to(dev).eval()(x)
    assert torch.equal(a, b)
