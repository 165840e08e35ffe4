"""IRCNN on the MI355X: the DnCNN step program with a dilation per conv against the module list in float64 on the host.

Bars (tests/test_ffdnet_gpu.py / test_srmd_gpu.py): fp32 output within 1e-4 relative (L2) of float64, every parameter
gradient within max(2e-3, 3 x the error of torch's own fp32 run); bf16 output 2e-2, worst gradient 0.2, mean gradient
1.05e-1.  bf16 runs both routes of the dilated 64 -> 64 layers -- kair_conv3x3_dil (dil_kernel=True) and the dilated
im2col GEMM (False) -- which must also agree with each other at the bf16 output bar; the kernel timing window shows
which route ran.  test_bf16_rounded_float64_reference_is_inside_the_bars keeps a float64 run with bf16 storage under
the same bars.  Then the fused trainer, the model bank (stale packs would fail it) and DPIR with the IRCNN prior.
Each test prints its figures (pytest -s)."""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.main_dpir import dpir_restore  # noqa: E402
from kair_amd.models.network_dncnn import IRCNN  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_model, utils_pnp, utils_sisr  # noqa: E402

dev = torch.device("cuda")
BF16_TOL = (2e-2, 0.2, 1.05e-1)   # output, worst gradient, mean gradient
F64 = torch.float64
CASES = {"gray": (1, 2, 24, 24), "color": (3, 1, 17, 23)}     # channels, B, h, w (the second ragged in both directions)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def twin(net, dtype=F64):
    """The module list on the host in `dtype`, out = x - model(x)."""
    ref = IRCNN(net.model[0].in_channels, net.model[12].out_channels, net.model[0].out_channels).to(dtype)
    ref.load_state_dict({k: v.detach().to(dtype).cpu() for k, v in net.state_dict().items()}, strict=True)
    return ref


def grad_errs(grads, gref):
    return {k: ((a.detach().double().cpu() - gref[k].double()).norm() / gref[k].double().norm()).item()
            for k, a in grads.items()}


def _ref_run(ref, x, R):
    dt = next(ref.parameters()).dtype
    for p in ref.parameters():
        p.grad = None
    out = ref(x.to(dt))
    (out * R.to(dt)).sum().backward()
    return out.detach(), {n: p.grad.clone() for n, p in ref.named_parameters()}


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(state_dict, x, R, (float64 output, gradients), (torch fp32 ...)): computed once, never modified."""
    C, B, h, w = CASES[name]
    torch.manual_seed(70 + C)
    net = IRCNN(C, C, 64)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(71 + C)
    x, R = torch.rand(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g)
    return sd, x, R, _ref_run(twin(net), x, R), _ref_run(twin(net, torch.float32), x, R)


def timed(fn, slots=512):
    torch.cuda.synchronize()
    H.ktime_begin(slots)
    try:
        out = fn()
    finally:
        nk = H.ktime_end()
    torch.cuda.synchronize()
    return out, [H.ktime_read(i)[1] for i in range(nk)]


def _engine_run(name, dt, dil_kernel=True):
    C = CASES[name][0]
    sd, x, R, (out64, g64), (_, g32) = case_ref(name)
    net = IRCNN(C, C, 64, compute_dtype=dt).set_dil_kernel(dil_kernel)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()

    def run():
        out = net(x.to(dev))
        (out * R.to(dev)).sum().backward()
        return out
    out, names = timed(run)
    grads = {n: p.grad for n, p in net.named_parameters()}
    ndil = sum("conv3x3_dil_kernel" in n for n in names)
    e_out, errs, floor = rel(out, out64), grad_errs(grads, g64), grad_errs(g32, g64)
    print(f"ircnn {name} {dt} dil_kernel={dil_kernel}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad "
          f"{sum(errs.values()) / len(errs):.3e} (torch fp32 worst {max(floor.values()):.3e}); {ndil} of {len(names)} "
          f"launches are conv3x3_dil_kernel")
    return out.detach(), e_out, errs, floor, ndil


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_forward_and_gradients_vs_float64(name):
    _, e_out, errs, floor, ndil = _engine_run(name, "fp32")
    assert ndil == 0                                            # the exact-fp32 engine stays on the generic path
    assert e_out < 1e-4
    bad = {k: (errs[k], floor[k]) for k in errs if errs[k] > max(2e-3, 3.0 * floor[k])}
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_both_routes_vs_float64_and_each_other(name):
    outs = {}
    for dk in (True, False):
        outs[dk], e_out, errs, _, ndil = _engine_run(name, "bf16", dk)
        # five dilated 64 -> 64 layers: forward and input gradient each on the new kernel, or none
        assert ndil == (10 if dk else 0), ndil
        assert e_out < BF16_TOL[0]
        bad = {k: e for k, e in errs.items() if e > BF16_TOL[1]}
        assert not bad, bad
        assert sum(errs.values()) / len(errs) < BF16_TOL[2]
    e = rel(outs[True], outs[False])
    print(f"ircnn {name} bf16: kair_conv3x3_dil route vs generic route {e:.3e}")
    assert e < BF16_TOL[0]


def test_bf16_width_outside_the_kernel_contract_takes_the_generic_path():
    """nc = 32: kair_conv3x3_dil's contract is C = N = 64, so the engine routes every layer to the dilated im2col GEMM."""
    torch.manual_seed(75)
    net = IRCNN(1, 1, 32, compute_dtype="bf16")
    ref = twin(net)
    net = net.to(dev).eval()
    x = torch.rand(1, 1, 14, 11, generator=torch.Generator().manual_seed(76))
    with torch.no_grad():
        out, names = timed(lambda: net(x.to(dev)))
        e = rel(out, ref(x.double()))
    print(f"ircnn nc 32 bf16: out {e:.3e}")
    assert not any("conv3x3_dil_kernel" in n for n in names) and e < BF16_TOL[0]


class _RoundBF16(torch.autograd.Function):
    """bf16 storage of a float64 tensor: rounded on the way forward, its gradient rounded on the way back."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_rounded_float64_reference_is_inside_the_bars(name):
    """The bars are reachable by the storage format alone: a float64 run (on the host) whose input, activations and
    output gradient are rounded to bf16."""
    sd, x, R, (out64, g64), _ = case_ref(name)
    C = CASES[name][0]
    ref = IRCNN(C, C, 64).double()
    ref.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    x0 = _RoundBF16.apply(x.double())
    h = x0
    for m in ref.model:
        if isinstance(m, nn.ReLU):
            h = _RoundBF16.apply(torch.relu(h))
        else:
            h = m(h)
    out = x.double() - h
    (out * R.double().bfloat16().double()).sum().backward()
    errs = grad_errs({n: p.grad for n, p in ref.named_parameters()}, g64)
    e_out = rel(out, out64)
    print(f"bf16-rounded float64 {name}: out {e_out:.3e} worst {max(errs.values()):.3e} mean {sum(errs.values()) / len(errs):.3e}")
    assert e_out < BF16_TOL[0] and max(errs.values()) < BF16_TOL[1] and sum(errs.values()) / len(errs) < BF16_TOL[2]


# ---- fused trainer ----------------------------------------------------------------------------------------------------
def _opt(use_graph, clip=None, loss="l1"):
    return {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
            "netG": {"net_type": "ircnn", "in_nc": 1, "out_nc": 1, "nc": 64, "init_type": "orthogonal",
                     "init_bn_type": "uniform", "init_gain": 0.2},
            "train": {"G_lossfn_type": loss, "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": clip,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                      "use_hip_graph": use_graph}}


def _model(use_graph, clip=None, loss="l1"):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(81)
    model = define_Model(dict_to_nonedict(_opt(use_graph, clip, loss)))
    model.init_train()
    return model


@pytest.mark.parametrize("use_graph,clip", [(True, None), (True, 0.004)])
def test_define_model_plain_step_vs_float64_adam(use_graph, clip):
    """Three graph-captured steps of define_Model('plain') (L1, Adam; one run with gradient-norm clipping) against the
    float64 module list under torch.optim.Adam: the loss of every step within 1e-4 relative."""
    from kair_amd.engine.dncnn_engine import IRCNNEngine
    from kair_amd.engine.trainer import FusedTrainer
    model = _model(use_graph, clip)
    assert isinstance(model.trainer, FusedTrainer) and type(model.trainer.engine) is IRCNNEngine
    assert model.trainer.engine.tdt == torch.float32
    assert model.trainer.segment_buckets() == [(0, sum(p.numel() for p in model.netG.parameters()))]
    ref = twin(model.netG)
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(82)
    norms = []
    for step in range(3):
        Hh = torch.rand(2, 1, 20, 18, generator=g)
        L = Hh + torch.randn(Hh.shape, generator=g) * (25 / 255)
        model.feed_data({"L": L, "H": Hh})
        model.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref(L.double()) - Hh.double()).abs().mean()
        lo.backward()
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=clip, norm_type=2)))
        adam.step()
        loss = model.log_dict["G_loss"]
        print(f"ircnn trainer step {step} clip {clip}: loss {loss:.8f} float64 {lo.item():.8f}")
        assert abs(loss - lo.item()) < 1e-4 * abs(lo.item()), (step, loss, lo.item())
    if clip:
        assert min(norms) > clip, norms                        # the clip was active
    assert model.trainer.graph is not None
    sd, sdr = model.netG.state_dict(), ref.state_dict()
    for key in sdr:
        assert rel(sd[key], sdr[key]) < (1e-3 if sdr[key].dim() == 1 else 1e-4), key


@pytest.mark.parametrize("loss", ["l2", "l2sum", "charbonnier", "ssim"])
def test_every_fused_pixel_loss_takes_a_step(loss):
    model = _model(True, loss=loss)
    g = torch.Generator().manual_seed(83)
    for step in range(2):
        Hh = torch.rand(2, 1, 24, 24, generator=g)
        model.feed_data({"L": Hh + torch.randn(Hh.shape, generator=g) * 0.1, "H": Hh})
        model.optimize_parameters(step)
        assert torch.isfinite(torch.tensor(model.log_dict["G_loss"]))
    assert all(torch.isfinite(p).all() for p in model.netG.parameters())


# ---- the model bank -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bank_select_reaches_the_engine(dt):
    """Three entries of distinct random weights: select(2) -> entry 0, select(5) -> entry 2; each forward matches the
    float64 forward of its own entry.  An engine that kept the packs of the previous entry fails the second."""
    torch.manual_seed(91)
    sds = {str(i): IRCNN(1, 1, 64).state_dict() for i in range(3)}
    bank = utils_model.IRCNNBank(IRCNN(1, 1, 64, compute_dtype=dt).to(dev).eval(), utils_model.load_ircnn_bank(sds))
    x = torch.rand(1, 1, 21, 19, generator=torch.Generator().manual_seed(92))
    ref = IRCNN(1, 1, 64).double()
    with torch.no_grad():
        for sigma, entry in ((2, 0), (5, 2), (1, 0)):
            out = bank.select(sigma)(x.to(dev))
            assert bank.current == entry
            ref.load_state_dict({k: v.double() for k, v in sds[str(entry)].items()})
            e = rel(out, ref(x.double()))
            print(f"bank {dt} sigma {sigma} -> entry {entry}: rel {e:.3e}")
            assert e < (1e-4 if dt == "fp32" else BF16_TOL[0])


# ---- DPIR with the IRCNN prior --------------------------------------------------------------------------------------------
def test_dpir_restore_with_the_ircnn_prior():
    """2 iterations on a 32 x 32 image against the same loop with the float64 data step on the host
    (utils_sisr.data_solution) and the float64 network of the selected entry, at the fp32 bar."""
    torch.manual_seed(95)
    sds = {str(i): IRCNN(1, 1, 64).state_dict() for i in range(25)}
    for sd in sds.values():          # small residuals: a prior step that stays near its input, as a trained one does
        sd["model.12.weight"].mul_(0.05)
    g = torch.Generator().manual_seed(96)
    L = torch.rand(1, 1, 32, 32, generator=g)
    k = torch.rand(5, 5, generator=g)
    k = k / k.sum()
    sigma, iters = 7.65 / 255, 2
    bank = utils_model.IRCNNBank(IRCNN(1, 1, 64).to(dev).eval(), utils_model.load_ircnn_bank(sds))
    E = dpir_restore(bank, L.to(dev), k.to(dev), sf=1, noise_level_img=sigma, iter_num=iters, x8=True, denoiser="ircnn")
    # the reference loop
    rhos, sigmas = utils_pnp.get_rho_sigma(max(0.255 / 255, sigma), iters, 49.0, max(0.255, 255 * sigma), 1.0)
    L64, ref = L.double(), IRCNN(1, 1, 64).double().eval()
    pre = utils_sisr.pre_calculate(L64, k.double().view(1, 1, 5, 5), 1)
    inverse = {0: 0, 1: 1, 2: 2, 3: 5, 4: 4, 5: 3, 6: 6, 7: 7}
    x, used = L64, []
    with torch.no_grad():
        for i in range(iters):
            x = utils_sisr.data_solution(x, *pre, float(torch.tensor(float(rhos[i]), dtype=torch.float32)), 1)
            x = util.augment_img_tensor4(x, i % 8)
            idx = utils_model.ircnn_index(float(sigmas[i]) * 255.0)
            used.append(idx)
            ref.load_state_dict({kk: v.double() for kk, v in sds[str(idx)].items()})
            x = util.augment_img_tensor4(ref(x), inverse[i % 8])
    e = rel(E, x)
    print(f"dpir ircnn: entries {used}, rel {e:.3e}")
    assert len(set(used)) == 2 and E.shape == L.shape and e < 1e-4
    with pytest.raises(ValueError, match="IRCNNBank"):
        dpir_restore(bank.net, L.to(dev), k.to(dev), iter_num=1, denoiser="ircnn")
    with pytest.raises(ValueError, match="neither"):
        dpir_restore(bank, L.to(dev), k.to(dev), iter_num=1, denoiser="dncnn")
