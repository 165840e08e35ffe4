"""kair_ssim_loss / kair_ssim_loss_nchw (G_lossfn_type 'ssim') on the MI355X against SSIMLoss in float64 on the CPU
(plain torch + autograd), and the fused step with loss_type 'ssim'.

fp32 bars.  The kernels get 4 x the error torch's own fp32 CPU SSIMLoss (value and autograd gradient) shows against
float64 on the NCHW cases' inputs -- the factor covers a different but equally valid fp32 summation order.  One
shape's fp32 error is a sample of rounding noise (the value's ranges from 3e-8, half an fp32 ulp of the value, to
4e-7 over the four shapes), so the bar is the largest over the four shapes; it is measured when the module runs
(fp32_bars) and was, when this was written:
    shape          |value - f64|   max|grad - f64| / max|grad f64|
    1x1x7x9          2.7e-8          3.5e-6
    2x3x37x45        2.3e-7          3.8e-5
    1x1x70x33        3.6e-7          2.5e-5
    2x1x64x64        1.6e-7          4.3e-5
so value 4 x 3.6e-7 = 1.4e-6 (times |weight|) and gradient 4 x 4.3e-5 = 1.7e-4 of the largest reference gradient.
The kernels measured (MI355X, weight -1): value 9.2e-8 / 1.1e-7 / 2.7e-9 / 2.2e-7, gradient 1.9e-6 / 1.2e-5 / 1.1e-5
/ 2.0e-5 on the four shapes.
bf16 rows: against the bf16 rounding of the float64 gradient within one bf16 ulp of the largest gradient, and, in the
form of tests/test_kernels_gpu.py test_pixel_loss_bf16_rows, against the unrounded gradient within 2^-8 of the largest
(measured: at most one ulp / 0.6 of that bar).

Fused step bars: the first step's loss and flat gradient against the same network's autograd path (SSIMLoss on net(L)
and backward(): the NCHW kernel, then the engine's backward_from_grad) may differ by 2 x what the same comparison
shows with the Charbonnier loss, measured in the same test run (figures in test_fused_step's docstring).
fp32_bars' value bar also holds the one fused FFDNet step against float64 SSIM of the same forward output.
"""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.model_plain import CharbonnierLoss, SSIMLoss  # noqa: E402
from kair_amd.models.network_dncnn import DnCNN  # noqa: E402
from kair_amd.models.network_swinir import SwinIR  # noqa: E402

dev = torch.device("cuda")
NCHW_SHAPES = [(1, 1, 7, 9),      # smaller than the window: everything is border
               (2, 3, 37, 45),    # no tile multiple
               (1, 1, 70, 33),    # several tiles down, a partial tile across
               (2, 1, 64, 64)]    # exact tiles


def make_pair(shape, seed):
    """(E, H) in [0, 1] with structure: a smooth ramp / wave + noise of amplitude 0.05 (H), E = H + 0.05 noise."""
    g = torch.Generator().manual_seed(seed)
    B, C, Hh, Ww = shape
    yy = torch.linspace(0, 1, Hh, dtype=torch.float64).view(1, 1, Hh, 1)
    xx = torch.linspace(0, 1, Ww, dtype=torch.float64).view(1, 1, 1, Ww)
    ph = torch.arange(B * C, dtype=torch.float64).view(B, C, 1, 1)
    ramp = 0.15 + 0.7 * (0.5 + 0.5 * torch.sin(2.0 * yy + 3.0 * xx + 0.7 * ph)) * (0.4 + 0.6 * xx)
    Ht = (ramp + 0.05 * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)).clamp(0, 1)
    E = (Ht + 0.05 * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)).clamp(0, 1)
    return E.float(), Ht.float()


def _torch_ssim(E, Ht, dtype):
    e = E.to(dtype).requires_grad_(True)
    loss = SSIMLoss()(e, Ht.to(dtype))
    loss.backward()
    return loss.item(), e.grad


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of a shape and their float64 reference (weight 1): computed once, shared, never modified."""
    E, Ht = make_pair(shape, 100 + sum(shape))
    val, grad = _torch_ssim(E, Ht, torch.float64)
    return E, Ht, val, grad


@functools.lru_cache(maxsize=None)
def fp32_bars():
    """4 x torch's fp32 CPU error against float64 over the NCHW cases -> (value bar, relative gradient bar)."""
    ev = eg = 0.0
    for shape in NCHW_SHAPES:
        E, Ht, val, grad = case(shape)
        v32, g32 = _torch_ssim(E, Ht, torch.float32)
        dg = ((g32.double() - grad).abs().max() / grad.abs().max()).item()
        print(f"fp32 torch vs float64 {shape}: value {abs(v32 - val):.3g} gradient {dg:.3g}")
        ev, eg = max(ev, abs(v32 - val)), max(eg, dg)
    return 4 * ev, 4 * eg


def run_kernel(E, Ht, weight, ldc=None, ps_r=1, dtype=torch.float32):
    """-> (loss, dE) of one call; rows layouts start from NaN so that every slot must be written."""
    B, C, Hh, Ww = E.shape
    loss = torch.full((1,), float("nan"), device=dev)
    if ldc is None:
        dE = torch.full(E.shape, float("nan"), device=dev)
    else:
        dE = torch.full((B * (Hh // ps_r) * (Ww // ps_r), ldc), float("nan"), device=dev, dtype=dtype)
    ws = H.ssim_workspace(B, C, Hh, Ww, dev)
    H.ssim_loss(E.to(dev), Ht.to(dev), loss, dE, ldc, weight, B, C, Hh, Ww, ws, ps_r=ps_r)
    torch.cuda.synchronize()
    return loss.item(), dE.cpu()


def rows_to_nchw(dE, shape, ldc, r):
    """The rows layout back to [B, C, H, W] + the pad slots."""
    B, C, Hh, Ww = shape
    t = dE.float().view(B, Hh // r, Ww // r, ldc)
    used = t[..., :C * r * r].reshape(B, Hh // r, Ww // r, C, r, r)
    img = used.permute(0, 3, 1, 4, 2, 5).reshape(B, C, Hh, Ww)
    return img, t[..., C * r * r:]


@pytest.mark.parametrize("weight", [-1.0, 0.5])
@pytest.mark.parametrize("shape", NCHW_SHAPES)
def test_nchw_value_and_gradient(shape, weight):
    E, Ht, val, grad = case(shape)
    bar_v, bar_g = fp32_bars()
    loss, dE = run_kernel(E, Ht, weight)
    ev = abs(loss - weight * val)
    eg = ((dE.double() - weight * grad).abs().max() / (abs(weight) * grad.abs().max())).item()
    print(f"ssim nchw {shape} w {weight}: value err {ev:.3g} (bar {abs(weight) * bar_v:.3g}) grad err {eg:.3g} (bar {bar_g:.3g})")
    assert ev <= abs(weight) * bar_v
    assert eg <= bar_g


ROWS = [   # (shape, dtype, ldc, ps_r): the layouts the engines' loss hooks use
    ((2, 3, 37, 45), torch.bfloat16, 16, 1),   # SwinIR / RRDBNet tails
    ((2, 3, 37, 45), torch.float32, 4, 1),     # the fp32x3 narrow conv_last
    ((2, 3, 37, 45), torch.float32, 16, 1),    # DnCNN
    ((2, 3, 37, 45), torch.float32, 8, 1),     # USRNet / DRUNet (C8 with C = 3)
    ((2, 1, 64, 64), torch.bfloat16, 16, 1),
    ((2, 3, 36, 44), torch.bfloat16, 16, 2),   # FFDNet / pixelshuffledirect x2
    ((2, 3, 36, 44), torch.float32, 16, 2),
    ((1, 3, 33, 45), torch.float32, 32, 3),    # pixelshuffledirect x3
    ((1, 3, 33, 45), torch.bfloat16, 32, 3),
]


@pytest.mark.parametrize("shape,dtype,ldc,r", ROWS)
def test_rows_layouts(shape, dtype, ldc, r):
    E, Ht, val, grad = case(shape)
    bar_v, bar_g = fp32_bars()
    weight = -1.0
    loss, dE = run_kernel(E, Ht, weight, ldc=ldc, ps_r=r, dtype=dtype)
    img, pad = rows_to_nchw(dE, shape, ldc, r)
    assert pad.numel() > 0 and (pad == 0).all()          # exactly zero (and written: the buffer started as NaN)
    assert abs(loss - weight * val) <= bar_v
    ref = weight * grad
    if dtype == torch.bfloat16:
        # against the bf16 rounding of the reference: one bf16 ulp (2^-7 of its binade) of the largest gradient -- a
        # stored value is the rounding of an fp32 number next to the reference, so it may land on the neighbouring
        # bf16 number; and test_pixel_loss_bf16_rows' own form, against the unrounded reference: 2^-8 of the largest
        mx = ref.abs().max().item()
        ulp = 2.0 ** (math.floor(math.log2(mx)) - 7)
        err = (img.double() - ref.float().bfloat16().double()).abs().max().item()
        err0 = (img.double() - ref).abs().max().item()
        print(f"ssim rows {shape} bf16 ldc {ldc} r {r}: vs bf16(ref) {err:.3g} (ulp {ulp:.3g}) vs ref {err0:.3g} "
              f"(bar {2 ** -8 * mx:.3g})")
        assert err <= ulp
        assert err0 <= 2 ** -8 * mx
    else:
        err = ((img.double() - ref).abs().max() / ref.abs().max()).item()
        print(f"ssim rows {shape} fp32 ldc {ldc} r {r}: rel err {err:.3g} bar {bar_g:.3g}")
        assert err <= bar_g


def test_rows_equal_nchw_and_repeat_bitwise():
    """Two calls on the same buffers are bit-identical (fixed-order sums, no atomics), and the fp32 rows hold the NCHW
    form's numbers."""
    shape = (2, 3, 37, 45)
    E, Ht, _, _ = case(shape)
    B, C, Hh, Ww = shape
    Ed, Hd = E.to(dev), Ht.to(dev)
    ws = H.ssim_workspace(B, C, Hh, Ww, dev)
    out = []
    for _ in range(2):
        loss, dE = torch.zeros(1, device=dev), torch.zeros(B * Hh * Ww, 16, device=dev, dtype=torch.bfloat16)
        H.ssim_loss(Ed, Hd, loss, dE, 16, -1.0, B, C, Hh, Ww, ws)
        out.append((loss.clone(), dE.clone()))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16))
    l1, g1 = run_kernel(E, Ht, -1.0)
    l2, g2 = run_kernel(E, Ht, -1.0, ldc=16)
    assert l1 == l2 == out[0][0].item()
    assert torch.equal(rows_to_nchw(g2, shape, 16, 1)[0], g1)


def test_argument_errors_launch_nothing():
    L = H.lib()
    E, Ht = (t.to(dev) for t in make_pair((1, 1, 7, 8), 1))
    loss = torch.full((1,), 7.0, device=dev)
    dE = torch.full((4 * 4, 16), 7.0, device=dev)
    ws = H.ssim_workspace(1, 1, 7, 8, dev)
    s = H.stream_ptr()
    args = lambda ps_r, w, ldc=16: (E.data_ptr(), Ht.data_ptr(), loss.data_ptr(), dE.data_ptr(), H.F32, ldc, ps_r, 1.0,
                                    1, 1, 7, 8, w, s)
    assert L.kair_ssim_loss(*args(2, ws.data_ptr())) == -1           # odd H with ps_r 2
    assert b"ps_r" in L.kair_last_error()
    assert L.kair_ssim_loss(*args(1, None)) == -1                    # null workspace
    assert L.kair_ssim_loss(*args(1, ws.data_ptr() + 4)) == -1       # misaligned workspace
    assert L.kair_ssim_loss(*args(1, ws.data_ptr(), ldc=0)) == -1    # C r^2 > ldc
    assert L.kair_ssim_loss_nchw(E.data_ptr(), Ht.data_ptr(), loss.data_ptr(), None, 1.0, 1, 1, 7, 8, ws.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and (dE == 7.0).all()


def test_workspace_query_monotone_and_sufficient():
    q = H.ssim_workspace_bytes
    assert q(0, 3, 8, 8) == 0
    base = (2, 3, 33, 45)
    for i in range(4):
        prev = 0
        for v in range(1, 100):
            a = list(base)
            a[i] = v
            cur = q(*a)
            assert cur % 16 == 0 and cur > prev, (a, cur, prev)
            prev = cur
    for shape in [(2, 3, 37, 45), (1, 1, 7, 9), (2, 1, 64, 64)]:
        B, C, Hh, Ww = shape
        n = q(*shape)
        buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        E, Ht, val, _ = case(shape)
        loss, dE = torch.empty(1, device=dev), torch.empty(shape, device=dev)
        H.ssim_loss(E.to(dev), Ht.to(dev), loss, dE, None, 1.0, B, C, Hh, Ww, buf[:n])
        torch.cuda.synchronize()
        assert (buf[n:] == 0xA5).all()
        assert abs(loss.item() - val) <= fp32_bars()[0]
    with pytest.raises(ValueError):
        H.ssim_loss(E.to(dev), Ht.to(dev), loss, dE, None, 1.0, B, C, Hh, Ww, buf[:n - 16])


# ---------------------------------------------------------------------------------------------------------------------
# the fused step
# ---------------------------------------------------------------------------------------------------------------------
def _dncnn(dt):
    return DnCNN(1, 1, 64, 4, "R", compute_dtype=dt)


def _swinir(dt):
    return SwinIR(upscale=2, in_chans=3, img_size=16, window_size=8, img_range=1.0, depths=[2], embed_dim=60,
                  num_heads=[6], mlp_ratio=2, upsampler="pixelshuffledirect", resi_connection="1conv",
                  drop_path_rate=0.0, compute_dtype=dt)


def _batch(kind):
    if kind == "dncnn":
        _, Ht = make_pair((2, 1, 24, 24), 7)
        g = torch.Generator().manual_seed(8)
        return (Ht + 0.1 * torch.randn(Ht.shape, generator=g)).to(dev), Ht.to(dev)
    _, Ht = make_pair((2, 3, 32, 32), 9)
    return torch.nn.functional.avg_pool2d(Ht, 2).to(dev), Ht.to(dev)


def _first_step_vs_autograd(mk, state, L, Ht, **loss_kw):
    """(relative loss difference, max gradient difference over the largest gradient) of a fused first step against
    the autograd path of the same network, and the fused trainer's 3-step (losses, parameters)."""
    net, twin = mk(), mk()
    net.load_state_dict(state)
    twin.load_state_dict(state)
    net, twin = net.to(dev).train(), twin.to(dev).train()
    tr = FusedTrainer(net, None, lr=1e-4, E_decay=0, loss_weight=-1.0, use_graph=False, **loss_kw)
    loss = tr.step(L, Ht).item()
    tr.check_range()
    g_fused = tr.flat_g.clone()
    fn = SSIMLoss() if loss_kw.get("loss_type") == "ssim" else CharbonnierLoss(loss_kw["charb_eps"])
    lo = -1.0 * fn(twin(L), Ht)
    lo.backward()
    g_auto = torch.cat([p.grad.reshape(-1) for p in twin.parameters()])
    torch.cuda.synchronize()
    return (abs(loss - lo.item()) / abs(lo.item()),
            ((g_fused - g_auto).abs().max() / g_auto.abs().max()).item())


@pytest.mark.parametrize("kind,dt", [("dncnn", "fp32"), ("dncnn", "bf16"), ("swinir", "fp32"), ("swinir", "bf16"),
                                     ("swinir", "fp32x3")])
def test_fused_step(kind, dt):
    """FusedTrainer(loss_type='ssim', loss_weight=-1), 3 steps: eager and graph-replayed steps bit-equal; the first
    step's loss and flat gradient against the autograd path within 2 x the Charbonnier comparison's differences.
    Measured (loss difference relative / gradient difference over the largest gradient; Charbonnier -> SSIM):
        dncnn fp32     0 / 7.1e-8       -> 0 / 0
        dncnn bf16     9.1e-8 / 0       -> 0 / 0
        swinir fp32    0 / 9.3e-8       -> 0 / 0
        swinir bf16    0 / 0            -> 0 / 0
        swinir fp32x3  0 / 1.9e-7       -> 0 / 1.8e-7
    (the SSIM kernels run the same arithmetic on both paths, so they agree bit for bit except on fp32x3, whose two
    paths pick different gradient exponents)."""
    mk = functools.partial(_dncnn if kind == "dncnn" else _swinir, dt)
    torch.manual_seed(21)
    state = copy.deepcopy(mk().state_dict())
    L, Ht = _batch(kind)
    runs = []
    for use_graph in (False, True):
        net = mk()
        net.load_state_dict(state)
        net = net.to(dev).train()
        tr = FusedTrainer(net, None, lr=1e-4, E_decay=0, loss_weight=-1.0, use_graph=use_graph, loss_type="ssim")
        losses = [tr.step(L, Ht).clone() for _ in range(3)]
        tr.check_range()
        torch.cuda.synchronize()
        assert (tr.graph is not None) == use_graph
        assert not tr.range_events
        runs.append((torch.cat(losses).cpu(), tr.flat_p.clone().cpu()))
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert all(-1.0 <= v < 0.0 for v in runs[0][0].tolist())
    assert runs[0][0][2] < runs[0][0][0]   # toward -1 on the fixed batch
    cl, cg = _first_step_vs_autograd(mk, state, L, Ht, charb_eps=1e-6)
    sl, sg = _first_step_vs_autograd(mk, state, L, Ht, loss_type="ssim")
    print(f"fused vs autograd {kind} {dt}: charbonnier loss {cl:.3g} grad {cg:.3g}; ssim loss {sl:.3g} grad {sg:.3g}")
    assert sl <= 2 * cl, (sl, cl)
    assert sg <= 2 * cg, (sg, cg)


def _opt(model, netG, use_graph=True):
    return {"model": model, "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
            "netG": netG,
            "train": {"G_lossfn_type": "ssim", "G_lossfn_weight": -1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                      "use_hip_graph": use_graph}}


def test_define_model_ssim_uses_the_fused_trainer():
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(31)
    model = define_Model(dict_to_nonedict(_opt("plain", {"net_type": "dncnn", "in_nc": 1, "out_nc": 1, "nc": 64, "nb": 4,
                                                          "act_mode": "R", "init_type": "orthogonal",
                                                          "init_bn_type": "uniform", "init_gain": 0.2})))
    model.init_train()
    assert isinstance(model.trainer, FusedTrainer) and model.trainer.loss_type == "ssim"
    L, Ht = _batch("dncnn")
    losses = []
    for step in range(4):
        model.feed_data({"L": L, "H": Ht})
        model.optimize_parameters(step)
        losses.append(model.log_dict["G_loss"])
    assert all(-1.0 <= v < 0.0 for v in losses) and losses[-1] < losses[0], losses
    assert model.trainer.graph is not None
    assert "ssim_ws" in model.trainer.engine.cur
    model.test()
    E = model.current_visuals()["E"]
    assert E.shape == (1, 24, 24) and torch.isfinite(E).all()
    # the logged loss is -SSIM of what the network then computes, to the one Adam step between them
    ref = SSIMLoss()(model.E.double().cpu(), Ht.double().cpu()).item()
    assert abs(-ref - losses[-1]) < 0.05


def test_ffdnet_plain2_fused_ssim_step():
    """The ps_r = 2 call site: FFDNet's loss hook writes the pre-PixelShuffle(2) rows."""
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    torch.manual_seed(41)
    netg = {"net_type": "ffdnet", "in_nc": 1, "out_nc": 1, "nc": 16, "nb": 4, "act_mode": "R", "init_type": "orthogonal",
            "init_bn_type": "uniform", "init_gain": 1.0}
    model = define_Model(dict_to_nonedict(_opt("plain2", netg, use_graph=False)))
    model.init_train()
    assert isinstance(model.trainer, FusedTrainer)
    L, Ht = _batch("dncnn")
    C = torch.tensor([15.0, 40.0]).view(2, 1, 1, 1) / 255
    with torch.no_grad():
        E0 = model.netG(L, C.to(dev)).double().cpu()
    want = -SSIMLoss()(E0, Ht.double().cpu()).item()
    model.feed_data({"L": L, "H": Ht, "C": C})
    model.optimize_parameters(0)
    got = model.log_dict["G_loss"]
    assert abs(got - want) <= fp32_bars()[0], (got, want)   # (the kernel's value bar: the same E on both sides)
    assert torch.isfinite(model.trainer.flat_g).all() and model.trainer.flat_g.abs().max() > 0
