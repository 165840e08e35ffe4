"""DPIR on the MI355X: the three-launch data step (utils_sisr.DataStep), the restoration loop on the DRUNet engines, USRNet
at HR grids that are not 2^a 3^b, and the command-line driver.

Float64 side: the host utilities of kair_amd/utils/utils_sisr.py (plain torch.fft) and, for the networks, the float64
modules of tests/test_drunet_gpu.py (RefUNetRes) and oracle/convnets.py (USRNet).  `rel` and the fixed bars (2e-5 for the
data step, TOL["fp32"] for USRNet) are those of tests/test_usrnet_gpu.py.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import main_dpir  # noqa: E402
from kair_amd.models.network_unet import UNetRes  # noqa: E402
from kair_amd.models.network_usrnet import USRNet  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_pnp, utils_sisr  # noqa: E402
from oracle import convnets as ocv  # noqa: E402
from test_drunet_gpu import RefUNetRes  # noqa: E402
from test_usrnet_gpu import TOL, _usrnet_fwd_bwd_check  # noqa: E402

dev = torch.device("cuda")
F64 = torch.float64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rand_kernel(B, n, g):
    k = torch.rand(B, 1, n, n, generator=g, dtype=F64)
    return k / k.sum((-2, -1), keepdim=True)


@pytest.mark.parametrize("Hh,Ww,sf", [(35, 26, 1), (481, 321, 1), (75, 51, 3)])
def test_data_step_vs_float64(Hh, Ww, sf):
    """DataStep.solve vs float64 data_solution: per-image kernels with a per-image alpha [B], one shared kernel with a
    number."""
    g = torch.Generator().manual_seed(Hh + sf)
    B, C = 2, 3
    y = torch.rand(B, C, Hh // sf, Ww // sf, generator=g, dtype=F64)
    x = torch.rand(B, C, Hh, Ww, generator=g, dtype=F64)
    alpha = torch.tensor([0.004, 0.31], dtype=F64)
    for k, al in ((rand_kernel(B, 13, g), alpha), (rand_kernel(1, 9, g), 0.02), (rand_kernel(1, 5, g)[0, 0], alpha[1:])):
        ref = utils_sisr.HostDataStep(y, k, sf).solve(x, al)
        got = utils_sisr.DataStep(y.float().to(dev), k.to(dev), sf).solve(x.float().to(dev), al)
        e = rel(got, ref)
        print(f"DataStep ({Hh}, {Ww}, sf {sf}), k {tuple(k.shape)}: rel {e:.3e}")
        assert got.shape == (B, C, Hh, Ww) and e < 2e-5


def test_data_step_limits():
    y = torch.rand(1, 1, 8, 2049, device=dev)
    k = torch.full((3, 3), 1.0 / 9, device=dev)
    with pytest.raises(ValueError, match="2048"):
        utils_sisr.DataStep(y, k, 1)
    with pytest.raises(ValueError, match="2048"):
        utils_sisr.DataStep(y.transpose(-1, -2).contiguous(), k, 1)
    with pytest.raises(ValueError, match="LDS"):           # (1800 + 2 * 5 * 1801) * 8 = 158480 bytes > 150 KB
        utils_sisr.DataStep(torch.rand(1, 1, 360, 1, device=dev), k, 5)
    with pytest.raises(ValueError, match="kernel"):
        utils_sisr.DataStep(torch.rand(1, 1, 2, 8, device=dev), k, 1)


def noiseless(Hh, Ww, sf, seed, B=1, C=1):
    g = torch.Generator().manual_seed(seed)
    x_true = torch.rand(B, C, Hh, Ww, generator=g, dtype=F64)
    k = rand_kernel(1, 7, g)[0, 0]
    y = utils_sisr.wrap_blur(x_true, k)[..., ::sf, ::sf].contiguous()
    return x_true, k, y


@pytest.mark.parametrize("Hh,Ww,sf", [(35, 26, 1), (52, 44, 4)])
def test_fixed_point_on_device(Hh, Ww, sf):
    x_true, k, y = noiseless(Hh, Ww, sf, 14 + sf, B=2, C=3)
    step = utils_sisr.DataStep(y.float().to(dev), k.to(dev), sf)
    for alpha in (0.003, 0.7):
        e = rel(step.solve(x_true.float().to(dev), alpha), x_true)
        print(f"fixed point ({Hh}, {Ww}, sf {sf}), alpha {alpha}: rel {e:.3e}")
        assert e < 2e-5


def test_proximal_point_monotonicity_on_device():
    x_true, k, y = noiseless(35, 26, 1, 5)
    seen = []

    def identity(x):
        seen.append(x[:, :-1])
        return x[:, :-1]

    main_dpir.dpir_restore(None, y.float().to(dev), k.to(dev), sf=1, noise_level_img=0.0, iter_num=8, x8=False,
                           denoiser=identity)
    d = [(x.double().cpu() - x_true).norm().item() for x in seen]
    assert len(d) == 8 and all(d[i + 1] <= d[i] + 1e-5 * d[0] for i in range(7)), d
    assert d[-1] < d[0]


# ------------------------------------------------------------------------------------------------------------------
# the loop on a small DRUNet against the same loop in float64
# ------------------------------------------------------------------------------------------------------------------
NC, NB, SIGMA, ITERS = (16, 32, 64, 64), 1, 7.65 / 255, 3


def reference_loop(net, L, k, sf, dtype):
    """The DPIR loop written out with the host utilities and a torch-module denoiser, in `dtype` on the CPU."""
    L, k = L.to(dtype), k.to(dtype)
    rhos, sigmas = utils_pnp.get_rho_sigma(max(0.255 / 255, SIGMA), ITERS, 49.0, max(0.255, 255 * SIGMA), 1.0)
    pre = utils_sisr.pre_calculate(L, k, sf)
    x = L if sf == 1 else util.imresize(L, sf).to(dtype)
    inverse = {0: 0, 1: 1, 2: 2, 3: 5, 4: 4, 5: 3, 6: 6, 7: 7}
    with torch.no_grad():
        for i in range(ITERS):
            x = utils_sisr.data_solution(x, *pre, float(torch.tensor(float(rhos[i]), dtype=L.dtype)), sf)
            x = util.augment_img_tensor4(x, i % 8)
            h, w = x.shape[-2:]
            x = torch.cat((x, x.new_full((x.shape[0], 1, h, w), float(sigmas[i]))), dim=1)
            x = torch.nn.functional.pad(x, (0, -w % 8, 0, -h % 8), mode="replicate")
            x = net(x)[..., :h, :w]
            x = util.augment_img_tensor4(x, inverse[i % 8])
    return x


@functools.lru_cache(maxsize=None)
def loop_case(sf):
    """(state_dict, L, k, float64 result, rel of the float32 CPU loop against it), computed once per sf."""
    torch.manual_seed(60 + sf)
    net = UNetRes(2, 1, NC, NB)
    sd = {key: v.detach().clone() for key, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(61 + sf)
    h, w = (35, 52) if sf == 1 else (18, 26)
    x_true = torch.rand(1, 1, h * sf, w * sf, generator=g, dtype=F64)
    k = rand_kernel(1, 7, g)[0, 0].float()
    L = utils_sisr.wrap_blur(x_true, k)[..., ::sf, ::sf] + SIGMA * torch.randn(1, 1, h, w, generator=g, dtype=F64)
    L = L.float()                                         # the float32 image every loop starts from
    ref = RefUNetRes(2, 1, NC, NB)
    ref.load_state_dict(sd, strict=True)
    E64 = reference_loop(ref.double(), L, k, sf, F64)
    E32 = reference_loop(ref.float(), L, k, sf, torch.float32)
    return sd, L, k, E64, rel(E32, E64)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("sf", [1, 2])
def test_loop_vs_float64(sf, dt):
    """3 iterations, x8, sigma 7.65, a random-weight DRUNet (nc 16/32/64/64, nb 1, in_nc 2): L 35x52 at sf 1, L 18x26 at
    sf 2 (HR 36x52).  The bar of the fp32 engine is 4x the error of the same loop run in float32 on the CPU (torch
    modules, torch.fft) against float64: another summation order is worth a small factor, not an order of magnitude.
    bf16 is printed, not gated.
    Measured on the MI355X, rel against float64 -- sf 1: fp32 engine 3.60e-7, float32 CPU loop 3.73e-7 (bar 1.49e-6),
    bf16 engine 4.2e-3; sf 2: fp32 engine 2.47e-7, float32 CPU loop 2.80e-7 (bar 1.12e-6), bf16 engine 2.6e-3."""
    sd, L, k, E64, e_cpu32 = loop_case(sf)
    net = UNetRes(2, 1, NC, NB, compute_dtype=dt)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    E = main_dpir.dpir_restore(net, L.to(dev), k.to(dev), sf=sf, noise_level_img=SIGMA, iter_num=ITERS, x8=True)
    e = rel(E, E64)
    print(f"dpir loop sf {sf} {dt}: rel {e:.3e}; float32 CPU loop rel {e_cpu32:.3e}, bar {4 * e_cpu32:.3e}")
    assert E.shape == E64.shape and torch.isfinite(E).all()
    if dt == "fp32":
        assert e < 4 * e_cpu32


@pytest.mark.parametrize("lq,sf", [((13, 11), 2), ((7, 9), 3)])
def test_usrnet_at_awkward_sizes(lq, sf):
    """The small USRNet of test_usrnet_vs_golden with fixed-seed weights on HR grids 26x22 (2.13, 2.11) and 21x27
    (3.7, 3^3) vs the CPU oracle of that file run in float64: output and every parameter gradient at TOL['fp32']."""
    torch.manual_seed(70 + sf)
    kw = dict(n_iter=2, h_nc=32, in_nc=4, out_nc=3, nc=[16, 32, 64, 64], nb=2)
    net = USRNet(compute_dtype="fp32", **kw)
    ref = ocv.USRNet(**kw)
    ref.load_state_dict(net.state_dict(), strict=True)
    ref = ref.double()
    g = torch.Generator().manual_seed(71 + sf)
    B = 2
    x = torch.rand(B, 3, *lq, generator=g)
    k = rand_kernel(B, 7, g).float()
    sigma = torch.rand(B, 1, 1, 1, generator=g) * (25.0 / 255)
    out_ref = ref(x.double(), k.double(), sf, sigma.double())
    gout = torch.randn(out_ref.shape, generator=g)
    out_ref.backward(gout.double())
    grads = {n: p.grad for n, p in ref.named_parameters()}
    assert TOL["fp32"] == (1e-4, 5e-3, 1e-3)
    _usrnet_fwd_bwd_check(net.to(dev).train(), x, k, sf, sigma, out_ref, gout, grads, "fp32")


def test_driver_synthesize(tmp_path, capsys):
    from PIL import Image
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(3)
    sizes = {"a": (35, 52), "b": (40, 33)}
    for name, (h, w) in sizes.items():
        base = rng.random((h // 4 + 2, w // 4 + 2))
        img = np.kron(base, np.ones((4, 4)))[:h, :w] * 200 + rng.random((h, w)) * 40
        Image.fromarray(img.astype(np.uint8)).save(src / f"{name}.png")
    torch.manual_seed(80)
    torch.save(UNetRes(2, 1, NC, NB).state_dict(), tmp_path / "net.pth")
    np.save(tmp_path / "k.npy", rand_kernel(1, 5, torch.Generator().manual_seed(81))[0, 0].numpy())
    res = main_dpir.main(["--task", "sisr", "--sf", "2", "--model_path", str(tmp_path / "net.pth"), "--input", str(src),
                          "--kernel", str(tmp_path / "k.npy"), "--iter_num", "2", "--synthesize", "--out", str(out)])
    assert [n for n, _ in res] == ["a", "b"] and all(p is not None and np.isfinite(p) for _, p in res)
    assert "PSNR" in capsys.readouterr().out
    files = sorted(os.listdir(out))
    assert len(files) == 2
    for f, (h, w) in zip(files, sizes.values()):
        assert Image.open(out / f).size == (w - w % 2, h - h % 2)
