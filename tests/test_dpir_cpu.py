"""DPIR on the host: the (rho, sigma) schedule, the torch.fft data step and the loop's bookkeeping, in float64.

No reference file backs these: they check properties the method has by construction (the schedule's end points and
its rho sigma^2 invariant, the data step's fixed point, the proximal map's monotone approach to it, the augmentation
round trip).
"""
import numpy as np
import torch

from kair_amd.main_dpir import dpir_restore
from kair_amd.utils import utils_pnp, utils_sisr

F64 = torch.float64


def gauss_kernel(n=7, s=1.6):
    ax = torch.arange(n, dtype=F64) - n // 2
    k = torch.exp(-(ax[:, None] ** 2 + 0.5 * ax[None, :] ** 2) / (2 * s * s))     # anisotropic: not flip-symmetric in shape
    k[0, 1] += 0.05                                                                # ... nor in values
    return k / k.sum()


def test_get_rho_sigma_schedule():
    sigma = 2.55 / 255
    rhos, sigmas = utils_pnp.get_rho_sigma(sigma, 8, 49.0, 2.55)
    want = np.logspace(np.log10(49.0), np.log10(2.55), 8).astype(np.float32)
    assert len(rhos) == 8 and sigmas.shape == (8,)
    np.testing.assert_allclose(sigmas * 255.0, want, rtol=3e-7, atol=0)      # one float32 rounding of the / 255 * 255
    assert abs(float(sigmas[0]) * 255 - 49.0) < 49.0 * 2.0 ** -22
    assert abs(float(sigmas[-1]) * 255 - 2.55) < 2.55 * 2.0 ** -22
    assert all(sigmas[i] > sigmas[i + 1] for i in range(7))
    for r, s in zip(rhos, sigmas):
        assert abs(float(r) * float(s) ** 2 - 0.23 * sigma ** 2) < 1e-6 * 0.23 * sigma ** 2
    _, lin = utils_pnp.get_rho_sigma(sigma, 8, 49.0, 2.55, w=0.0)
    np.testing.assert_allclose(lin * 255.0, np.linspace(49.0, 2.55, 8).astype(np.float32), rtol=3e-7, atol=0)
    _, mix = utils_pnp.get_rho_sigma(sigma, 8, 49.0, 2.55, w=0.25)
    np.testing.assert_allclose(mix, 0.25 * sigmas + 0.75 * lin, rtol=1e-6, atol=0)


def blurred(Hh, Ww, sf, seed, C=3, B=2):
    g = torch.Generator().manual_seed(seed)
    x_true = torch.rand(B, C, Hh, Ww, generator=g, dtype=F64)
    k = gauss_kernel()
    y = utils_sisr.wrap_blur(x_true, k)[..., ::sf, ::sf].contiguous()
    return x_true, k, y


def test_host_functions_match_their_definitions():
    """p2o is the transfer function of wrap_blur; upsample zero-fills; splits groups the sf^2 aliases."""
    x_true, k, y = blurred(35, 26, 1, 3)
    FB = utils_sisr.p2o(k[None, None], (35, 26))
    via_fft = torch.real(torch.fft.ifft2(FB * torch.fft.fft2(x_true)))
    assert (via_fft - y).abs().max() < 1e-12
    u = utils_sisr.upsample(y, 3)
    assert u.shape[-2:] == (105, 78) and torch.equal(u[..., ::3, ::3], y) and u.sum() == y.sum()
    a = torch.arange(12 * 8, dtype=F64).view(1, 1, 12, 8)
    s = utils_sisr.splits(a, 2)
    assert s.shape == (1, 1, 6, 4, 4)
    assert sorted(s[0, 0, 1, 2].tolist()) == sorted([a[0, 0, 1 + p * 6, 2 + q * 4].item() for p in (0, 1) for q in (0, 1)])


def test_data_solution_fixed_point():
    """Noiseless y = (k (*) x_true)[::sf, ::sf]: x_true minimises both terms, so the step maps it to itself."""
    for Hh, Ww, sf in [(35, 26, 1), (52, 44, 4)]:
        x_true, k, y = blurred(Hh, Ww, sf, 11 + sf)
        pre = utils_sisr.pre_calculate(y, k, sf)
        for alpha in (0.003, 0.7):
            z = utils_sisr.data_solution(x_true, *pre, alpha, sf)
            assert z.dtype == F64 and z.shape == x_true.shape
            assert (z - x_true).abs().max() < 1e-10, (Hh, Ww, sf, alpha)
        al = torch.tensor([0.003, 0.7], dtype=F64)
        z = utils_sisr.HostDataStep(y, k, sf).solve(x_true, al)                  # per-image alpha
        assert (z - x_true).abs().max() < 1e-10


def test_proximal_point_monotonicity():
    """With the identity as the denoiser the loop is the proximal-point iteration of the data term: the distance to
    its minimiser x_true never grows (the proximal map is firmly nonexpansive and x_true is a fixed point)."""
    x_true, k, y = blurred(35, 26, 1, 5, C=1, B=1)
    seen = []

    def identity(x):
        seen.append(x[:, :-1].clone())
        return x[:, :-1]

    E = dpir_restore(None, y, k, sf=1, noise_level_img=0.0, iter_num=8, x8=False, denoiser=identity)
    assert len(seen) == 8 and torch.equal(E, seen[-1])
    d = [(x - x_true).norm().item() for x in seen]
    assert all(d[i + 1] <= d[i] for i in range(7)), d
    assert d[-1] < d[0] and d[0] < (y - x_true).norm().item()


def test_x8_bookkeeping():
    x_true, k, y = blurred(18, 26, 1, 9, C=1, B=2)
    g = torch.Generator().manual_seed(10)
    patterns = {}

    def asymmetric(x):                       # shape-preserving; a fixed per-pixel pattern for each orientation
        hw = tuple(x.shape[-2:])
        if hw not in patterns:
            patterns[hw] = 0.01 * torch.rand(hw, generator=g, dtype=F64)
        return x[:, :-1] + patterns[hw]

    E = dpir_restore(None, y, k, iter_num=8, x8=True, denoiser=asymmetric)
    assert E.shape == y.shape and len(patterns) == 2        # both orientations were denoised, the result is upright
    scale = lambda x: 0.9 * x[:, :-1] + 0.05                # noqa: E731  (commutes with every augmentation)
    E8 = dpir_restore(None, y, k, iter_num=8, x8=True, denoiser=scale)
    E1 = dpir_restore(None, y, k, iter_num=8, x8=False, denoiser=scale)
    assert (E8 - E1).abs().max() < 1e-12
    # sf 2: the x sf start and the HR grid
    x_true, k, y = blurred(36, 52, 2, 12, C=1, B=1)
    E8 = dpir_restore(None, y, k, sf=2, iter_num=8, x8=True, denoiser=scale)
    E1 = dpir_restore(None, y, k, sf=2, iter_num=8, x8=False, denoiser=scale)
    assert E8.shape == (1, 1, 36, 52) and (E8 - E1).abs().max() < 1e-12
