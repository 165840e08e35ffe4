"""The penalty / noise-level schedule of DPIR (the reference's utils/utils_pnp.py get_rho_sigma).

The reference file was not available when this was written: the schedule is restated from the DPIR paper (Zhang et
al., "Plug-and-Play Image Restoration with Deep Denoiser Prior", eq. 6-8 and its released scripts' defaults) as
specified in this project's DPIR issue, and is pinned by tests/test_dpir_cpu.py.
"""
import numpy as np


def get_rho_sigma(sigma=2.55 / 255, iter_num=15, modelSigma1=49.0, modelSigma2=2.55, w=1.0, lamda=0.23):
    """(rhos, sigmas) of the iter_num half-quadratic-splitting iterations.

    sigmas: the denoiser's noise levels, from modelSigma1 / 255 down to modelSigma2 / 255 -- log-spaced (w = 1),
    linearly spaced (w = 0) or their blend, float32;  rhos[i] = lamda * sigma^2 / sigmas[i]^2, the weight of the
    quadratic coupling in the data step (`alpha` of utils_sisr.data_solution), sigma being the image's noise level
    (already divided by 255)."""
    S_log = np.logspace(np.log10(modelSigma1), np.log10(modelSigma2), iter_num).astype(np.float32)
    S_lin = np.linspace(modelSigma1, modelSigma2, iter_num).astype(np.float32)
    sigmas = (S_log * w + S_lin * (1 - w)) / 255.0
    rhos = [lamda * (sigma ** 2) / (s ** 2) for s in sigmas]
    return rhos, sigmas
