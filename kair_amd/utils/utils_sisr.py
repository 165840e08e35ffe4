"""The parts of the reference's utils/utils_sisr.py that USRNet's training data needs.

gen_kernel: the anisotropic Gaussian blur kernel of utils_sisr.py:172-215, restated in float64 on the host with
            the random draws as arguments.  The device form is kair_usr_gauss_kernels (csrc/synth_usr.hip).
degrade:    the classical degradation  L = (k (*) H, circular)[0::sf, 0::sf] + sigma N  of whole images on the
            device (kair_usr_degrade), the forward model USRNet's data step (p2o centring) assumes.
wrap_blur:  the same blur on the host (float64 torch conv2d over a wrapped pad), for the file-based dataset.
"""
import math
import random

import torch

from . import utils_image as util


def gen_kernel(k_size=25, lambda_1=None, lambda_2=None, theta=None, sf_k=None, mode_k=0, min_var=0.6, max_var=12.0,
               rng=None):
    """Normalised k_size x k_size Gaussian kernel, float64 tensor.

    Sigma = Q diag(lambda_1, lambda_2) Q^T with Q = [[cos, -sin], [sin, cos]](theta); the mean sits at
    mu = k_size // 2 + 0.5 (sf_k - k_size % 2) on both axes (the reference's shift for a x sf_k grid);
    raw[y][x] = exp(-0.5 z^T Sigma^-1 z), z = (x - mu, y - mu); divided by its sum; then the augment mode mode_k.
    Arguments left None are drawn from rng (random.Random; default the module-level generator) in the order
    lambda_1, lambda_2 ~ U(min_var, max_var), theta ~ U(0, pi), sf_k from [1, 2, 3, 4]."""
    rng = rng or random
    if lambda_1 is None:
        lambda_1 = rng.uniform(min_var, max_var)
    if lambda_2 is None:
        lambda_2 = rng.uniform(min_var, max_var)
    if theta is None:
        theta = rng.uniform(0.0, math.pi)
    if sf_k is None:
        sf_k = rng.choice([1, 2, 3, 4])
    cs, sn = math.cos(theta), math.sin(theta)
    Q = torch.tensor([[cs, -sn], [sn, cs]], dtype=torch.float64)
    inv = Q @ torch.diag(torch.tensor([1.0 / lambda_1, 1.0 / lambda_2], dtype=torch.float64)) @ Q.T
    mu = k_size // 2 + 0.5 * (sf_k - k_size % 2)
    ax = torch.arange(k_size, dtype=torch.float64) - mu
    zy, zx = torch.meshgrid(ax, ax, indexing="ij")
    raw = torch.exp(-0.5 * (inv[0, 0] * zx * zx + 2.0 * inv[0, 1] * zx * zy + inv[1, 1] * zy * zy))
    k = raw / raw.sum()
    return util.augment_img_tensor4(k[None, None], int(mode_k))[0, 0].contiguous()


def wrap_blur(x, k):
    """sum_{u, v} k[u, v] x[..., (i + kh // 2 - u) mod H, (j + kw // 2 - v) mod W]: scipy's
    ndimage.convolve(mode='wrap') for x [C, H, W] (or [N, C, H, W]) and one kernel [kh, kw], in float64.
    The pad is an index wrap, so it also holds for images smaller than the kernel."""
    lead = x.dim() == 3
    x = (x[None] if lead else x).double()
    kh, kw = k.shape[-2:]
    Hh, Ww = x.shape[-2:]
    rows = torch.arange(-(kh - 1 - kh // 2), Hh + kh // 2) % Hh
    cols = torch.arange(-(kw - 1 - kw // 2), Ww + kw // 2) % Ww
    xp = x[..., rows, :][..., cols]
    C = x.shape[1]
    w = k.double().flip(-1, -2).reshape(1, 1, kh, kw).expand(C, 1, kh, kw)
    y = torch.nn.functional.conv2d(xp, w, groups=C)
    return y[0] if lead else y


def degrade(H, k, sf, sigma=0, trunc8=False, seed=0, step=0):
    """L [N, C, ceil(Hs / sf), ceil(Ws / sf)] of device images H [N, C, Hs, Ws] (any Hs, Ws) on the device.

    k: [N, 1, kh, kw] per image, or one [kh, kw] / [1, 1, kh, kw] kernel for all; sigma: a number or a tensor of
    N noise levels (already divided by 255), 0 adds nothing; trunc8: floor(255 L0) / 255 before the noise, the
    reference loader's uint8 blur; (seed, step) key the noise."""
    from .. import _hip
    if H.dim() != 4 or not H.is_cuda:
        raise ValueError("degrade: H must be a device tensor [N, C, Hs, Ws]")
    N, C, Hs, Ws = H.shape
    H = H.float().contiguous()
    k = k.to(H.device, torch.float32).contiguous()
    if torch.is_tensor(sigma):
        sig = sigma.to(H.device, torch.float32).reshape(-1)
        sig = sig.expand(N).contiguous() if sig.numel() == 1 else sig.contiguous()
    else:
        sig = None if sigma == 0 else torch.full((N,), float(sigma), device=H.device)
    L = torch.empty(N, C, -(-Hs // sf), -(-Ws // sf), device=H.device)
    _hip.usr_degrade(H, k, int(sf), sig, trunc8, seed, step, L)
    return L
