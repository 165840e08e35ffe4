"""The parts of the reference's utils/utils_sisr.py that USRNet's training data needs.

gen_kernel: the anisotropic Gaussian blur kernel of utils_sisr.py:172-215, restated in float64 on the host with
            the random draws as arguments.  The device form is kair_usr_gauss_kernels (csrc/synth_usr.hip).
degrade:    the classical degradation  L = (k (*) H, circular)[0::sf, 0::sf] + sigma N  of whole images on the
            device (kair_usr_degrade), the forward model USRNet's data step (p2o centring) assumes.
wrap_blur:  the same blur on the host (float64 torch conv2d over a wrapped pad), for the file-based dataset.

The closed-form data step of plug-and-play restoration (DPIR, kair_amd/main_dpir.py), for that forward model:
p2o, upsample, pre_calculate, data_solution: the reference's functions as plain torch.fft, in the dtype and on the
            device of their arguments -- the host path and the tests' float64 reference.  The reference file was not
            available when they were written; they restate network_usrnet_v1.py's p2o / upsample / DataNet.forward,
            which the reference's utils_sisr.py shares.
HostDataStep / DataStep: the data step of one (y, k, sf) as an object with solve(x, alpha): torch.fft, and the
            three-launch HIP path (csrc/fft.hip) with FB, the alias mean of |FB|^2 and conj(FB) F(y up) resident in
            the kernels' transposed layout.

The degradation of SRMD (network_srmd.py, data/dataset_srmd.py; the reference's utils_sisr.py restated from the
published method), in the dtype and on the device of the arguments -- the host path and the tests' float64 side:
anisotropic_gaussian, cal_pca_matrix, load_pca_matrix: the 15 x 15 kernel, and the PCA basis of its code;
srmd_degradation_map: the kernel's code (and the noise level) stretched over the LR grid;
srmd_degrade: circular blur, MATLAB-bicubic x1/sf, AWGN.  The device form is csrc/synth_srmd.hip.
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


# ------------------------------------------------------------------------------------------
# the closed-form data step  argmin_z ||(k (*) z)[::sf, ::sf] - y||^2 + alpha ||z - x||^2
# ------------------------------------------------------------------------------------------
FFT_MAX_LEN = 2048            # csrc/fft.hip: a line DFT is LDS-resident
FFT_MAX_LDS = 150 * 1024      # kair_usr_fft_cols: sf column lines, two buffers and the twiddle table


def splits(a, sf):
    """[..., H, W] -> [..., H / sf, W / sf, sf * sf]: the sf x sf blocks of a spectrum that alias onto one
    frequency of the sf-fold downsampled grid."""
    b = torch.stack(torch.chunk(a, sf, dim=-2), dim=-1)
    return torch.cat(torch.chunk(b, sf, dim=-2), dim=-1)


def p2o(psf, shape):
    """PSF [..., kh, kw] -> OTF [..., H, W]: zero-pad to shape, roll the centre tap (kh // 2, kw // 2) to the
    origin, fft2."""
    kh, kw = psf.shape[-2:]
    otf = psf.new_zeros(psf.shape[:-2] + tuple(shape))
    otf[..., :kh, :kw] = psf
    otf = torch.roll(otf, (-(kh // 2), -(kw // 2)), dims=(-2, -1))
    return torch.fft.fft2(otf)


def upsample(x, sf=3):
    """Zero-filling upsampler: x at [..., ::sf, ::sf] of an sf-fold larger grid."""
    z = x.new_zeros(x.shape[:-2] + (x.shape[-2] * sf, x.shape[-1] * sf))
    z[..., ::sf, ::sf] = x
    return z


def pre_calculate(y, k, sf):
    """(FB, FBC, F2B, FBFy) of LQ images y [B, C, h, w] and kernels k [B or 1, 1, kh, kw] (or [kh, kw]):
    FB = p2o(k) on the HR grid, its conjugate, |FB|^2, and conj(FB) fft2(upsample(y, sf))."""
    if k.dim() == 2:
        k = k[None, None]
    h, w = y.shape[-2:]
    FB = p2o(k.to(y.dtype), (h * sf, w * sf))
    FBC = torch.conj(FB)
    F2B = torch.abs(FB) ** 2
    FBFy = FBC * torch.fft.fft2(upsample(y, sf))
    return FB, FBC, F2B, FBFy


def data_solution(x, FB, FBC, F2B, FBFy, alpha, sf):
    """The minimiser of ||(k (*) z)[::sf, ::sf] - y||^2 + alpha ||z - x||^2 (circular blur), in closed form.
    alpha: a number or a tensor broadcastable against x ([B, 1, 1, 1])."""
    FR = FBFy + torch.fft.fft2(alpha * x)
    FBR = torch.mean(splits(FB * FR, sf), dim=-1)
    invW = torch.mean(splits(F2B, sf), dim=-1)
    invWBR = FBR / (invW + alpha)
    FX = (FR - FBC * invWBR.repeat(1, 1, sf, sf)) / alpha
    return torch.real(torch.fft.ifft2(FX))


def _alpha_of(alpha, B, device, dtype):
    """alpha (a number, a one-element tensor or [B]) as a tensor of 1 or B elements on `device`; no host read."""
    if torch.is_tensor(alpha):
        al = alpha.to(device=device, dtype=dtype).reshape(-1)
        if al.numel() not in (1, B):
            raise ValueError(f"data step: alpha has {al.numel()} elements for a batch of {B}")
        return al
    return torch.full((1,), float(alpha), device=device, dtype=dtype)


class HostDataStep:
    """solve(x, alpha) = data_solution(x, ..., alpha, sf) for one (y, k, sf), in y's dtype on y's device."""

    def __init__(self, y, k, sf=1):
        self.sf = int(sf)
        self.B = y.shape[0]
        self.pre = pre_calculate(y, k.to(y.device), self.sf)

    def solve(self, x, alpha):
        al = _alpha_of(alpha, self.B, x.device, x.dtype).reshape(-1, 1, 1, 1)
        return data_solution(x, *self.pre, al, self.sf)


class DataStep:
    """The data step on the device: FB, invW = mean(splits(|FB|^2, sf)) and FBFy are built once by the rows / cols
    passes of csrc/fft.hip and stay in the kernels' transposed float2 layout; solve(x, alpha) is three launches
    (rows DFT, columns DFT + closed form + inverse columns DFT, inverse rows DFT) and no host synchronisation.

    y: [B, C, h, w] device tensor; k: [B, 1, kh, kw], or one [1, 1, kh, kw] / [kh, kw] kernel for all images;
    alpha of solve: a number or a tensor of 1 or B elements.  The HR grid h sf x w sf may have any side lengths in
    [2, 2048]; sf whole column lines have to fit the 150 KB of LDS the columns pass uses."""

    def __init__(self, y, k, sf=1):
        from .. import _hip
        if y.dim() != 4 or not y.is_cuda:
            raise ValueError("DataStep: y must be a device tensor [B, C, h, w]")
        sf = int(sf)
        B, C, h, w = y.shape
        Hh, Ww = h * sf, w * sf
        if sf < 1 or not (2 <= Hh <= FFT_MAX_LEN and 2 <= Ww <= FFT_MAX_LEN):
            raise ValueError(f"DataStep: the HR grid {Hh} x {Ww} is outside the line-DFT range [2, {FFT_MAX_LEN}]")
        lds = (Hh + 2 * sf * (Hh + 1)) * 8
        if lds > FFT_MAX_LDS:
            raise ValueError(f"DataStep: sf {sf} column lines of {Hh} need {lds} bytes of LDS (limit {FFT_MAX_LDS})")
        if k.dim() == 2:
            k = k[None, None]
        if k.dim() != 4 or k.shape[1] != 1 or k.shape[0] not in (1, B):
            raise ValueError(f"DataStep: k {tuple(k.shape)} is neither [B, 1, kh, kw] nor one kernel")
        kh, kw = k.shape[-2:]
        if kh > Hh or kw > Ww:
            raise ValueError(f"DataStep: the {kh} x {kw} kernel is larger than the {Hh} x {Ww} grid")
        dev = y.device
        k = k.to(dev, torch.float32).expand(B, 1, kh, kw).contiguous()
        y = y.float().contiguous()
        self.shape, self.sf = (B, C, Hh, Ww), sf
        self.FB = torch.empty(B * Hh * Ww * 2, device=dev)
        self.invW = torch.empty(B * (Hh // sf) * (Ww // sf), device=dev)
        self.FBFy = torch.empty(B * C * Hh * Ww * 2, device=dev)
        self.T = torch.empty_like(self.FBFy)
        _hip.usr_fft_rows(k, _hip.USR_SRC_PSF, 1, 0, kh, kw, 1, self.FB, B, Hh, Ww)
        _hip.usr_fft_cols(_hip.USR_COL_FB, self.FB, self.FB, None, None, None, self.invW, None, 0, None, B, 1, Hh, Ww, sf)
        _hip.usr_fft_rows(y, _hip.USR_SRC_ZUP, C, 0, 0, 0, sf, self.FBFy, B * C, Hh, Ww)
        _hip.usr_fft_cols(_hip.USR_COL_FBFY, self.FBFy, self.FBFy, self.FB, None, None, self.invW, None, 0, None, B * C,
                          C, Hh, Ww, sf)

    def solve(self, x, alpha):
        from .. import _hip
        B, C, Hh, Ww = self.shape
        if tuple(x.shape) != self.shape or x.device != self.FB.device:
            raise ValueError(f"DataStep.solve: x {tuple(x.shape)} on {x.device}, expected {self.shape} on {self.FB.device}")
        al = _alpha_of(alpha, B, x.device, torch.float32)
        z = torch.empty(B, C, Hh, Ww, device=x.device)
        _hip.usr_fft_rows(x.float().contiguous(), _hip.USR_SRC_NCHW, C, 0, 0, 0, 1, self.T, B * C, Hh, Ww)
        _hip.usr_fft_cols(_hip.USR_COL_DATA_FWD, self.T, self.T, self.FB, self.FBFy, None, self.invW, al,
                          int(al.numel() > 1), None, B * C, C, Hh, Ww, self.sf)
        _hip.usr_ifft_rows(self.T, z, False, C, 0, 1.0 / (Hh * Ww), B * C, Hh, Ww)
        return z


# ------------------------------------------------------------------------------------------
# SRMD: degradation maps  (kernel -> PCA code -> stretched map) and the degradation itself
# ------------------------------------------------------------------------------------------
SRMD_KSIZE, SRMD_DIM_PCA = 15, 15


def anisotropic_gaussian(ksize=15, theta=0.0, l1=6.0, l2=6.0, dtype=torch.float64, device="cpu"):
    """k(x) ~ exp(-x^T Sigma^-1 x / 2) on the integer grid centred at (ksize - 1) / 2, sum 1: [ksize, ksize], rows y,
    columns x.  Sigma = R(theta) diag(l1, l2) R(theta)^T, R = [[cos, -sin], [sin, cos]]; l1, l2 are its eigenvalues
    (variances, in pixels^2)."""
    cs, sn = math.cos(theta), math.sin(theta)
    a11 = cs * cs / l1 + sn * sn / l2
    a12 = cs * sn * (1.0 / l1 - 1.0 / l2)
    a22 = sn * sn / l1 + cs * cs / l2
    ax = torch.arange(ksize, dtype=dtype, device=device) - (ksize - 1) / 2.0
    zy, zx = torch.meshgrid(ax, ax, indexing="ij")
    raw = torch.exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy))
    return raw / raw.sum()


def vec_f(k):
    """[..., kh, kw] -> [..., kh kw], column-major (numpy's order='F'): element c kh + r is k[r][c]."""
    return k.transpose(-1, -2).reshape(*k.shape[:-2], -1)


def draw_srmd_kernel(rng, l_max=10.0):
    """(theta, l1, l2) of one training kernel: theta ~ U(0, pi), l1 ~ U(0.1, l_max), l2 ~ U(0.1, l1), in that order
    from rng (random.Random)."""
    theta = rng.uniform(0.0, math.pi)
    l1 = rng.uniform(0.1, l_max)
    return theta, l1, rng.uniform(0.1, l1)


_PCA_CACHE = {}


def cal_pca_matrix(ksize=15, l_max=10.0, dim_pca=15, num_samples=500, seed=0):
    """The PCA basis of the kernel codes, [dim_pca, ksize^2] float64: num_samples kernels drawn by draw_srmd_kernel
    from random.Random(seed), flattened column-major into the columns of X [ksize^2, n]; the first dim_pca left
    singular vectors of X X^T as rows (no mean subtraction).  Each row's sign is fixed so that its entry of largest
    magnitude is positive; the result is the same for the same arguments."""
    key = (ksize, float(l_max), dim_pca, num_samples, seed)
    if key not in _PCA_CACHE:
        rng = random.Random(seed)
        X = torch.stack([vec_f(anisotropic_gaussian(ksize, *draw_srmd_kernel(rng, l_max))) for _ in range(num_samples)], 1)
        U = torch.linalg.svd(X @ X.T)[0]
        P = U[:, :dim_pca].T.contiguous()
        lead = P.gather(1, P.abs().argmax(1, keepdim=True))
        _PCA_CACHE[key] = P * torch.where(lead < 0, -1.0, 1.0)
    return _PCA_CACHE[key].clone()


def load_pca_matrix(path):
    """A PCA basis [dim_pca, ksize^2] from a .npy or .pt file (e.g. `p` of the reference's srmd_pca_matlab.mat exported
    with numpy.save), float64."""
    if str(path).endswith(".npy"):
        import numpy as np
        P = torch.from_numpy(np.load(path))
    elif str(path).endswith(".pt"):
        P = torch.as_tensor(torch.load(path, map_location="cpu"))
    else:
        raise ValueError(f"load_pca_matrix: {path!r} is neither .npy nor .pt")
    if P.dim() != 2:
        raise ValueError(f"load_pca_matrix: expected a [dim_pca, ksize^2] matrix, got {tuple(P.shape)}")
    return P.double().contiguous()


def srmd_degradation_map(k, sigma, P, h, w, noise_channel=True):
    """[B, dim_pca (+ 1), h, w]: the code P @ vec_F(k) of each kernel k [B, 1, ks, ks], followed by the noise level
    sigma [B] when noise_channel, each constant over h x w.  In k's dtype, on k's device."""
    B = k.shape[0]
    P = torch.as_tensor(P).to(k)
    if k.dim() != 4 or k.shape[1] != 1 or P.dim() != 2 or P.shape[1] != k.shape[-2] * k.shape[-1]:
        raise ValueError(f"srmd_degradation_map: k {tuple(k.shape)} and P {tuple(P.shape)} do not fit")
    code = vec_f(k[:, 0]) @ P.T
    if noise_channel:
        s = torch.as_tensor(sigma).to(k).reshape(-1)
        if s.numel() != B:
            raise ValueError(f"srmd_degradation_map: sigma holds {s.numel()} levels for {B} kernels")
        code = torch.cat((code, s.view(B, 1)), 1)
    return code.view(B, -1, 1, 1).expand(B, code.shape[1], h, w).contiguous()


def wrap_blur_each(x, k):
    """wrap_blur with one kernel per sample, in x's dtype: x [B, C, H, W], k [B, 1, kh, kw] (or [kh, kw] for all)."""
    B, C, Hh, Ww = x.shape
    k = k.to(x)
    if k.dim() == 2:
        k = k[None, None].expand(B, 1, *k.shape)
    kh, kw = k.shape[-2:]
    rows = torch.arange(-(kh - 1 - kh // 2), Hh + kh // 2, device=x.device) % Hh
    cols = torch.arange(-(kw - 1 - kw // 2), Ww + kw // 2, device=x.device) % Ww
    xp = x[..., rows, :][..., cols].reshape(1, B * C, rows.numel(), cols.numel())
    wgt = k.flip(-1, -2).expand(B, C, kh, kw).reshape(B * C, 1, kh, kw)
    return torch.nn.functional.conv2d(xp, wgt, groups=B * C).view(B, C, Hh, Ww)


def srmd_degrade(x, k, sf, sigma=None, seed=0):
    """SRMD's degradation of x [B, C, H, W] (or [C, H, W]), in x's dtype: the circular (wrap) blur with each sample's
    kernel k [B, 1, ks, ks] (or one [ks, ks]), the MATLAB-bicubic utils_image.imresize by 1 / sf (antialiased; its
    fp32 weights, applied in x's dtype), then AWGN of per-sample std sigma ([B] or a number, already divided by 255;
    None or 0: none) from torch.Generator().manual_seed(seed)."""
    lead = x.dim() == 3
    x = x[None] if lead else x
    B = x.shape[0]
    y = wrap_blur_each(x, k)
    if sf != 1:
        Hh, Ww = y.shape[-2:]
        Mh = util.resize_matrix(Hh, math.ceil(Hh / sf), 1.0 / sf, True, y.device).to(y.dtype)
        Mw = util.resize_matrix(Ww, math.ceil(Ww / sf), 1.0 / sf, True, y.device).to(y.dtype)
        y = torch.matmul(torch.matmul(Mh, y), Mw.T)
    if sigma is not None:
        s = torch.as_tensor(sigma, dtype=y.dtype).reshape(-1)
        s = s.expand(B) if s.numel() == 1 else s
        if s.numel() != B:
            raise ValueError(f"srmd_degrade: sigma holds {s.numel()} levels for a batch of {B}")
        if bool((s != 0).any()):
            n = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed), dtype=y.dtype)
            y = y + s.view(B, 1, 1, 1).to(y.device) * n.to(y.device)
    return y[0] if lead else y
