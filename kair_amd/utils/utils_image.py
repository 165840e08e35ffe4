"""Image utilities on the parity-defining path (mirror of /root/reference/utils/utils_image.py).

calculate_psnr  utils_image.py:629-644   (uint8 HxW[xC], float64 MSE, border shave)
calculate_ssim  utils_image.py:650-697   (11x11 Gaussian sigma 1.5, 'valid' window; cv2.filter2D is
                a correlation whose border never enters the valid region, restated with numpy)
rgb2ycbcr / bgr2ycbcr / ycbcr2rgb  utils_image.py:536-602 (MATLAB coefficients)
augment_img / augment_img_tensor4  utils_image.py:387-426 (the 8 flip/rot90 modes)
modcrop / shave utils_image.py:501-531
imread_uint / imsave  utils_image.py:192-221 (PIL instead of cv2: cv2 is not in this image;
                grayscale is ITU-R 601-2 luma in both)
tensor2uint     utils_image.py:296-300
single2uint     utils_image.py:261-263
uint2tensor3/4  utils_image.py:281-292
imresize        utils_image.py:938-1005  MATLAB bicubic (a = -0.5, antialias when shrinking,
                symmetric border).  Written as two separable resampling-matrix products so it runs
                batched on the device (the data-synthesis step feeding the hot path).
"""
import math
import os

import numpy as np
import torch

IMG_EXTENSIONS = [".jpg", ".JPG", ".jpeg", ".JPEG", ".png", ".PNG", ".ppm", ".PPM", ".bmp", ".BMP", ".tif"]


def _cubic(x):
    ax = x.abs()
    return ((1.5 * ax ** 3 - 2.5 * ax ** 2 + 1) * (ax <= 1).to(x.dtype)
            + (-0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2) * ((ax > 1) & (ax <= 2)).to(x.dtype))


_MAT_CACHE = {}


def resize_matrix(n_in, n_out, scale, antialias=True, device="cpu"):
    key = (n_in, n_out, float(scale), antialias, str(device))
    if key in _MAT_CACHE:
        return _MAT_CACHE[key]
    kw = 4.0 / scale if (scale < 1 and antialias) else 4.0
    u = torch.arange(1, n_out + 1, dtype=torch.float64) / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kw / 2)
    P = math.ceil(kw) + 2
    idx = left[:, None] + torch.arange(P, dtype=torch.float64)[None]
    d = u[:, None] - idx
    w = (scale * _cubic(d * scale)) if (scale < 1 and antialias) else _cubic(d)
    w = (w / w.sum(1, keepdim=True)).float()
    # the reference drops an all-zero first/last column (same result either way)
    i = idx.long() - 1
    i = torch.where(i < 0, -i - 1, i)
    i = torch.where(i >= n_in, 2 * n_in - 1 - i, i)
    M = torch.zeros(n_out, n_in, dtype=torch.float32)
    M.index_put_((torch.arange(n_out)[:, None].expand_as(i), i), w, accumulate=True)
    M = M.to(device)
    _MAT_CACHE[key] = M
    return M


def bicubic_taps(n_in, n_out, scale, antialias=True):
    """calculate_weights_indices (utils_image.py:880-932) in the reference's float32 arithmetic, as
    per-output-pixel taps: (indices int32 [n_out, P] with the symmetric border already reflected,
    weights fp32 [n_out, P]).  Zero-weight border taps are kept (they add 0)."""
    kw = 4.0 / scale if (scale < 1 and antialias) else 4.0
    x = torch.linspace(1, n_out, n_out)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kw / 2)
    P = math.ceil(kw) + 2
    idx = left.view(n_out, 1).expand(n_out, P) + torch.linspace(0, P - 1, P).view(1, P).expand(n_out, P)
    d = u.view(n_out, 1).expand(n_out, P) - idx
    w = (scale * _cubic(d * scale)) if (scale < 1 and antialias) else _cubic(d)
    w = w / torch.sum(w, 1).view(n_out, 1)
    i = idx.long() - 1
    i = torch.where(i < 0, -i - 1, i)
    i = torch.where(i >= n_in, 2 * n_in - 1 - i, i)
    return i.int().contiguous(), w.float().contiguous()


def imresize(img, scale, antialiasing=True):
    """img: [..., H, W] float tensor in [0, 1] (CHW, HW or a batch NCHW), any device."""
    Hh, Ww = img.shape[-2:]
    oh, ow = math.ceil(Hh * scale), math.ceil(Ww * scale)
    Mh = resize_matrix(Hh, oh, scale, antialiasing, img.device)
    Mw = resize_matrix(Ww, ow, scale, antialiasing, img.device)
    return torch.matmul(torch.matmul(Mh, img.float()), Mw.T)


def single2uint(img):
    return np.uint8((img.clip(0, 1) * 255.0).round())


def uint2single(img):
    return np.float32(img / 255.0)


def uint2tensor3(img):
    if img.ndim == 2:
        img = np.expand_dims(img, axis=2)
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255.0)


def uint2tensor4(img):
    return uint2tensor3(img).unsqueeze(0)


def tensor2uint(img):
    img = img.detach().squeeze().float().clamp(0, 1).cpu().numpy()
    if img.ndim == 3:
        img = np.transpose(img, (1, 2, 0))
    return np.uint8((img * 255.0).round())


def calculate_psnr(img1, img2, border=0):
    if img1.shape != img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    h, w = img1.shape[:2]
    a = img1[border:h - border, border:w - border].astype(np.float64)
    b = img2[border:h - border, border:w - border].astype(np.float64)
    mse = np.mean((a - b) ** 2)
    return float("inf") if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))


def psnr_float(E, H):
    mse = torch.mean((E.double().clamp(0, 1) - H.double()) ** 2).item()
    return float("inf") if mse == 0 else -10 * math.log10(mse)


def synth_sr_batch(B, lq, scale, seed=0, device="cpu"):
    """Seeded synthetic SR patches: HR = clamp(bicubic-up(U[0,1) at HR/8) + 0.02 N, 0, 1),
    LQ = MATLAB-bicubic x1/scale of HR.  Generated on CPU with a torch.Generator, then moved."""
    g = torch.Generator().manual_seed(seed)
    hr = lq * scale
    base = torch.rand(B, 3, max(1, hr // 8), max(1, hr // 8), generator=g)
    Hh = torch.nn.functional.interpolate(base, size=(hr, hr), mode="bicubic", align_corners=False)
    Hh = (Hh + 0.02 * torch.randn(Hh.shape, generator=g)).clamp(0, 1)
    L = imresize(Hh, 1.0 / scale)
    return L.to(device), Hh.to(device)


# ------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------
def is_image_file(filename):
    return any(filename.endswith(ext) for ext in IMG_EXTENSIONS)


def get_image_paths(dataroot):
    """utils_image.py:70-91: sorted image files under a directory (or a list of directories)."""
    if dataroot is None:
        return None
    roots = [dataroot] if isinstance(dataroot, str) else list(dataroot)
    paths = []
    for root in roots:
        if not os.path.isdir(root):
            raise AssertionError(f"{root} is not a valid directory")
        found = [os.path.join(d, f) for d, _, fs in sorted(os.walk(root)) for f in sorted(fs) if is_image_file(f)]
        if not found:
            raise AssertionError(f"{root} has no valid image file")
        paths += sorted(found)
    return paths


def imread_uint(path, n_channels=3):
    """HxWx3 RGB (or GGG) / HxWx1 gray uint8."""
    from PIL import Image
    im = Image.open(path)
    if n_channels == 1:
        return np.expand_dims(np.asarray(im.convert("L")), axis=2)
    return np.asarray(im.convert("RGB"))


def imsave(img, img_path):
    from PIL import Image
    Image.fromarray(np.squeeze(img)).save(img_path)


# ------------------------------------------------------------------------------------------
# layout / augmentation
# ------------------------------------------------------------------------------------------
def single2tensor3(img):
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float()


def tensor2single(img):
    img = img.detach().squeeze().float().cpu().numpy()
    return np.transpose(img, (1, 2, 0)) if img.ndim == 3 else img


def augment_img(img, mode=0):
    """numpy HxW[xC]: the 8 dihedral modes of utils_image.py:387-405."""
    if mode == 0:
        return img
    if mode == 1:
        return np.flipud(np.rot90(img))
    if mode == 2:
        return np.flipud(img)
    if mode == 3:
        return np.rot90(img, k=3)
    if mode == 4:
        return np.flipud(np.rot90(img, k=2))
    if mode == 5:
        return np.rot90(img)
    if mode == 6:
        return np.rot90(img, k=2)
    if mode == 7:
        return np.flipud(np.rot90(img, k=3))
    raise ValueError(mode)


def augment_img_tensor4(img, mode=0):
    """NCHW tensor, utils_image.py:408-426."""
    if mode == 0:
        return img
    if mode == 1:
        return img.rot90(1, [2, 3]).flip([2])
    if mode == 2:
        return img.flip([2])
    if mode == 3:
        return img.rot90(3, [2, 3])
    if mode == 4:
        return img.rot90(2, [2, 3]).flip([2])
    if mode == 5:
        return img.rot90(1, [2, 3])
    if mode == 6:
        return img.rot90(2, [2, 3])
    if mode == 7:
        return img.rot90(3, [2, 3]).flip([2])
    raise ValueError(mode)


def add_noise_map(x, sigma_255):
    """[B, C, H, W] -> [B, C + 1, H, W]: the noise-level map sigma_255 / 255 as the last channel, the input of the
    FDnCNN / DRUNet denoisers (`net(add_noise_map(img, 25))`).  sigma_255: a number, or a tensor of B levels."""
    B, _, H, W = x.shape
    if torch.is_tensor(sigma_255):
        m = (sigma_255.to(device=x.device, dtype=x.dtype) / 255.0).reshape(-1, 1, 1, 1).expand(B, 1, H, W)
    else:
        m = x.new_full((B, 1, H, W), float(sigma_255) / 255.0)
    return torch.cat((x, m), dim=1)


def modcrop(img_in, scale):
    img = np.copy(img_in)
    if img.ndim not in (2, 3):
        raise ValueError("Wrong img ndim: [{:d}].".format(img.ndim))
    H, W = img.shape[:2]
    return img[:H - H % scale, :W - W % scale, ...]


def shave(img_in, border=0):
    img = np.copy(img_in)
    h, w = img.shape[:2]
    return img[border:h - border, border:w - border]


# ------------------------------------------------------------------------------------------
# colour (MATLAB rgb2ycbcr coefficients)
# ------------------------------------------------------------------------------------------
_YCC = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])


def _ycbcr(img, only_y, coef):
    in_type = img.dtype
    x = img.astype(np.float64) if in_type == np.uint8 else img.astype(np.float64) * 255.0
    if only_y:
        rlt = np.dot(x, coef[:, 0]) / 255.0 + 16.0
    else:
        rlt = np.matmul(x, coef) / 255.0 + [16, 128, 128]
    rlt = rlt.round() if in_type == np.uint8 else rlt / 255.0
    return rlt.astype(in_type)


def rgb2ycbcr(img, only_y=True):
    return _ycbcr(img, only_y, _YCC)


def bgr2ycbcr(img, only_y=True):
    return _ycbcr(img, only_y, _YCC[::-1])


def ycbcr2rgb(img):
    in_type = img.dtype
    x = img.astype(np.float64) if in_type == np.uint8 else img.astype(np.float64) * 255.0
    rlt = np.matmul(x, [[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071],
                        [0.00625893, -0.00318811, 0]]) * 255.0 + [-222.921, 135.576, -276.836]
    rlt = np.clip(rlt, 0, 255)
    rlt = rlt.round() if in_type == np.uint8 else rlt / 255.0
    return rlt.astype(in_type)


# ------------------------------------------------------------------------------------------
# SSIM
# ------------------------------------------------------------------------------------------
def _gauss_window(k=11, sigma=1.5):
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2
    g = np.exp(-x * x / (2 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g)


def _filter_valid(img, win):
    """correlation of img with win over the fully-overlapping region (cv2.filter2D(...)[5:-5, 5:-5])."""
    k = win.shape[0]
    from numpy.lib.stride_tricks import sliding_window_view
    v = sliding_window_view(img, (k, k))
    return np.einsum("ijkl,kl->ij", v, win)


def ssim(img1, img2):
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    w = _gauss_window()
    mu1, mu2 = _filter_valid(a, w), _filter_valid(b, w)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(a * a, w) - mu1_sq
    s2 = _filter_valid(b * b, w) - mu2_sq
    s12 = _filter_valid(a * b, w) - mu12
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean()


def calculate_ssim(img1, img2, border=0):
    if img1.shape != img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    h, w = img1.shape[:2]
    a, b = img1[border:h - border, border:w - border], img2[border:h - border, border:w - border]
    if a.ndim == 2:
        return ssim(a, b)
    if a.ndim == 3:
        if a.shape[2] in (2, 3):
            return np.array([ssim(a[:, :, i], b[:, :, i]) for i in range(a.shape[2])]).mean()
        if a.shape[2] == 1:
            return ssim(np.squeeze(a), np.squeeze(b))
    raise ValueError("Wrong input image dimensions.")


# ------------------------------------------------------------------------------------------
# tensor-level evaluation metrics (the uint8 PSNR / SSIM above, on the device through kair_image_metrics)
# ------------------------------------------------------------------------------------------
def rgb2y_uint8(img):
    """Y of rgb2ycbcr(uint8 HxWx3 (or ...x3), only_y=True) in exact integer arithmetic: with N = 65481 r + 128553 g +
    24966 b, Y = 16 + round_half_even(N / 255000) from the integer quotient and remainder.  The float64 np.dot of
    rgb2ycbcr differs from it only at exact ties N = 127500 (mod 255000): 194 of the 2^24 triples, 24 of which numpy
    rounds the other way, by one level.  This rule is what the device kernel computes."""
    if img.dtype != np.uint8 or img.shape[-1] != 3:
        raise ValueError("rgb2y_uint8 takes a uint8 array of RGB triples")
    x = img.astype(np.int64)
    n = 65481 * x[..., 0] + 128553 * x[..., 1] + 24966 * x[..., 2]
    q, rem = n // 255000, n % 255000
    q = q + ((rem > 127500) | ((rem == 127500) & (q % 2 == 1)))
    return (16 + q).astype(np.uint8)


def _tensor2uint_hwc(img):
    """[C, H, W] float tensor -> uint8 HxW (C = 1) or HxWxC with tensor2uint's arithmetic, whatever H and W are
    (tensor2uint squeezes, so it is applied per channel plane and the shape restored)."""
    C, H, W = img.shape
    planes = [tensor2uint(img[c]).reshape(H, W) for c in range(C)]
    return planes[0] if C == 1 else np.stack(planes, axis=2)


def tensor_metrics(E, H, border=0, y_channel=False, ssim=True):
    """Per-image uint8 (PSNR dB, SSIM) of float images E, H ([B, C, H, W] or [C, H, W], C 1 or 3, any float dtype, any
    strides) as a float64 tensor [B, 2] on the images' device: tensor2uint's quantisation, optionally the Y channel
    (C = 3; rgb2y_uint8's integer rule), `border` pixels cropped from every side, then calculate_psnr and
    calculate_ssim.  PSNR is inf for identical images; with ssim=False column 1 is NaN.

    Device tensors: one kair_image_metrics call (csrc/metrics.hip) and kair_psnr_db, which turns the exact SSE into dB
    with the host C library's log10 arithmetic (torch.log10 on the device differs from it in the last place on every
    fifth value); nothing is read back, so a validation loop can collect the results and synchronise once.  CPU
    tensors: the host functions of this file per image."""
    if not (torch.is_tensor(E) and torch.is_tensor(H)):
        raise TypeError("tensor_metrics takes tensors")
    if E.shape != H.shape:
        raise ValueError(f"tensor_metrics: E {tuple(E.shape)} and H {tuple(H.shape)} differ in shape")
    if E.device != H.device:
        raise ValueError(f"tensor_metrics: E on {E.device}, H on {H.device}")
    if E.dim() == 3:
        E, H = E.unsqueeze(0), H.unsqueeze(0)
    if E.dim() != 4:
        raise ValueError(f"tensor_metrics: images are [B, C, H, W] or [C, H, W] (got {E.dim()} dimensions)")
    if not (E.is_floating_point() and H.is_floating_point()):
        raise TypeError("tensor_metrics: float images in [0, 1]")
    B, C, Hh, Ww = E.shape
    border = int(border)
    if C not in (1, 3):
        raise ValueError(f"tensor_metrics: C = {C} (1 or 3)")
    if y_channel and C != 3:
        raise ValueError(f"tensor_metrics: the Y channel needs C = 3 (got {C})")
    hr, wr = Hh - 2 * border, Ww - 2 * border
    if B < 1 or border < 0 or hr < 1 or wr < 1:
        raise ValueError(f"tensor_metrics: border {border} leaves no pixel of {B} x {Hh} x {Ww}")
    if ssim and (hr < 11 or wr < 11):
        raise ValueError(f"tensor_metrics: the SSIM window is 11 x 11, the cropped region {hr} x {wr}")
    E, H = E.detach().float().contiguous(), H.detach().float().contiguous()
    if E.is_cuda:
        from .. import _hip
        flags = (_hip.METRIC_Y if y_channel else 0) | (_hip.METRIC_SSIM if ssim else 0)
        out = torch.full((B, 2), float("nan"), dtype=torch.float64, device=E.device)
        ws = _hip.image_metrics_workspace(B, C, Hh, Ww, border, flags, E.device)
        _hip.image_metrics(E, H, out, B, C, Hh, Ww, border, flags, ws)
        # SSE -> dB in place (inf at 0): kair_psnr_db reproduces the host's log10, which torch.log10 on the device does not
        _hip.psnr_db(out[:, 0], out[:, 0], hr * wr * (1 if y_channel else C))
        return out
    out = torch.full((B, 2), float("nan"), dtype=torch.float64)
    for b in range(B):
        e, h = _tensor2uint_hwc(E[b]), _tensor2uint_hwc(H[b])
        if y_channel:
            e, h = rgb2y_uint8(e), rgb2y_uint8(h)
        out[b, 0] = calculate_psnr(e, h, border=border)
        if ssim:
            out[b, 1] = float(calculate_ssim(e, h, border=border))
    return out
