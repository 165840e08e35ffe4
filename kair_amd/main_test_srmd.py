"""SRMD / SRMDNF testing with a checkpoint (the counterpart of the reference's main_test_srmd.py):

    python -m kair_amd.main_test_srmd --model_path P --input DIR --sf N
        (--kernel_width W | --kernel K.npy) --noise_level S [--pca P.npy] [--synthesize] [--x8]

The network's widths, depth and channel counts are read off the state_dict (srmd_x4.pth / srmdnf_x4.pth style keys
model.{0, 2, ...}); in_nc - n_channels = 16 is SRMD, 15 the noise-free SRMDNF.  The degradation map of every image is
utils_sisr.srmd_degradation_map of the given kernel -- an isotropic Gaussian of standard deviation --kernel_width
pixels, or a 15 x 15 kernel file -- and the noise level (0-255 scale); the PCA basis is --pca (.npy / .pt, e.g. the
reference's srmd_pca_matlab.mat exported) or utils_sisr.cal_pca_matrix().  A model trained with one basis has to be
tested with the same one.  The forward runs through utils_model.test_mode (mode 0, or 3 with --x8: the eight
flips / rotations of the image, with the map of the same kernel -- exact for isotropic kernels only).

--synthesize: the inputs are ground truth; they are mod-cropped, degraded with utils_sisr.srmd_degrade (that kernel,
bicubic x1/sf, noise from seed 0) and the PSNR of the result is reported through utils_image.tensor_metrics.
"""
import argparse
import os

import torch

from .utils import utils_image as util
from .utils import utils_model, utils_sisr


def load_srmd(model_path, sf, n_channels=3, compute_dtype="fp32", device="cuda"):
    """SRMD with nc, nb and in_nc read off the state_dict, on `device` in eval mode."""
    from .models.network_srmd import SRMD
    sd = torch.load(model_path, map_location="cpu")
    sd = sd.get("params", sd) if isinstance(sd, dict) else sd
    convs = sorted(int(key.split(".")[1]) for key in sd if key.endswith(".weight"))
    nc, in_nc = sd["model.0.weight"].shape[:2]
    out_ch = sd[f"model.{convs[-1]}.weight"].shape[0]
    if out_ch != n_channels * sf * sf:
        raise ValueError(f"{model_path}: the last conv writes {out_ch} channels, not {n_channels} x {sf}^2")
    net = SRMD(in_nc=in_nc, out_nc=n_channels, nc=nc, nb=len(convs), upscale=sf, compute_dtype=compute_dtype)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval()


def load_kernel(path):
    """A [15, 15] float64 kernel from a .npy array or a torch-saved tensor, normalised to sum 1."""
    k = utils_sisr.load_pca_matrix(path)   # (the same two file kinds, a 2-D float64 array)
    if tuple(k.shape) != (utils_sisr.SRMD_KSIZE,) * 2:
        raise ValueError(f"{path}: a 15 x 15 kernel is expected (got {tuple(k.shape)})")
    return k / k.sum()


def main(argv=None):
    """Returns [(image name, PSNR or None)]."""
    ap = argparse.ArgumentParser(description="SRMD super-resolution with a checkpoint")
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--input", required=True, help="directory of images")
    ap.add_argument("--sf", type=int, required=True, choices=[2, 3, 4])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--kernel_width", type=float, help="standard deviation (pixels) of an isotropic Gaussian kernel")
    g.add_argument("--kernel", help="a 15 x 15 blur kernel, .npy or torch-saved (.pt)")
    ap.add_argument("--noise_level", type=float, default=0.0, help="noise level of the input on the 0-255 scale")
    ap.add_argument("--pca", default=None, help="PCA basis [15, 225], .npy or .pt (default: cal_pca_matrix())")
    ap.add_argument("--synthesize", action="store_true",
                    help="the inputs are ground truth: degrade them (blur, bicubic, noise) and report PSNR")
    ap.add_argument("--x8", action="store_true")
    ap.add_argument("--n_channels", type=int, default=3)
    ap.add_argument("--out", default=None, help="output directory (default: <input>_srmd_x<sf>)")
    ap.add_argument("--compute_dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    sf, dev = a.sf, torch.device(a.device)
    out_dir = a.out or f"{a.input.rstrip(os.sep)}_srmd_x{sf}"
    os.makedirs(out_dir, exist_ok=True)
    net = load_srmd(a.model_path, sf, a.n_channels, a.compute_dtype, dev)
    noise_channel = net.in_nc - a.n_channels == utils_sisr.SRMD_DIM_PCA + 1
    if net.in_nc - a.n_channels not in (utils_sisr.SRMD_DIM_PCA, utils_sisr.SRMD_DIM_PCA + 1):
        raise ValueError(f"{a.model_path}: in_nc {net.in_nc} is neither n_channels + 15 nor n_channels + 16")
    P = utils_sisr.load_pca_matrix(a.pca) if a.pca else utils_sisr.cal_pca_matrix()
    k = (load_kernel(a.kernel) if a.kernel else
         utils_sisr.anisotropic_gaussian(utils_sisr.SRMD_KSIZE, 0.0, a.kernel_width ** 2, a.kernel_width ** 2))
    k = k.float()[None, None].to(dev)
    sigma = torch.tensor([a.noise_level / 255.0 if noise_channel else 0.0], device=dev)
    names, metrics = [], []
    for path in util.get_image_paths(a.input):
        img = util.uint2tensor4(util.imread_uint(path, a.n_channels)).to(dev)
        Himg = None
        if a.synthesize:
            Himg = img[..., :img.shape[-2] - img.shape[-2] % sf, :img.shape[-1] - img.shape[-1] % sf].contiguous()
            L = utils_sisr.srmd_degrade(Himg, k, sf, sigma=sigma.cpu(), seed=0)
        else:
            L = img
        m = utils_sisr.srmd_degradation_map(k, sigma, P, *L.shape[-2:], noise_channel)
        with torch.no_grad():
            E = utils_model.test_mode(net, torch.cat((L, m), 1), mode=3 if a.x8 else 0, sf=sf)
        metrics.append(util.tensor_metrics(E, Himg, border=sf, ssim=False)[0, 0] if Himg is not None else None)
        name = os.path.splitext(os.path.basename(path))[0]
        util.imsave(util.tensor2uint(E), os.path.join(out_dir, f"{name}_srmd_x{sf}.png"))
        names.append(name)
    out = []
    for name, m in zip(names, metrics):                 # read the metrics back once, after the last image
        psnr = None if m is None else float(m)
        print(f"{name}: " + ("restored" if psnr is None else f"PSNR {psnr:.2f} dB"))
        out.append((name, psnr))
    if a.synthesize and out:
        print(f"average PSNR {sum(p for _, p in out) / len(out):.2f} dB over {len(out)} images")
    return out


if __name__ == "__main__":
    main()
