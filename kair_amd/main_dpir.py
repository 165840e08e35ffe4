"""DPIR: plug-and-play deblurring and super-resolution with the DRUNet denoiser as the prior (Zhang et al., "Plug-and-Play
Image Restoration with Deep Denoiser Prior"; the reference's main_dpir_deblur.py / main_dpir_sisr.py).

The reference scripts were not available when this was written: the loop is restated from memory of the published
method, and tests/test_dpir_cpu.py / tests/test_dpir_gpu.py pin what it computes.

With denoiser="ircnn" the prior step is the IRCNN model bank instead (network_dncnn.IRCNN; utils_model.IRCNNBank picks
the entry of sigma_i), without a noise-map channel.

    x_0 = L (sf 1) or the bicubic x sf of L
    for i < iter_num:   x <- argmin_z ||(k (*) z)[::sf, ::sf] - L||^2 + rho_i ||z - x||^2   (utils_sisr.DataStep, HIP)
                        x <- DRUNet(cat(x, sigma_i map))                                    (x8: under augmentation i % 8)

with (rho_i, sigma_i) from utils_pnp.get_rho_sigma.  The data step runs in three launches of csrc/fft.hip on the HR
grid, whose sides may have any length up to 2048.

Departures from the reference, and what is out of scope:
  * x_0 for sf > 1 is utils_image.imresize (MATLAB bicubic); the reference uses cv2's bicubic plus a half-pixel
    shift for its "classical" kernels.  A caller may pass its own x0.
  * the blur is circular (the forward model of utils_sisr.degrade, as in the reference's synthetic benchmarks):
    no wrap_boundary_liu or other boundary handling for real photographs;
  * no demosaicing task, no .mat kernel banks (kernels are .npy / .pt arrays), no image above 2048 on a side.

    python -m kair_amd.main_dpir --task {deblur,sisr} --model_path drunet_color.pth --input DIR --kernel K.npy
        [--sf N] [--noise_level_img S] [--iter_num N] [--x8 / --no-x8] [--out DIR] [--synthesize]
"""
import argparse
import os

import numpy as np
import torch

from .utils import utils_image as util
from .utils import utils_model, utils_pnp, utils_sisr


def _unaugment(x, mode):
    """The inverse of augment_img_tensor4(., mode): modes 3 and 5 (the two quarter turns) undo each other, every other
    mode is its own inverse."""
    return util.augment_img_tensor4(x, 8 - mode if mode in (3, 5) else mode)


def dpir_restore(net, L, k, sf=1, noise_level_img=0.0, iter_num=8, modelSigma1=49.0, w=1.0, x8=True, x0=None,
                 denoiser=None, split_min_size=None):
    """E [B, C, h sf, w sf] of L [B, C, h, w] in [0, 1].

    net: the DRUNet (in_nc = C + 1), on L's device; k: [B, 1, kh, kw] or one kernel for all images;
    noise_level_img: L's noise level, already divided by 255; x8: iteration i runs the denoiser under augmentation
    mode i % 8; x0: the starting point instead of L / its bicubic upscale; denoiser: None or "drunet" (the network), any
    callable [B, C + 1, H, W] -> [B, C, H, W] instead of the network (then net may be None), or "ircnn": net is a
    utils_model.IRCNNBank and iteration i's prior step is net.select(sigma_i * 255)(x), the IRCNN entry of that noise
    level on the whole image, with no noise-map channel (the original plug-and-play prior DRUNet supersedes; data step,
    schedule and x8 handling are the same); split_min_size: run the network by
    utils_model.test_mode's recursive 4-way split (mode 2) with this min_size instead of whole (mode 1).  Device
    tensors take the HIP data step (utils_sisr.DataStep), CPU tensors torch.fft in L's dtype (HostDataStep); nothing
    inside the loop reads a device value back."""
    if L.dim() != 4:
        raise ValueError(f"dpir_restore: L is [B, C, h, w] (got {tuple(L.shape)})")
    sf = int(sf)
    modelSigma2 = max(0.255, 255.0 * noise_level_img)
    rhos, sigmas = utils_pnp.get_rho_sigma(max(0.255 / 255.0, noise_level_img), iter_num, modelSigma1, modelSigma2, w)
    ircnn = isinstance(denoiser, str) and denoiser == "ircnn"
    if isinstance(denoiser, str):
        if denoiser not in ("drunet", "ircnn"):
            raise ValueError(f"dpir_restore: denoiser {denoiser!r} is neither 'drunet', 'ircnn' nor a callable")
        denoiser = None
    if ircnn:
        if not hasattr(net, "select"):
            raise ValueError("dpir_restore: denoiser='ircnn' takes a utils_model.IRCNNBank as net")
        net.net.eval()
    elif denoiser is None:
        if net is None:
            raise ValueError("dpir_restore: a network or a denoiser")
        net.eval()
        if split_min_size is None:
            denoiser = lambda x: utils_model.test_mode(net, x, mode=1, modulo=8)                     # noqa: E731
        else:
            denoiser = lambda x: utils_model.test_mode(net, x, mode=2, refield=32, min_size=split_min_size,  # noqa: E731
                                                       modulo=8)
    with torch.no_grad():
        data = (utils_sisr.DataStep if L.is_cuda else utils_sisr.HostDataStep)(L, k, sf)
        if x0 is not None:
            x = x0.to(L.device, L.dtype)
        else:
            x = L if sf == 1 else util.imresize(L, sf).to(L.dtype)
        B = L.shape[0]
        rho_t = torch.tensor([float(r) for r in rhos], dtype=L.dtype).to(L.device)     # one copy, before the loop
        for i in range(iter_num):
            x = data.solve(x, rho_t[i:i + 1])
            mode = i % 8 if x8 else 0
            x = util.augment_img_tensor4(x, mode)
            if ircnn:
                x = _unaugment(net.select(float(sigmas[i]) * 255.0)(x.contiguous()), mode).to(L.dtype)
                continue
            noise_map = x.new_full((B, 1) + tuple(x.shape[-2:]), float(sigmas[i]))
            x = denoiser(torch.cat((x, noise_map), dim=1))
            x = _unaugment(x, mode).to(L.dtype)
    return x


def load_drunet(model_path, compute_dtype="fp32", device="cuda"):
    """UNetRes with the widths, depth and channel counts read off a drunet_gray.pth / drunet_color.pth style
    state_dict, on `device` in eval mode."""
    from .models.network_unet import UNetRes
    sd = torch.load(model_path, map_location="cpu")
    sd = sd.get("params", sd) if isinstance(sd, dict) else sd
    nb = max(int(key.split(".")[1]) for key in sd if key.startswith("m_down1."))
    nc = [sd["m_head.weight"].shape[0]] + [sd[f"m_down{j}.{nb}.weight"].shape[0] for j in (1, 2, 3)]
    net = UNetRes(in_nc=sd["m_head.weight"].shape[1], out_nc=sd["m_tail.weight"].shape[0], nc=nc, nb=nb,
                  compute_dtype=compute_dtype)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval()


def load_kernel(path):
    """A [kh, kw] float tensor from a .npy array or a torch-saved tensor, normalised to sum 1."""
    k = torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.as_tensor(torch.load(path, map_location="cpu"))
    k = k.double().squeeze()
    if k.dim() != 2:
        raise ValueError(f"{path}: a single 2-D kernel is expected (got {tuple(k.shape)})")
    return (k / k.sum()).float()


def main(argv=None):
    """Returns [(image name, PSNR or None)]."""
    ap = argparse.ArgumentParser(description="DPIR deblurring / super-resolution with a DRUNet checkpoint")
    ap.add_argument("--task", choices=["deblur", "sisr"], required=True)
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--input", required=True, help="directory of images")
    ap.add_argument("--kernel", required=True, help="blur kernel, .npy or torch-saved (.pt)")
    ap.add_argument("--sf", type=int, default=None, help="scale factor (sisr; default 4)")
    ap.add_argument("--noise_level_img", type=float, default=None,
                    help="noise level of the input on the 0-255 scale (default: deblur 7.65, sisr 0)")
    ap.add_argument("--iter_num", type=int, default=None, help="default: deblur 8, sisr 24")
    ap.add_argument("--x8", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--out", default=None, help="output directory (default: <input>_dpir_<task>)")
    ap.add_argument("--synthesize", action="store_true",
                    help="the inputs are ground truth: degrade them (blur, downsample, noise) and report PSNR")
    ap.add_argument("--compute_dtype", choices=["fp32", "fp32x3", "bf16"], default="fp32")
    ap.add_argument("--split_min_size", type=int, default=None)
    ap.add_argument("--denoiser", choices=["drunet", "ircnn"], default="drunet",
                    help="the prior: a DRUNet checkpoint, or an IRCNN model bank (ircnn_gray.pth / ircnn_color.pth)")
    a = ap.parse_args(argv)
    if a.task == "deblur" and a.sf not in (None, 1):
        raise SystemExit("--task deblur has no scale factor")
    sf = 1 if a.task == "deblur" else (a.sf or 4)
    sigma = (a.noise_level_img if a.noise_level_img is not None else (7.65 if a.task == "deblur" else 0.0)) / 255.0
    iter_num = a.iter_num or (8 if a.task == "deblur" else 24)
    out_dir = a.out or f"{a.input.rstrip(os.sep)}_dpir_{a.task}"
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda")
    if a.denoiser == "ircnn":
        from .main_test_ircnn_denoiser import load_ircnn
        from .utils.utils_model import load_ircnn_bank
        n_channels = next(iter(load_ircnn_bank(a.model_path).values()))["model.0.weight"].shape[1]
        net = load_ircnn(a.model_path, n_channels, a.compute_dtype, dev)
    else:
        net = load_drunet(a.model_path, a.compute_dtype, dev)
        n_channels = net.m_head.weight.shape[1] - 1
    k = load_kernel(a.kernel).to(dev)
    results, metrics = [], []
    for idx, path in enumerate(util.get_image_paths(a.input)):
        img = util.uint2tensor4(util.imread_uint(path, n_channels)).to(dev)
        H = None
        if a.synthesize:
            H = img[..., :img.shape[-2] - img.shape[-2] % sf, :img.shape[-1] - img.shape[-1] % sf].contiguous()
            L = utils_sisr.degrade(H, k, sf, sigma=sigma, seed=0, step=idx)
        else:
            L = img
        E = dpir_restore(net, L, k, sf=sf, noise_level_img=sigma, iter_num=iter_num, x8=a.x8,
                         split_min_size=a.split_min_size, denoiser=a.denoiser if a.denoiser == "ircnn" else None)
        metrics.append(util.tensor_metrics(E, H, border=sf, ssim=False)[0, 0] if H is not None else None)
        name = os.path.splitext(os.path.basename(path))[0]
        util.imsave(util.tensor2uint(E), os.path.join(out_dir, f"{name}_dpir_{a.task}_x{sf}.png"))
        results.append(name)
    out = []
    for name, m in zip(results, metrics):                 # read the metrics back once, after the last image
        psnr = None if m is None else float(m)
        print(f"{name}: " + ("restored" if psnr is None else f"PSNR {psnr:.2f} dB"))
        out.append((name, psnr))
    if a.synthesize and out:
        print(f"average PSNR {sum(p for _, p in out) / len(out):.2f} dB over {len(out)} images")
    return out


if __name__ == "__main__":
    main()
