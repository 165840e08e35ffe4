"""SCUNet denoising with a checkpoint (the counterpart of the reference's main_test_scunet_*_gaussian.py scripts):

    python -m kair_amd.main_test_scunet --model_path P --input DIR --noise_level S --n_channels {1,3} [--x8] [--output DIR]

`config` and `dim` are read off the state_dict (scunet_color_*.pth / scunet_gray_*.pth style keys).  With
--noise_level S > 0 the inputs are ground truth: AWGN of standard deviation S / 255 is added from a fixed seed and the
PSNR of the result against the input is reported through utils_image.tensor_metrics; with S = 0 the inputs are restored
as they are.  The network runs on whole images (the replicate pad to multiples of 64 and the crop are its own); --x8
averages the eight flips / rotations (utils_model.test_x8).
"""
import argparse
import os

import torch

from .utils import utils_image as util
from .utils import utils_model

STAGES = ("m_down1", "m_down2", "m_down3", "m_body", "m_up3", "m_up2", "m_up1")


def config_of(sd):
    """(in_nc, config, dim) of an SCUNet state_dict."""
    dim, in_nc = sd["m_head.0.weight"].shape[:2]
    config = [len({k.split(".")[1] for k in sd if k.startswith(s + ".") and ".trans_block." in k}) for s in STAGES]
    return in_nc, config, dim


def load_scunet(model_path, n_channels=3, compute_dtype="fp32", device="cuda"):
    """SCUNet with config and dim read off the state_dict, on `device` in eval mode."""
    from .models.network_scunet import SCUNet
    sd = torch.load(model_path, map_location="cpu")
    sd = sd.get("params", sd) if isinstance(sd, dict) else sd
    in_nc, config, dim = config_of(sd)
    if in_nc != n_channels:
        raise ValueError(f"{model_path}: the network takes {in_nc} channels, not {n_channels}")
    net = SCUNet(in_nc=in_nc, config=config, dim=dim, compute_dtype=compute_dtype)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval()


def main(argv=None):
    """Returns [(image name, PSNR or None)]."""
    ap = argparse.ArgumentParser(description="SCUNet denoising with a checkpoint")
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--input", required=True, help="directory of images")
    ap.add_argument("--noise_level", type=float, default=0.0, help="AWGN level to add, 0-255 scale (0: restore as is)")
    ap.add_argument("--n_channels", type=int, default=3, choices=[1, 3])
    ap.add_argument("--x8", action="store_true")
    ap.add_argument("--output", default=None, help="output directory (default: <input>_scunet)")
    ap.add_argument("--compute_dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    out_dir = a.output or f"{a.input.rstrip(os.sep)}_scunet"
    os.makedirs(out_dir, exist_ok=True)
    net = load_scunet(a.model_path, a.n_channels, a.compute_dtype, dev)
    gen = torch.Generator().manual_seed(0)
    names, metrics = [], []
    for path in util.get_image_paths(a.input):
        img = util.uint2tensor4(util.imread_uint(path, a.n_channels))
        L, Himg = img, None
        if a.noise_level > 0:
            Himg = img.to(dev)
            L = img + torch.randn(img.shape, generator=gen) * (a.noise_level / 255.0)
        with torch.no_grad():
            E = utils_model.test_x8(net, L.to(dev)) if a.x8 else net(L.to(dev))
        metrics.append(util.tensor_metrics(E, Himg, ssim=False)[0, 0] if Himg is not None else None)
        name = os.path.splitext(os.path.basename(path))[0]
        util.imsave(util.tensor2uint(E), os.path.join(out_dir, f"{name}_scunet.png"))
        names.append(name)
    out = []
    for name, m in zip(names, metrics):                 # read the metrics back once, after the last image
        psnr = None if m is None else float(m)
        print(f"{name}: " + ("restored" if psnr is None else f"PSNR {psnr:.2f} dB"))
        out.append((name, psnr))
    if a.noise_level > 0 and out:
        print(f"average PSNR {sum(p for _, p in out) / len(out):.2f} dB over {len(out)} images")
    return out


if __name__ == "__main__":
    main()
