"""DatasetUSRNet (restatement of /root/reference/data/dataset_usrnet.py:23-126): blurred, decimated, noisy LR
images with their blur kernel, scale factor and noise level, for USRNet (ModelPlain4).

train: uint8 'H_size' crop (68-72), one of the 8 flip/rot modes (77-78), a blur kernel (80-93), a noise level
       (95-98: 0 with probability 1/8, else randint(0, sigma_max) / 255), L = the circular ('wrap') blur of the
       uint8 patch truncated back to uint8 (101: ndimage.convolve keeps the input's dtype), [0::sf, 0::sf] (102),
       plus N(0, 1) * noise level (103).  The scale factor is redrawn from `scales` once per batch: every
       'dataloader_batch_size'-th item (54-58), so a batch shares it (num_workers = 0, as the reference needs).
test:  whole image, a fixed kernel, 'sf_validation' (default 3), no noise (105-113).

Kernels: the reference mixes utils_deblur.blurkernel_synthesis (motion blur; cv2.resize + scipy.interpolate) with
utils_sisr.gen_kernel half and half.  The motion-blur synthesis is not built here; 'kernel_bank' (a .npy / .pt file
or an array of [K, ks, ks] kernels, e.g. exported motion kernels) takes that branch, and without a bank every
kernel is a gen_kernel Gaussian.  The test kernel is kernel_bank[0] normalised, or a seeded gen_kernel.  The blur
is a float64 torch conv2d over a wrapped pad (utils_sisr.wrap_blur), so scipy is not needed.

kair_amd.data.gpu_synth.PatchSynth(task="usrnet") produces the same batches from an HBM-resident image pool on the
GPU (csrc/synth_usr.hip).
"""
import random

import numpy as np
import torch
import torch.utils.data as data

from ..utils import utils_image as util
from ..utils import utils_sisr as sisr


def load_kernel_bank(bank, ks):
    """[K, ks, ks] float64 tensor from a .npy / .pt path, an array or a tensor; None stays None."""
    if bank is None:
        return None
    if isinstance(bank, str):
        bank = np.load(bank) if bank.endswith(".npy") else torch.load(bank, map_location="cpu")
    bank = torch.as_tensor(bank).double()
    if bank.dim() != 3 or tuple(bank.shape[-2:]) != (ks, ks):
        raise ValueError(f"kernel_bank must be [K, {ks}, {ks}], got {tuple(bank.shape)}")
    return bank


class DatasetUSRNet(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.n_channels = opt.get("n_channels") or 3
        self.patch_size = opt.get("H_size") or 96
        self.sigma_max = opt.get("sigma_max") if opt.get("sigma_max") is not None else 25
        self.scales = opt.get("scales") or [1, 2, 3, 4]
        self.sf_validation = opt.get("sf_validation") or 3
        self.ks = opt.get("kernel_size") or 25
        self.bank = load_kernel_bank(opt.get("kernel_bank"), self.ks)
        self.batch_size = opt.get("dataloader_batch_size") or 1
        self.paths_H = util.get_image_paths(opt["dataroot_H"])
        assert self.paths_H, "Error: H path is empty."
        if opt["phase"] == "train":
            bad = [s for s in self.scales if self.patch_size % s]
            if bad:
                raise ValueError(f"H_size {self.patch_size} is not divisible by the scales {bad}")
        self.count = 0
        self.sf = self.scales[0]
        if self.bank is not None:
            self.k_test = self.bank[0] / self.bank[0].sum()
        else:
            self.k_test = sisr.gen_kernel(self.ks, rng=random.Random(0), mode_k=0)

    def _train_kernel(self):
        if random.randint(0, 7) > 3 and self.bank is not None:
            k = self.bank[random.randint(0, self.bank.shape[0] - 1)]
            return k / k.sum()
        return sisr.gen_kernel(self.ks, mode_k=random.randint(0, 7))

    def __getitem__(self, index):
        H_path = self.paths_H[index]
        img_H = util.imread_uint(H_path, self.n_channels)
        if self.opt["phase"] == "train":
            if self.count % self.batch_size == 0:
                self.sf = random.choice(self.scales)
            self.count += 1
            H, W, _ = img_H.shape
            rnd_h = random.randint(0, max(0, H - self.patch_size))
            rnd_w = random.randint(0, max(0, W - self.patch_size))
            patch = img_H[rnd_h:rnd_h + self.patch_size, rnd_w:rnd_w + self.patch_size, :]
            patch = util.augment_img(patch, mode=random.randint(0, 7))
            k = self._train_kernel()
            noise_level = 0.0 if random.randint(0, 7) == 1 else random.randint(0, self.sigma_max - 1) / 255.0
            img_H = util.uint2tensor3(patch)
            x8 = torch.from_numpy(np.ascontiguousarray(patch)).permute(2, 0, 1)
            # ndimage.convolve on the uint8 patch: the float result cast back to uint8
            img_L = torch.floor(sisr.wrap_blur(x8, k)).clamp_(0, 255)[..., 0::self.sf, 0::self.sf]
            img_L = (img_L / 255.0).float()
            img_L = img_L + torch.randn(img_L.shape) * noise_level
            sf = self.sf
        else:
            k = self.k_test
            sf = self.sf_validation
            noise_level = 0.0
            x8 = torch.from_numpy(np.array(img_H)).permute(2, 0, 1)
            img_L = torch.floor(sisr.wrap_blur(x8, k)).clamp_(0, 255)[..., 0::sf, 0::sf]
            img_L = (img_L / 255.0).float()
            img_H = util.uint2tensor3(img_H)
        return {"L": img_L, "H": img_H, "k": k.float()[None], "sigma": torch.full((1, 1, 1), noise_level),
                "sf": sf, "L_path": H_path, "H_path": H_path}

    def __len__(self):
        return len(self.paths_H)
