"""DatasetSRMD (the reference's data/dataset_srmd.py restated from the published method; the reference sources were not
at hand): SR pairs for SRMD, whose L is the degraded image followed by its degradation map -- the 15 PCA coefficients of
the blur kernel and (noise_channel) the noise level, constant over the LR grid.

Options: scale; H_size (96); sigma ([0, 50]); sigma_test (0); n_channels (3); pca_path (null: the basis
utils_sisr.cal_pca_matrix(l_max=l_max) computes; else a .npy / .pt file, utils_sisr.load_pca_matrix); l_max (10);
noise_channel (true; false is the noise-free SRMDNF: 15 map channels and no noise); test_kernel_width.

train: random H_size crop (DatasetSR's crop and file handling), one of the 8 flip/rot modes, a kernel
       theta ~ U(0, pi), l1 ~ U(0.1, l_max), l2 ~ U(0.1, l1) (15 x 15, utils_sisr.anisotropic_gaussian), the noise level
       np.random.uniform(sigma[0], sigma[1]) / 255 (DatasetFDnCNN's rule), L = utils_sisr.srmd_degrade(H, k, scale, level)
       (circular blur, MATLAB-bicubic x1/scale, AWGN), then the map.
test:  the whole image mod-cropped to the scale, an isotropic Gaussian kernel of standard deviation test_kernel_width
       pixels (default 0.7 / 1.5 / 2.0 for x2 / x3 / x4, the widths the published models call the default for sharp
       images), the level sigma_test / 255 with noise from seed 0: the same item every time.
Nothing is clipped.  Returns {"L": [C + 16, h, w], "H": [C, scale h, scale w], "L_path", "H_path"}.

Departures from the reference, for lack of its files: the PCA basis is computed (cal_pca_matrix) unless pca_path gives
one, and the training kernels are drawn instead of read from the reference's .mat kernel banks.

The GPU-resident equivalent that feeds the fused trainer without a host loader is
kair_amd.data.gpu_synth.PatchSynth(task="srmd") (csrc/synth_srmd.hip, two launches per batch).
"""
import random

import numpy as np
import torch
import torch.utils.data as data

from ..utils import utils_image as util
from ..utils import utils_sisr as sisr

TEST_KERNEL_WIDTH = {2: 0.7, 3: 1.5, 4: 2.0}


class DatasetSRMD(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.n_channels = opt.get("n_channels") or 3
        self.sf = opt.get("scale") or 4
        if self.sf not in (2, 3, 4):
            raise ValueError(f"DatasetSRMD: scale must be 2, 3 or 4 (got {self.sf!r})")
        self.patch_size = opt.get("H_size") or 96
        if self.patch_size % self.sf:
            raise ValueError(f"DatasetSRMD: H_size {self.patch_size} is not divisible by the scale {self.sf}")
        sigma = opt.get("sigma")
        self.sigma = list(sigma) if sigma is not None else [0, 50]
        if len(self.sigma) != 2 or self.sigma[0] > self.sigma[1]:
            raise ValueError(f"DatasetSRMD: sigma must be [min, max] (got {sigma!r})")
        self.sigma_test = opt.get("sigma_test") or 0
        self.l_max = float(opt.get("l_max") or 10.0)
        nch = opt.get("noise_channel")
        self.noise_channel = True if nch is None else bool(nch)
        self.test_kernel_width = float(opt.get("test_kernel_width") or TEST_KERNEL_WIDTH[self.sf])
        path = opt.get("pca_path")
        self.pca = sisr.load_pca_matrix(path) if path else sisr.cal_pca_matrix(l_max=self.l_max)
        if tuple(self.pca.shape) != (sisr.SRMD_DIM_PCA, sisr.SRMD_KSIZE ** 2):
            raise ValueError(f"DatasetSRMD: the PCA basis is {tuple(self.pca.shape)}, expected [15, 225]")
        self.paths_H = util.get_image_paths(opt["dataroot_H"])
        assert self.paths_H, "Error: H path is empty."

    def __getitem__(self, index):
        H_path = self.paths_H[index]
        img_H = util.imread_uint(H_path, self.n_channels)
        if self.opt["phase"] == "train":
            Hh, Ww, _ = img_H.shape
            rnd_h = random.randint(0, max(0, Hh - self.patch_size))
            rnd_w = random.randint(0, max(0, Ww - self.patch_size))
            patch = img_H[rnd_h:rnd_h + self.patch_size, rnd_w:rnd_w + self.patch_size, :]
            patch = util.augment_img(patch, mode=random.randint(0, 7))
            img_H = util.uint2tensor3(patch)
            k = sisr.anisotropic_gaussian(sisr.SRMD_KSIZE, *sisr.draw_srmd_kernel(random, self.l_max))
            level = float(np.random.uniform(self.sigma[0], self.sigma[1])) / 255.0 if self.noise_channel else 0.0
            seed = random.getrandbits(31)
        else:
            img_H = util.uint2tensor3(util.modcrop(img_H, self.sf))
            var = self.test_kernel_width ** 2
            k = sisr.anisotropic_gaussian(sisr.SRMD_KSIZE, 0.0, var, var)
            level = self.sigma_test / 255.0 if self.noise_channel else 0.0
            seed = 0
        k = k.float()[None, None]
        img_L = sisr.srmd_degrade(img_H[None], k, self.sf, sigma=level, seed=seed)
        m = sisr.srmd_degradation_map(k, torch.tensor([level]), self.pca, *img_L.shape[-2:], self.noise_channel)
        return {"L": torch.cat((img_L, m), 1)[0], "H": img_H, "L_path": H_path, "H_path": H_path}

    def __len__(self):
        return len(self.paths_H)
