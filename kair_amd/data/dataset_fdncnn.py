"""DatasetFDnCNN (restatement of the reference's data/dataset_fdncnn.py): AWGN denoising pairs whose L carries the
noise-level map as its last channel, the input of FDnCNN and DRUNet (define_Dataset types 'fdncnn' and 'drunet').

train: random 'H_size' crop, one of the 8 flip/rot modes (np.random.randint(0, 8)), one noise level per sample
       noise_level = np.random.uniform(sigma[0], sigma[1]) / 255, L = H + noise_level * N(0, 1) from torch's global
       RNG, then L = cat(L, noise_level * ones(1, h, w));
test:  whole image, L = H + numpy N(0, sigma_test / 255) after np.random.seed(0), the map filled with
       sigma_test / 255.
Nothing is clipped.

The GPU-resident equivalent that feeds the fused trainer without a host loader is
kair_amd.data.gpu_synth.PatchSynth(task="fdncnn") (kair_synth_dn_map, one launch per batch).
"""
import random

import numpy as np
import torch
import torch.utils.data as data

from ..utils import utils_image as util


class DatasetFDnCNN(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.n_channels = opt.get("n_channels") or 3
        self.patch_size = opt.get("H_size") or 64
        sigma = opt.get("sigma")
        self.sigma = list(sigma) if sigma is not None else [0, 75]
        if len(self.sigma) != 2 or self.sigma[0] > self.sigma[1]:
            raise ValueError(f"DatasetFDnCNN: sigma must be [min, max] (got {sigma!r})")
        self.sigma_min, self.sigma_max = self.sigma
        st = opt.get("sigma_test")
        self.sigma_test = 25 if st is None else st
        self.paths_H = util.get_image_paths(opt["dataroot_H"])

    def __getitem__(self, index):
        H_path = self.paths_H[index]
        img_H = util.imread_uint(H_path, self.n_channels)
        if self.opt["phase"] == "train":
            H, W, _ = img_H.shape
            rnd_h = random.randint(0, max(0, H - self.patch_size))
            rnd_w = random.randint(0, max(0, W - self.patch_size))
            patch = img_H[rnd_h:rnd_h + self.patch_size, rnd_w:rnd_w + self.patch_size, :]
            patch = util.augment_img(patch, mode=np.random.randint(0, 8))
            img_H = util.uint2tensor3(patch)
            img_L = img_H.clone()
            noise_level = torch.FloatTensor([np.random.uniform(self.sigma_min, self.sigma_max)]) / 255.0
            img_L.add_(torch.randn(img_L.size()).mul_(noise_level))
        else:
            img_H = util.uint2single(img_H)
            img_L = np.copy(img_H)
            np.random.seed(seed=0)
            img_L += np.random.normal(0, self.sigma_test / 255.0, img_L.shape)
            noise_level = torch.FloatTensor([self.sigma_test / 255.0])
            img_L, img_H = util.single2tensor3(img_L), util.single2tensor3(img_H)
        return {**self._with_level(img_L, img_H, noise_level), "L_path": H_path, "H_path": H_path}

    def _with_level(self, img_L, img_H, noise_level):
        """The last step of __getitem__, where the level joins the pair: here as the map channel of L (DatasetFFDNet
        returns it as "C")."""
        noise_map = noise_level.view(1, 1, 1).repeat(1, img_L.size(1), img_L.size(2))
        return {"L": torch.cat((img_L, noise_map), 0), "H": img_H}

    def __len__(self):
        return len(self.paths_H)
