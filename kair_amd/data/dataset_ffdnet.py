"""DatasetFFDNet (restatement of the reference's data/dataset_ffdnet.py, which was not at hand: it follows
DatasetFDnCNN as this tree states it): AWGN denoising pairs with the noise level as a second input, for FFDNet
(define_Dataset type 'ffdnet', trained by ModelPlain2).

train: random 'H_size' crop, one of the 8 flip/rot modes (np.random.randint(0, 8)), one noise level per sample
       noise_level = np.random.uniform(sigma[0], sigma[1]) / 255, L = H + noise_level * N(0, 1) from torch's global RNG;
test:  whole image, L = H + numpy N(0, sigma_test / 255) after np.random.seed(0), the level sigma_test / 255.
The level is not concatenated into L: both branches return it as "C" of shape [1, 1, 1], so a collated batch carries
[B, 1, 1, 1].  Nothing is clipped.

The GPU-resident equivalent is kair_amd.data.gpu_synth.PatchSynth(task="ffdnet") (kair_synth_dn_level, one launch).
"""
import random

import numpy as np
import torch

from ..utils import utils_image as util
from .dataset_fdncnn import DatasetFDnCNN


class DatasetFFDNet(DatasetFDnCNN):
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
        return {"L": img_L, "H": img_H, "C": noise_level.view(1, 1, 1), "L_path": H_path, "H_path": H_path}
