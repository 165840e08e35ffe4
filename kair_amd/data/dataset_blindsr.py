"""DatasetBlindSR (the reference's data/dataset_blindsr.py): real-world SR pairs for BSRNet / BSRGAN and the
real-world SwinIR (train_bsrgan_x4_psnr.json, train_swinir_sr_realworld_x4_psnr.json; "dataset_type": "blindsr").

train: the image as RGB, a random 'H_size' crop, one of the 8 flip/rot modes, uint2single, then the BSRGAN
       degradation of utils/utils_blindsr.py (two blurs, two resizes, noise, JPEG in a random order, a final JPEG and
       the aligned 'lq_patchsize' / 'lq_patchsize' x 'scale' crops).  Draws, in this order: rnd_h, rnd_w, the mode,
       then utils_blindsr.draw_bsrgan -- all from `self.rng` (the `random` module unless a random.Random is put there).
test:  the paired L from 'dataroot_L' when given, else the MATLAB-bicubic L of the mod-cropped H, as DatasetSR.

'degradation_type' is "bsrgan" only; "bsrgan_plus" raises NotImplementedError.
kair_amd.data.gpu_synth.PatchSynth(task="blindsr") takes the same decisions for the same seed and produces the
pixels on the GPU (csrc/synth_blindsr.hip).
"""
import random

import numpy as np
import torch
import torch.utils.data as data

from ..utils import utils_blindsr as blindsr
from ..utils import utils_image as util


class DatasetBlindSR(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.n_channels = opt.get("n_channels") or 3
        self.sf = opt.get("scale") or 4
        self.patch_size = opt.get("H_size") or 96
        self.lq_patchsize = opt.get("lq_patchsize") or 64
        self.degradation_type = opt.get("degradation_type") or "bsrgan"
        if self.degradation_type != "bsrgan":
            raise NotImplementedError(f"DatasetBlindSR: degradation_type [{self.degradation_type}] is not built "
                                      "(bsrgan only)")
        if self.n_channels != 3:
            raise ValueError("DatasetBlindSR: n_channels must be 3 (the JPEG steps are colour)")
        blindsr.check_sizes(self.patch_size, self.sf, self.lq_patchsize)
        self.paths_H = util.get_image_paths(opt["dataroot_H"])
        self.paths_L = util.get_image_paths(opt.get("dataroot_L"))
        assert self.paths_H, "Error: H path is empty."
        self.rng = random
        self._noise_off = False   # tests only: utils_blindsr.draw_bsrgan(noise_off=True)

    def __getitem__(self, index):
        H_path = self.paths_H[index]
        L_path = None
        img_H = util.imread_uint(H_path, 3)
        if self.opt["phase"] == "train":
            H, W = img_H.shape[:2]
            ps = self.patch_size
            if H < ps or W < ps:
                raise ValueError(f"DatasetBlindSR: {H_path} is smaller than H_size {ps}")
            rnd_h = self.rng.randint(0, H - ps)
            rnd_w = self.rng.randint(0, W - ps)
            patch = img_H[rnd_h:rnd_h + ps, rnd_w:rnd_w + ps, :]
            patch = np.ascontiguousarray(util.augment_img(patch, mode=self.rng.randint(0, 7)))
            img_L, img_H = blindsr.degradation_bsrgan(util.uint2single(patch), self.sf, self.lq_patchsize, self.rng,
                                                      np.float32, self._noise_off)
        else:
            img_H = util.modcrop(util.uint2single(img_H), self.sf)
            if self.paths_L:
                L_path = self.paths_L[index]
                img_L = util.uint2single(util.imread_uint(L_path, 3))
            else:
                t = torch.from_numpy(np.ascontiguousarray(img_H)).permute(2, 0, 1)
                img_L = util.imresize(t, 1 / self.sf, True).permute(1, 2, 0).numpy()
        return {"L": util.single2tensor3(img_L), "H": util.single2tensor3(img_H), "L_path": L_path or H_path,
                "H_path": H_path}

    def __len__(self):
        return len(self.paths_H)
