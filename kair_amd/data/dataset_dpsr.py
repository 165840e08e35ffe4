"""DatasetDPSR (the reference's data/dataset_dpsr.py restated from upstream cszn/KAIR; the reference sources were not at
hand, and the restatement has not been checked against them): SR pairs for the DPSR super-resolver prior, whose L is
the noisy bicubic LR image followed by one constant noise-level channel.

It is DatasetSR's crop, augmentation and MATLAB-bicubic x1/sf (data/dataset_sr.py; the random draws come in the same
order, so under one seed the crop and the flip/rot mode are DatasetSR's), then one noise level per sample:
  train: level = np.random.uniform(sigma[0], sigma[1]) / 255 (sigma default [0, 50]), L += level * N(0, 1) from torch's
         generator (DatasetFDnCNN's rule);
  test:  level = sigma_test / 255 (default 0), noise from np.random.seed(0).
Returns {"L": [C + 1, h, w], "H": [C, sf h, sf w], "L_path", "H_path"}.

kair_amd.data.gpu_synth.PatchSynth(task="dpsr") makes the same batches on the device in one launch (kair_synth_dpsr,
csrc/synth.hip).
"""
import numpy as np
import torch

from .dataset_sr import DatasetSR


class DatasetDPSR(DatasetSR):
    def __init__(self, opt):
        super().__init__(opt)
        sigma = opt.get("sigma") if opt.get("sigma") is not None else [0, 50]
        if not isinstance(sigma, (list, tuple)) or len(sigma) != 2 or not 0 <= sigma[0] <= sigma[1]:
            raise ValueError(f"DatasetDPSR: sigma must be [min, max], 0 <= min <= max (got {sigma!r})")
        self.sigma_min, self.sigma_max = float(sigma[0]), float(sigma[1])
        self.sigma_test = float(opt.get("sigma_test") or 0)

    def __getitem__(self, index):
        d = super().__getitem__(index)
        img_L = d["L"]
        if self.opt["phase"] == "train":
            level = np.float32(np.random.uniform(self.sigma_min, self.sigma_max) / 255.0)
            noise = torch.randn(img_L.shape)
        else:
            level = np.float32(self.sigma_test / 255.0)
            np.random.seed(seed=0)
            noise = torch.from_numpy(np.random.normal(0, 1, tuple(img_L.shape)).astype(np.float32))
        if level > 0:
            img_L = img_L + float(level) * noise
        m = torch.full((1,) + tuple(img_L.shape[-2:]), float(level), dtype=img_L.dtype)
        d["L"] = torch.cat((img_L, m), 0)
        return d
