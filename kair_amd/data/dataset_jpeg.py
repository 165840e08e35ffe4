"""DatasetJPEG (restatement of /root/reference/data/dataset_jpeg.py:12-118): JPEG-compressed L and clean H for the
compression artifact reduction SwinIR (train_swinir_car_jpeg.json).

train: the image as RGB (40-43), a random 'H_size' + 8 crop (52-57), one of the 8 flip/rot modes (59-61); colour:
       H is the patch and L its JPEG round trip at 'quality_factor' (4:2:0, as cv2.imencode writes it; 63-69); gray:
       H is the rgb2ycbcr Y or the RGB2GRAY of the patch, picked by random.random() > 0.5, and L the gray JPEG round
       trip (70-80); then, with probability 1/2, a second 'H_size' crop of both at random offsets in [0, 8], else at
       (0, 0) (82-88), so the 8 x 8 block grid does not always sit at the patch's corner.
test:  the whole image, gray by rgb2ycbcr, 'quality_factor_test' (90-108).

The codec is Pillow's libjpeg (the reference uses cv2's; both wrap libjpeg at the default ISLOW DCT); without Pillow
it is utils_jpeg.jpeg_roundtrip_np, the same integer arithmetic (tests/test_jpeg_cpu.py compares the two bit for
bit).  kair_amd.data.gpu_synth.PatchSynth(task="jpeg") produces the same batches on the GPU (csrc/synth_jpeg.hip).
"""
import random

import numpy as np
import torch.utils.data as data

from ..utils import utils_image as util
from ..utils import utils_jpeg as jpg


def codec_roundtrip(img, quality):
    """uint8 [H, W] / [H, W, 3] through a JPEG encode + decode: Pillow when it imports, else the numpy statement."""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return jpg.jpeg_roundtrip_np(img, quality)
    return jpg.jpeg_roundtrip_pil(img, quality)


class DatasetJPEG(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.n_channels = opt.get("n_channels") or 3
        self.patch_size = opt.get("H_size") or 128
        self.quality_factor = opt.get("quality_factor") or 40
        self.quality_factor_test = opt.get("quality_factor_test") or 40
        self.is_color = bool(opt.get("is_color") or False)
        self.paths_H = util.get_image_paths(opt["dataroot_H"])
        assert self.paths_H, "Error: H path is empty."

    def __getitem__(self, index):
        H_path = self.paths_H[index]
        img_H = util.imread_uint(H_path, 3)
        if self.opt["phase"] == "train":
            H, W = img_H.shape[:2]
            ps = self.patch_size + 8
            rnd_h = random.randint(0, max(0, H - ps))
            rnd_w = random.randint(0, max(0, W - ps))
            patch = img_H[rnd_h:rnd_h + ps, rnd_w:rnd_w + ps, :]
            patch = np.ascontiguousarray(util.augment_img(patch, mode=random.randint(0, 7)))
            if self.is_color:
                img_H = patch
            elif random.random() > 0.5:
                img_H = util.rgb2ycbcr(patch)
            else:
                img_H = jpg.rgb2gray_cv(patch)
            img_L = codec_roundtrip(img_H, self.quality_factor)
            rnd_h = rnd_w = 0
            if random.random() > 0.5:
                rnd_h, rnd_w = random.randint(0, 8), random.randint(0, 8)
            img_H = img_H[rnd_h:rnd_h + self.patch_size, rnd_w:rnd_w + self.patch_size]
            img_L = img_L[rnd_h:rnd_h + self.patch_size, rnd_w:rnd_w + self.patch_size]
        else:
            if not self.is_color:
                img_H = util.rgb2ycbcr(img_H)
            img_L = codec_roundtrip(img_H, self.quality_factor_test)
        return {"L": util.uint2tensor3(img_L), "H": util.uint2tensor3(img_H), "L_path": H_path, "H_path": H_path}

    def __len__(self):
        return len(self.paths_H)
