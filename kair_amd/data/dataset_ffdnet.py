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
from .dataset_fdncnn import DatasetFDnCNN


class DatasetFFDNet(DatasetFDnCNN):
    def _with_level(self, img_L, img_H, noise_level):
        return {"L": img_L, "H": img_H, "C": noise_level.view(1, 1, 1)}
