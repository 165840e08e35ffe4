"""HBM-resident training-patch synthesis: the batches of the Dataset* loaders made by HIP launches
from an image pool on the device, so 8 GPUs are not fed by Python loaders.

    synth = PatchSynth(pool, task="sr", scale=4, H_size=192, seed=0)    # pool [N, C, Hs, Ws] fp32 [0, 1]
    L, H = synth.next(32)                                               # device tensors, NCHW

Sampling follows the reference loaders: the image order is a seeded shuffled epoch (DataLoader(shuffle=True),
main_train_psnr.py:122-130; with `rank`/`world` the DistributedSampler's rank-strided slice of it), then per sample
random.randint for the crop rows / columns and the augment mode in the order __getitem__ draws them, then the task's
own draws.  The draws are made on the host (a few numbers per sample, one int32 table per batch), the pixels on the
device.

The module has two halves.  A task object (TASKS: one class per batch kind, its docstring the description of that
kind) holds the task's options and their checks, the sampler and the host draws; patch_draws() builds one from shapes
alone, so the tables can be drawn and checked on a machine without a device.  The same object knows its launch
sequence.  PatchSynth adds the device side every task shares: the pool, the pinned upload of the table, the step
counter that keys the noise, next() and next_dict().
"""
import math
import random

import torch

from .. import _hip as H
from ..utils import utils_blindsr as blindsr
from ..utils import utils_image as util
from ..utils import utils_sisr as sisr


BSR_COLS = 8 + blindsr.NSLOT * blindsr.NCOL   # the blind-SR program table's row


def _table(ints, floats=None):
    """The int32 table of a batch: its integer columns, then the float32 bits of its float columns."""
    t = torch.tensor(ints, dtype=torch.int32)
    if floats is None:
        return t
    return torch.cat((t, torch.tensor(floats, dtype=torch.float32).view(torch.int32)), 1)


class _Task:
    """What every batch kind shares: the geometry, the sampler and the four draws {image, rnd_h, rnd_w, mode} each
    sample starts with.  A subclass states its options (options), its draw (draw), the device tensors it prepares
    once (prepare), its launches (fill for the tasks of one launch, else launch) and, where it has one, its dict form
    (as_dict).

    sf: the scale factor between H and L (1: same size).  extra: the channels L has beyond H's.  takes_out:
    next(B, out=(L, H)) fills the caller's tensors."""
    sf, extra, takes_out = 1, 0, True

    def __init__(self, N, C, Hs, Ws, H_size=96, seed=0, rank=0, world=1, **options):
        self.N, self.C, self.Hs, self.Ws, self.PS = N, C, Hs, Ws, H_size
        self.Co = C   # the batch's channels
        self.options(**options)
        if self.PS > min(self.Hs, self.Ws):
            raise ValueError("PatchSynth: H_size larger than the pool images")
        self.seed = seed
        self.rng = random.Random(seed)
        self.rank, self.world = rank, world
        self.epoch, self.order, self.pos = 0, [], 0

    def _next_index(self):
        if self.pos >= len(self.order):
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            perm = torch.randperm(self.N, generator=g).tolist()
            self.order = perm[self.rank::self.world] if self.world > 1 else perm
            self.epoch += 1
            self.pos = 0
        i = self.order[self.pos]
        self.pos += 1
        return i

    def head(self, max_h, max_w):
        """One sample's {image, rnd_h, rnd_w, mode}, the corner drawn from [0, max_h] x [0, max_w]."""
        return [self._next_index(), self.rng.randint(0, max_h), self.rng.randint(0, max_w), self.rng.randint(0, 7)]

    def draw(self, B):
        """Host draws of the next batch: ([B, 4] int32 {image, rnd_h, rnd_w, mode}, the batch's scale factor).  The
        corner is in L's pixels (DatasetSR crops L and takes H at the corner x sf)."""
        ls = self.PS // self.sf
        max_h, max_w = max(0, self.Hs // self.sf - ls), max(0, self.Ws // self.sf - ls)
        return _table([self.head(max_h, max_w) for _ in range(B)]), self.sf

    def prepare(self, dev):
        pass

    def launch(self, s, B, par, host, sf, out):
        """The batch of a one-launch task: fill() writes L and H (the caller's `out`, or fresh tensors) and returns
        what else the batch has."""
        Co, ls, PS, dev = self.Co, self.PS // sf, self.PS, par.device
        Lp, Hp = out or (torch.empty(B, Co + self.extra, ls, ls, device=dev), torch.empty(B, Co, PS, PS, device=dev))
        return (Lp, Hp, *self.fill(s, B, par, sf, Hp, Lp))

    def as_dict(self, next_batch, B):
        raise ValueError("PatchSynth.next_dict: tasks 'usrnet', 'fdncnn', 'ffdnet' and 'srmd' only")


class _SR(_Task):
    """task="sr": DatasetSR batches (data/dataset_sr.py:78-91), the pool modcropped to the scale (dataset_sr.py:51).

        synth = PatchSynth(pool, task="sr", scale=4, H_size=192, seed=0)
        L, H = synth.next(32)                        # [B, C, 48, 48], [B, C, 192, 192]

    One launch (kair_synth_sr, csrc/synth.hip): L is the crop of the MATLAB-bicubic downscale of the whole image, H the
    aligned crop, both augmented.  `last_params` is the [B, 4] int32 table {image, rnd_h, rnd_w, mode}."""

    def options(self, scale=4):
        self.sf = scale
        self.Hs, self.Ws = self.Hs - self.Hs % scale, self.Ws - self.Ws % scale

    def prepare(self, dev):
        ih, wh = util.bicubic_taps(self.Hs, self.Hs // self.sf, 1.0 / self.sf)
        iw, ww = util.bicubic_taps(self.Ws, self.Ws // self.sf, 1.0 / self.sf)
        self.taps_h = (ih.to(dev), wh.to(dev))
        self.taps_w = (iw.to(dev), ww.to(dev))

    def fill(self, s, B, par, sf, Hp, Lp):
        H.synth_sr(s.pool, par, B, self.PS, sf, self.taps_h, self.taps_w, Hp, Lp)
        return ()


class _DN(_Task):
    """task="dn": DatasetDnCNN batches (data/dataset_dncnn.py:59-66): crop, augment, AWGN of one fixed sigma.

        synth = PatchSynth(pool, task="dn", H_size=40, sigma=25, seed=0)
        L, H = synth.next(64)                        # [B, C, 40, 40] twice

    One launch (kair_synth_dn, csrc/synth.hip; Philox normals keyed by seed and step).  `last_params` is the [B, 4]
    int32 table {image, rnd_h, rnd_w, mode}."""

    def options(self, sigma=25):
        self.sigma = sigma / 255.0

    def fill(self, s, B, par, sf, Hp, Lp):
        H.synth_dn(s.pool, par, B, self.PS, self.sigma, self.seed, s.step, Hp, Lp)
        return ()


class _FDnCNN(_Task):
    """task="fdncnn": DatasetFDnCNN batches (data/dataset_fdncnn.py) for FDnCNN and DRUNet: the noisy patch with its
    noise-level map as the last channel.

        synth = PatchSynth(pool, task="fdncnn", H_size=128, sigma=(0, 50), seed=0)
        L, H = synth.next(64)                        # [B, C + 1, 128, 128], [B, C, 128, 128]
        model.feed_data(synth.next_dict(64))         # the dict ModelPlain.feed_data reads

    Per sample, in this order: the image, rnd_h, rnd_w, the augment mode, then sigma = rng.uniform(min, max).  One
    launch (kair_synth_dn_map, csrc/synth.hip) does the crop, the augment, the per-sample AWGN (kair_synth_dn's Philox
    normals) and the map channel.  `last_params` is the [B, 5] int32 table {image, rnd_h, rnd_w, mode} plus the
    float32 bits of sigma / 255 (`last_params[:, 4:].view(torch.float32)`)."""
    name, extra = "fdncnn", 1

    def options(self, sigma=25):
        self.sigma_range = tuple(float(v) for v in sigma) if isinstance(sigma, (tuple, list)) else (float(sigma),) * 2
        if len(self.sigma_range) != 2 or not 0 <= self.sigma_range[0] <= self.sigma_range[1]:
            raise ValueError(f"PatchSynth: task '{self.name}' takes sigma as (min, max), 0 <= min <= max (got {sigma!r})")

    def draw(self, B):
        ints, lev = [], []
        for _ in range(B):
            ints.append(self.head(self.Hs - self.PS, self.Ws - self.PS))
            lev.append([self.rng.uniform(*self.sigma_range) / 255.0])
        return _table(ints, lev), 1

    def fill(self, s, B, par, sf, Hp, Lp):
        H.synth_dn_map(s.pool, par, B, self.PS, self.seed, s.step, Hp, Lp)
        return ()

    def as_dict(self, next_batch, B):
        return dict(zip(("L", "H", "C"), next_batch(B)))


class _FFDNet(_FDnCNN):
    """task="ffdnet": DatasetFFDNet batches (data/dataset_ffdnet.py) for FFDNet: task "fdncnn"'s draws, Philox key and
    counters, but the level is a second tensor instead of a map channel.

        synth = PatchSynth(pool, task="ffdnet", H_size=64, sigma=(0, 75), seed=0)
        L, H, C = synth.next(64)                     # [B, C, 64, 64] twice, the levels sigma / 255 as [B, 1, 1, 1]
        model.feed_data(synth.next_dict(64))         # the {"L", "H", "C"} dict ModelPlain2.feed_data reads

    One launch (kair_synth_dn_level: kair_synth_dn_map's device code); with the same arguments L equals task
    "fdncnn"'s L[:, :C] and C its map value, bit for bit.  next(B, out=(L, H)) allocates C itself."""
    name, extra = "ffdnet", 0

    def fill(self, s, B, par, sf, Hp, Lp):
        Cp = torch.empty(B, 1, 1, 1, device=par.device)
        H.synth_dn_level(s.pool, par, B, self.PS, self.seed, s.step, Hp, Lp, Cp)
        return (Cp,)


class _JPEG(_Task):
    """task="jpeg": DatasetJPEG batches (data/dataset_jpeg.py:40-96) for the JPEG artifact-reduction SwinIR.

        synth = PatchSynth(pool, task="jpeg", H_size=126, quality_factor=40, is_color=False, seed=0)
        L, H = synth.next(8)                         # [B, 1 (or 3 with is_color), 126, 126]

    Per sample, in this order: the image, rnd_h and rnd_w of the (H_size + 8)^2 crop, the augment mode, the gray
    conversion (not with is_color; random() > 0.5: rgb2ycbcr Y, mode 0, else OpenCV's RGB2GRAY, mode 1), the quality
    (an int as in the reference, or a list to draw from uniformly: blind CAR, an extension) and one random() > 0.5
    that decides whether the second H_size^2 crop sits at random offsets rh2, rw2 in [0, 8] or at (0, 0).  One launch
    (kair_synth_jpeg, csrc/synth_jpeg.hip) does the crop, augment, uint8 and gray conversion, the JPEG round trip and
    the second crop.  `last_params` is the [B, 8] int32 table {image, rnd_h, rnd_w, mode, gray_mode, quality, rh2,
    rw2}."""

    def options(self, quality_factor=40, is_color=False):
        self.qualities = [int(quality_factor)] if isinstance(quality_factor, int) else [int(q) for q in quality_factor]
        if not self.qualities or any(q < 1 or q > 100 for q in self.qualities):
            raise ValueError("PatchSynth: quality_factor must be an int or a list of ints in 1..100")
        self.q_drawn = not isinstance(quality_factor, int)   # an int (the reference's option) costs no draw
        self.is_color = bool(is_color)
        self.Co = 3 if self.is_color else 1
        if self.C not in (1, 3) or (self.is_color and self.C != 3):
            raise ValueError("PatchSynth: task 'jpeg' needs a 1- or 3-channel pool (3 with is_color)")
        if self.PS + 8 > min(self.Hs, self.Ws):
            raise ValueError(f"PatchSynth: task 'jpeg' crops H_size + 8 = {self.PS + 8}; the pool images are smaller")

    def draw(self, B):
        rows = []
        max_h, max_w = max(0, self.Hs - self.PS - 8), max(0, self.Ws - self.PS - 8)
        for _ in range(B):
            row = self.head(max_h, max_w)
            gray_mode = 0 if self.is_color or self.rng.random() > 0.5 else 1   # with is_color nothing is drawn
            q = self.rng.choice(self.qualities) if self.q_drawn else self.qualities[0]
            rh2 = rw2 = 0
            if self.rng.random() > 0.5:
                rh2, rw2 = self.rng.randint(0, 8), self.rng.randint(0, 8)
            rows.append(row + [gray_mode, q, rh2, rw2])
        return _table(rows), 1

    def fill(self, s, B, par, sf, Hp, Lp):
        H.synth_jpeg(s.pool, par, B, self.PS, self.is_color, Hp, Lp)
        return ()


class _USRNet(_Task):
    """task="usrnet": DatasetUSRNet batches (data/dataset_usrnet.py:46-113).

        synth = PatchSynth(pool, task="usrnet", H_size=96, scales=[1, 2, 3, 4], sigma_max=25, seed=0)
        L, H, k, sf, sigma = synth.next(48)          # k [B, 1, 25, 25], sf an int, sigma [B, 1, 1, 1]
        model.feed_data(synth.next_dict(48))         # the dict ModelPlain4.feed_data reads (sf an int64 tensor [B])

    Per batch one scale factor from `scales` (dataset_usrnet.py:54-58); per sample, in this order, the image, rnd_h,
    rnd_w, the augment mode, the kernel draw r in [0, 8) (r > 3 and a kernel bank present: a uniform bank row;
    otherwise a Gaussian with lambda_1, lambda_2 ~ U(0.6, 12), theta ~ U(0, pi), sf_k from [1, 2, 3, 4], augment
    mode_k) and the noise level (0 with probability 1/8, else randint(0, sigma_max - 1) / 255).  The reference's
    motion-blur branch (utils_deblur.blurkernel_synthesis) is not built; `kernel_bank` ([K, ks, ks], e.g. exported
    motion kernels) stands in for it, and without a bank every kernel is Gaussian.  The kernels
    (kair_usr_gauss_kernels) and the batch (kair_synth_usr: crop, augment, circular blur, [0::sf] decimation, AWGN)
    are two launches of csrc/synth_usr.hip.  `last_params` is the [B, 12] int32 table: columns 0-3 {image, rnd_h,
    rnd_w, mode}, 4-7 {kernel source (0 Gaussian, 1 bank), bank_idx, sf_k, mode_k}, 8-11 the float32 bits of
    {lambda_1, lambda_2, theta, sigma} (`last_params[:, 8:].view(torch.float32)`)."""
    takes_out = False

    def options(self, scales=(1, 2, 3, 4), sigma_max=25, kernel_size=25, kernel_bank=None, trunc8=False):
        self.scales = [int(s) for s in scales]
        bad = [s for s in self.scales if s < 1 or self.PS % s]
        if not self.scales or bad:
            raise ValueError(f"PatchSynth: H_size {self.PS} is not divisible by the scales {bad or self.scales}")
        self.sigma_max, self.ks, self.trunc8 = int(sigma_max), int(kernel_size), bool(trunc8)
        if self.sigma_max < 1 or self.ks < 1:
            raise ValueError("PatchSynth: sigma_max and kernel_size must be positive")
        self.bank = None
        if kernel_bank is not None:   # a tensor on any device; prepare() moves it
            self.bank = torch.as_tensor(kernel_bank)
            if self.bank.dim() != 3 or tuple(self.bank.shape[-2:]) != (self.ks, self.ks):
                raise ValueError(f"PatchSynth: kernel_bank must be [K, {self.ks}, {self.ks}]")

    def draw(self, B):
        sf = self.rng.choice(self.scales)
        ints, flts = [], []
        K = 0 if self.bank is None else self.bank.shape[0]
        for _ in range(B):
            row = self.head(self.Hs - self.PS, self.Ws - self.PS) + [0, 0, 1, 0]
            fl = [0.0, 0.0, 0.0, 0.0]
            if self.rng.randint(0, 7) > 3 and K:
                row[4], row[5] = 1, self.rng.randint(0, K - 1)
            else:
                fl[:3] = self.rng.uniform(0.6, 12.0), self.rng.uniform(0.6, 12.0), self.rng.uniform(0.0, math.pi)
                row[6], row[7] = self.rng.choice([1, 2, 3, 4]), self.rng.randint(0, 7)
            if self.rng.randint(0, 7) != 1:
                fl[3] = self.rng.randint(0, self.sigma_max - 1) / 255.0
            ints.append(row)
            flts.append(fl)
        return _table(ints, flts), sf

    def prepare(self, dev):
        if self.bank is not None:
            self.bank = self.bank.to(dev, torch.float32).contiguous()

    def fill(self, s, B, par, sf, Hp, Lp):
        fl = par[:, 8:].view(torch.float32)
        k = torch.empty(B, 1, self.ks, self.ks, device=par.device)
        H.usr_gauss_kernels(fl, par[:, 4:8], self.bank, k)
        H.synth_usr(s.pool, par, B, self.PS, sf, k, fl[:, 3], self.trunc8, self.seed, s.step, Hp, Lp)
        return k, sf, fl[:, 3].reshape(B, 1, 1, 1).contiguous()

    def as_dict(self, next_batch, B):
        L, Hh, k, sf, sigma = next_batch(B)
        return {"L": L, "H": Hh, "k": k, "sf": torch.full((B,), sf, dtype=torch.int64), "sigma": sigma}


class _SRMD(_Task):
    """task="srmd": DatasetSRMD batches (data/dataset_srmd.py) for SRMD: the blurred, bicubically downscaled and noisy
    patch, followed by its degradation map.

        synth = PatchSynth(pool, task="srmd", scale=4, H_size=96, sigma=(0, 50), seed=0)
        L, H = synth.next(64)                        # [B, C + 16, 24, 24], [B, C, 96, 96]
        model.feed_data(synth.next_dict(64))         # the {"L", "H"} dict ModelPlain.feed_data reads

    Per sample, in this order: the image, rnd_h, rnd_w (the H crop's corner), the augment mode, the kernel draw
    theta ~ U(0, pi), l1 ~ U(0.1, l_max), l2 ~ U(0.1, l1) (utils_sisr.draw_srmd_kernel) and
    sigma = rng.uniform(min, max) / 255 (task "fdncnn"'s rule).  Two launches of csrc/synth_srmd.hip: the kernels with
    their PCA codes (kair_srmd_kernels; `pca` [15, 225], default utils_sisr.cal_pca_matrix()), and the batch
    (kair_synth_srmd: crop, augment, circular 15 x 15 blur, MATLAB-bicubic x1/scale of the patch, AWGN, map channels).
    noise_channel=False is the noise-free SRMDNF: L has C + 15 channels, sigma is not drawn and nothing is added.
    `last_params` is the [B, 8] int32 table: columns 0-3 {image, rnd_h, rnd_w, mode}, 4-7 the float32 bits of {theta,
    l1, l2, sigma} (`last_params[:, 4:].view(torch.float32)`); `last_kernels` the [B, 1, 15, 15] kernels and
    `last_codes` their [B, 15] codes."""

    def options(self, scale=4, sigma=(0, 50), l_max=10.0, pca=None, noise_channel=True):
        self.sf = int(scale)
        if self.sf not in (2, 3, 4):
            raise ValueError(f"PatchSynth: task 'srmd' takes scale 2, 3 or 4 (got {scale!r})")
        if self.PS % self.sf:
            raise ValueError(f"PatchSynth: H_size {self.PS} is not divisible by the scale {self.sf}")
        self.sigma_range = tuple(float(v) for v in sigma) if isinstance(sigma, (tuple, list)) else (float(sigma),) * 2
        if len(self.sigma_range) != 2 or not 0 <= self.sigma_range[0] <= self.sigma_range[1]:
            raise ValueError(f"PatchSynth: task 'srmd' takes sigma as (min, max), 0 <= min <= max (got {sigma!r})")
        self.l_max = float(l_max)
        if not self.l_max > 0.1:
            raise ValueError(f"PatchSynth: task 'srmd' draws l1 from U(0.1, l_max): l_max > 0.1 (got {l_max!r})")
        self.noise_channel = bool(noise_channel)
        ks, dim = sisr.SRMD_KSIZE, sisr.SRMD_DIM_PCA
        P = sisr.cal_pca_matrix(ks, self.l_max, dim) if pca is None else torch.as_tensor(pca)
        if tuple(P.shape) != (dim, ks * ks):
            raise ValueError(f"PatchSynth: pca must be [{dim}, {ks * ks}] (got {tuple(P.shape)})")
        self.pca = P.float().contiguous()
        self.extra = dim + int(self.noise_channel)
        it, wt = util.bicubic_taps(self.PS, self.PS // self.sf, 1.0 / self.sf)
        if int(it.min()) < 0 or int(it.max()) >= self.PS:
            raise ValueError(f"PatchSynth: H_size {self.PS} is too small for the bicubic x1/{self.sf} taps")
        self.taps = (it, wt)

    def draw(self, B):
        ints, flts = [], []
        for _ in range(B):
            ints.append(self.head(self.Hs - self.PS, self.Ws - self.PS))
            theta, l1, l2 = sisr.draw_srmd_kernel(self.rng, self.l_max)
            flts.append([theta, l1, l2, self.rng.uniform(*self.sigma_range) / 255.0 if self.noise_channel else 0.0])
        return _table(ints, flts), self.sf

    def prepare(self, dev):
        self.pca = self.pca.to(dev)
        self.taps = tuple(t.to(dev) for t in self.taps)

    def fill(self, s, B, par, sf, Hp, Lp):
        fl = par[:, 4:].view(torch.float32)
        self.last_kernels = torch.empty(B, 1, sisr.SRMD_KSIZE, sisr.SRMD_KSIZE, device=par.device)
        self.last_codes = torch.empty(B, self.pca.shape[0], device=par.device)
        H.srmd_kernels(fl, self.pca, self.last_kernels, self.last_codes)
        H.synth_srmd(s.pool, par, B, self.PS, sf, self.last_kernels, self.last_codes, self.noise_channel, self.taps,
                     self.seed, s.step, Hp, Lp, sigma_col=7)
        return ()

    def as_dict(self, next_batch, B):
        return dict(zip(("L", "H"), next_batch(B)))


class _DPSR(_SR):
    """task="dpsr": DatasetDPSR batches (data/dataset_dpsr.py) for the DPSR prior: task "sr"'s pair, AWGN of one level
    per sample on L, and the level as L's last channel.

        synth = PatchSynth(pool, task="dpsr", scale=4, H_size=96, sigma=(0, 50), seed=0)
        L, H = synth.next(16)                        # [B, C + 1, 24, 24], [B, C, 96, 96]
        model.feed_data(synth.next_dict(16))         # the {"L", "H"} dict ModelPlain.feed_data reads

    Per sample task "sr"'s four draws from the same generator -- so under one seed the crops and modes are task "sr"'s
    -- and sigma = uniform(min, max) / 255 from a generator of its own (seeded by the task's seed).  One launch
    (kair_synth_dpsr, csrc/synth.hip: kair_synth_sr's banded kernel with the noise, kair_synth_dn_map's Philox
    convention, and the level plane).  `last_params` is the [B, 8] int32 table {image, rnd_h, rnd_w, mode}, the float32
    bits of sigma / 255 (`last_params[:, 4:5].view(torch.float32)`), three unused columns."""
    name, extra = "dpsr", 1

    def options(self, scale=4, sigma=(0, 50)):
        if scale not in (2, 3, 4):
            raise ValueError(f"PatchSynth: task 'dpsr' takes scale 2, 3 or 4 (got {scale!r})")
        if self.PS % scale:
            raise ValueError(f"PatchSynth: H_size {self.PS} is not divisible by the scale {scale}")
        super().options(scale)
        self.sigma_range = tuple(float(v) for v in sigma) if isinstance(sigma, (tuple, list)) else (float(sigma),) * 2
        if len(self.sigma_range) != 2 or not 0 <= self.sigma_range[0] <= self.sigma_range[1]:
            raise ValueError(f"PatchSynth: task 'dpsr' takes sigma as (min, max), 0 <= min <= max (got {sigma!r})")
        self.level_rng = None

    def draw(self, B):
        if self.level_rng is None:
            self.level_rng = random.Random(self.seed * 2654435761 + 0xD95)
        heads, sf = super().draw(B)
        lev = [[self.level_rng.uniform(*self.sigma_range) / 255.0, 0.0, 0.0, 0.0] for _ in range(B)]
        return _table(heads.tolist(), lev), sf

    def fill(self, s, B, par, sf, Hp, Lp):
        H.synth_dpsr(s.pool, par, B, self.PS, sf, self.taps_h, self.taps_w, self.seed, s.step, Hp, Lp)
        return ()

    def as_dict(self, next_batch, B):
        return dict(zip(("L", "H"), next_batch(B)))


class _BlindSR(_Task):
    """task="blindsr": DatasetBlindSR batches (data/dataset_blindsr.py; the BSRGAN degradation of BSRNet / BSRGAN and
    the real-world SwinIR) from a 3-channel pool.

        synth = PatchSynth(pool, task="blindsr", scale=4, H_size=256, lq_patchsize=64, seed=0)
        L, H = synth.next(32)                        # [B, 3, 64, 64], [B, 3, 256, 256]

    Per sample, in this order: the image, rnd_h and rnd_w of the H_size^2 crop, the augment mode, then every draw of
    utils_blindsr.draw_bsrgan (that module's docstring lists them) from the same random.Random, so DatasetBlindSR with
    that generator takes identical decisions.  The pixels are made by a fixed sequence of launches whatever was drawn
    (csrc/synth_blindsr.hip, kair_jpeg_roundtrip_var): crop + augment, the blur kernels, slot 0 (the optional x1/2
    pre-downscale), slots 1-6 (an op launch and a JPEG launch pair each; whichever does not apply to a sample copies
    it or leaves it), the final JPEG, the two crops.  `last_params` is the [B, 136] int32 program table: columns 0-5
    {image, rnd_h, rnd_w, mode, lq_h, lq_w} (lq_* the corner of the L crop in the degraded image; H is cut at lq_* x
    scale), 6-7 unused, then 8 slots of 16 columns, slot s at 8 + 16 s: {op, h_in, w_in, h_out, w_out, i0, i1,
    quality} and eight float32 bits, as utils_blindsr's docstring describes them (`last_params[:, 8:].view(B, 8, 16)`
    is the stack of the samples' `prog` tables).  debug_stages=True makes next() return (L, H, stages): stages[0] the
    cropped patches and stages[1 + s] the buffer after slot s, each (tensor [B, 3, H_size, H_size], [(h, w)] per
    sample), for the tests."""
    takes_out = False

    def options(self, scale=4, lq_patchsize=64, debug_stages=False):
        blindsr.check_sizes(self.PS, scale, lq_patchsize)
        if self.C != 3:
            raise ValueError("PatchSynth: task 'blindsr' needs a 3-channel pool (the JPEG steps are colour)")
        if self.PS // 8 < 5:
            raise ValueError("PatchSynth: task 'blindsr' needs H_size >= 40 (a working image of H_size / 8 must "
                             "keep the colour JPEG's minimum width of 5)")
        self.sf, self.lq, self.debug_stages = int(scale), int(lq_patchsize), bool(debug_stages)
        self._noise_off = False   # tests only: utils_blindsr.draw_bsrgan(noise_off=True)

    def draw(self, B):
        tab = torch.zeros(B, BSR_COLS, dtype=torch.int32)
        for b in range(B):
            row = self.head(self.Hs - self.PS, self.Ws - self.PS)
            prog, lh, lw = blindsr.draw_bsrgan(self.rng, self.PS, self.sf, self.lq, self._noise_off)
            tab[b, :6] = torch.tensor(row + [lh, lw], dtype=torch.int32)
            tab[b, 8:] = torch.from_numpy(prog.reshape(-1))
        return tab, self.sf

    def prepare(self, dev):
        ih, wh = util.bicubic_taps(self.PS, self.PS // 2, 0.5)   # the MATLAB x1/2 of slot 0
        self.taps_half = (ih.to(dev), wh.to(dev), ih.to(dev), wh.to(dev), self.PS, self.PS)
        self._bsr_ws = None

    def launch(self, s, B, par, host, sf, out):
        dev = par.device
        PS, S, W = self.PS, blindsr.NSLOT, blindsr.NCOL
        if self._bsr_ws is None or self._bsr_ws[0] != B:
            self._bsr_ws = (B, torch.empty(B, 3, PS, PS, device=dev), torch.empty(B, 3, PS, PS, device=dev),
                            torch.empty(S, B, 25, 25, device=dev), H.jpeg_var_workspace(B, PS, PS, dev))
        _, a, b, kern, jws = self._bsr_ws
        slot = lambda i: par[:, 8 + W * i:8 + W * (i + 1)]   # noqa: E731
        stages = []

        def keep(buf, hw_cols):
            if self.debug_stages:
                stages.append((buf.clone(), [tuple(r) for r in host[:, hw_cols[0]:hw_cols[1]].tolist()]))

        w_min = PS // 8
        H.bsr_crop(s.pool, par, B, PS, a)
        keep(a, (8 + 1, 8 + 3))
        H.bsr_kernels(par[:, 8:], S, W, kern)
        for i in range(S - 1):   # slot 0 the pre-downscale, 1-6 the drawn ops; a <-> b
            H.bsr_ops(a, b, slot(i), kern[i], self.taps_half if i == 0 else None, self.seed, s.step, i)
            if i:
                H.jpeg_roundtrip_var(b, slot(i)[:, 3:5], w_min, slot(i)[:, 7], b, jws)
            a, b = b, a
            keep(a, (8 + W * i + 3, 8 + W * i + 5))
        i = S - 1   # the final JPEG, in place
        H.jpeg_roundtrip_var(a, slot(i)[:, 3:5], w_min, slot(i)[:, 7], a, jws)
        keep(a, (8 + W * i + 3, 8 + W * i + 5))
        Lp = torch.empty(B, 3, self.lq, self.lq, device=dev)
        Hp = torch.empty(B, 3, self.lq * sf, self.lq * sf, device=dev)
        H.bsr_finish(s.pool, par, B, PS, sf, self.lq, a, Lp, Hp)
        return (Lp, Hp, stages) if self.debug_stages else (Lp, Hp)


TASKS = {"sr": _SR, "dn": _DN, "fdncnn": _FDnCNN, "ffdnet": _FFDNet, "jpeg": _JPEG, "usrnet": _USRNet,
         "blindsr": _BlindSR}
# TASKS is the set tests/test_patch_draws_cpu.py pins draw for draw against tables recorded before the task classes
# existed (it asserts that its cases cover exactly TASKS); a task with no such recorded parent is registered here and
# has its draws tested in a file of its own (tests/test_srmd_cpu.py, tests/test_ressr_cpu.py)
NEW_TASKS = {"srmd": _SRMD, "dpsr": _DPSR}


def patch_draws(task, N, C, Hs, Ws, H_size=96, seed=0, rank=0, world=1, **options):
    """The host half of PatchSynth for a pool of shape [N, C, Hs, Ws]: the task object with its options checked, whose
    draw(B) gives (the next batch's int32 table, its scale factor).  Needs no device."""
    if task not in TASKS and task not in NEW_TASKS:
        raise ValueError(task)
    return (TASKS.get(task) or NEW_TASKS[task])(N, C, Hs, Ws, H_size, seed, rank, world, **options)


class PatchSynth:
    """The batches of one task (TASKS, NEW_TASKS) from a device pool [N, C, Hs, Ws]; `options` are that task's (its class's
    docstring and options()).  The geometry and the sampler (N, C, Hs, Ws, PS, seed, rng, rank, world) are on the
    task object, `kind`."""

    def __init__(self, pool, task="sr", *, H_size=96, seed=0, rank=0, world=1, **options):
        if pool.dim() != 4 or not pool.is_cuda:
            raise ValueError("PatchSynth: pool must be a device tensor [N, C, Hs, Ws]")
        self.kind = k = patch_draws(task, *pool.shape, H_size, seed, rank, world, **options)
        self.pool = pool[..., :k.Hs, :k.Ws].float().contiguous()   # task "sr" modcrops
        k.prepare(self.pool.device)
        self.step = 0
        self._par_host = None
        self._par_ev = None

    last_kernels = property(lambda self: self.kind.last_kernels)   # task "srmd": the last batch's kernels and codes
    last_codes = property(lambda self: self.kind.last_codes)
    # tests/test_blindsr_gpu.py sets and reads these two on the synth; they are the blind-SR task object's
    _noise_off = property(lambda self: self.kind._noise_off, lambda self, v: setattr(self.kind, "_noise_off", v))
    _bsr_ws = property(lambda self: self.kind._bsr_ws)

    def _upload(self, host):
        """The host table on the device, through a pinned staging buffer with an async copy, so a training loop that
        calls next() every step never blocks the host on the device."""
        B = host.shape[0]
        if self._par_host is None or self._par_host.shape[0] < B:
            self._par_host = torch.empty(B, host.shape[1], dtype=torch.int32).pin_memory()
            self._par_ev = None
        if self._par_ev is not None:
            self._par_ev.synchronize()   # the previous batch's copy has read the staging buffer
        self._par_host[:B].copy_(host)
        par = self._par_host[:B].to(self.pool.device, non_blocking=True)
        self._par_ev = torch.cuda.Event()
        self._par_ev.record()
        return par

    def next(self, B, out=None):
        """The next batch, produced on the current stream: (L, H); task "usrnet": (L, H, k, sf, sigma); task "ffdnet":
        (L, H, C), C the levels [B, 1, 1, 1].  out=(L, H): tensors to fill instead of fresh ones, for the tasks of
        one launch; "usrnet" (L's size is drawn) and "blindsr" refuse it with a ValueError."""
        if out is not None and not self.kind.takes_out:
            raise ValueError("PatchSynth.next: this task allocates its own outputs (out= is not supported)")
        host, sf = self.kind.draw(B)
        par = self._upload(host)
        batch = self.kind.launch(self, B, par, host, sf, out)
        self.step += 1
        self.last_params = par
        return batch

    def next_dict(self, B):
        """The next batch as the dict the task's model reads in feed_data: "usrnet" {"L", "H", "k", "sf", "sigma"}
        (ModelPlain4), "fdncnn", "srmd" and "dpsr" {"L", "H"} (ModelPlain), "ffdnet" {"L", "H", "C"} (ModelPlain2); a ValueError
        for the other tasks."""
        return self.kind.as_dict(self.next, B)


def synthetic_pool(N, C, Hs, Ws, seed=0, device="cuda"):
    """Seeded natural-ish images for the pool when no dataset is on the box (SURVEY §8d recipe:
    bicubic-upsampled uniform noise + 0.02 N, clamped to [0, 1])."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(N, C, max(1, Hs // 8), max(1, Ws // 8), generator=g)
    img = torch.nn.functional.interpolate(base, size=(Hs, Ws), mode="bicubic", align_corners=False)
    img = (img + 0.02 * torch.randn(img.shape, generator=g)).clamp(0, 1)
    return img.to(device)
