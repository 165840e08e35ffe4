"""HBM-resident training-patch synthesis: DatasetSR / DatasetDnCNN batches made
by one HIP launch from an image pool on the device, so 8 GPUs are not fed by Python loaders.

    synth = PatchSynth(pool, task="sr", scale=4, H_size=192, seed=0)    # pool [N, C, Hs, Ws] fp32 [0, 1]
    L, H = synth.next(32)                                               # device tensors, NCHW

Sampling follows the reference loaders: the image order is a seeded shuffled epoch
(DataLoader(shuffle=True), main_train_psnr.py:122-130; with `rank`/`world` the DistributedSampler's
rank-strided slice of it), then per sample random.randint for the crop rows / columns and the
augment mode in the order __getitem__ draws them (data/dataset_sr.py:78-91,
data/dataset_dncnn.py:59-66).  The per-sample geometry is drawn on the host (a few ints), the
pixels are produced on the device (kair_synth_sr / kair_synth_dn in csrc/synth.hip).

task="usrnet" makes DatasetUSRNet batches (data/dataset_usrnet.py:46-113) the same way:

    synth = PatchSynth(pool, task="usrnet", H_size=96, scales=[1, 2, 3, 4], sigma_max=25, seed=0)
    L, H, k, sf, sigma = synth.next(48)          # k [B, 1, 25, 25], sf an int, sigma [B, 1, 1, 1]
    model.feed_data(synth.next_dict(48))         # the dict ModelPlain4.feed_data reads

Per batch one scale factor from `scales` (dataset_usrnet.py:54-58); per sample, in this order, the image, rnd_h,
rnd_w, the augment mode, the kernel draw r in [0, 8) (r > 3 and a kernel bank present: a uniform bank row;
otherwise a Gaussian with lambda_1, lambda_2 ~ U(0.6, 12), theta ~ U(0, pi), sf_k from [1, 2, 3, 4], augment mode_k)
and the noise level (0 with probability 1/8, else randint(0, sigma_max - 1) / 255).  The reference's motion-blur
branch (utils_deblur.blurkernel_synthesis) is not built; `kernel_bank` ([K, ks, ks], e.g. exported motion kernels)
stands in for it, and without a bank every kernel is Gaussian.  The kernels (kair_usr_gauss_kernels) and the batch
(kair_synth_usr: crop, augment, circular blur, [0::sf] decimation, AWGN) are two launches of csrc/synth_usr.hip.
`last_params` is then the [B, 12] int32 table that went up: columns 0-3 {image, rnd_h, rnd_w, mode}, 4-7
{kernel source (0 Gaussian, 1 bank), bank_idx, sf_k, mode_k}, 8-11 the float32 bits of {lambda_1, lambda_2, theta,
sigma} (`last_params[:, 8:].view(torch.float32)`).

task="jpeg" makes DatasetJPEG batches (data/dataset_jpeg.py:40-96) for the JPEG artifact-reduction SwinIR:

    synth = PatchSynth(pool, task="jpeg", H_size=126, quality_factor=40, is_color=False, seed=0)
    L, H = synth.next(8)                         # [B, 1 (or 3 with is_color), 126, 126]

Per sample, in this order: the image, rnd_h and rnd_w of the (H_size + 8)^2 crop, the augment mode, the gray conversion
(not with is_color; random() > 0.5: rgb2ycbcr Y, mode 0, else OpenCV's RGB2GRAY, mode 1), the quality (an int as in the
reference, or a list to draw from uniformly: blind CAR, an extension) and one random() > 0.5 that decides whether the
second H_size^2 crop sits at random offsets rh2, rw2 in [0, 8] or at (0, 0).  One launch (kair_synth_jpeg,
csrc/synth_jpeg.hip) does the crop, augment, uint8 and gray conversion, the JPEG round trip and the second crop.
`last_params` is the [B, 8] int32 table {image, rnd_h, rnd_w, mode, gray_mode, quality, rh2, rw2}.

task="blindsr" makes DatasetBlindSR batches (data/dataset_blindsr.py; the BSRGAN degradation of BSRNet / BSRGAN and the
real-world SwinIR) from a 3-channel pool:

    synth = PatchSynth(pool, task="blindsr", scale=4, H_size=256, lq_patchsize=64, seed=0)
    L, H = synth.next(32)                        # [B, 3, 64, 64], [B, 3, 256, 256]

Per sample, in this order: the image, rnd_h and rnd_w of the H_size^2 crop, the augment mode, then every draw of
utils_blindsr.draw_bsrgan (that module's docstring lists them) from the same random.Random, so DatasetBlindSR with that
generator takes identical decisions.  The pixels are made by a fixed sequence of launches whatever was drawn
(csrc/synth_blindsr.hip, kair_jpeg_roundtrip_var): crop + augment, the blur kernels, slot 0 (the optional x1/2
pre-downscale), slots 1-6 (an op launch and a JPEG launch pair each; whichever does not apply to a sample copies it or
leaves it), the final JPEG, the two crops.  `last_params` is the [B, 136] int32 program table: columns 0-5 {image,
rnd_h, rnd_w, mode, lq_h, lq_w} (lq_* the corner of the L crop in the degraded image; H is cut at lq_* x scale),
6-7 unused, then 8 slots of 16 columns, slot s at 8 + 16 s: {op, h_in, w_in, h_out, w_out, i0, i1, quality} and eight
float32 bits, as utils_blindsr's docstring describes them (`last_params[:, 8:].view(B, 8, 16)` is the stack of the
samples' `prog` tables).  debug_stages=True makes next() return (L, H, stages): stages[0] the cropped patches and
stages[1 + s] the buffer after slot s, each (tensor [B, 3, H_size, H_size], [(h, w)] per sample), for the tests.

task="fdncnn" makes DatasetFDnCNN batches (data/dataset_fdncnn.py) for FDnCNN and DRUNet: the noisy patch with its
noise-level map as the last channel.

    synth = PatchSynth(pool, task="fdncnn", H_size=128, sigma=(0, 50), seed=0)
    L, H = synth.next(64)                        # [B, C + 1, 128, 128], [B, C, 128, 128]
    model.feed_data(synth.next_dict(64))         # the dict ModelPlain.feed_data reads

Per sample, in this order: the image, rnd_h, rnd_w, the augment mode, then sigma = rng.uniform(min, max).  One launch
(kair_synth_dn_map, csrc/synth.hip) does the crop, the augment, the per-sample AWGN (kair_synth_dn's Philox normals) and
the map channel.  `last_params` is the [B, 5] int32 table {image, rnd_h, rnd_w, mode} plus the float32 bits of
sigma / 255 (`last_params[:, 4:].view(torch.float32)`).

task="ffdnet" makes DatasetFFDNet batches (data/dataset_ffdnet.py) for FFDNet: the same draws (_draw_fdncnn), Philox key
and counters, but the level is a second tensor instead of a map channel.

    synth = PatchSynth(pool, task="ffdnet", H_size=64, sigma=(0, 75), seed=0)
    L, H, C = synth.next(64)                     # [B, C, 64, 64] twice, the levels sigma / 255 as [B, 1, 1, 1]
    model.feed_data(synth.next_dict(64))         # the {"L", "H", "C"} dict ModelPlain2.feed_data reads

One launch (kair_synth_dn_level: kair_synth_dn_map's device code); with the same arguments L equals task "fdncnn"'s
L[:, :C] and C its map value, bit for bit.
"""
import math
import random

import torch

from .. import _hip as H
from ..utils import utils_blindsr as blindsr
from ..utils import utils_image as util


BSR_COLS = 8 + blindsr.NSLOT * blindsr.NCOL   # the blind-SR program table's row


class PatchSynth:
    def __init__(self, pool, task="sr", scale=4, H_size=96, sigma=25, seed=0, rank=0, world=1, scales=(1, 2, 3, 4),
                 sigma_max=25, kernel_size=25, kernel_bank=None, trunc8=False, quality_factor=40, is_color=False,
                 lq_patchsize=64, debug_stages=False):
        if pool.dim() != 4 or not pool.is_cuda:
            raise ValueError("PatchSynth: pool must be a device tensor [N, C, Hs, Ws]")
        self.task = task
        if task == "usrnet":
            self.scales = [int(s) for s in scales]
            bad = [s for s in self.scales if s < 1 or H_size % s]
            if not self.scales or bad:
                raise ValueError(f"PatchSynth: H_size {H_size} is not divisible by the scales {bad or self.scales}")
            self.sigma_max, self.ks, self.trunc8 = int(sigma_max), int(kernel_size), bool(trunc8)
            if self.sigma_max < 1 or self.ks < 1:
                raise ValueError("PatchSynth: sigma_max and kernel_size must be positive")
            self.bank = None
            if kernel_bank is not None:
                bank = torch.as_tensor(kernel_bank).to(pool.device, torch.float32).contiguous()
                if bank.dim() != 3 or tuple(bank.shape[-2:]) != (self.ks, self.ks):
                    raise ValueError(f"PatchSynth: kernel_bank must be [K, {self.ks}, {self.ks}]")
                self.bank = bank
        if task == "jpeg":
            self.qualities = [int(quality_factor)] if isinstance(quality_factor, int) else [int(q) for q in quality_factor]
            if not self.qualities or any(q < 1 or q > 100 for q in self.qualities):
                raise ValueError("PatchSynth: quality_factor must be an int or a list of ints in 1..100")
            self.q_drawn = not isinstance(quality_factor, int)   # an int (the reference's option) costs no draw
            self.is_color = bool(is_color)
            if pool.shape[1] not in (1, 3) or (self.is_color and pool.shape[1] != 3):
                raise ValueError("PatchSynth: task 'jpeg' needs a 1- or 3-channel pool (3 with is_color)")
            if H_size + 8 > min(pool.shape[-2:]):
                raise ValueError(f"PatchSynth: task 'jpeg' crops H_size + 8 = {H_size + 8}; the pool images are smaller")
        if task == "blindsr":
            blindsr.check_sizes(H_size, scale, lq_patchsize)
            if pool.shape[1] != 3:
                raise ValueError("PatchSynth: task 'blindsr' needs a 3-channel pool (the JPEG steps are colour)")
            if H_size // 8 < 5:
                raise ValueError("PatchSynth: task 'blindsr' needs H_size >= 40 (a working image of H_size / 8 must "
                                 "keep the colour JPEG's minimum width of 5)")
            self.lq, self.bsr_sf, self.debug_stages = int(lq_patchsize), int(scale), bool(debug_stages)
            self._noise_off = False   # tests only: utils_blindsr.draw_bsrgan(noise_off=True)
        if task in ("fdncnn", "ffdnet"):
            self.sigma_range = tuple(float(v) for v in sigma) if isinstance(sigma, (tuple, list)) else (float(sigma),) * 2
            if len(self.sigma_range) != 2 or not 0 <= self.sigma_range[0] <= self.sigma_range[1]:
                raise ValueError(f"PatchSynth: task '{task}' takes sigma as (min, max), 0 <= min <= max (got {sigma!r})")
            sigma = self.sigma_range[1]
        self.sf = scale if task == "sr" else 1
        Hs, Ws = pool.shape[-2:]
        if task == "sr":   # modcrop (dataset_sr.py:51)
            pool = pool[..., :Hs - Hs % self.sf, :Ws - Ws % self.sf]
        self.pool = pool.float().contiguous()
        self.N, self.C, self.Hs, self.Ws = self.pool.shape
        self.PS = H_size
        if self.PS > min(self.Hs, self.Ws):
            raise ValueError("PatchSynth: H_size larger than the pool images")
        self.sigma = sigma / 255.0
        self.seed = seed
        self.rng = random.Random(seed)
        self.rank, self.world = rank, world
        self.epoch, self.order, self.pos = 0, [], 0
        self.step = 0
        dev = self.pool.device
        if task == "sr":
            ih, wh = util.bicubic_taps(self.Hs, self.Hs // self.sf, 1.0 / self.sf)
            iw, ww = util.bicubic_taps(self.Ws, self.Ws // self.sf, 1.0 / self.sf)
            self.taps_h = (ih.to(dev), wh.to(dev))
            self.taps_w = (iw.to(dev), ww.to(dev))
        elif task == "blindsr":
            ih, wh = util.bicubic_taps(self.PS, self.PS // 2, 0.5)   # the MATLAB x1/2 of slot 0
            self.taps_half = (ih.to(dev), wh.to(dev), ih.to(dev), wh.to(dev), self.PS, self.PS)
            self._bsr_ws = None
        elif task not in ("dn", "usrnet", "jpeg", "fdncnn", "ffdnet"):
            raise ValueError(task)
        self._par_host = None
        self._par_ev = None

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

    def draw(self, B):
        """Host-side geometry of the next batch: [B, 4] int32 {image, rnd_h, rnd_w, mode}."""
        rows = []
        ls = self.PS // self.sf
        hl, wl = self.Hs // self.sf, self.Ws // self.sf
        for _ in range(B):
            img = self._next_index()
            rh = self.rng.randint(0, max(0, hl - ls))
            rw = self.rng.randint(0, max(0, wl - ls))
            mode = self.rng.randint(0, 7)
            rows.append((img, rh, rw, mode))
        return torch.tensor(rows, dtype=torch.int32)

    def next(self, B, out=None):
        """The next batch (L, H), produced on the current stream.  The per-sample geometry goes up
        through a pinned staging buffer with an async copy, so a training loop that calls next()
        every step never blocks the host on the device.  task "usrnet": (L, H, k, sf, sigma); task "ffdnet":
        (L, H, C), C the levels [B, 1, 1, 1]."""
        if self.task == "usrnet":
            return self._next_usr(B)
        if self.task == "blindsr":
            return self._next_blindsr(B)
        dev = self.pool.device
        jpeg, fdn, ffd = self.task == "jpeg", self.task == "fdncnn", self.task == "ffdnet"
        host = self._draw_jpeg(B) if jpeg else self._draw_fdncnn(B) if fdn or ffd else self.draw(B)
        if self._par_host is None or self._par_host.shape[0] < B:
            self._par_host = torch.empty(B, host.shape[1], dtype=torch.int32).pin_memory()
            self._par_ev = None
        if self._par_ev is not None:
            self._par_ev.synchronize()   # the previous batch's copy has read the staging buffer
        self._par_host[:B].copy_(host)
        par = self._par_host[:B].to(dev, non_blocking=True)
        self._par_ev = torch.cuda.Event()
        self._par_ev.record()
        ls = self.PS // self.sf
        Co = (3 if self.is_color else 1) if jpeg else self.C
        if out is None:
            Hp = torch.empty(B, Co, self.PS, self.PS, device=dev)
            Lp = torch.empty(B, Co + 1 if fdn else Co, ls, ls, device=dev)
        else:
            Lp, Hp = out
        if jpeg:
            H.synth_jpeg(self.pool, par, B, self.PS, self.is_color, Hp, Lp)
        elif fdn:
            H.synth_dn_map(self.pool, par, B, self.PS, self.seed, self.step, Hp, Lp)
        elif ffd:
            Cp = torch.empty(B, 1, 1, 1, device=dev)
            H.synth_dn_level(self.pool, par, B, self.PS, self.seed, self.step, Hp, Lp, Cp)
        elif self.task == "sr":
            H.synth_sr(self.pool, par, B, self.PS, self.sf, self.taps_h, self.taps_w, Hp, Lp)
        else:
            H.synth_dn(self.pool, par, B, self.PS, self.sigma, self.seed, self.step, Hp, Lp)
        self.step += 1
        self.last_params = par
        return (Lp, Hp, Cp) if ffd else (Lp, Hp)

    def _draw_fdncnn(self, B):
        """Host draws of the next FDnCNN / DRUNet / FFDNet batch: [B, 5] int32 {image, rnd_h, rnd_w, mode, bits of sigma / 255}."""
        ints = torch.zeros(B, 5, dtype=torch.int32)
        lev = torch.zeros(B, 1, dtype=torch.float32)
        for b in range(B):
            img = self._next_index()
            rh = self.rng.randint(0, self.Hs - self.PS)
            rw = self.rng.randint(0, self.Ws - self.PS)
            mode = self.rng.randint(0, 7)
            lev[b, 0] = self.rng.uniform(*self.sigma_range) / 255.0
            ints[b, :4] = torch.tensor([img, rh, rw, mode], dtype=torch.int32)
        ints[:, 4:] = lev.view(torch.int32)
        return ints

    def _draw_jpeg(self, B):
        """Host draws of the next JPEG batch: [B, 8] int32 {image, rnd_h, rnd_w, mode, gray_mode, quality, rh2, rw2}."""
        rows = []
        for _ in range(B):
            img = self._next_index()
            rh = self.rng.randint(0, max(0, self.Hs - self.PS - 8))
            rw = self.rng.randint(0, max(0, self.Ws - self.PS - 8))
            mode = self.rng.randint(0, 7)
            gray_mode = 0
            if not self.is_color:
                gray_mode = 0 if self.rng.random() > 0.5 else 1
            q = self.rng.choice(self.qualities) if self.q_drawn else self.qualities[0]
            rh2 = rw2 = 0
            if self.rng.random() > 0.5:
                rh2, rw2 = self.rng.randint(0, 8), self.rng.randint(0, 8)
            rows.append((img, rh, rw, mode, gray_mode, q, rh2, rw2))
        return torch.tensor(rows, dtype=torch.int32)

    def _draw_usr(self, B):
        """Host draws of the next USRNet batch: (sf, [B, 12] int32 table; see the module docstring)."""
        sf = self.rng.choice(self.scales)
        ints = torch.zeros(B, 12, dtype=torch.int32)
        flts = torch.zeros(B, 4, dtype=torch.float32)
        K = 0 if self.bank is None else self.bank.shape[0]
        for b in range(B):
            img = self._next_index()
            rh = self.rng.randint(0, self.Hs - self.PS)
            rw = self.rng.randint(0, self.Ws - self.PS)
            mode = self.rng.randint(0, 7)
            row = [img, rh, rw, mode, 0, 0, 1, 0]
            if self.rng.randint(0, 7) > 3 and K:
                row[4], row[5] = 1, self.rng.randint(0, K - 1)
            else:
                flts[b, 0] = self.rng.uniform(0.6, 12.0)
                flts[b, 1] = self.rng.uniform(0.6, 12.0)
                flts[b, 2] = self.rng.uniform(0.0, math.pi)
                row[6] = self.rng.choice([1, 2, 3, 4])
                row[7] = self.rng.randint(0, 7)
            if self.rng.randint(0, 7) != 1:
                flts[b, 3] = self.rng.randint(0, self.sigma_max - 1) / 255.0
            ints[b, :8] = torch.tensor(row, dtype=torch.int32)
        ints[:, 8:] = flts.view(torch.int32)
        return sf, ints

    def _next_usr(self, B):
        dev = self.pool.device
        sf, host = self._draw_usr(B)
        if self._par_host is None or self._par_host.shape[0] < B:
            self._par_host = torch.empty(B, 12, dtype=torch.int32).pin_memory()
            self._par_ev = None
        if self._par_ev is not None:
            self._par_ev.synchronize()   # the previous batch's copy has read the staging buffer
        self._par_host[:B].copy_(host)
        par = self._par_host[:B].to(dev, non_blocking=True)
        self._par_ev = torch.cuda.Event()
        self._par_ev.record()
        fl = par[:, 8:].view(torch.float32)
        k = torch.empty(B, 1, self.ks, self.ks, device=dev)
        Hp = torch.empty(B, self.C, self.PS, self.PS, device=dev)
        Lp = torch.empty(B, self.C, self.PS // sf, self.PS // sf, device=dev)
        H.usr_gauss_kernels(fl, par[:, 4:8], self.bank, k)
        H.synth_usr(self.pool, par, B, self.PS, sf, k, fl[:, 3], self.trunc8, self.seed, self.step, Hp, Lp)
        self.step += 1
        self.last_params = par
        return Lp, Hp, k, sf, fl[:, 3].reshape(B, 1, 1, 1).contiguous()

    def _draw_blindsr(self, B):
        """Host draws of the next blind-SR batch: the [B, 136] int32 program table (module docstring)."""
        tab = torch.zeros(B, BSR_COLS, dtype=torch.int32)
        for b in range(B):
            img = self._next_index()
            rh = self.rng.randint(0, self.Hs - self.PS)
            rw = self.rng.randint(0, self.Ws - self.PS)
            mode = self.rng.randint(0, 7)
            prog, lh, lw = blindsr.draw_bsrgan(self.rng, self.PS, self.bsr_sf, self.lq, self._noise_off)
            tab[b, :6] = torch.tensor([img, rh, rw, mode, lh, lw], dtype=torch.int32)
            tab[b, 8:] = torch.from_numpy(prog.reshape(-1))
        return tab

    def _next_blindsr(self, B):
        dev = self.pool.device
        host = self._draw_blindsr(B)
        if self._par_host is None or self._par_host.shape[0] < B:
            self._par_host = torch.empty(B, BSR_COLS, dtype=torch.int32).pin_memory()
            self._par_ev = None
        if self._par_ev is not None:
            self._par_ev.synchronize()   # the previous batch's copy has read the staging buffer
        self._par_host[:B].copy_(host)
        par = self._par_host[:B].to(dev, non_blocking=True)
        self._par_ev = torch.cuda.Event()
        self._par_ev.record()
        PS, S, W = self.PS, blindsr.NSLOT, blindsr.NCOL
        if self._bsr_ws is None or self._bsr_ws[0] != B:
            self._bsr_ws = (B, torch.empty(B, 3, PS, PS, device=dev), torch.empty(B, 3, PS, PS, device=dev),
                            torch.empty(S, B, 25, 25, device=dev), H.jpeg_var_workspace(B, PS, PS, dev))
        _, a, b, kern, jws = self._bsr_ws
        slot = lambda s: par[:, 8 + W * s:8 + W * (s + 1)]   # noqa: E731
        stages = []

        def keep(buf, hw_cols):
            if self.debug_stages:
                stages.append((buf.clone(), [tuple(r) for r in host[:, hw_cols[0]:hw_cols[1]].tolist()]))

        w_min = PS // 8
        H.bsr_crop(self.pool, par, B, PS, a)
        keep(a, (8 + 1, 8 + 3))
        H.bsr_kernels(par[:, 8:], S, W, kern)
        for s in range(S - 1):   # slot 0 the pre-downscale, 1-6 the drawn ops; a <-> b
            H.bsr_ops(a, b, slot(s), kern[s], self.taps_half if s == 0 else None, self.seed, self.step, s)
            if s:
                H.jpeg_roundtrip_var(b, slot(s)[:, 3:5], w_min, slot(s)[:, 7], b, jws)
            a, b = b, a
            keep(a, (8 + W * s + 3, 8 + W * s + 5))
        s = S - 1   # the final JPEG, in place
        H.jpeg_roundtrip_var(a, slot(s)[:, 3:5], w_min, slot(s)[:, 7], a, jws)
        keep(a, (8 + W * s + 3, 8 + W * s + 5))
        Lp = torch.empty(B, 3, self.lq, self.lq, device=dev)
        Hp = torch.empty(B, 3, self.lq * self.bsr_sf, self.lq * self.bsr_sf, device=dev)
        H.bsr_finish(self.pool, par, B, PS, self.bsr_sf, self.lq, a, Lp, Hp)
        self.step += 1
        self.last_params = par
        return (Lp, Hp, stages) if self.debug_stages else (Lp, Hp)

    def next_dict(self, B):
        """The next USRNet batch as the dict ModelPlain4.feed_data reads (sf an int64 tensor [B]); task "fdncnn": the
        {"L", "H"} dict ModelPlain.feed_data reads; task "ffdnet": {"L", "H", "C"} for ModelPlain2.feed_data."""
        if self.task == "ffdnet":
            L, Hh, C = self.next(B)
            return {"L": L, "H": Hh, "C": C}
        if self.task == "fdncnn":
            L, Hh = self.next(B)
            return {"L": L, "H": Hh}
        if self.task != "usrnet":
            raise ValueError("PatchSynth.next_dict: tasks 'usrnet', 'fdncnn' and 'ffdnet' only")
        L, Hh, k, sf, sigma = self._next_usr(B)
        return {"L": L, "H": Hh, "k": k, "sf": torch.full((B,), sf, dtype=torch.int64), "sigma": sigma}


def synthetic_pool(N, C, Hs, Ws, seed=0, device="cuda"):
    """Seeded natural-ish images for the pool when no dataset is on the box (SURVEY §8d recipe:
    bicubic-upsampled uniform noise + 0.02 N, clamped to [0, 1])."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(N, C, max(1, Hs // 8), max(1, Ws // 8), generator=g)
    img = torch.nn.functional.interpolate(base, size=(Hs, Ws), mode="bicubic", align_corners=False)
    img = (img + 0.02 * torch.randn(img.shape, generator=g)).clamp(0, 1)
    return img.to(device)
