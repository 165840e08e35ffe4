"""Blind-SR training data on the GPU (csrc/synth_blindsr.hip, kair_jpeg_roundtrip_var, PatchSynth(task="blindsr"))
against the host statement utils/utils_blindsr.py in float64.

Bars.  Blur: ksize^2 fp32 fmafs of inputs in [0, 1] with a kernel summing to 1 stay within ksize^2 2^-24 <= 3.7e-5 < 4e-5
of the exact sum (the derivation of tests/test_usrnet_data_gpu.py), with the kernel values read back from the device;
the kernels themselves within 1e-6 of the float64 formula (that file's bar for kair_usr_gauss_kernels).  Resize: 1e-4
absolute; coordinates are fp64 on the device, so what is left is the fp32 rounding of at most 10 x 10 weights and
fmafs on data in [0, 1], < 2e-5 (measured maximum on the MI355X: see test_resize).  JPEG: equal integers.  Noise: statistics."""
import math
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.utils import utils_blindsr as bsr  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_jpeg as jpg  # noqa: E402

dev = torch.device("cuda")
TOL_BLUR, TOL_KERNEL, TOL_RESIZE = 4e-5, 1e-6, 1e-4
SENTINEL = -7.0


def row_of(op, h_in, w_in, h_out, w_out, i0=0, i1=0, q=0, f=()):
    row = np.zeros(16, np.int32)
    row[:8] = (op, h_in, w_in, h_out, w_out, i0, i1, q)
    row.view(np.float32)[8:8 + len(f)] = f
    return row


def natural(h, w, seed):
    """smooth + noise, HWC float32 in [0, 1]"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([0.5 + 0.35 * np.sin(x / (3.0 + c) + seed) * np.cos(y / (4.0 + c)) for c in range(3)], -1)
    return np.clip(img + g.normal(0, 0.08, img.shape), 0, 1).astype(np.float32)


def pack(imgs, Hmax, Wmax):
    buf = torch.full((len(imgs), 3, Hmax, Wmax), 0.25)
    for b, im in enumerate(imgs):
        buf[b, :, :im.shape[0], :im.shape[1]] = torch.from_numpy(im).permute(2, 0, 1)
    return buf.to(dev)


def run_ops(imgs, rows, Hmax, Wmax, kmax=25, taps=None, direct=False, seed=0, step=0, slot=0):
    """One kair_bsr_ops launch: (outputs HWC float64 per sample, kernels [B, kmax, kmax] cpu, raw output buffer)."""
    B = len(imgs)
    src = pack(imgs, Hmax, Wmax)
    dst = torch.full_like(src, SENTINEL)
    tab = torch.from_numpy(np.stack(rows)).to(dev)
    k = torch.zeros(1, B, kmax, kmax, device=dev)
    H.bsr_kernels(tab, 1, 16, k)
    H.bsr_ops(src, dst, tab, k[0], taps, seed, step, slot, direct)
    torch.cuda.synchronize()
    out = dst.cpu()
    res = []
    for b, r in enumerate(rows):
        ho, wo = int(r[3]), int(r[4])
        res.append(out[b, :, :ho, :wo].permute(1, 2, 0).double().numpy())
        rest = out[b].clone()
        rest[:, :ho, :wo] = SENTINEL
        assert float(rest.min()) == float(rest.max()) == SENTINEL, b   # nothing outside (h_out, w_out) is written
    return res, k[0].cpu(), out


def kernel_of(k, b, ks):
    return k[b].flatten()[:ks * ks].reshape(ks, ks).double().numpy()


# ---- 1. blur ------------------------------------------------------------------------------------------------------
BLUR_CASES = [((24, 24), 7, (3.1, 0.4, 0.7)), ((37, 29), 13, (2.2, 2.2, 0.0)), ((72, 56), 25, (7.5, 1.3, 2.4)),
              ((9, 11), 25, (5.0, 5.0, 0.0)), ((37, 29), 25, (0.01, 6.0, 1.1)), ((72, 56), 7, (0.5, 0.5, 0.0))]


def test_blur_batch_of_mixed_sizes_lds_and_fallback():
    """Different (h, w) and ksize per sample in one launch; (9, 11) with ksize 25 folds the mirror index more than once."""
    imgs = [natural(h, w, 10 + i) for i, ((h, w), _, _) in enumerate(BLUR_CASES)]
    rows = [row_of(bsr.OP_BLUR, h, w, h, w, ks, f=f) for (h, w), ks, f in BLUR_CASES]
    got, k, raw = run_ops(imgs, rows, 72, 56)
    got_d, _, raw_d = run_ops(imgs, rows, 72, 56, direct=True)
    assert torch.equal(raw, raw_d)   # the one-thread-per-output fallback: the same fmaf chain
    for b, ((h, w), ks, f) in enumerate(BLUR_CASES):
        kd = kernel_of(k, b, ks)
        fl = rows[b].view(np.float32)
        kerr = np.abs(kd - bsr.gauss_kernel(ks, float(fl[8]), float(fl[9]), float(fl[10]))).max()
        want = np.stack([ndimage.convolve(imgs[b][..., c].astype(np.float64), kd, mode="mirror") for c in range(3)], -1)
        err = np.abs(got[b] - np.clip(want, 0, 1)).max()
        print(f"blur {h}x{w} ks {ks}: kernel err {kerr:.2e}, max err {err:.2e}")
        assert kerr < TOL_KERNEL and abs(kd.sum() - 1) < 1e-6
        assert err < TOL_BLUR
        assert np.abs(got[b] - bsr.apply_op(imgs[b], rows[b], kernel=kd)).max() < TOL_BLUR


def test_blur_ksize_above_the_lds_tile_takes_the_fallback():
    """ksize 31 > 25 does not fit the static LDS tile: the same launch runs it on the global-memory loop.  Bar, derived
    as above: 31^2 2^-24 = 5.8e-5."""
    imgs = [natural(40, 33, 3), natural(20, 70, 4)]
    rows = [row_of(bsr.OP_BLUR, 40, 33, 40, 33, 31, f=(9.0, 2.0, 0.3)), row_of(bsr.OP_BLUR, 20, 70, 20, 70, 9, f=(1.0, 3.0, 2.0))]
    got, k, _ = run_ops(imgs, rows, 40, 70, kmax=31)
    for b, ks in enumerate([31, 9]):
        kd = kernel_of(k, b, ks)
        assert np.abs(got[b] - bsr.apply_op(imgs[b], rows[b], kernel=kd)).max() < ks * ks * 2.0 ** -24 + 1e-9


@pytest.mark.parametrize("sf_w", [2, 4])
def test_blur_decimate(sf_w):
    imgs = [natural(48, 40, 20 + sf_w), natural(31, 23, 30 + sf_w)]
    rows = [row_of(bsr.OP_BLURDEC, h, w, -(-h // sf_w), -(-w // sf_w), 25, sf_w, f=(s * s, s * s, 0.0))
            for (h, w), s in zip([(48, 40), (31, 23)], [0.6 * sf_w, 0.35])]
    got, k, _ = run_ops(imgs, rows, 48, 40)
    for b in range(2):
        kd = kernel_of(k, b, 25)
        fl = rows[b].view(np.float32)
        assert np.abs(kd - bsr.gauss_kernel(25, float(fl[8]), float(fl[9]), 0.0, sf_w)).max() < TOL_KERNEL
        full = np.stack([ndimage.convolve(imgs[b][..., c].astype(np.float64), kd, mode="mirror") for c in range(3)], -1)
        err = np.abs(got[b] - full[0::sf_w, 0::sf_w]).max()
        print(f"blur + decimate sf_w {sf_w} sample {b}: max err {err:.2e}")
        assert err < TOL_BLUR


# ---- 2. resize ----------------------------------------------------------------------------------------------------
def test_resize():
    """Kinds 1, 2, 3 from (40, 56) to (10, 14), (17, 23), (39, 55) and, growing, (53, 61), with two samples of other
    input sizes mixed into the same launch; the MATLAB kind at its x1/2, (20, 28), with the uploaded taps.
    Measured maximum on the MI355X: 1.5e-7, and 1.7e-7 over the pipeline test's resize slots (below 2e-5)."""
    outs = [(10, 14), (17, 23), (39, 55), (53, 61)]
    cases = [((40, 56), o, k) for k in (1, 2, 3) for o in outs] + [((24, 31), (11, 9), 2), ((13, 17), (53, 61), 3),
                                                                    ((24, 31), (24, 31), 1)]
    imgs = [natural(i[0], i[1], 40 + n) for n, (i, _, _) in enumerate(cases)]
    rows = [row_of(bsr.OP_RESIZE, i[0], i[1], o[0], o[1], k) for i, o, k in cases]
    got, _, _ = run_ops(imgs, rows, 53, 61)
    worst = 0.0
    for b, (i, o, kind) in enumerate(cases):
        err = np.abs(got[b] - bsr.apply_op(imgs[b], rows[b])).max()
        worst = max(worst, err)
        print(f"resize kind {kind} {i} -> {o}: max err {err:.2e}")
        assert err < TOL_RESIZE
    assert np.array_equal(got[-1], imgs[-1].astype(np.float64))   # bilinear at the same size is the identity
    ih, wh = util.bicubic_taps(40, 20, 0.5)
    iw, ww = util.bicubic_taps(56, 28, 0.5)
    taps = (ih.to(dev), wh.to(dev), iw.to(dev), ww.to(dev), 40, 56)
    img = natural(40, 56, 60)
    row = row_of(bsr.OP_RESIZE, 40, 56, 20, 28, bsr.KIND_MATLAB_HALF)
    got, _, _ = run_ops([img, img], [row, row], 40, 56, taps=taps)
    want = bsr.apply_op(img, row)
    err = np.abs(got[1] - want).max()
    print(f"resize MATLAB x1/2: max err {err:.2e}; worst of the others {worst:.2e}")
    assert err < TOL_RESIZE
    ref = util.imresize(torch.from_numpy(img).permute(2, 0, 1), 0.5, True).permute(1, 2, 0).clamp(0, 1).numpy()
    assert np.abs(want - ref).max() < 1e-5   # the host statement is utils_image.imresize


# ---- 3. noise -----------------------------------------------------------------------------------------------------
def noise_run(mode, f, seed=3, step=5, slot=2):
    imgs = [np.full((64, 64, 3), 0.5, np.float32)] * 8
    rows = [row_of(bsr.OP_NOISE, 64, 64, 64, 64, mode, f=f)] * 8
    got, _, raw = run_ops(imgs, rows, 64, 64, seed=seed, step=step, slot=slot)
    return np.stack(got) - 0.5, raw   # [8, 64, 64, 3]


def test_noise_modes():
    s = 25 / 255
    res, raw = noise_run(bsr.NOISE_GRAY, (s,))
    assert np.array_equal(res[..., 0], res[..., 1]) and np.array_equal(res[..., 0], res[..., 2])
    assert abs(res[..., 0].std() / s - 1) < 0.03
    res, raw_c = noise_run(bsr.NOISE_COLOR, (s,))
    flat = res.reshape(-1, 3)
    assert flat.shape[0] == 32768
    for c in range(3):
        assert abs(flat[:, c].std() / s - 1) < 0.03, c
    cc = np.corrcoef(flat.T)
    print("colour noise: std / sigma", (flat.std(0) / s).round(4), "corr", cc[0, 1].round(4), cc[0, 2].round(4), cc[1, 2].round(4))
    assert max(abs(cc[0, 1]), abs(cc[0, 2]), abs(cc[1, 2])) < 0.03
    # two steps differ, two slots differ, the same (seed, step, slot) repeats
    assert torch.equal(noise_run(bsr.NOISE_COLOR, (s,))[1], raw_c)
    assert not torch.equal(noise_run(bsr.NOISE_COLOR, (s,), step=6)[1], raw_c)
    assert not torch.equal(noise_run(bsr.NOISE_COLOR, (s,), slot=3)[1], raw_c)
    assert not torch.equal(noise_run(bsr.NOISE_COLOR, (s,), seed=4)[1], raw_c)


def test_noise_correlated():
    rng = random.Random(8)
    D = np.diag([rng.random() for _ in range(3)])
    U = np.linalg.qr(np.array([[rng.random() for _ in range(3)] for _ in range(3)]))[0]
    L = bsr.psd_cholesky(np.abs((25 / 255) ** 2 * (U.T @ D @ U)))
    f = (0.0, L[0, 0], L[1, 0], L[1, 1], L[2, 0], L[2, 1], L[2, 2])
    Lf = np.zeros((3, 3))
    Lf[np.tril_indices(3)] = np.array(f[1:], np.float32)
    cov = Lf @ Lf.T   # the uploaded one
    bar = 0.05 * (25 / 255) ** 2
    # the bar holds for the statistic itself at this N: numpy normals through the same factor
    ref = np.random.default_rng(0).standard_normal((32768, 3)) @ Lf.T
    assert np.abs(np.cov(ref.T) - cov).max() < bar
    res, _ = noise_run(bsr.NOISE_CORR, f)
    got = np.cov(res.reshape(-1, 3).T)
    print("correlated noise: cov error / (25/255)^2", (np.abs(got - cov) / (25 / 255) ** 2).max().round(4))
    assert np.abs(got - cov).max() < bar
    assert abs(cov[0, 1]) > 2 * bar   # the case has a cross term to get wrong


# ---- 4. kair_jpeg_roundtrip_var -------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
def test_jpeg_roundtrip_var(in_place):
    sizes, qs = [(16, 16), (13, 21), (40, 56)], [30, 95, 0]
    g = np.random.default_rng(5)
    imgs = [natural(40, 56, 70), g.random((40, 56, 3)).astype(np.float32), natural(40, 56, 72)]   # whole buffers
    x = pack(imgs, 40, 56)
    out = x if in_place else torch.full_like(x, SENTINEL)
    keep = x.clone()
    hw = torch.tensor(sizes, dtype=torch.int32, device=dev)
    H.jpeg_roundtrip_var(x, hw, 13, torch.tensor(qs, dtype=torch.int32, device=dev), out)
    torch.cuda.synchronize()
    o, keep = out.cpu(), keep.cpu()
    for b, ((h, w), q) in enumerate(zip(sizes, qs)):
        rest = o[b].clone()
        rest[:, :h, :w] = keep[b][:, :h, :w] if in_place else SENTINEL
        assert torch.equal(rest, keep[b] if in_place else torch.full_like(rest, SENTINEL)), b   # outside (h, w): untouched
        got = o[b, :, :h, :w]
        if q == 0:
            assert torch.equal(got, keep[b, :, :h, :w])
            continue
        u = np.rint(np.float32(255) * imgs[b][:h, :w]).astype(np.uint8)
        want = torch.from_numpy(jpg.jpeg_roundtrip_np(u, q)).permute(2, 0, 1).to(torch.int32)
        gi = (got.double() * 255).round().to(torch.int32)
        assert torch.equal(gi, want), (b, int((gi != want).sum()))
        assert float((got.double() - want.double() / 255).abs().max()) <= 1e-7
    with pytest.raises(RuntimeError, match="width"):
        H.jpeg_roundtrip_var(x, hw, 4, torch.tensor(qs, dtype=torch.int32, device=dev), out)


# ---- 5. the pipeline, teacher-forced ------------------------------------------------------------------------------
def host_tables(seed, scale, steps, lq, B=8, Hs=80, Ws=72, PS=64):
    """The tables PatchSynth will draw (its image order comes from another generator)."""
    rng = random.Random(seed)
    out = []
    for _ in range(steps * B):
        rng.randint(0, Hs - PS), rng.randint(0, Ws - PS), rng.randint(0, 7)
        out.append(bsr.draw_bsrgan(rng, PS, scale, lq)[0])
    return out


def aug_crop(pool, img, rh, rw, mode, PS):
    return util.augment_img_tensor4(pool[img:img + 1, :, rh:rh + PS, rw:rw + PS], mode)[0]


@pytest.mark.parametrize("scale,seed", [(4, 0), (2, 0)])
def test_pipeline_stagewise(scale, seed):
    """Every slot of every sample: the host apply_op on the GPU's slot input against the GPU's slot output, so a one-ulp
    difference before a rint cannot cascade.  JPEG slots are compared as integers, noise slots by their residual's std."""
    PS, lq, B, steps = 64, 16, 8, 3
    progs = host_tables(seed, scale, steps, lq)
    ops = {int(p[s, 0]) for p in progs for s in range(8)}
    assert ops == set(range(6)), ops
    assert {int(p[0, 0]) for p in progs} == ({bsr.OP_COPY, bsr.OP_RESIZE} if scale == 4 else {bsr.OP_COPY})
    assert any(bsr.OP_COPY in p[1:7, 0] for p in progs)   # a skipped JPEG
    assert {int(p[s, 5]) for p in progs for s in range(1, 7) if p[s, 0] == bsr.OP_NOISE} == {0, 1, 2}
    pool = synthetic_pool(6, 3, 80, 72, seed=3)
    cpu_pool = pool.cpu()
    a = PatchSynth(pool, task="blindsr", H_size=PS, lq_patchsize=lq, scale=scale, seed=seed, debug_stages=True)
    p = PatchSynth(pool, task="blindsr", H_size=PS, lq_patchsize=lq, scale=scale, seed=seed)
    z, nz, worst = [], 0, {"blur": 0.0, "resize": 0.0}
    for step in range(steps):
        L, Hh, stages = a.next(B)
        L2, H2 = p.next(B)
        torch.cuda.synchronize()
        assert torch.equal(L, L2) and torch.equal(Hh, H2)
        assert L.shape == (B, 3, lq, lq) and Hh.shape == (B, 3, lq * scale, lq * scale) and len(stages) == 9
        par = a.last_params.cpu()
        assert par.shape == (B, 136) and par.dtype == torch.int32
        kern = a._bsr_ws[3].cpu()
        for b in range(B):
            prog = par[b, 8:].reshape(8, 16).numpy()
            assert np.array_equal(prog, progs[step * B + b])
            img, rh, rw, mode, lh, lw = par[b, :6].tolist()
            patch = aug_crop(cpu_pool, img, rh, rw, mode, PS)
            assert torch.equal(stages[0][0][b].cpu(), patch) and stages[0][1][b] == (PS, PS)
            assert torch.equal(Hh[b].cpu(), patch[:, lh * scale:(lh + lq) * scale, lw * scale:(lw + lq) * scale])
            for s in range(8):
                row = prog[s]
                op, hi, wi, ho, wo, i0 = (int(v) for v in row[:6])
                assert stages[s][1][b] == (hi, wi) and stages[s + 1][1][b] == (ho, wo)
                x = stages[s][0][b, :, :hi, :wi].permute(1, 2, 0).cpu().numpy()
                y = stages[s + 1][0][b, :, :ho, :wo].permute(1, 2, 0).cpu().numpy()
                assert y.min() >= 0.0 and y.max() <= 1.0
                if op == bsr.OP_COPY:
                    assert np.array_equal(x, y)
                elif op == bsr.OP_JPEG:
                    want = bsr.apply_op(x, row, np.float32)
                    assert np.array_equal(np.rint(255 * y.astype(np.float64)), np.rint(255 * want.astype(np.float64))), (step, b, s)
                elif op == bsr.OP_NOISE:
                    fl = row.view(np.float32)
                    sd = float(fl[8]) if i0 != bsr.NOISE_CORR else float(fl[9])
                    r = (y.astype(np.float64) - x)[..., 0]
                    assert np.abs(r).max() > 0
                    if i0 == bsr.NOISE_GRAY:   # one field on all three channels (where nothing was clipped)
                        inner = (y > 0).all(-1) & (y < 1).all(-1)
                        d = y.astype(np.float64) - x
                        assert np.abs(d[inner][:, 0:1] - d[inner]).max() < 1e-6
                    keep = (x[..., 0] > 4.5 * sd) & (x[..., 0] < 1 - 4.5 * sd)   # no clipping there
                    if sd > 0:
                        z.append(r[keep] / sd)
                        nz += 1
                else:
                    kd = None
                    if op in (bsr.OP_BLUR, bsr.OP_BLURDEC):
                        kd = kernel_of(kern[s], b, i0)
                        fl = row.view(np.float32)
                        assert np.abs(kd - bsr.gauss_kernel(i0, float(fl[8]), float(fl[9]), float(fl[10]),
                                                            int(row[6]) if op == bsr.OP_BLURDEC else 1)).max() < TOL_KERNEL
                    err = np.abs(y - bsr.apply_op(x, row, kernel=kd)).max()
                    name = "resize" if op == bsr.OP_RESIZE else "blur"
                    worst[name] = max(worst[name], err)
                    assert err < (TOL_RESIZE if op == bsr.OP_RESIZE else TOL_BLUR), (step, b, s, op, err)
            assert torch.equal(L[b].cpu(), stages[8][0][b, :, lh:lh + lq, lw:lw + lq].cpu())
    # the noise residuals, pooled (channel 0 only, so the gray mode counts once): N(0, 1) within 5 standard errors
    z = np.concatenate(z)
    print(f"scale {scale}: worst blur {worst['blur']:.2e} resize {worst['resize']:.2e}; {nz} noise slots, "
          f"{z.size} residuals, std {z.std():.4f}")
    assert nz == steps * B and z.size >= 500
    assert abs(z.std() - 1) < 5 / math.sqrt(2 * z.size)


# ---- 6. the loader and the synth take the same decisions -----------------------------------------------------------
def test_synth_matches_dataset(tmp_path):
    """Noise levels forced to zero on both sides; the loader runs the chain in float32 numpy, the synth on the device.
    They agree to 2/255 on >= 99 % of the pixels: the rest are rint flips before a JPEG step spreading through an 8 x 8
    block (the two host chains, float32 against float64, differ on 0 of 18432 pixels in tests/test_blindsr_cpu.py).
    Observed on the MI355X: 0 of 12288 pixels beyond 2/255."""
    from kair_amd.data.select_dataset import define_Dataset
    g = torch.Generator().manual_seed(4)
    base = torch.rand(6, 3, 10, 9, generator=g)
    u8 = (torch.nn.functional.interpolate(base, size=(80, 72), mode="bicubic", align_corners=False)
          + 0.03 * torch.randn(6, 3, 80, 72, generator=g)).clamp(0, 1).mul(255).round().to(torch.uint8)
    for n in range(6):
        util.imsave(u8[n].permute(1, 2, 0).numpy(), str(tmp_path / f"im{n}.png"))
    pool = (u8.float() / 255.0).to(dev)
    ds = define_Dataset({"dataset_type": "blindsr", "phase": "train", "dataroot_H": str(tmp_path), "H_size": 64,
                         "lq_patchsize": 16, "scale": 4, "n_channels": 3})
    s = PatchSynth(pool, task="blindsr", H_size=64, lq_patchsize=16, scale=4, seed=9)
    ds.rng = random.Random(9)
    ds._noise_off = s._noise_off = True
    bad = tot = 0
    for _ in range(2):
        L, Hh = s.next(8)
        torch.cuda.synchronize()
        for b, img in enumerate(s.last_params[:, 0].tolist()):
            item = ds[img]   # the same generator state: the same crop, mode and program
            assert torch.equal(item["H"], Hh[b].cpu())
            d = (item["L"] - L[b].cpu()).abs()
            bad += int((d > 2 / 255).sum())
            tot += d.numel()
    print(f"loader vs synth: {bad} of {tot} pixels differ by more than 2/255")
    assert bad <= 0.01 * tot


# ---- 7. arguments and one training step -----------------------------------------------------------------------------
def test_refused_arguments():
    pool = synthetic_pool(2, 3, 80, 72, seed=1)
    with pytest.raises(ValueError):
        PatchSynth(pool, task="blindsr", H_size=66, lq_patchsize=16, scale=4)    # H_size % sf
    with pytest.raises(ValueError):
        PatchSynth(pool, task="blindsr", H_size=64, lq_patchsize=17, scale=4)    # lq sf > H_size
    with pytest.raises(ValueError):
        PatchSynth(pool, task="blindsr", H_size=76, lq_patchsize=16, scale=4)    # pool smaller than H_size
    with pytest.raises(ValueError):
        PatchSynth(pool[:, :1].contiguous(), task="blindsr", H_size=64, lq_patchsize=16, scale=4)
    with pytest.raises(ValueError):
        PatchSynth(pool, task="blindsr", H_size=63, lq_patchsize=16, scale=3)
    buf = torch.zeros(2, 3, 16, 16, device=dev)
    tab = torch.zeros(2, 16, dtype=torch.int32, device=dev)
    k = torch.zeros(2, 25, 25, device=dev)
    with pytest.raises(ValueError):
        H.bsr_ops(buf, buf, tab, k)                      # in place
    with pytest.raises(RuntimeError, match="slot"):
        H.bsr_ops(buf, buf.clone(), tab, k, slot=8)
    with pytest.raises(RuntimeError, match="3-channel"):
        H.check(H.lib().kair_bsr_crop(H.ptr(buf), 2, 1, 16, 16, H.ptr(tab), 16, 2, 16, H.ptr(buf), H.stream_ptr()), "bsr_crop")


def test_patchsynth_blindsr_feeds_modelplain(tmp_path):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 4, "n_channels": 3,
           "path": {"models": str(tmp_path)},
           "netG": {"net_type": "rrdbnet", "in_nc": 3, "out_nc": 3, "nf": 16, "nb": 1, "gc": 8, "scale": 4,
                    "init_type": "default"},
           "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                     "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                     "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                     "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True}}
    torch.manual_seed(0)
    model = define_Model(dict_to_nonedict(opt))
    model.init_train()
    s = PatchSynth(synthetic_pool(4, 3, 72, 80, seed=2), task="blindsr", H_size=64, lq_patchsize=16, scale=4, seed=6)
    before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    for step in range(2):
        L, Hh = s.next(2)
        assert L.shape == (2, 3, 16, 16) and Hh.shape == (2, 3, 64, 64)
        model.feed_data({"L": L, "H": Hh})
        model.optimize_parameters(step)
        loss = model.log_dict["G_loss"]
        assert np.isfinite(loss) and loss > 0
    after = model.netG.state_dict()
    assert any((after[k] - before[k]).abs().max() > 0 for k in before)
