"""The BSRGAN blind-SR degradation (the reference's utils_blindsr.degradation_bsrgan) as a drawn program and a
per-op executor.  This file is the readable statement of the pipeline and the reference of the tests; the device
form is csrc/synth_blindsr.hip (kair_bsr_ops, kair_jpeg_roundtrip_var), driven by the same draws.

    prog, rnd_h, rnd_w = draw_bsrgan(rng, H_size, sf, lq_patchsize)   # every random decision, no pixels
    for row in prog: img = apply_op(img, row)                          # float64 (or float32) numpy, HWC in [0, 1]
    L = img[rnd_h:rnd_h + lq, rnd_w:rnd_w + lq]                        # H: the crop at (rnd_h sf, rnd_w sf), lq sf wide

The program is an int32 table [NSLOT = 8, NCOL = 16]; the last 8 columns hold float32 bits (`prog.view(np.float32)`):

    col 0     op: 0 copy (slot unused or draw not taken), 1 blur, 2 resize, 3 blur + decimate, 4 noise, 5 JPEG
    col 1-4   h_in, w_in, h_out, w_out
    col 5, 6  blur: ksize, -;  resize: kind (1 bilinear, 2 bicubic, 3 area, 4 MATLAB bicubic x1/2), -;
              blur + decimate: 25, sf_w;  noise: mode (0 per channel, 1 gray, 2 correlated), host noise seed;
              JPEG: quality, -
    col 7     the quality again on a JPEG row, 0 on every other row (what kair_jpeg_roundtrip_var reads)
    col 8-15  blur, blur + decimate: lambda_1, lambda_2, theta;  noise: level / 255, then the lower Cholesky factor
              L00, L10, L11, L20, L21, L22 of the correlated mode's covariance

Slot 0 is the optional x1/2 pre-downscale, slots 1-6 the six ops in their drawn order (the camera-ISP op holds no
slot), slot 7 the final JPEG.  Every op is followed by a clip to [0, 1].

Draws, all from one random.Random (or the `random` module), in this order: [sf 4 only] random() < 0.25 takes the
pre-downscale, then random() < 0.5 ? choice([1, 2, 3]) : MATLAB x1/2; order = sample(range(7), 7) with 3 moved behind
2; per op in that order -- blur (0, 1): random() < 0.5 aniso ? (l1, l2 = (4 + sf_w) random() each, theta = pi random())
: (s = (2 + 0.2 sf_w) random(), l1 = l2 = s s), then ksize = 2 randint(2, 11) + 3; downsample2 (2): random() < 0.75 ?
(sf1 = uniform(1, 2 sf_w), kind = choice([1, 2, 3])) : s = uniform(0.1, 0.6 sf_w); downsample3 (3): kind =
choice([1, 2, 3]); noise (4): level = randint(2, 25), r = random(), [0.4 <= r <= 0.6: 3 random() for D, 9 for the
matrix whose QR basis is U], getrandbits(31) (the seed of the host's normals; the device has its own Philox);
JPEG (5): random() < 0.9 ? quality = randint(30, 95) : skipped; camera ISP (6): no draw -- then the final quality
randint(30, 95) and rnd_h, rnd_w = randint(0, h - lq) each.

Departures from the reference (as recalled; neither it nor OpenCV was at hand when this was written):
  * one random.Random makes every draw; the reference mixes `random` and `np.random`;
  * lambda_1, lambda_2 are floored at 0.01; the reference does not floor and meets a near-singular covariance;
  * the shifted kernel of downsample2's blur branch is the closed form with the centre moved by (sf_w - 1) / 2 pixels
    (gen_kernel's centre, sf_k = sf_w); the reference shifts an unshifted kernel by interpolating it;
  * the resizers are written out here (half-pixel centres, replicate borders, no antialias for bilinear / bicubic
    a = -0.75, exact footprint mean for area) and are not bit-equal to OpenCV's fixed-point ones; area uses the same
    footprint formula when the size grows, where OpenCV switches to a bilinear variant;
  * the correlated noise's covariance |(25 / 255)^2 U^T D U| (an elementwise absolute value, so not always positive
    semi-definite) has its negative eigenvalues clipped to 0 before the Cholesky factor is taken;
    np.random.multivariate_normal would use their absolute values;
  * U is the QR basis, not scipy.linalg.orth's SVD basis;
  * JPEG is utils_jpeg's libjpeg arithmetic on rint(255 clip(x)) in float32, RGB 4:2:0 (cv2.imencode's default);
  * the camera-ISP op is not built (the reference runs it only with an isp_model, which its option files do not
    give), and 'bsrgan_plus' is not built.
"""
import math

import numpy as np

from . import utils_image as util
from . import utils_jpeg as jpg
from . import utils_sisr as sisr

OP_COPY, OP_BLUR, OP_RESIZE, OP_BLURDEC, OP_NOISE, OP_JPEG = range(6)
KIND_BILINEAR, KIND_BICUBIC, KIND_AREA, KIND_MATLAB_HALF = 1, 2, 3, 4
NOISE_COLOR, NOISE_GRAY, NOISE_CORR = 0, 1, 2
NSLOT, NCOL = 8, 16
LAMBDA_FLOOR = 0.01


def check_sizes(H_size, sf, lq_patchsize):
    if sf not in (2, 4):
        raise ValueError(f"blindsr: scale must be 2 or 4 (got {sf})")
    if H_size <= 0 or H_size % sf:
        raise ValueError(f"blindsr: H_size {H_size} is not a positive multiple of the scale {sf}")
    if lq_patchsize < 1 or lq_patchsize * sf > H_size:
        raise ValueError(f"blindsr: lq_patchsize {lq_patchsize} x scale {sf} exceeds H_size {H_size}")


def psd_cholesky(C):
    """Lower factor L (L L^T = the nearest PSD matrix to the symmetric C in Frobenius norm); a zero pivot gives a
    zero column, so a singular C is fine."""
    lam, V = np.linalg.eigh(np.asarray(C, np.float64))
    A = (V * np.maximum(lam, 0.0)) @ V.T
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if d <= 1e-18:
            continue
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def draw_bsrgan(rng, H_size, sf, lq_patchsize, noise_off=False):
    """(prog int32 [8, 16], rnd_h, rnd_w): every random decision of one sample (module docstring).  noise_off (tests
    only) makes the same draws but writes zero noise levels."""
    check_sizes(H_size, sf, lq_patchsize)
    prog = np.zeros((NSLOT, NCOL), np.int32)
    fl = prog.view(np.float32)
    size = [H_size, H_size]   # h, w

    def put(s, op, ho, wo, i0=0, i1=0, q=0, f=()):
        prog[s, :8] = (op, size[0], size[1], ho, wo, i0, i1, q)
        fl[s, 8:8 + len(f)] = f
        size[0], size[1] = ho, wo

    sf_w = sf
    if sf == 4 and rng.random() < 0.25:
        kind = rng.choice([1, 2, 3]) if rng.random() < 0.5 else KIND_MATLAB_HALF
        put(0, OP_RESIZE, size[0] // 2, size[1] // 2, kind)
        sf_w = 2
    else:
        put(0, OP_COPY, size[0], size[1])
    order = rng.sample(range(7), 7)
    i2, i3 = order.index(2), order.index(3)
    if i3 < i2:
        order[i2], order[i3] = order[i3], order[i2]
    s = 1
    a = b = None
    for op in order:
        h, w = size
        if op in (0, 1):
            if rng.random() < 0.5:
                l1, l2 = (4 + sf_w) * rng.random(), (4 + sf_w) * rng.random()
                theta = math.pi * rng.random()
            else:
                sd = (2 + 0.2 * sf_w) * rng.random()
                l1 = l2 = sd * sd
                theta = 0.0
            ksize = 2 * rng.randint(2, 11) + 3
            put(s, OP_BLUR, h, w, ksize, f=(max(l1, LAMBDA_FLOOR), max(l2, LAMBDA_FLOOR), theta))
        elif op == 2:
            a, b = w, h
            if rng.random() < 0.75:
                sf1 = rng.uniform(1, 2 * sf_w)
                kind = rng.choice([1, 2, 3])
                put(s, OP_RESIZE, int(h / sf1), int(w / sf1), kind)
            else:
                sd = rng.uniform(0.1, 0.6 * sf_w)
                put(s, OP_BLURDEC, -(-h // sf_w), -(-w // sf_w), 25, sf_w, f=(sd * sd, sd * sd, 0.0))
        elif op == 3:
            put(s, OP_RESIZE, int(b / sf_w), int(a / sf_w), rng.choice([1, 2, 3]))
        elif op == 4:
            level = rng.randint(2, 25)
            r = rng.random()
            mode = NOISE_COLOR if r > 0.6 else NOISE_GRAY if r < 0.4 else NOISE_CORR
            chol = np.zeros((3, 3))
            if mode == NOISE_CORR:
                D = np.diag([rng.random() for _ in range(3)])
                U = np.linalg.qr(np.array([[rng.random() for _ in range(3)] for _ in range(3)]))[0]
                chol = psd_cholesky(np.abs((25.0 / 255.0) ** 2 * (U.T @ D @ U)))
            seed = rng.getrandbits(31)
            sigma = level / 255.0
            if noise_off:
                sigma, chol = 0.0, np.zeros((3, 3))
            put(s, OP_NOISE, h, w, mode, seed,
                f=(sigma, chol[0, 0], chol[1, 0], chol[1, 1], chol[2, 0], chol[2, 1], chol[2, 2]))
        elif op == 5:
            if rng.random() < 0.9:
                q = rng.randint(30, 95)
                put(s, OP_JPEG, h, w, q, q=q)
            else:
                put(s, OP_COPY, h, w)
        else:
            continue   # camera ISP: not built, no draw, no slot
        s += 1
    q = rng.randint(30, 95)
    put(7, OP_JPEG, size[0], size[1], q, q=q)
    rnd_h = rng.randint(0, size[0] - lq_patchsize)
    rnd_w = rng.randint(0, size[1] - lq_patchsize)
    return prog, rnd_h, rnd_w


def gauss_kernel(ksize, l1, l2, theta, sf_k=1):
    """float64 [ksize, ksize]: exp(-z^T Sigma^-1 z / 2) normalised over its support, Sigma = Q diag(l1, l2) Q^T, the
    centre at the centre tap moved by (sf_k - 1) / 2 pixels in x and y (utils_sisr.gen_kernel, ksize odd)."""
    return sisr.gen_kernel(ksize, l1, l2, theta, sf_k, 0).numpy()


def _keys(d, a=-0.75):
    d = abs(d)
    if d <= 1.0:
        return ((a + 2.0) * d - (a + 3.0)) * d * d + 1.0
    if d < 2.0:
        return ((a * d - 5.0 * a) * d + 8.0 * a) * d - 4.0 * a
    return 0.0


def resize_weights(n_in, n_out, kind):
    """float64 [n_out, n_in]: one axis of the resize as a matrix (half-pixel centres, replicate border)."""
    M = np.zeros((n_out, n_in))
    if kind == KIND_MATLAB_HALF:
        if n_out != -(-n_in // 2):
            raise ValueError("resize: the MATLAB kind is x1/2 only")
        idx, w = util.bicubic_taps(n_in, n_out, 0.5)
        for i in range(n_out):
            for y, v in zip(idx[i].tolist(), w[i].tolist()):
                M[i, y] += v
        return M
    s = n_in / n_out
    for i in range(n_out):
        if kind == KIND_AREA:
            lo, hi = i * s, (i + 1) * s
            for y in range(int(math.floor(lo)), min(int(math.ceil(hi)), n_in)):
                ov = min(hi, y + 1.0) - max(lo, float(y))
                if ov > 0:
                    M[i, y] += ov / s
            continue
        x = (i + 0.5) * s - 0.5
        x0 = int(math.floor(x))
        f = x - x0
        if kind == KIND_BILINEAR:
            taps = [(x0, 1.0 - f), (x0 + 1, f)]
        elif kind == KIND_BICUBIC:
            taps = [(x0 - 1, _keys(1.0 + f)), (x0, _keys(f)), (x0 + 1, _keys(1.0 - f)), (x0 + 2, _keys(2.0 - f))]
        else:
            raise ValueError(f"resize: unknown kind {kind}")
        for y, v in taps:
            M[i, min(max(y, 0), n_in - 1)] += v
    return M


def apply_op(img, row, dtype=np.float64, kernel=None):
    """One program row on img [h_in, w_in, 3] -> [h_out, w_out, 3], computed in `dtype` and clipped to [0, 1].
    kernel: the blur kernel to use instead of the row's Gaussian (tests pass the device's values)."""
    from scipy import ndimage
    row = np.ascontiguousarray(np.asarray(row, np.int32))
    fl = row.view(np.float32)
    op, h_in, w_in, h_out, w_out, i0, i1 = (int(v) for v in row[:7])
    img = np.asarray(img, dtype)
    if img.shape != (h_in, w_in, 3):
        raise ValueError(f"apply_op: the row expects {(h_in, w_in, 3)}, the image is {img.shape}")
    if op == OP_COPY:
        return img
    if op in (OP_BLUR, OP_BLURDEC):
        if kernel is None:
            kernel = gauss_kernel(i0, float(fl[8]), float(fl[9]), float(fl[10]), i1 if op == OP_BLURDEC else 1)
        k = np.asarray(kernel, dtype)
        out = ndimage.convolve(img, k[:, :, None], mode="mirror")
        if op == OP_BLURDEC:
            out = out[0::i1, 0::i1]
    elif op == OP_RESIZE:
        Wy = resize_weights(h_in, h_out, i0).astype(dtype)
        Wx = resize_weights(w_in, w_out, i0).astype(dtype)
        out = np.einsum("iy,yxc,jx->ijc", Wy, img, Wx)
    elif op == OP_NOISE:
        g = np.random.default_rng(i1)
        sigma = float(fl[8])
        if i0 == NOISE_COLOR:
            n = sigma * g.standard_normal((h_in, w_in, 3))
        elif i0 == NOISE_GRAY:
            n = np.repeat(sigma * g.standard_normal((h_in, w_in, 1)), 3, axis=2)
        else:
            L = np.zeros((3, 3))
            L[np.tril_indices(3)] = fl[9:15]
            n = g.standard_normal((h_in, w_in, 3)) @ L.T
        out = img + n.astype(dtype)
    elif op == OP_JPEG:
        u = np.rint(np.float32(255.0) * np.clip(img.astype(np.float32), 0, 1)).astype(np.uint8)
        out = (jpg.jpeg_roundtrip_np(u, i0).astype(np.float32) / np.float32(255.0)).astype(dtype)
    else:
        raise ValueError(f"apply_op: unknown op {op}")
    if out.shape != (h_out, w_out, 3):
        raise ValueError(f"apply_op: the row promises {(h_out, w_out, 3)}, the op gave {out.shape}")
    return np.clip(out, 0, 1).astype(dtype)


def degradation_bsrgan(img, sf=4, lq_patchsize=64, rng=None, dtype=np.float32, noise_off=False):
    """img [H_size, H_size, 3] in [0, 1] -> (L [lq, lq, 3], H [lq sf, lq sf, 3]) of `dtype`."""
    import random
    H_size = img.shape[0]
    if img.ndim != 3 or img.shape[1] != H_size or img.shape[2] != 3:
        raise ValueError("degradation_bsrgan: a square RGB image [H_size, H_size, 3]")
    prog, rnd_h, rnd_w = draw_bsrgan(rng or random, H_size, sf, lq_patchsize, noise_off)
    x = np.asarray(img, dtype)
    for row in prog:
        x = apply_op(x, row, dtype)
    lq = lq_patchsize
    L = x[rnd_h:rnd_h + lq, rnd_w:rnd_w + lq]
    Hh = np.asarray(img, dtype)[rnd_h * sf:(rnd_h + lq) * sf, rnd_w * sf:(rnd_w + lq) * sf]
    return L, Hh
