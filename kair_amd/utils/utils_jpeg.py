"""JPEG compression artifacts for the CAR (compression artifact reduction) data: the lossy part of a baseline JPEG
encode + decode, as libjpeg computes it (jfdctint / jidctint "ISLOW" DCTs, Annex-K tables scaled by the quality,
4:2:0 chroma with the h2v2 "fancy" upsampler).  Entropy coding is lossless and is left out, so the round trip is
32-bit integer arithmetic, and this module gives the same pixels as Pillow's save + open (tests/test_jpeg_cpu.py).

quality_table      the 64 quantiser steps of a quality factor
jpeg_roundtrip_np  uint8 image -> decoded uint8 image, numpy, vectorised over blocks (the reference's
                   cv2.imencode + cv2.imdecode, data/dataset_jpeg.py:67-69)
rgb2gray_cv        cv2.cvtColor(img, cv2.COLOR_RGB2GRAY) for uint8
jpeg_compress      the tensor-level entry: device tensors go to kair_jpeg_roundtrip (csrc/synth_jpeg.hip), CPU
                   tensors to jpeg_roundtrip_np
"""
import numpy as np
import torch

_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                  14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int32)
_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int32)

# FIX(x) = round(x * 2^13) of jfdctint.c / jidctint.c
_F0298, _F0390, _F0541, _F0765, _F0899, _F1175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1501, _F1847, _F1961, _F2053, _F2562, _F3072 = 12299, 15137, 16069, 16819, 20995, 25172


def quality_table(q, chroma=False):
    """[8, 8] int32 quantiser steps of quality q (clamped to 1..100): jpeg_quality_scaling + jpeg_add_quant_table
    with force_baseline."""
    q = min(max(int(q), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = _CHROMA if chroma else _LUMA
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.int32).reshape(8, 8)


def _ds(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd(t4, t5, t6, t7):
    """The odd part shared by the forward and the inverse transform: the four rotated sums."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F1175
    t4, t5, t6, t7 = t4 * _F0298, t5 * _F2053, t6 * _F3072, t7 * _F1501
    z1, z2 = z1 * -_F0899, z2 * -_F2562
    z3, z4 = z3 * -_F1961 + z5, z4 * -_F0390 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, first):
    """One 1-D pass of jfdctint over the last axis of d [..., 8] (int32)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0, o4 = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (_ds(t10 + t11, 2), _ds(t10 - t11, 2))
    z1 = (t12 + t13) * _F0541
    o2, o6 = _ds(z1 + t13 * _F0765, n), _ds(z1 - t12 * _F1847, n)
    a, b, c, e = _odd(t4, t5, t6, t7)
    return np.stack([o0, _ds(e, n), o2, _ds(c, n), o4, _ds(b, n), o6, _ds(a, n)], -1)


def _idct_pass(d, first):
    """One 1-D pass of jidctint over the last axis of d [..., 8] (int32)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    z1 = (d2 + d6) * _F0541
    t2, t3 = z1 - d6 * _F1847, z1 + d2 * _F0765
    t0, t1 = (d0 + d4) << 13, (d0 - d4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _odd(d7, d5, d3, d1)
    n = 11 if first else 18
    return np.stack([_ds(t10 + t3, n), _ds(t11 + t2, n), _ds(t12 + t1, n), _ds(t13 + t0, n), _ds(t13 - t0, n),
                     _ds(t12 - t1, n), _ds(t11 - t2, n), _ds(t10 - t3, n)], -1)


def _plane_roundtrip(p, Q):
    """uint8 plane [H, W] -> decoded uint8 plane: edge-replicate to multiples of 8, forward DCT (rows, then
    columns; 8x the DCT), quantise by Q << 3 rounding half away from zero, dequantise, inverse DCT (columns, then
    rows), + 128, clamp, crop."""
    H, W = p.shape
    x = np.pad(p.astype(np.int32), ((0, -H % 8), (0, -W % 8)), mode="edge") - 128
    b = x.reshape(x.shape[0] // 8, 8, x.shape[1] // 8, 8).transpose(0, 2, 1, 3)   # [by, bx, row, col]
    c = _fdct_pass(b, True)
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    dv = Q << 3
    qc = np.sign(c) * ((np.abs(c) + (dv >> 1)) // dv)
    c = (qc * Q).astype(np.int32)
    c = _idct_pass(c.swapaxes(-1, -2), True).swapaxes(-1, -2)
    c = np.clip(_idct_pass(c, False) + 128, 0, 255)
    return c.transpose(0, 2, 1, 3).reshape(x.shape)[:H, :W].astype(np.uint8)


def _fancy_h2v2(c, H, W):
    """libjpeg's h2v2_fancy_upsample of a chroma plane [ceil(H/2), ceil(W/2)] to [H, W] (int32)."""
    c = c.astype(np.int32)
    up, dn = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int32)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + dn
    lf, rt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * s + lf + 8) >> 4, (3 * s + rt + 7) >> 4
    return out[:H, :W]


def _color_roundtrip(img, q):
    H, W, _ = img.shape
    if W < 5:
        raise ValueError("jpeg_roundtrip_np: colour images need a width of at least 5 (libjpeg uses another "
                         "upsampler below that)")
    x = np.pad(img.astype(np.int32), ((0, H % 2), (0, -W % 16), (0, 0)), mode="edge")
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2], np.int32), x.shape[1] // 4)

    def down(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2

    ch, cw = (H + 1) // 2, (W + 1) // 2
    Ql, Qc = quality_table(q), quality_table(q, chroma=True)
    y = _plane_roundtrip(Y.astype(np.uint8), Ql)[:H, :W].astype(np.int32)
    cb = _fancy_h2v2(_plane_roundtrip(down(Cb).astype(np.uint8), Qc)[:ch, :cw], H, W) - 128
    cr = _fancy_h2v2(_plane_roundtrip(down(Cr).astype(np.uint8), Qc)[:ch, :cw], H, W) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def jpeg_roundtrip_np(img, q):
    """uint8 [H, W], [H, W, 1] (gray JPEG) or [H, W, 3] (RGB, 4:2:0) -> the decoded image, same shape."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError("jpeg_roundtrip_np: uint8 images only")
    if img.ndim == 2:
        return _plane_roundtrip(img, quality_table(q))
    if img.ndim == 3 and img.shape[2] == 1:
        return _plane_roundtrip(img[..., 0], quality_table(q))[..., None]
    if img.ndim == 3 and img.shape[2] == 3:
        return _color_roundtrip(img, q)
    raise ValueError(f"jpeg_roundtrip_np: expected [H, W], [H, W, 1] or [H, W, 3], got {img.shape}")


def jpeg_roundtrip_pil(img, q):
    """The same round trip through Pillow's libjpeg (save + open in memory)."""
    import io

    from PIL import Image
    img = np.asarray(img)
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.ndim == 3 and img.shape[2] == 1 else img).save(buf, "JPEG", quality=int(q))
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    return out[..., None] if img.ndim == 3 and img.shape[2] == 1 else out


def rgb2gray_cv(img):
    """cv2.cvtColor(img, cv2.COLOR_RGB2GRAY) for uint8 [H, W, 3] -> [H, W]: (4899 R + 9617 G + 1868 B + 8192) >> 14,
    the 14-bit fixed-point form of 0.299 / 0.587 / 0.114.  The constants are OpenCV's as recalled from its source;
    OpenCV was not available to check them against (the three sum to 2^14, so gray stays gray)."""
    x = np.asarray(img).astype(np.int32)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).astype(np.uint8)


def _qualities(quality, N):
    qs = [int(quality)] * N if isinstance(quality, int) else [int(q) for q in quality]
    if len(qs) != N or any(q < 1 or q > 100 for q in qs):
        raise ValueError(f"jpeg_compress: quality must be an int or {N} ints in 1..100")
    return qs


def jpeg_compress(x, quality):
    """JPEG round trip of x [N, C, H, W] fp32 in [0, 1], C 1 (gray JPEG) or 3 (RGB, 4:2:0), at `quality` (an int, or
    one per sample): decoded / 255, same shape.  The samples are rint(255 clamp(x)).  A device tensor runs on
    kair_jpeg_roundtrip, a CPU tensor on jpeg_roundtrip_np."""
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError("jpeg_compress: x must be [N, 1 or 3, H, W]")
    N = x.shape[0]
    qs = _qualities(quality, N)
    if x.is_cuda:
        from .. import _hip
        x = x.float().contiguous()
        q = torch.tensor(qs, dtype=torch.int32).to(x.device)
        out = torch.empty_like(x)
        _hip.jpeg_roundtrip(x, q, out)
        return out
    u = (x.float().clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    dec = np.stack([jpeg_roundtrip_np(u[n], qs[n]) for n in range(N)])
    return torch.from_numpy(dec).permute(0, 3, 1, 2).float().div(255.0)
