"""Writes tests/golden/jpeg_roundtrip.npz: small images and what Pillow's libjpeg (Image.save(..., "JPEG", quality=q)
then Image.open) decodes them to, so utils_jpeg.jpeg_roundtrip_np stays pinned to the real codec on a machine
without Pillow.

    python tests/golden/make_golden_jpeg.py

Two gray and two RGB cases, odd sizes (edge replication, a partial last MCU, chroma planes of odd size)."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def smooth(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    ch = [127 + 100 * np.sin(x / (3.0 + k) + k) * np.cos(y / (4.0 + k)) for k in range(c)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def pil_roundtrip(img, q):
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, "JPEG", quality=q)
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    return out[..., None] if img.shape[2] == 1 else out


def main():
    rng = np.random.default_rng(2024)
    cases = [("gray_smooth", smooth(13, 21, 1), 40), ("gray_noise", rng.integers(0, 256, (16, 24, 1), dtype=np.uint8), 10),
             ("rgb_smooth", smooth(17, 7, 3), 75), ("rgb_noise", rng.integers(0, 256, (30, 18, 3), dtype=np.uint8), 1)]
    out = {}
    for name, img, q in cases:
        out[name + ".in"] = img
        out[name + ".q"] = np.int32(q)
        out[name + ".out"] = pil_roundtrip(img, q)
    np.savez_compressed(os.path.join(HERE, "jpeg_roundtrip.npz"), **out)


if __name__ == "__main__":
    main()
