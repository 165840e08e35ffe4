"""JPEG CAR data on the host: utils_jpeg.jpeg_roundtrip_np against Pillow's libjpeg (equality: both are the same
32-bit integer arithmetic), the Pillow-made golden file, DatasetJPEG against the draws re-made here, and the 'jpeg'
entry of define_Dataset."""
import io
import os
import random

import numpy as np
import pytest
import torch

from kair_amd.utils import utils_image as util
from kair_amd.utils import utils_jpeg as jpg

from conftest import load_golden

GRAY_SIZES = [(8, 8), (16, 24), (13, 21), (134, 134)]
RGB_SIZES = [(16, 16), (16, 32), (13, 21), (6, 5), (9, 9), (10, 12), (17, 7), (24, 40), (30, 18), (134, 134)]
QUALITIES = [1, 10, 40, 75, 95, 100]


def smooth(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    ch = [127 + 100 * np.sin(x / (3.0 + k) + k) * np.cos(y / (4.0 + k)) for k in range(c)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def noise(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def pil_roundtrip(img, q):
    """Written out here (not utils_jpeg.jpeg_roundtrip_pil): the test's own statement of the reference."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.ndim == 3 and img.shape[2] == 1 else img).save(buf, "JPEG", quality=q)
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    return out[..., None] if img.ndim == 3 and img.shape[2] == 1 else out


@pytest.mark.parametrize("c,size", [(1, s) for s in GRAY_SIZES] + [(3, s) for s in RGB_SIZES])
def test_roundtrip_np_equals_pillow(c, size):
    pytest.importorskip("PIL")
    h, w = size
    for kind, img in (("smooth", smooth(h, w, c)), ("noise", noise(h, w, c, 7 * h + w + c))):
        for q in QUALITIES:
            got, want = jpg.jpeg_roundtrip_np(img, q), pil_roundtrip(img, q)
            assert got.shape == want.shape == img.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (kind, c, size, q, int(np.abs(got.astype(int) - want).max()))
    if c == 1:   # [H, W] is the same gray JPEG
        assert np.array_equal(jpg.jpeg_roundtrip_np(img[..., 0], 40), jpg.jpeg_roundtrip_np(img, 40)[..., 0])


def test_roundtrip_np_equals_golden():
    z = load_golden("jpeg_roundtrip")
    names = sorted(k[:-3] for k in z.files if k.endswith(".in"))
    assert names == ["gray_noise", "gray_smooth", "rgb_noise", "rgb_smooth"]
    for n in names:
        assert np.array_equal(jpg.jpeg_roundtrip_np(z[n + ".in"], int(z[n + ".q"])), z[n + ".out"]), n


def test_quality_tables_and_argument_checks():
    assert jpg.quality_table(50)[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61]
    assert jpg.quality_table(50, chroma=True)[0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99]
    assert (jpg.quality_table(100) == 1).all() and (jpg.quality_table(1) == 255).all()
    assert jpg.quality_table(25)[0, 0] == 32 and jpg.quality_table(75)[0, 0] == 8
    assert np.array_equal(jpg.quality_table(0), jpg.quality_table(1))
    assert np.array_equal(jpg.quality_table(400), jpg.quality_table(100))
    with pytest.raises(ValueError):
        jpg.jpeg_roundtrip_np(np.zeros((8, 4, 3), np.uint8), 40)   # colour narrower than 5
    with pytest.raises(ValueError):
        jpg.jpeg_roundtrip_np(np.zeros((8, 8), np.float32), 40)
    with pytest.raises(ValueError):
        jpg.jpeg_compress(torch.zeros(2, 1, 8, 8), [40])
    with pytest.raises(ValueError):
        jpg.jpeg_compress(torch.zeros(1, 1, 8, 8), 0)


def test_rgb2gray_cv_formula():
    img = noise(9, 11, 3, 5)
    R, G, B = (img[..., k].astype(np.int64) for k in range(3))
    assert np.array_equal(jpg.rgb2gray_cv(img), (4899 * R + 9617 * G + 1868 * B + 8192) >> 14)
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)
    assert np.array_equal(jpg.rgb2gray_cv(gray)[:, 0], np.arange(256))


def test_jpeg_compress_cpu_tensor():
    x = torch.from_numpy(noise(13, 21, 3, 3)).permute(2, 0, 1)[None].float().div(255.0)
    x = torch.cat([x, x.flip(-1)])
    out = jpg.jpeg_compress(x, [10, 90])
    assert out.shape == x.shape and out.dtype == torch.float32
    for n, q in enumerate([10, 90]):
        u = (x[n] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
        assert torch.equal(out[n], util.uint2tensor3(jpg.jpeg_roundtrip_np(u, q)))
    g = jpg.jpeg_compress(x[:, :1], 40)
    u = (x[0, 0] * 255).round().to(torch.uint8).numpy()
    assert torch.equal(g[0, 0], torch.from_numpy(jpg.jpeg_roundtrip_np(u, 40)).float().div(255.0))


# ---- DatasetJPEG ------------------------------------------------------------------------------------------------
def _write_images(tmp_path):
    from PIL import Image
    os.makedirs(tmp_path, exist_ok=True)
    imgs = [smooth(40, 56, 3), noise(37, 45, 3, 11)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(os.path.join(tmp_path, f"im{i}.png"))
    return imgs


def _roundtrip(img, q):
    try:
        return pil_roundtrip(img, q)
    except ImportError:
        return jpg.jpeg_roundtrip_np(img, q)


@pytest.mark.parametrize("is_color", [False, True])
def test_dataset_jpeg_train(tmp_path, is_color):
    pytest.importorskip("PIL")
    from kair_amd.data.dataset_jpeg import DatasetJPEG
    imgs = _write_images(str(tmp_path))
    ds = DatasetJPEG({"phase": "train", "dataroot_H": str(tmp_path), "H_size": 16, "quality_factor": 30,
                      "is_color": is_color, "n_channels": 3 if is_color else 1})
    assert len(ds) == 2
    seen_gray, seen_crop = set(), set()
    for seed in range(12):
        idx = seed % 2
        random.seed(seed)
        item = ds[idx]
        random.seed(seed)
        img = imgs[idx]
        rh, rw = random.randint(0, img.shape[0] - 24), random.randint(0, img.shape[1] - 24)
        patch = np.ascontiguousarray(util.augment_img(img[rh:rh + 24, rw:rw + 24], mode=random.randint(0, 7)))
        if is_color:
            Hh = patch
        else:
            ycc = random.random() > 0.5
            seen_gray.add(ycc)
            Hh = util.rgb2ycbcr(patch) if ycc else jpg.rgb2gray_cv(patch)
        L = _roundtrip(Hh, 30)
        second = random.random() > 0.5
        seen_crop.add(second)
        r2, c2 = (random.randint(0, 8), random.randint(0, 8)) if second else (0, 0)
        Hh, L = Hh[r2:r2 + 16, c2:c2 + 16], L[r2:r2 + 16, c2:c2 + 16]
        C = 3 if is_color else 1
        assert item["H"].shape == item["L"].shape == (C, 16, 16)
        assert torch.equal(item["H"], util.uint2tensor3(Hh)) and torch.equal(item["L"], util.uint2tensor3(L))
        assert not torch.equal(item["L"], item["H"])
        assert item["H_path"] == item["L_path"] == os.path.join(str(tmp_path), f"im{idx}.png")
    assert seen_crop == {False, True} and (is_color or seen_gray == {False, True})


@pytest.mark.parametrize("is_color", [False, True])
def test_dataset_jpeg_test_phase(tmp_path, is_color):
    pytest.importorskip("PIL")
    from kair_amd.data.dataset_jpeg import DatasetJPEG
    imgs = _write_images(str(tmp_path))
    ds = DatasetJPEG({"phase": "test", "dataroot_H": str(tmp_path), "quality_factor": 30, "quality_factor_test": 15,
                      "is_color": is_color})
    for idx, img in enumerate(imgs):
        item = ds[idx]
        Hh = img if is_color else util.rgb2ycbcr(img)
        assert torch.equal(item["H"], util.uint2tensor3(Hh))
        assert torch.equal(item["L"], util.uint2tensor3(_roundtrip(Hh, 15)))
        assert item["H"].shape == (3 if is_color else 1, img.shape[0], img.shape[1])


def test_define_dataset_jpeg(tmp_path):
    pytest.importorskip("PIL")
    from kair_amd.data.dataset_jpeg import DatasetJPEG
    from kair_amd.data.select_dataset import define_Dataset
    _write_images(str(tmp_path))
    ds = define_Dataset({"dataset_type": "jpeg", "phase": "train", "dataroot_H": str(tmp_path)})
    assert isinstance(ds, DatasetJPEG)
    assert (ds.patch_size, ds.quality_factor, ds.quality_factor_test, ds.is_color, ds.n_channels) == (128, 40, 40, False, 3)
