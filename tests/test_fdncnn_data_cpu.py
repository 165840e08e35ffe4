"""DatasetFDnCNN on the host (no GPU): the factory entries ('fdncnn' and its alias 'drunet'), the C + 1 channel item,
the constant noise-level map inside [min / 255, max / 255], L[:C] - H = level * n with torch.randn recorded, and the
deterministic test phase (np.random.seed(0) + normal, the map at sigma_test / 255)."""
import os
import random

import numpy as np
import pytest
import torch

from kair_amd.data.select_dataset import define_Dataset
from kair_amd.utils import utils_image as util


@pytest.fixture()
def png_dir(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(7)
    d = tmp_path / "H"
    d.mkdir()
    for i, (h, w) in enumerate([(40, 52), (36, 33), (48, 48)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"im{i}.png"))
    return str(d)


def opt_of(png_dir, phase, t="fdncnn", **kw):
    return {"dataset_type": t, "phase": phase, "dataroot_H": png_dir, "n_channels": 3, "H_size": 32, "sigma": [5, 60],
            "sigma_test": 25, **kw}


@pytest.mark.parametrize("t", ["fdncnn", "drunet"])
def test_define_dataset_binds(png_dir, t):
    from kair_amd.data.dataset_fdncnn import DatasetFDnCNN
    ds = define_Dataset(opt_of(png_dir, "train", t))
    assert isinstance(ds, DatasetFDnCNN) and len(ds) == 3
    assert (ds.patch_size, ds.sigma, ds.sigma_test) == (32, [5, 60], 25)


def test_defaults(png_dir):
    ds = define_Dataset({"dataset_type": "fdncnn", "phase": "train", "dataroot_H": png_dir, "n_channels": 1})
    assert (ds.patch_size, ds.sigma, ds.sigma_test) == (64, [0, 75], 25)


@pytest.mark.parametrize("C", [1, 3])
def test_train_item(png_dir, C, monkeypatch):
    ds = define_Dataset(opt_of(png_dir, "train", n_channels=C))
    rec = []
    randn = torch.randn

    def recorded(*a, **k):
        rec.append(randn(*a, **k))
        return rec[-1].clone()
    monkeypatch.setattr(torch, "randn", recorded)
    levels = []
    for idx in (0, 1, 2, 0):
        random.seed(11 + idx)
        np.random.seed(12 + idx)
        del rec[:]
        it = ds[idx]
        assert set(it) == {"L", "H", "L_path", "H_path"} and it["L_path"] == it["H_path"]
        L, H = it["L"], it["H"]
        assert L.shape == (C + 1, 32, 32) and H.shape == (C, 32, 32) and L.dtype == torch.float32
        level = L[C, 0, 0].item()
        assert torch.equal(L[C], torch.full((32, 32), level))                    # the map is constant ...
        assert 5 / 255.0 - 1e-7 <= level <= 60 / 255.0 + 1e-7                    # ... and inside [min, max] / 255
        assert len(rec) == 1 and rec[0].shape == H.shape
        assert torch.equal(L[:C], H + rec[0] * torch.tensor([level]))            # L = H + level * n, nothing clipped
        # the draws, in the documented order: rnd_h, rnd_w (random), then the mode and the level (np.random)
        random.seed(11 + idx)
        np.random.seed(12 + idx)
        img = util.imread_uint(it["H_path"], C)
        rh = random.randint(0, img.shape[0] - 32)
        rw = random.randint(0, img.shape[1] - 32)
        mode = np.random.randint(0, 8)
        assert abs(np.random.uniform(5, 60) / 255.0 - level) < 1e-7
        assert torch.equal(H, util.uint2tensor3(util.augment_img(img[rh:rh + 32, rw:rw + 32, :], mode)))
        levels.append(level)
    assert len(set(levels)) > 1   # one level per sample, not per dataset


def test_test_phase_is_deterministic(png_dir):
    ds = define_Dataset(opt_of(png_dir, "test", sigma_test=15))
    a, b = ds[1], ds[1]
    assert torch.equal(a["L"], b["L"]) and torch.equal(a["H"], b["H"])
    H = util.uint2single(util.imread_uint(a["H_path"], 3))
    assert a["H"].shape == (3, 36, 33) and a["L"].shape == (4, 36, 33)
    np.random.seed(0)
    want = np.copy(H)
    want += np.random.normal(0, 15 / 255.0, H.shape)
    assert torch.equal(a["L"][:3], util.single2tensor3(want))
    assert torch.equal(a["L"][3], torch.full((36, 33), np.float32(15 / 255.0).item()))
    assert (a["L"][:3] < 0).any() or (a["L"][:3] > 1).any()   # no clipping
