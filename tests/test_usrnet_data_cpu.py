"""DatasetUSRNet and utils_sisr.gen_kernel on the host (no GPU): the factory entry, the kernel's normalisation and
centre, the documented item layout of both phases, and a DataLoader batch through ModelPlain4.feed_data's reading
of 'sf'."""
import math
import os

import numpy as np
import pytest
import torch

from kair_amd.data.select_dataset import define_Dataset
from kair_amd.utils import utils_sisr as sisr


@pytest.fixture()
def png_dir(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(5)
    d = tmp_path / "H"
    d.mkdir()
    for i, (h, w) in enumerate([(60, 72), (64, 50), (49, 55), (70, 70)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"im{i}.png"))
    return str(d)


def opt_of(png_dir, phase, **kw):
    return {"dataset_type": "usrnet", "phase": phase, "dataroot_H": png_dir, "n_channels": 3, "H_size": 48,
            "sigma_max": 25, "scales": [1, 2, 3, 4], "dataloader_batch_size": 2, **kw}


def test_define_dataset_usrnet(png_dir):
    from kair_amd.data.dataset_usrnet import DatasetUSRNet
    ds = define_Dataset(opt_of(png_dir, "train"))
    assert isinstance(ds, DatasetUSRNet) and len(ds) == 4
    with pytest.raises(ValueError):
        define_Dataset(opt_of(png_dir, "train", H_size=50))


@pytest.mark.parametrize("sf_k", [1, 2, 3, 4])
def test_gen_kernel_normalised_and_centred(sf_k):
    ax = torch.arange(25, dtype=torch.float64)
    mu = 12 + 0.5 * (sf_k - 1)
    for l1, l2, th in [(0.6, 2.0, 0.3), (2.0, 0.6, 2.5), (1.3, 1.3, 0.0), (12.0, 0.6, 1.0)]:
        k = sisr.gen_kernel(25, l1, l2, th, sf_k, 0)
        assert k.shape == (25, 25) and k.dtype == torch.float64
        assert abs(k.sum().item() - 1.0) < 1e-12 and k.min() >= 0
        if max(l1, l2) <= 2:   # the mass stays inside the 25-tap support
            cy, cx = (k.sum(1) * ax).sum().item(), (k.sum(0) * ax).sum().item()
            assert abs(cy - mu) < 0.05 and abs(cx - mu) < 0.05, (cy, cx, mu)
    # the elongated axis follows theta: variance 12 along (cos, sin), 0.6 across it
    k = sisr.gen_kernel(25, 12.0, 0.6, 0.0, 1, 0)
    assert k[12, 4] > 1e3 * k[4, 12]
    # mode_k is the augment map of the un-augmented kernel; drawn parameters are reproducible per rng
    import random
    k0 = sisr.gen_kernel(25, 3.0, 0.8, 0.7, 2, 0)
    for m in range(8):
        from kair_amd.utils.utils_image import augment_img
        assert np.array_equal(sisr.gen_kernel(25, 3.0, 0.8, 0.7, 2, m).numpy(), augment_img(k0.numpy(), m))
    assert torch.equal(sisr.gen_kernel(rng=random.Random(4)), sisr.gen_kernel(rng=random.Random(4)))


def test_wrap_blur_is_the_circular_convolution():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 9, 7, generator=g, dtype=torch.float64)    # smaller than the kernel: wraps twice
    k = torch.rand(25, 25, generator=g, dtype=torch.float64)
    y = sisr.wrap_blur(x, k)
    want = torch.zeros_like(x)
    for u in range(25):
        for v in range(25):
            want += k[u, v] * torch.roll(x, shifts=(u - 12, v - 12), dims=(-2, -1))
    assert (y - want).abs().max() < 1e-11


def test_train_item(png_dir):
    ds = define_Dataset(opt_of(png_dir, "train"))
    seen = set()
    for it in range(12):
        torch.manual_seed(it)
        d = ds[it % 4]
        assert set(d) == {"L", "H", "k", "sigma", "sf", "L_path", "H_path"}
        sf = d["sf"]
        seen.add(sf)
        assert sf in (1, 2, 3, 4)
        assert d["H"].shape == (3, 48, 48) and d["L"].shape == (3, 48 // sf, 48 // sf)
        assert d["H"].dtype == d["L"].dtype == d["k"].dtype == torch.float32
        assert d["k"].shape == (1, 25, 25) and abs(d["k"].sum().item() - 1) < 1e-5
        assert d["sigma"].shape == (1, 1, 1)
        s255 = d["sigma"].item() * 255
        assert abs(s255 - round(s255)) < 1e-4 and 0 <= round(s255) < 25
        torch.manual_seed(it)   # the item's own noise, redrawn
        clean = (d["L"] - torch.randn(d["L"].shape) * d["sigma"].item()).double() * 255
        if d["sigma"].item() == 0:
            assert (clean - clean.round()).abs().max() < 1e-4   # the blur is truncated to uint8
        # L is the truncated wrap blur of H, decimated
        want = torch.floor(sisr.wrap_blur(d["H"].double() * 255, d["k"][0].double()) + 1e-6)[..., ::sf, ::sf]
        assert (clean - want).abs().max() < 1.0 + 1e-3   # k went through float32: a floor may move by one level
        assert ((clean - want).abs() > 1e-3).double().mean() < 0.02
    assert len(seen) > 1
    # one scale factor per 'dataloader_batch_size' items
    ds2 = define_Dataset(opt_of(png_dir, "train"))
    sfs = [ds2[i % 4]["sf"] for i in range(16)]
    assert all(sfs[i] == sfs[i + 1] for i in range(0, 16, 2))


def test_test_item(png_dir):
    ds = define_Dataset(opt_of(png_dir, "test", sf_validation=2))
    d, d2 = ds[0], ds[0]
    assert d["sf"] == 2 and d["sigma"].item() == 0.0
    assert d["H"].shape == (3, 60, 72) and d["L"].shape == (3, 30, 36)
    assert torch.equal(d["L"], d2["L"]) and torch.equal(d["k"], d2["k"])   # fixed kernel, no noise
    v = d["L"].double() * 255
    assert (v - v.round()).abs().max() < 1e-4
    assert define_Dataset(opt_of(png_dir, "test"))[1]["sf"] == 3   # the default
    bank = torch.rand(3, 25, 25, generator=torch.Generator().manual_seed(1))
    ds = define_Dataset(opt_of(png_dir, "test", kernel_bank=bank))
    assert torch.allclose(ds[2]["k"][0], (bank[0] / bank[0].sum()).float())


def test_dataloader_batch_feeds_modelplain4(png_dir):
    """The collated 'sf' is what ModelPlain4.feed_data indexes (model_plain4.py: data['sf'][0, ...])."""
    from torch.utils.data import DataLoader
    from kair_amd.models.model_plain4 import ModelPlain4
    ds = define_Dataset(opt_of(png_dir, "train"))
    batch = next(iter(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)))
    assert batch["k"].shape == (2, 1, 25, 25) and batch["sigma"].shape == (2, 1, 1, 1)
    sf = int(batch["sf"][0])
    assert batch["L"].shape == (2, 3, 48 // sf, 48 // sf) and batch["H"].shape == (2, 3, 48, 48)
    m = ModelPlain4.__new__(ModelPlain4)
    m.device = torch.device("cpu")
    m.feed_data(batch)
    assert m.sf == sf and m.k.shape == (2, 1, 25, 25) and m.L.shape[-1] * m.sf == m.H.shape[-1]
    assert m._step_cond()[1] == sf
    assert math.isfinite(m.L.sum().item())
