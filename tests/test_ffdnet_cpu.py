"""FFDNet without a GPU: the module tree and its selection (define_G 'ffdnet'), the host forward against the restated
reference, ModelPlain2 ('plain2') on the autograd path against torch Adam, DatasetFFDNet, and the new entry points'
declarations (tests/test_boundary.py checks that the library exports them)."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAY = {"net_type": "ffdnet", "in_nc": 1, "out_nc": 1, "nc": 64, "nb": 15, "act_mode": "R"}
COLOUR = {"net_type": "ffdnet", "in_nc": 3, "out_nc": 3, "nc": 96, "nb": 12, "act_mode": "R"}


class RefFFDNet(nn.Module):
    """The issue's restatement of the reference FFDNet (act_mode 'R'), plain torch."""

    def __init__(self, in_nc, out_nc, nc, nb):
        super().__init__()
        mods = [nn.Conv2d(in_nc * 4 + 1, nc, 3, 1, 1), nn.ReLU()]
        for _ in range(nb - 2):
            mods += [nn.Conv2d(nc, nc, 3, 1, 1), nn.ReLU()]
        mods.append(nn.Conv2d(nc, out_nc * 4, 3, 1, 1))
        self.model = nn.Sequential(*mods)

    def forward(self, x, sigma):
        h, w = x.shape[-2:]
        x = F.pad(x, (0, math.ceil(w / 2) * 2 - w, 0, math.ceil(h / 2) * 2 - h), mode="replicate")
        x = F.pixel_unshuffle(x, 2)
        x = torch.cat((x, sigma.repeat(1, 1, x.shape[2], x.shape[3])), 1)
        return F.pixel_shuffle(self.model(x), 2)[..., :h, :w]


def _define(cfg, **extra):
    from kair_amd.models.select_network import define_G
    from kair_amd.utils.utils_option import dict_to_nonedict
    return define_G(dict_to_nonedict({"is_train": False, "netG": dict(cfg), **extra}))


@pytest.mark.parametrize("cfg, first, last, nb", [(GRAY, [64, 5, 3, 3], [4, 64, 3, 3], 15),
                                                  (COLOUR, [96, 13, 3, 3], [12, 96, 3, 3], 12)])
def test_define_g_layout(cfg, first, last, nb):
    from kair_amd.models.network_ffdnet import FFDNet
    net = _define(cfg)
    assert type(net) is FFDNet and net.compute_dtype == "fp32"
    sd = net.state_dict()
    want = [f"model.{2 * i}.{p}" for i in range(nb) for p in ("weight", "bias")]
    assert list(sd) == want
    assert list(sd["model.0.weight"].shape) == first and list(sd[f"model.{2 * (nb - 1)}.weight"].shape) == last
    assert _define(cfg, train={"amp_enabled": True}).compute_dtype == "bf16"


def test_define_g_refuses_fp32x3():
    with pytest.raises(ValueError):
        _define({**GRAY, "compute_dtype": "fp32x3"})


@pytest.mark.parametrize("kw", [dict(nc=12), dict(out_nc=5), dict(act_mode="IR"), dict(nb=1)])
def test_constructor_guards(kw):
    from kair_amd.models.network_ffdnet import FFDNet
    with pytest.raises(NotImplementedError):
        FFDNet(**{**dict(in_nc=1, out_nc=1, nc=16, nb=4, act_mode="R"), **kw})


@pytest.mark.parametrize("shape, nc, nb", [((2, 1, 5, 7), 16, 4), ((1, 3, 6, 4), 24, 3)])
def test_cpu_forward_equals_reference(shape, nc, nb):
    from kair_amd.models.network_ffdnet import FFDNet
    torch.manual_seed(0)
    B, C = shape[:2]
    net = FFDNet(C, C, nc, nb, "R").eval()
    ref = RefFFDNet(C, C, nc, nb).eval()
    ref.load_state_dict(net.state_dict(), strict=True)
    x = torch.rand(shape)
    sigma = (torch.tensor([5.0, 50.0])[:B] / 255).view(B, 1, 1, 1)
    with torch.no_grad():
        out, want = net(x, sigma), ref(x, sigma)
    assert out.shape == x.shape
    assert torch.allclose(out, want, rtol=1e-6, atol=1e-6)
    if B > 1:   # the level reaches the output, per sample
        with torch.no_grad():
            assert not torch.allclose(net(x, sigma.flip(0)), want, atol=1e-6)


def test_plain2_trains_on_the_cpu(tmp_path):
    from kair_amd.models.model_plain2 import ModelPlain2
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = dict_to_nonedict({
        "model": "plain2", "gpu_ids": None, "is_train": True, "dist": False,
        "path": {"models": str(tmp_path), "pretrained_netG": None},
        "netG": {"net_type": "ffdnet", "in_nc": 1, "out_nc": 1, "nc": 16, "nb": 4, "act_mode": "R", "init_type": "default"},
        "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-3,
                  "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_scheduler_type": "MultiStepLR",
                  "G_scheduler_milestones": [100], "G_scheduler_gamma": 0.5, "E_decay": 0, "G_param_strict": True,
                  "G_optimizer_reuse": False}})
    torch.manual_seed(1)
    m = define_Model(opt)
    assert type(m) is ModelPlain2
    m.init_train()
    assert m.trainer is None   # the host runs the autograd path
    ref = RefFFDNet(1, 1, 16, 4)
    ref.load_state_dict(m.netG.state_dict(), strict=True)
    adam = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.999))
    g = torch.Generator().manual_seed(2)
    for step in (1, 2):
        L, Hh = torch.rand(3, 1, 10, 14, generator=g), torch.rand(3, 1, 10, 14, generator=g)
        C = torch.rand(3, 1, 1, 1, generator=g) * 75 / 255
        m.feed_data({"L": L, "H": Hh, "C": C})
        m.optimize_parameters(step)
        adam.zero_grad()
        loss = F.l1_loss(ref(L, C), Hh)
        loss.backward()
        adam.step()
        assert abs(m.current_log()["G_loss"] - loss.item()) <= 1e-6 * loss.item()
    m.test()
    assert m.current_visuals()["E"].shape == (1, 10, 14)


@pytest.fixture()
def png_dir(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(7)
    d = tmp_path / "H"
    d.mkdir()
    for i, (h, w) in enumerate([(40, 52), (36, 33)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"im{i}.png"))
    return str(d)


def _ds(png_dir, phase, C, **kw):
    from kair_amd.data.select_dataset import define_Dataset
    return define_Dataset({"dataset_type": "ffdnet", "phase": phase, "dataroot_H": png_dir, "n_channels": C, "H_size": 32,
                           "sigma": [5, 60], "sigma_test": 25, **kw})


@pytest.mark.parametrize("C", [1, 3])
def test_dataset_train_item(png_dir, C):
    from kair_amd.data.dataset_ffdnet import DatasetFFDNet
    ds = _ds(png_dir, "train", C)
    assert type(ds) is DatasetFFDNet and len(ds) == 2
    torch.manual_seed(3)
    levels = []
    for idx in (0, 1, 0, 1):
        it = ds[idx]
        assert set(it) == {"L", "H", "C", "L_path", "H_path"}
        L, H, lev = it["L"], it["H"], it["C"]
        assert L.shape == (C, 32, 32) and H.shape == (C, 32, 32) and lev.shape == (1, 1, 1) and lev.dtype == torch.float32
        assert 5 / 255.0 - 1e-7 <= lev.item() <= 60 / 255.0 + 1e-7
        # L - H = level * n, n ~ N(0, 1) over C * 1024 samples: the sample deviation is within 6 / sqrt(2 n) of level
        n = C * 32 * 32
        assert abs((L - H).std().item() / lev.item() - 1) < 6 / math.sqrt(2 * n)
        levels.append(lev.item())
    assert len(set(levels)) > 1
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert batch["C"].shape == (2, 1, 1, 1) and batch["L"].shape == (2, C, 32, 32)


def test_dataset_test_item_is_deterministic(png_dir):
    ds = _ds(png_dir, "test", 3, sigma_test=15)
    a, b = ds[1], ds[1]
    assert torch.equal(a["L"], b["L"]) and torch.equal(a["H"], b["H"]) and torch.equal(a["C"], b["C"])
    assert a["L"].shape == (3, 36, 33) and a["H"].shape == (3, 36, 33) and a["C"].shape == (1, 1, 1)
    assert a["C"].item() == np.float32(15 / 255.0).item()
    assert (a["L"] < 0).any() or (a["L"] > 1).any()   # nothing clipped


def test_unknown_dataset_type_still_raises(png_dir):
    from kair_amd.data.select_dataset import define_Dataset
    with pytest.raises(NotImplementedError):
        define_Dataset({"dataset_type": "ffdnet2", "phase": "train", "dataroot_H": png_dir})


def test_entry_points_declared():
    from kair_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kair_hip.h")).read(), flags=re.S)
    for name, nargs in (("kair_ffd_pack", 10), ("kair_synth_dn_level", 16)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_hip._SIGS[name])
    assert callable(_hip.ffd_pack) and callable(_hip.synth_dn_level)
