"""MSRResNet0, the DPSR prior and IMDN without a device: parameter counts, state_dict key lists, the CPU forward in
float64 against a functional reference written here from the state_dict alone (F.conv2d, split, cat, F.interpolate,
F.pixel_shuffle, leaky_relu 0.05), define_G from the option files, the refusals, and DatasetDPSR on a folder of tiny PNGs.

ref_forward() is also the float64 twin of tests/test_ressr_gpu.py.
"""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kair_amd.models.network_dpsr import MSRResNet_prior
from kair_amd.models.network_imdn import IMDN
from kair_amd.models.network_msrresnet import MSRResNet0
from kair_amd.utils import utils_image as util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# the functional references: sd maps the module's state_dict keys to tensors (or Parameters) of one dtype
# ---------------------------------------------------------------------------------------------------------------------
def _conv(sd, key, x):
    w = sd[key + ".weight"]
    return F.conv2d(x, w, sd.get(key + ".bias"), 1, w.shape[-1] // 2)


def ref_msrresnet(sd, x, nb, upscale, rnd=lambda t: t, mode="upconv"):
    """rnd: applied where the engine stores an activation in its compute dtype (identity: the plain float64 twin)."""
    fea = _conv(sd, "model.0", rnd(x))
    h = fea
    for i in range(nb):
        a = rnd(F.relu(_conv(sd, f"model.1.sub.{i}.res.0", rnd(h))))
        h = h + _conv(sd, f"model.1.sub.{i}.res.2", a)
    h = rnd(fea + _conv(sd, f"model.1.sub.{nb}", rnd(h)))
    idx = 3
    for r in ([3] if upscale == 3 else [2] * (upscale // 2)):
        if mode == "upconv":
            h = rnd(F.relu(_conv(sd, f"model.{idx}", F.interpolate(h, scale_factor=2, mode="nearest"))))
        else:
            h = rnd(F.relu(F.pixel_shuffle(_conv(sd, f"model.{idx - 1}", h), r)))
        idx += 3
    h = rnd(F.relu(_conv(sd, f"model.{idx - 1}", h)))
    return _conv(sd, f"model.{idx + 1}", h)


def ref_imdn(sd, x, nb, upscale, rnd=lambda t: t):
    fea = _conv(sd, "model.0", rnd(x))
    h = fea
    nc = fea.shape[1]
    d = nc // 4
    lr = lambda t: rnd(F.leaky_relu(t, 0.05))
    for i in range(nb):
        p = f"model.1.sub.{i}."
        d1, r1 = torch.split(lr(_conv(sd, p + "conv1.0", rnd(h))), (d, nc - d), dim=1)
        d2, r2 = torch.split(lr(_conv(sd, p + "conv2.0", r1)), (d, nc - d), dim=1)
        d3, r3 = torch.split(lr(_conv(sd, p + "conv3.0", r2)), (d, nc - d), dim=1)
        d4 = rnd(_conv(sd, p + "conv4", r3))
        h = h + _conv(sd, p + "conv1x1", torch.cat((d1, d2, d3, d4), dim=1))
    h = rnd(fea + _conv(sd, f"model.1.sub.{nb}", rnd(h)))
    return F.pixel_shuffle(_conv(sd, "model.2", h), upscale)


def ref_forward(net, sd, x, rnd=lambda t: t):
    if isinstance(net, IMDN):
        return ref_imdn(sd, x, net.nb, net.upscale, rnd)
    return ref_msrresnet(sd, x, net.nb, net.upscale, rnd, net.upsample_mode)


def sd_of(net, dtype=F64):
    return {k: v.detach().clone().to(dtype) for k, v in net.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------
# module trees
# ---------------------------------------------------------------------------------------------------------------------
def test_parameter_counts():
    assert sum(p.numel() for p in IMDN(3, 3, 64, 8, 4).parameters()) == 893936
    assert sum(p.numel() for p in MSRResNet0(3, 3, 64, 16, 4).parameters()) == 1332928


def _wb(*keys):
    return [f"{k}.{p}" for k in keys for p in ("weight", "bias")]


@pytest.mark.parametrize("mode,sf", [("upconv", 2), ("upconv", 4), ("pixelshuffle", 2), ("pixelshuffle", 3),
                                     ("pixelshuffle", 4)])
@pytest.mark.parametrize("cls,in_nc,nc", [(MSRResNet0, 3, 16), (MSRResNet_prior, 4, 24)])
def test_msrresnet_keys(cls, in_nc, nc, mode, sf):
    nb = 3
    net = cls(in_nc, 3, nc, nb, sf, upsample_mode=mode)
    body = [f"model.1.sub.{i}.res.{j}" for i in range(nb) for j in (0, 2)] + [f"model.1.sub.{nb}"]
    u = 3 if mode == "upconv" else 2                                # the conv's place in its upsampling block
    ups, tail = ([f"model.{u}"], ("model.5", "model.7")) if sf < 4 else ([f"model.{u}", f"model.{u + 3}"], ("model.8", "model.10"))
    r = 3 if sf == 3 else 2
    assert net.state_dict()[ups[0] + ".weight"].shape == ((nc if mode == "upconv" else nc * r * r), nc, 3, 3)
    want = _wb("model.0", *body, *ups, tail[0]) + [tail[1] + ".weight"]
    assert list(net.state_dict()) == want
    assert tail[1] + ".bias" not in net.state_dict()            # the final conv has no bias
    assert net.state_dict()["model.0.weight"].shape == (nc, in_nc, 3, 3)


@pytest.mark.parametrize("sf", [2, 3, 4])
def test_imdn_keys(sf):
    nb = 2
    net = IMDN(3, 3, 32, nb, sf)
    body = [f"model.1.sub.{i}.{c}" for i in range(nb) for c in ("conv1.0", "conv2.0", "conv3.0", "conv4", "conv1x1")]
    assert list(net.state_dict()) == _wb("model.0", *body, f"model.1.sub.{nb}", "model.2")
    sd = net.state_dict()
    assert sd["model.1.sub.0.conv2.0.weight"].shape == (32, 24, 3, 3) and sd["model.1.sub.0.conv4.weight"].shape == (8, 24, 3, 3)
    assert sd["model.1.sub.0.conv1x1.weight"].shape == (32, 32, 1, 1) and sd["model.2.weight"].shape == (3 * sf * sf, 32, 3, 3)


CPU_CASES = [(MSRResNet0, dict(in_nc=3, nc=16, nb=2, upscale=2)), (MSRResNet0, dict(in_nc=1, out_nc=1, nc=16, nb=2, upscale=4)),
             (MSRResNet_prior, dict(in_nc=4, nc=24, nb=2, upscale=4)), (IMDN, dict(nc=32, nb=2, upscale=2)),
             (MSRResNet0, dict(nc=16, nb=2, upscale=2, upsample_mode="pixelshuffle")),
             (MSRResNet0, dict(nc=16, nb=2, upscale=3, upsample_mode="pixelshuffle")),
             (MSRResNet_prior, dict(nc=16, nb=1, upscale=4, upsample_mode="pixelshuffle")),
             (IMDN, dict(nc=32, nb=2, upscale=3)), (IMDN, dict(in_nc=1, out_nc=1, nc=64, nb=1, upscale=4))]


@pytest.mark.parametrize("cls,kw", CPU_CASES)
def test_cpu_forward_equals_the_functional_reference_in_float64(cls, kw):
    torch.manual_seed(3)
    net = cls(**kw).double()
    x = torch.rand(2, net.in_nc, 9, 7, dtype=F64)
    with torch.no_grad():
        out, want = net(x), ref_forward(net, sd_of(net), x)
    assert out.shape == (2, net.out_nc, 9 * net.upscale, 7 * net.upscale) == want.shape
    assert ((out - want).norm() / want.norm()).item() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# define_G
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname,cls,in_nc,nc,nb", [("train_msrresnet_psnr.json", MSRResNet0, 3, 64, 16),
                                                   ("train_imdn.json", IMDN, 3, 64, 8),
                                                   ("train_dpsr.json", MSRResNet_prior, 4, 96, 16)])
def test_define_G_from_the_option_files(fname, cls, in_nc, nc, nb):
    from kair_amd.models.select_network import define_G
    from kair_amd.utils import utils_option as option
    opt = option.parse(os.path.join(ROOT, "options", fname), is_train=True)
    assert opt["model"] == "plain" and opt["train"]["G_lossfn_type"] == "l1"
    assert opt["datasets"]["train"]["H_size"] == 96
    assert opt["datasets"]["train"]["dataset_type"] == ("dpsr" if cls is MSRResNet_prior else "sr")
    net = define_G(opt)
    assert type(net) is cls and (net.in_nc, net.nc, net.nb, net.upscale) == (in_nc, nc, nb, 4)
    assert net.compute_dtype == "fp32"


def _netg(**kw):
    o = {"net_type": "msrresnet0", "in_nc": 3, "out_nc": 3, "nc": 16, "nb": 2, "scale": 4, "act_mode": "R",
         "upsample_mode": "upconv"}
    o.update(kw)
    return {"netG": o, "is_train": False}


@pytest.mark.parametrize("kw,fragment", [
    (dict(net_type="msrresnet1"), "msrresnet1"), (dict(upsample_mode="convtranspose"), "convtranspose"),
    (dict(scale=3), "upscale 3"), (dict(scale=5, upsample_mode="pixelshuffle"), "upscale 5"), (dict(act_mode="L"), "'L'"), (dict(nc=20), "nc 20"),
    (dict(net_type="dpsr", in_nc=4, act_mode="BR"), "'BR'"),
    (dict(net_type="imdn", act_mode="L", upsample_mode="pixelshuffle", nc=48), "nc 48"),
    (dict(net_type="imdn", act_mode="R", upsample_mode="pixelshuffle", nc=32), "'R'"),
    (dict(net_type="imdn", act_mode="L", upsample_mode="upconv", nc=32), "upconv"),
    (dict(net_type="imdn", act_mode="L", upsample_mode="pixelshuffle", nc=32, out_nc=4), "<= 48"),
])
def test_unsupported_values_raise_naming_them(kw, fragment):
    from kair_amd.models.select_network import define_G
    with pytest.raises(NotImplementedError, match=fragment):
        define_G(_netg(**kw))


@pytest.mark.parametrize("t,kw", [("msrresnet0", {}), ("dpsr", dict(in_nc=4)),
                                  ("imdn", dict(act_mode="L", upsample_mode="pixelshuffle", nc=32))])
def test_fp32x3_is_refused(t, kw):
    from kair_amd.models.select_network import define_G
    with pytest.raises(ValueError, match="fp32x3"):
        define_G(_netg(net_type=t, compute_dtype="fp32x3", **kw))
    assert define_G(_netg(net_type=t, compute_dtype="bf16", **kw)).compute_dtype == "bf16"


# ---------------------------------------------------------------------------------------------------------------------
# DatasetDPSR
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("dpsr_imgs")
    rng = np.random.RandomState(0)
    for i, (h, w) in enumerate([(40, 37), (38, 50), (45, 41)]):
        util.imsave(rng.randint(0, 256, (h, w, 3), dtype=np.uint8), str(d / f"im{i}.png"))
    return str(d)


@pytest.mark.parametrize("sf", [2, 3, 4])
def test_dataset_dpsr_items(png_dir, sf):
    from kair_amd.data.select_dataset import define_Dataset
    opt = {"dataset_type": "dpsr", "dataroot_H": png_dir, "scale": sf, "H_size": 24, "n_channels": 3, "phase": "train"}
    ds = define_Dataset(opt)
    assert len(ds) == 3
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    levels = []
    for i in range(3):
        it = ds[i]
        assert set(it) == {"L", "H", "L_path", "H_path"}
        L, Hh = it["L"], it["H"]
        assert L.shape == (4, 24 // sf, 24 // sf) and Hh.shape == (3, 24, 24) and L.dtype == torch.float32
        assert torch.equal(L[3], L[3, :1, :1].expand_as(L[3]))       # the level channel is constant per sample
        assert 0 <= L[3, 0, 0] <= 50 / 255 + 1e-7
        levels.append(L[3, 0, 0].item())
    assert len(set(levels)) == 3
    np.random.seed(0)
    want = [np.float32(np.random.uniform(0, 50) / 255.0) for _ in range(3)]
    assert levels == [float(v) for v in want]                        # level / 255, the draw itself
    # sigma [0, 0]: the image channels are DatasetSR's L for the same file and seed, the level channel is 0
    for i in range(3):
        random.seed(7 + i)
        a = define_Dataset({**opt, "sigma": [0, 0]})[i]
        random.seed(7 + i)
        b = define_Dataset({**opt, "dataset_type": "sr"})[i]
        assert torch.equal(a["L"][:3], b["L"]) and torch.equal(a["H"], b["H"]) and (a["L"][3] == 0).all()
    # test phase: the whole image mod-cropped, the same bytes twice, the level sigma_test / 255
    tst = define_Dataset({**opt, "phase": "test", "sigma_test": 15})
    a, b = tst[1], tst[1]
    h, w = 38 // sf, 50 // sf
    assert a["H"].shape == (3, h * sf, w * sf) and a["L"].shape == (4, h, w)
    assert torch.equal(a["L"], b["L"]) and torch.equal(a["H"], b["H"])
    assert abs(a["L"][3, 0, 0].item() - 15 / 255) < 1e-7 and torch.equal(a["L"][3], a["L"][3, :1, :1].expand(h, w))
    clean = define_Dataset({**opt, "phase": "test"})[1]["L"]         # sigma_test 0 by default: no noise
    assert (clean[3] == 0).all() and torch.equal(clean[:3], define_Dataset({**opt, "dataset_type": "sr", "phase": "test"})[1]["L"])
    assert 10 / 255 < (a["L"][:3] - clean[:3]).std() < 20 / 255


def test_dataset_dpsr_refusals(png_dir):
    from kair_amd.data.select_dataset import define_Dataset
    for bad in ([50, 0], [-1, 5], 25):
        with pytest.raises(ValueError, match="sigma"):
            define_Dataset({"dataset_type": "dpsr", "dataroot_H": png_dir, "phase": "train", "sigma": bad})


# ---------------------------------------------------------------------------------------------------------------------
# PatchSynth(task="dpsr"): the host draws
# ---------------------------------------------------------------------------------------------------------------------
def test_dpsr_task_host_draws_are_reproducible():
    from kair_amd.data.gpu_synth import patch_draws
    N, HS, WS = 7, 81, 74
    mk = lambda **kw: patch_draws("dpsr", N, 3, HS, WS, **{"H_size": 32, "seed": 5, "scale": 4, **kw})
    d = mk(sigma=(5, 50))
    tabs = [d.draw(9) for _ in range(3)]
    for t, sf in tabs:
        assert t.dtype == torch.int32 and t.shape == (9, 8) and t.is_contiguous() and sf == 4
        assert ((t[:, 0] >= 0) & (t[:, 0] < N)).all() and ((t[:, 3] >= 0) & (t[:, 3] <= 7)).all()
        assert ((t[:, 1] >= 0) & (t[:, 1] <= 80 // 4 - 8) & (t[:, 2] >= 0) & (t[:, 2] <= 72 // 4 - 8)).all()
        lev = t[:, 4:5].view(torch.float32).flatten() * 255
        assert ((lev >= 5 - 1e-4) & (lev <= 50 + 1e-4)).all() and len(set(lev.tolist())) == 9
        assert (t[:, 5:] == 0).all()
    again = mk(sigma=(5, 50))
    assert all(torch.equal(again.draw(9)[0], t) for t, _ in tabs)
    assert not torch.equal(mk(sigma=(5, 50), seed=6).draw(9)[0], tabs[0][0])
    # the crops and modes are task "sr"'s under the same seed; sigma (0, 0) draws level 0
    sr = patch_draws("sr", N, 3, HS, WS, H_size=32, seed=5, scale=4)
    z = mk(sigma=(0, 0))
    for t, _ in tabs:
        assert torch.equal(t[:, :4], sr.draw(9)[0])
        assert (z.draw(9)[0][:, 4:] == 0).all()
    assert d.extra == 1 and (d.Hs, d.Ws) == (80, 72)
    for kw, frag in ((dict(scale=5), "scale 2, 3 or 4"), (dict(scale=3), "not divisible"), (dict(sigma=(9, 1)), "takes sigma"),
                     (dict(H_size=96), "larger than the pool")):
        with pytest.raises(ValueError, match=frag):
            mk(**kw)
