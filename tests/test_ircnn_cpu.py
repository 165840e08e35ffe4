"""IRCNN without a GPU: the module tree (restated from upstream cszn/KAIR's network_dncnn.py), define_G, the host
forward, the model-bank index and loader, and the option file."""
import os

import pytest
import torch
import torch.nn as nn

from kair_amd.models.network_dncnn import IRCNN, IRCNN_DILATIONS
from kair_amd.models.select_network import compute_dtype_of, define_G
from kair_amd.utils import utils_model, utils_option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_tree_keys_shapes_and_parameter_counts():
    net = IRCNN()
    sd = net.state_dict()
    assert list(sd) == [f"model.{i}.{p}" for i in range(0, 13, 2) for p in ("weight", "bias")]
    assert tuple(sd["model.0.weight"].shape) == (64, 1, 3, 3) and tuple(sd["model.12.weight"].shape) == (1, 64, 3, 3)
    assert all(tuple(sd[f"model.{i}.weight"].shape) == (64, 64, 3, 3) for i in range(2, 12, 2))
    convs = [m for m in net.model if isinstance(m, nn.Conv2d)]
    assert [c.dilation for c in convs] == [(d, d) for d in IRCNN_DILATIONS] == [c.padding for c in convs]
    assert IRCNN_DILATIONS == (1, 2, 3, 4, 3, 2, 1)
    assert not any(isinstance(m, nn.BatchNorm2d) for m in net.model)
    assert sum(p.numel() for p in net.parameters()) == 185857
    assert sum(p.numel() for p in IRCNN(3, 3).parameters()) == 188163
    assert net.compute_dtype == "fp32"


def _opt(**kw):
    o = {"netG": {"net_type": "ircnn", "in_nc": 3, "out_nc": 3, "nc": 32}, "is_train": False}
    o.update(kw)
    return o


def test_define_g_and_compute_dtype():
    net = define_G(_opt())
    assert type(net) is IRCNN and net.compute_dtype == "fp32"
    assert tuple(net.model[0].weight.shape) == (32, 3, 3, 3) and tuple(net.model[12].weight.shape) == (3, 32, 3, 3)
    assert compute_dtype_of(_opt()) == "fp32"
    assert compute_dtype_of(_opt(train={"amp_enabled": True})) == "bf16"
    assert define_G(_opt(train={"amp_enabled": True})).compute_dtype == "bf16"
    bad = _opt()
    bad["netG"]["compute_dtype"] = "fp32x3"
    with pytest.raises(ValueError, match="fp32x3"):
        define_G(bad)
    assert net.set_dil_kernel(False) is net and net.dil_kernel is False


def test_cpu_forward_is_x_minus_sequential():
    torch.manual_seed(3)
    net = IRCNN(3, 3, 16).eval()
    seq = nn.Sequential(*[nn.Conv2d(m.in_channels, m.out_channels, 3, 1, m.padding, m.dilation) if isinstance(m, nn.Conv2d)
                          else nn.ReLU() for m in net.model])
    seq.load_state_dict({k[len("model."):]: v for k, v in net.state_dict().items()})
    x = torch.rand(2, 3, 11, 9)
    with torch.no_grad():
        assert torch.equal(net(x), x - seq(x))


def test_ircnn_index():
    assert [utils_model.ircnn_index(s) for s in (0, 1, 2, 3, 25, 48, 49, 50, 75)] == [0, 0, 0, 1, 12, 23, 24, 24, 24]
    assert utils_model.ircnn_index(2.0001) == 1 and utils_model.ircnn_index(7.65) == 3


def test_bank_loader_layouts_and_errors(tmp_path):
    sds = {str(i): IRCNN(1, 1, 16).state_dict() for i in range(25)}
    torch.save(sds, tmp_path / "bank.pth")
    bank = utils_model.load_ircnn_bank(str(tmp_path / "bank.pth"))
    assert sorted(bank) == list(range(25)) and torch.equal(bank[7]["model.4.bias"], sds["7"]["model.4.bias"])
    torch.save(sds["3"], tmp_path / "one.pth")
    one = utils_model.load_ircnn_bank(str(tmp_path / "one.pth"))
    assert list(one) == [0] and torch.equal(one[0]["model.0.weight"], sds["3"]["model.0.weight"])
    assert utils_model.load_ircnn_bank(sds).keys() == bank.keys()             # an already loaded object
    wrong = {k: dict(v) for k, v in sds.items()}
    wrong["5"]["model.6.weight"] = torch.zeros(16, 16, 5, 5)
    with pytest.raises(ValueError, match=r"entry 5.*model\.6\.weight.*\(16, 16, 5, 5\)"):
        utils_model.load_ircnn_bank(wrong)
    missing = {k: dict(v) for k, v in sds.items()}
    del missing["2"]["model.12.bias"]
    with pytest.raises(ValueError, match=r"model\.12\.bias"):
        utils_model.load_ircnn_bank(missing)
    with pytest.raises(ValueError, match="'25'|25"):
        utils_model.load_ircnn_bank({**sds, "25": sds["0"]})
    mixed = {**sds, "4": IRCNN(1, 1, 32).state_dict()}
    with pytest.raises(ValueError, match="different widths"):
        utils_model.load_ircnn_bank(mixed)


def test_bank_select_loads_only_on_index_change():
    torch.manual_seed(5)
    bank = {i: IRCNN(1, 1, 8).state_dict() for i in range(3)}
    net = IRCNN(1, 1, 8)
    b = utils_model.IRCNNBank(net, bank)
    assert b.select(2) is net and b.current == 0
    v0 = net.model[0].weight._version
    b.select(1.5)
    assert net.model[0].weight._version == v0                                   # same entry: nothing copied
    b.select(5)
    assert b.current == 2 and net.model[0].weight._version > v0
    assert torch.equal(net.model[4].weight, bank[2]["model.4.weight"])
    assert b.index(50) == 2                                                    # a short bank: the nearest entry below


def test_train_option_file_parses():
    opt = utils_option.parse(os.path.join(ROOT, "options", "train_ircnn.json"), is_train=True)
    assert opt["model"] == "plain" and opt["netG"]["net_type"] == "ircnn" and opt["n_channels"] == 1
    assert (opt["netG"]["in_nc"], opt["netG"]["out_nc"], opt["netG"]["nc"]) == (1, 1, 64)
    tr = opt["datasets"]["train"]
    assert (tr["dataset_type"], tr["sigma"], tr["H_size"]) == ("dncnn", 25, 40)
    assert opt["train"]["G_lossfn_type"] == "l1"
    net = define_G(opt)
    assert type(net) is IRCNN and net.compute_dtype == "fp32"


def test_denoiser_driver_on_the_host(tmp_path):
    """main_test_ircnn_denoiser end to end with --device cpu (the module list): images of two sizes, a 25-entry bank,
    AWGN from the fixed seed, PSNR reported, outputs written."""
    from kair_amd import main_test_ircnn_denoiser as drv
    from kair_amd.utils import utils_image as util
    torch.manual_seed(7)
    sds = {str(i): IRCNN(1, 1, 8).state_dict() for i in range(25)}
    for sd in sds.values():
        sd["model.12.weight"].mul_(0.01)
    torch.save(sds, tmp_path / "ircnn_gray.pth")
    (tmp_path / "in").mkdir()
    for name, (h, w) in (("a", (21, 17)), ("b", (16, 30))):
        util.imsave((torch.rand(h, w, 1) * 255).byte().numpy(), str(tmp_path / "in" / f"{name}.png"))
    args = ["--model_path", str(tmp_path / "ircnn_gray.pth"), "--input", str(tmp_path / "in"), "--noise_level", "25",
            "--n_channels", "1", "--output", str(tmp_path / "out"), "--device", "cpu"]
    res = drv.main(args)
    assert [n for n, _ in res] == ["a", "b"] and all(10 < p < 40 for _, p in res)
    assert sorted(os.listdir(tmp_path / "out")) == ["a_ircnn.png", "b_ircnn.png"]
    assert drv.main(args) == res                                              # the fixed seed
    assert [p for _, p in drv.main(args[:4] + ["--noise_level", "0"] + args[6:] + ["--x8"])] == [None, None]
    with pytest.raises(ValueError, match="channels"):
        drv.main(args[:6] + ["--n_channels", "3"] + args[8:])
