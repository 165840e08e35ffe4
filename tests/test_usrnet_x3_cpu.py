"""USRNet's arithmetic is an option-file decision (select_network.compute_dtype_of): 'fp32x3' on request, the
exact-fp32 engine by default, bf16 under amp_enabled."""
from kair_amd.models.select_network import compute_dtype_of


def test_usrnet_accepts_fp32x3():
    assert compute_dtype_of({"netG": {"net_type": "usrnet", "compute_dtype": "fp32x3"}}) == "fp32x3"
    assert compute_dtype_of({"netG": {"net_type": "usrnet", "compute_dtype": "fp32x3"},
                             "train": {"amp_enabled": True}}) == "fp32x3"


def test_usrnet_defaults_unchanged():
    assert compute_dtype_of({"netG": {"net_type": "usrnet"}}) == "fp32"
    assert compute_dtype_of({"netG": {"net_type": "usrnet"}, "train": {"amp_enabled": False}}) == "fp32"
    assert compute_dtype_of({"netG": {"net_type": "usrnet"}, "train": {"amp_enabled": True}}) == "bf16"
