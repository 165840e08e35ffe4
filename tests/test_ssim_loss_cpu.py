"""SSIMLoss (G_lossfn_type 'ssim') on the host: the plain-torch form that is the reference of tests/test_ssim_loss_gpu.py,
against a direct float64 numpy restatement, under gradcheck, and through define_Model's autograd path.
"""
import numpy as np
import torch

from kair_amd.models.model_plain import SSIMLoss
from kair_amd.utils.utils_image import _gauss_window


def numpy_ssim(x, y):
    """mean SSIM by the definition: every pixel's 11 x 11 zero-padded Gaussian window, float64, no torch."""
    w = _gauss_window()
    B, C, H, W = x.shape
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    xp = np.pad(x, ((0, 0), (0, 0), (5, 5), (5, 5)))
    yp = np.pad(y, ((0, 0), (0, 0), (5, 5), (5, 5)))
    S = np.empty_like(x)
    for i in range(H):
        for j in range(W):
            a, b = xp[:, :, i:i + 11, j:j + 11], yp[:, :, i:i + 11, j:j + 11]
            m1, m2 = (a * w).sum((2, 3)), (b * w).sum((2, 3))
            s11, s22 = (a * a * w).sum((2, 3)) - m1 * m1, (b * b * w).sum((2, 3)) - m2 * m2
            s12 = (a * b * w).sum((2, 3)) - m1 * m2
            S[:, :, i, j] = (2 * m1 * m2 + C1) * (2 * s12 + C2) / ((m1 * m1 + m2 * m2 + C1) * (s11 + s22 + C2))
    return S.mean()


def test_identity_symmetry_and_numpy_value():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 13, 17, generator=g, dtype=torch.float64)
    y = (x + 0.2 * (torch.rand(2, 3, 13, 17, generator=g, dtype=torch.float64) - 0.5)).clamp(0, 1)
    loss = SSIMLoss()
    assert abs(loss(x, x).item() - 1.0) < 1e-12
    assert abs(loss(x.float(), x.float()).item() - 1.0) < 1e-5
    v = loss(x, y).item()
    assert 0.0 < v < 1.0
    assert abs(v - loss(y, x).item()) < 1e-14
    assert abs(v - numpy_ssim(x.numpy(), y.numpy())) < 1e-13


def test_gradcheck_float64():
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 2, 9, 12, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.rand(1, 2, 9, 12, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(SSIMLoss(), (x, y), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_define_model_ssim_trains_on_the_cpu(tmp_path):
    """G_lossfn_type 'ssim' with weight -1 (the SSIM itself is returned, so maximising it takes a negative weight):
    the autograd path on the host, G_loss in [-1, 0) and moving toward -1 on a fixed batch."""
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = dict_to_nonedict({
        "model": "plain", "gpu_ids": None, "is_train": True, "dist": False, "scale": 1,
        "path": {"models": str(tmp_path), "pretrained_netG": None},
        "netG": {"net_type": "dncnn", "in_nc": 1, "out_nc": 1, "nc": 16, "nb": 3, "act_mode": "R", "init_type": "default"},
        "train": {"G_lossfn_type": "ssim", "G_lossfn_weight": -1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-3,
                  "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_scheduler_type": "MultiStepLR",
                  "G_scheduler_milestones": [100], "G_scheduler_gamma": 0.5, "E_decay": 0, "G_param_strict": True,
                  "G_optimizer_reuse": False}})
    torch.manual_seed(5)
    m = define_Model(opt)
    m.init_train()
    assert m.trainer is None
    g = torch.Generator().manual_seed(6)
    yy, xx = torch.linspace(0, 1, 20).view(1, 1, 20, 1), torch.linspace(0, 1, 24).view(1, 1, 1, 24)
    Hh = (0.2 + 0.3 * yy + 0.3 * xx + 0.05 * torch.rand(2, 1, 20, 24, generator=g)).clamp(0, 1)
    L = (Hh + 0.1 * torch.randn(2, 1, 20, 24, generator=g)).clamp(0, 1)
    losses = []
    for step in range(1, 7):
        m.feed_data({"L": L, "H": Hh})
        m.optimize_parameters(step)
        losses.append(m.current_log()["G_loss"])
        assert -1.0 <= losses[-1] < 0.0, losses
    assert losses[1] != losses[0]
    assert losses[-1] < losses[0], losses   # toward -1
    m.test()
    assert m.current_visuals()["E"].shape == (1, 20, 24)
