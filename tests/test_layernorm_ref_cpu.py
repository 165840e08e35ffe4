"""tests/layernorm_ref.py against torch itself: the closed-form LayerNorm backward against autograd through
torch.nn.functional.layer_norm in float64, and window_rows against the oracle's roll + window partition of a data
image (oracle/swinir.py, the CPU restatement of network_swinir.py the whole-network tests trust)."""
import pytest
import torch

import layernorm_ref as R
from oracle import swinir as osw


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("C", [30, 60, 180])
def test_closed_form_matches_autograd(C):
    g = torch.Generator().manual_seed(C)
    M, eps = 257, 1e-5
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    y = torch.nn.functional.layer_norm(x, (C,), gamma, beta, eps)
    y.backward(dy)
    yr, mean, rstd = R.ln_fwd(x.detach(), gamma.detach(), beta.detach(), eps)
    dx, dgamma, dbeta = R.ln_bwd(x.detach(), dy, gamma.detach(), eps)
    assert _rel(yr, y.detach()) < 1e-12
    assert _rel(mean, x.detach().mean(1)) < 1e-12
    assert _rel(rstd, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + eps)) < 1e-12
    assert _rel(dx, x.grad) < 1e-12
    assert _rel(dgamma, gamma.grad) < 1e-12
    assert _rel(dbeta, beta.grad) < 1e-12
    assert all(t.dtype == torch.float64 for t in (yr, mean, rstd, dx, dgamma, dbeta))


def test_reference_takes_fp32_inputs_in_float64():
    """fp32 (or bf16-rounded) kernel inputs are widened, never computed on in their own precision."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 30, generator=g)
    gamma, beta, dy = torch.rand(30, generator=g), torch.randn(30, generator=g), torch.randn(9, 30, generator=g)
    y, _, _ = R.ln_fwd(x, gamma, beta, 1e-5)
    y64, _, _ = R.ln_fwd(x.double(), gamma.double(), beta.double(), 1e-5)
    assert y.dtype == torch.float64 and torch.equal(y, y64)
    dx, dg, db = R.ln_bwd(x, dy.bfloat16(), gamma, 1e-5)
    dx64, dg64, db64 = R.ln_bwd(x.double(), dy.bfloat16().double(), gamma.double(), 1e-5)
    assert torch.equal(dx, dx64) and torch.equal(dg, dg64) and torch.equal(db, db64)


@pytest.mark.parametrize("B,H,W,ws,shift", [(2, 16, 24, 8, 4), (2, 14, 21, 7, 3)])
def test_window_rows_is_roll_then_partition(B, H, W, ws, shift):
    g = torch.Generator().manual_seed(ws)
    C = 5
    img = torch.randn(B, H, W, C, generator=g)
    tok = img.reshape(B * H * W, C)
    for s in (0, shift):
        rows = R.window_rows(B, H, W, ws, s)
        assert rows.dtype == torch.long and rows.shape == (B * H * W,)
        assert torch.equal(torch.sort(rows)[0], torch.arange(B * H * W))   # a permutation
        rolled = torch.roll(img, (-s, -s), (1, 2)) if s else img
        assert torch.equal(tok[rows], osw.to_windows(rolled, ws).reshape(-1, C))
    assert not torch.equal(R.window_rows(B, H, W, ws, 0), R.window_rows(B, H, W, ws, shift))
    # the first window of the shifted map starts at pixel (shift, shift) of image 0 and runs along a row
    rows = R.window_rows(B, H, W, ws, shift)
    assert rows[0].item() == shift * W + shift and rows[1].item() == shift * W + shift + 1
    assert rows[ws].item() == (shift + 1) * W + shift
