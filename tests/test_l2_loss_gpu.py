"""kair_l2_loss (G_lossfn_type 'l2' / 'l2sum') on the MI355X against float64 torch on the CPU: value, gradient rows in
every layout of kair_l1_loss, pad slots, repeatability.

Inputs: torch.rand images, the first rows of H copied from E (exact zeros of d = E - H), dE prefilled with NaN (every
slot must be written).  Weights 1.0 and -0.5, reductions mean and sum.

Bars.
  fp32 gradient, per element: 4 * 2^-24 * |g64| -- three roundings (the difference, the scale constant 2 w / numel,
  the product), each 2^-24 relative, plus one for second-order terms; exactly 0 where d == 0.
  bf16 rows: the two checks of tests/test_kernels_gpu.py test_pixel_loss_bf16_rows.  Its L1 form, equality with the
  bf16 rounding of the fp32 gradient: here the fp32 gradient is fp32(E - H) * fp32(2 w / numel), two correctly rounded
  operations whatever computes them, so its bf16 rounding is the kernel's bit for bit.  Its Charbonnier form: within
  2^-8 of the largest gradient from the float64 gradient.
  Pad slots: exactly zero.
  Value: 4 x the largest error of torch's own fp32 CPU nn.MSELoss() against float64 over the six shapes (the factor
  covers a different but equally valid fp32 summation order), times |weight|, and times numel for the sum.  Measured
  when the module runs (value_bar), and was, when this was written (torch fp32 CPU vs float64, mean; the value):
      2x3x12x8   5.3e-9 (0.1356)    1x3x12x9   4.2e-9 (0.1266)    2x3x8x8   3.1e-10 (0.1014)    1x1x5x7   2.6e-9 (0.0889)
  so the bar is 4 x 5.3e-9 = 2.1e-8: 1.4 fp32 ulps of the two larger values, 2.8 of the two smaller.  The kernel's
  figures are in test_value_gradient_pad_and_repeat's docstring.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402

dev = torch.device("cuda")
U = 2.0 ** -24

CASES = [   # (shape, rows dtype, ldc, ps_r): the smallest that reach every kernel and index path
    ((2, 3, 12, 8), torch.float32, 4, 1),      # pixel-per-thread fp32 rows of 4
    ((2, 3, 12, 8), torch.bfloat16, 16, 1),    # pixel-per-thread bf16 rows of 16
    ((2, 3, 12, 8), torch.float32, 16, 2),     # generic
    ((1, 3, 12, 9), torch.bfloat16, 32, 3),    # generic
    ((2, 3, 8, 8), torch.bfloat16, 64, 4),     # generic
    ((1, 1, 5, 7), torch.float32, 8, 1),       # generic, fewer elements than one workgroup
]
SHAPES = sorted({c[0] for c in CASES})


@functools.lru_cache(maxsize=None)
def case(shape):
    """(E, H, d in float64, mean of d^2 in float64) of a shape: computed once, shared, never modified."""
    g = torch.Generator().manual_seed(300 + sum(shape))
    E = torch.rand(shape, generator=g)
    Ht = torch.rand(shape, generator=g)
    Ht[:, :, :2] = E[:, :, :2]   # exact zeros of d
    d = E.double() - Ht.double()
    return E, Ht, d, (d * d).mean().item()


@functools.lru_cache(maxsize=None)
def value_bar():
    """4 x the largest |torch fp32 CPU MSELoss - float64| over the shapes (weight 1, mean)."""
    worst = 0.0
    for shape in SHAPES:
        E, Ht, _, mean64 = case(shape)
        e = abs(torch.nn.MSELoss()(E, Ht).item() - mean64)
        print(f"fp32 torch MSELoss vs float64 {shape}: {e:.3g} (value {mean64:.6g})")
        worst = max(worst, e)
    assert worst > 0
    return 4 * worst


def run_kernel(E, Ht, weight, reduction, dtype, ldc, r):
    B, C, Hh, Ww = E.shape
    loss = torch.full((1,), float("nan"), device=dev)
    dE = torch.full((B * (Hh // r) * (Ww // r), ldc), float("nan"), device=dev, dtype=dtype)
    ws = torch.empty(1024, device=dev)
    H.l2_loss(E.to(dev), Ht.to(dev), loss, dE, ldc, weight, B, C, Hh, Ww, ws, ps_r=r, reduction=reduction)
    torch.cuda.synchronize()
    return loss.cpu(), dE.cpu()


def rows_to_nchw(dE, shape, ldc, r):
    """The rows layout [b][y/r][x/r][c r r + (y%r) r + x%r] back to [B, C, H, W], and the pad slots."""
    B, C, Hh, Ww = shape
    t = dE.view(B, Hh // r, Ww // r, ldc)
    used = t[..., :C * r * r].reshape(B, Hh // r, Ww // r, C, r, r)
    return used.permute(0, 3, 1, 4, 2, 5).reshape(B, C, Hh, Ww), t[..., C * r * r:]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("weight", [1.0, -0.5])
@pytest.mark.parametrize("shape,dtype,ldc,r", CASES)
def test_value_gradient_pad_and_repeat(shape, dtype, ldc, r, weight, reduction):
    """Measured on the MI355X, |value - float64| over |weight| (and over numel for the sum), the same for every rows
    layout of a shape and for both weights; the bar is 2.1e-8:
        shape       mean      sum
        2x3x12x8    5.3e-9    3.6e-9
        1x3x12x9    4.2e-9    1.8e-9
        2x3x8x8     7.1e-9    2.2e-9
        1x1x5x7     4.9e-9    5.1e-9
    fp32 gradients: at most 1.1 x 2^-24 |g64| per element for the mean (bar 4), exact for the sum (the constant 2 w is
    a power of two).  bf16 rows: equal to the bf16 rounding bit for bit; at most 0.8 of the 2^-8 bar from float64."""
    E, Ht, d, mean64 = case(shape)
    numel = d.numel()
    div = 1.0 if reduction == "sum" else float(numel)
    want = weight * mean64 * (numel / div)
    g64 = 2.0 * weight * d / div
    loss, dE = run_kernel(E, Ht, weight, reduction, dtype, ldc, r)
    bar_v = value_bar() * abs(weight) * (numel / div)
    ev = abs(loss.item() - want)
    print(f"l2 {reduction} {shape} w {weight}: value {loss.item():.8g} want {want:.8g} err {ev:.3g} bar {bar_v:.3g} "
          f"(per unit {ev / (abs(weight) * (numel / div)):.3g})")
    img, pad = rows_to_nchw(dE, shape, ldc, r)
    assert pad.numel() > 0 and (pad == 0).all()   # exactly zero, and written: the buffer started as NaN
    assert torch.isfinite(img.float()).all()
    zero = d == 0
    assert zero.any() and (img[zero] == 0).all()
    if dtype == torch.float32:
        err = (img.double() - g64).abs()
        ratio = (err[~zero] / g64[~zero].abs()).max().item() / U
        print(f"  fp32 rows ldc {ldc} r {r}: worst gradient error {ratio:.3g} x 2^-24 |g64| (bar 4)")
        assert (err <= 4 * U * g64.abs()).all()
    else:
        gs32 = torch.tensor(np.float32(2.0 * weight / div))
        ref32 = (E - Ht) * gs32                 # fp32(E - H) * fp32(2 w / numel): the kernel's two operations
        mx = g64.abs().max().item()
        e0 = (img.double() - g64).abs().max().item()
        print(f"  bf16 rows ldc {ldc} r {r}: vs float64 {e0:.3g} (bar {2 ** -8 * mx:.3g}), bits equal "
              f"{torch.equal(img.float(), ref32.bfloat16().float())}")
        assert torch.equal(img.float(), ref32.bfloat16().float())
        assert e0 <= 2 ** -8 * mx
    assert ev <= bar_v
    # a second call on fresh buffers: bit-identical (fixed-order sums, no atomics)
    loss2, dE2 = run_kernel(E, Ht, weight, reduction, dtype, ldc, r)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    assert torch.equal(dE.view(bits), dE2.view(bits))


def test_sum_is_numel_times_mean_and_wrapper_errors():
    """The two reductions on the same inputs: the sum is numel x the mean to the fp32 roundings of the two scale
    constants and final products (4 x 2^-24 relative: both run the same partial sums); a bad reduction name, a short
    r and a null-sized call raise before any launch."""
    shape, dtype, ldc, r = CASES[0]
    E, Ht, d, _ = case(shape)
    lm, gm = run_kernel(E, Ht, 1.0, "mean", dtype, ldc, r)
    ls, gs = run_kernel(E, Ht, 1.0, "sum", dtype, ldc, r)
    n = d.numel()
    assert abs(ls.item() - n * lm.item()) <= 4 * U * abs(ls.item())
    assert ((gs.double() - n * gm.double()).abs() <= 4 * U * gs.double().abs()).all()
    B, C, Hh, Ww = shape
    loss, dE, ws = torch.full((1,), 7.0, device=dev), torch.full((B * Hh * Ww, ldc), 7.0, device=dev), torch.empty(1024, device=dev)
    with pytest.raises(ValueError):
        H.l2_loss(E.to(dev), Ht.to(dev), loss, dE, ldc, 1.0, B, C, Hh, Ww, ws, reduction="none")
    with pytest.raises(RuntimeError, match="l2_loss"):
        H.l2_loss(E.to(dev), Ht.to(dev), loss, dE, ldc, 1.0, B, C, Hh, Ww, ws, ps_r=5)
    with pytest.raises(RuntimeError, match="l2_loss"):
        H.l2_loss(E.to(dev), Ht.to(dev), loss, dE, ldc, 1.0, B, C, Hh, Ww, None)
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and (dE == 7.0).all()


def test_l1_and_charbonnier_are_what_they_were():
    """The mode parameter left the other two arithmetics alone: L1 gradients are +-w / numel or 0 exactly and the loss
    is the fp32 mean; Charbonnier against float64 (the form of test_pixel_loss_bf16_rows)."""
    shape = (2, 3, 12, 8)
    E, Ht, d, _ = case(shape)
    B, C, Hh, Ww = shape
    for eps in (None, 1e-3):
        loss = torch.empty(1, device=dev)
        dE = torch.full((B * Hh * Ww, 4), float("nan"), device=dev)
        H.l1_loss(E.to(dev), Ht.to(dev), loss, dE, 4, 1.0, B, C, Hh, Ww, torch.empty(1024, device=dev), charb_eps=eps)
        img, pad = rows_to_nchw(dE.cpu(), shape, 4, 1)
        assert (pad == 0).all()
        if eps is None:
            assert torch.equal(img, torch.sign(d).float() * np.float32(1.0 / d.numel()))
            assert abs(loss.item() - d.abs().mean().item()) <= 4 * U * math.sqrt(d.numel())
        else:
            q = torch.sqrt(d * d + eps)
            assert abs(loss.item() - q.mean().item()) <= 1e-6 * q.mean().item()
            assert ((img.double() - d / q / d.numel()).abs().max() <= 1e-6 / d.numel())
