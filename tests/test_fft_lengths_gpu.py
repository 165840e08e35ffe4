"""Line DFTs of any length 2 <= n <= 2048 (csrc/fft.hip): radix 5 / 7 butterflies, the generic prime-radix stage and
the per-stage-radix plan, through the USRNet data-step kernels on HR grids that are not 2^a 3^b.

The float64 side is oracle/convnets.py (p2o, splits, datanet, zero_upsample); `rel` and the bars are those of
tests/test_usrnet_gpu.py: FB and invW within 2e-6, the forward data step within 2e-5, dL/dx within 5e-5 and dL/dalpha
within 1e-4.  The PSF is the largest odd square up to 13 that fits the grid (p2o needs kh <= H, kw <= W).

Paths: (10, 14) radix 2.5 / 2.7; (35, 25) 5.7 / 5.5; (45, 28) 3.3.5 / 4.7; (11, 13) generic primes alone;
(121, 49) a repeated generic prime / 7.7; (210, 330) 2.3.5.7 / 2.3.5.11; (481, 321) = 13.37 x 3.107, the BSD68 size, odd H
(one row per CTA); (509, 6), (6, 2039), (2047 = 23.89, 4): prime and near-2048 lines, one O(n^2) stage; sf 2 / 3 / 4 alias
groups on (70, 22), (75, 51), (44, 52).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from oracle import convnets as ocv  # noqa: E402

dev = torch.device("cuda")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def untranspose(t, planes, Hh, Ww):
    """kernel layout float2 [planes][W][H] -> complex128 [planes, H, W] on the CPU"""
    return torch.view_as_complex(t.view(planes, Ww, Hh, 2).double().cpu().contiguous()).transpose(-1, -2)


def fb_gpu(k, Hh, Ww, sf):
    B = k.shape[0]
    FB = torch.empty(B * Hh * Ww * 2, device=dev)
    invW = torch.empty(B * (Hh // sf) * (Ww // sf), device=dev)
    kd = k.float().to(dev).contiguous()
    H.usr_fft_rows(kd, H.USR_SRC_PSF, 1, 0, k.shape[-2], k.shape[-1], 1, FB, B, Hh, Ww)
    H.usr_fft_cols(H.USR_COL_FB, FB, FB, None, None, None, invW, None, 0, None, B, 1, Hh, Ww, sf)
    return FB, invW


def fbfy_gpu(FB, invW, y, sf):
    B, C, h, w = y.shape
    Hh, Ww = h * sf, w * sf
    FBFy = torch.empty(B * C * Hh * Ww * 2, device=dev)
    H.usr_fft_rows(y.float().to(dev).contiguous(), H.USR_SRC_ZUP, C, 0, 0, 0, sf, FBFy, B * C, Hh, Ww)
    H.usr_fft_cols(H.USR_COL_FBFY, FBFy, FBFy, FB, None, None, invW, None, 0, None, B * C, C, Hh, Ww, sf)
    return FBFy


def rand_kernel(B, Hh, Ww, g):
    n = min(13, Hh, Ww)
    n -= 1 - n % 2
    k = torch.rand(B, 1, n, n, generator=g, dtype=torch.float64)
    return k / k.sum((-2, -1), keepdim=True)


FB_CASES = [(10, 14, 1), (35, 25, 1), (45, 28, 1), (11, 13, 1), (121, 49, 1), (210, 330, 1), (481, 321, 1), (509, 6, 1),
            (6, 2039, 1), (2047, 4, 1), (70, 22, 2), (75, 51, 3), (44, 52, 4)]


@pytest.mark.parametrize("Hh,Ww,sf", FB_CASES)
def test_fb_and_alias_mean_vs_float64(Hh, Ww, sf):
    """FB = p2o(k) and invW = mean(splits(|FB|^2, sf)) vs float64 torch.fft, at test_p2o_and_alias_mean_vs_torch's bar."""
    g = torch.Generator().manual_seed(Hh + Ww + sf)
    k = rand_kernel(2, Hh, Ww, g)
    FB, invW = fb_gpu(k, Hh, Ww, sf)
    ref = ocv.p2o(k, (Hh, Ww))
    e_fb = rel(torch.view_as_real(untranspose(FB, 2, Hh, Ww)), torch.view_as_real(ref[:, 0]))
    ref_w = ocv.splits(torch.abs(ref) ** 2, sf).mean(-1)
    got_w = invW.view(2, Ww // sf, Hh // sf).transpose(-1, -2).cpu().double()
    e_w = rel(got_w, ref_w[:, 0])
    print(f"fft lengths ({Hh}, {Ww}, sf {sf}): FB rel {e_fb:.3e}, invW rel {e_w:.3e}")
    assert e_fb < 2e-6
    assert e_w < 2e-6


@pytest.mark.parametrize("Hh,Ww,sf", [(35, 26, 1), (70, 22, 2), (75, 51, 3), (52, 44, 4)])
def test_data_step_forward_backward_vs_float64(Hh, Ww, sf):
    """The closed-form step, dL/dx and dL/dalpha vs float64 autograd through the oracle (B 2, C 3), at
    test_datanet_backward_vs_autograd's bars."""
    g = torch.Generator().manual_seed(7 * Hh + sf)
    B, C = 2, 3
    k = rand_kernel(B, Hh, Ww, g)
    y = torch.rand(B, C, Hh // sf, Ww // sf, generator=g, dtype=torch.float64)
    x = torch.rand(B, C, Hh, Ww, generator=g, dtype=torch.float64, requires_grad=True)
    alpha = (torch.rand(B, 1, 1, 1, generator=g, dtype=torch.float64) * 0.2 + 0.01).requires_grad_(True)
    gz = torch.randn(B, C, Hh, Ww, generator=g, dtype=torch.float64)
    FBr = ocv.p2o(k, (Hh, Ww))
    FBFyr = torch.conj(FBr) * torch.fft.fftn(ocv.zero_upsample(y, sf), dim=(-2, -1))
    zr = ocv.datanet(x, FBr, torch.conj(FBr), torch.abs(FBr) ** 2, FBFyr, alpha, sf)
    zr.backward(gz)
    FB, invW = fb_gpu(k, Hh, Ww, sf)
    FBFy = fbfy_gpu(FB, invW, y, sf)
    FR = torch.empty(B * C * Hh * Ww * 2, device=dev)
    al = alpha.detach().view(B).float().to(dev)
    T = torch.empty_like(FR)
    zg = torch.empty(B, C, Hh, Ww, device=dev)
    H.usr_fft_rows(x.detach().float().to(dev).contiguous(), H.USR_SRC_NCHW, C, 0, 0, 0, 1, T, B * C, Hh, Ww)
    H.usr_fft_cols(H.USR_COL_DATA_FWD, T, T, FB, FBFy, FR, invW, al, 1, None, B * C, C, Hh, Ww, sf)
    H.usr_ifft_rows(T, zg, False, C, 0, 1.0 / (Hh * Ww), B * C, Hh, Ww)
    # backward: rows of dL/dz (NHWC source, ld 8) -> closed-form adjoint -> inverse rows
    gx_nhwc = torch.zeros(B, Hh, Ww, 8, device=dev)
    gx_nhwc[..., :C] = gz.permute(0, 2, 3, 1).float().to(dev)
    part = torch.empty(B * C * (Ww // sf), device=dev)
    gal = torch.empty(B, device=dev)
    H.usr_fft_rows(gx_nhwc, H.USR_SRC_NHWC, C, 8, 0, 0, 1, T, B * C, Hh, Ww)
    H.usr_fft_cols(H.USR_COL_DATA_BWD, T, T, FB, FBFy, FR, invW, al, 1, part, B * C, C, Hh, Ww, sf)
    H.usr_seg_sum(part, C * (Ww // sf), B, 1.0 / (Hh * Ww), gal, 1)
    gx = torch.empty(B, C, Hh, Ww, device=dev)
    H.usr_ifft_rows(T, gx, False, C, 0, 1.0 / (Hh * Ww), B * C, Hh, Ww)
    e_z, e_x, e_a = rel(zg, zr), rel(gx, x.grad), rel(gal, alpha.grad.view(B))
    print(f"data step ({Hh}, {Ww}, sf {sf}): z rel {e_z:.3e}, dL/dx rel {e_x:.3e}, dL/dalpha rel {e_a:.3e}")
    assert e_z < 2e-5
    assert e_x < 5e-5
    assert e_a < 1e-4


@pytest.mark.parametrize("Hh,Ww,sf", [(64, 48, 2), (96, 96, 3)])
def test_old_lengths_are_deterministic(Hh, Ww, sf):
    """The FB bytes of two 2^a 3^b grids: a call, a second call and a call on another stream agree bit for bit.  (That
    they are also the bytes the radix-4/2/3-only plan gave was checked once, by hand, against the parent commit.)"""
    g = torch.Generator().manual_seed(5)
    k = torch.rand(2, 1, 25, 25, generator=g, dtype=torch.float64)
    k = k / k.sum((-2, -1), keepdim=True)
    FB1, W1 = fb_gpu(k, Hh, Ww, sf)
    FB2, W2 = fb_gpu(k, Hh, Ww, sf)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FB3, W3 = fb_gpu(k, Hh, Ww, sf)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in ((FB1, FB2), (FB1, FB3), (W1, W2), (W1, W3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("Hh,Ww", [(2049, 8), (8, 2049), (1, 8), (8, 1)])
def test_out_of_range_lengths_are_argument_errors(Hh, Ww):
    """Length 2049 and a length-1 axis are still KAIR_ERR_ARG (-1): the forward rows pass checks both axes, the columns
    pass the axis it transforms (H), the inverse rows pass W."""
    k = torch.full((1, 1, 1, 1), 1.0, device=dev)
    T = torch.empty(Hh * Ww * 2, device=dev)
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        H.usr_fft_rows(k, H.USR_SRC_PSF, 1, 0, 1, 1, 1, T, 1, Hh, Ww)
    if Hh in (1, 2049):
        invW = torch.empty(Hh * Ww, device=dev)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            H.usr_fft_cols(H.USR_COL_FB, T, T, None, None, None, invW, None, 0, None, 1, 1, Hh, Ww, 1)
    else:
        z = torch.empty(1, 1, Hh, Ww, device=dev)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            H.usr_ifft_rows(T, z, False, 1, 0, 1.0, 1, Hh, Ww)
