"""kair_conv3x3_wr_x3 (csrc/conv_wr.hip): the halo-resident, register-streamed-weight 3x3 conv in the fp16-pair
("fp32x3") arithmetic -- the fp32x3 engine's 192 -> 192 convs (RSTB.conv / conv_after_body) and their input
gradients -- and its weight packs (kinds 22 / 23).

Kernel results against torch.nn.functional.conv2d in float64 on the CPU, and against the x3 NT-ring im2col GEMM
of the same call, at the bar and norm of the kernel-level tests of tests/test_x3_gpu.py (2e-6, relative in the
Frobenius norm).  Geometries: the tile query gives 48-pixel tiles to small problems wherever 48 pixels fit the row
geometry, so the 96-pixel tile is reached with W = 32 (three-row tiles; 48 % 32 != 0) and at the classical x4
per-image grid with a full round of tiles (B = 8, 48 x 48: 192 two-row tiles)."""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.swinir_engine import SwinIREngine  # noqa: E402

dev = torch.device("cuda")
C, Cp = 180, 192

# (B, H, W) -> tile: two-row 48-pixel tiles with top / bottom halo rows and a batch seam; one 96-pixel row in two
# pieces; W < 48; three-row 96-pixel tiles; the engine's geometry (two-row 96-pixel tiles, more tiles than one
# workgroup round would need at small CU counts)
GEOMS = [((2, 6, 24), 48), ((2, 6, 48), 48), ((2, 3, 96), 48), ((2, 6, 32), 96), ((8, 48, 48), 96)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _weight(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, C, 3, 3, generator=g) * 0.05, torch.randn(C, generator=g) * 0.1


def _pack(w, kind, n_elems, dtype=torch.float16):
    out = torch.full((n_elems,), float("nan"), device=dev, dtype=dtype)
    H.pack_weight(w.to(dev), out, H.wmap(kind, C, C, (1, C, Cp), (1, C, Cp)))
    return out


def _padded_rows(t):
    """[M, C] -> fp32 rows [M, Cp], pad columns zero."""
    out = torch.zeros(t.shape[0], Cp)
    out[:, :C] = t
    return out


def _nchw64(rows, B, Hh, Ww):
    return rows[:, :C].double().view(B, Hh, Ww, C).permute(0, 3, 1, 2).contiguous()


def _rows_of(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, C)


@pytest.mark.parametrize("kind", [22, 23])
def test_pack_kinds_22_23(kind):
    """De-interleave [rows / 16][9 * 192 / 32][2][64 lanes][8] (lane l: row 16 rb + l % 16, k 32 kb + 8 (l / 16) + j):
    hi + lo = w 2^KAIR_X3_WEXP to 2^-22 (relative, Frobenius norm: each fp16 half keeps 11 bits), pads exactly zero.
    Kind 22: rows = output channels, k = tap * Cip + ci; kind 23: rows = input channels, k = tap * Cop + co."""
    w, _ = _weight(5)
    sp = _pack(w, kind, 2 * Cp * 9 * Cp)
    torch.cuda.synchronize()
    s = sp.double().cpu().view(Cp // 16, 9 * Cp // 32, 2, 4, 16, 8)   # [rb][kb][half][l / 16][l % 16][j]
    assert torch.isfinite(s).all()
    recon = (s[:, :, 0] + s[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(Cp, 9, Cp)   # [row][tap][col]
    wt = w.double().view(C, C, 9) * 2.0 ** H.X3_WEXP                               # [co][ci][tap]
    want = wt.permute(0, 2, 1) if kind == 22 else wt.permute(1, 2, 0)              # [row][tap][col]
    assert rel(recon[:C, :, :C], want) < 2.0 ** -22
    hi = s[:, :, 0].permute(0, 3, 1, 2, 4).reshape(Cp, 9, Cp)
    assert (hi[:C, :, :C] == want.to(torch.float16).double()).all()   # hi is the rounded value itself
    assert (recon[C:] == 0).all() and (recon[:, :, C:] == 0).all()


@pytest.mark.parametrize("geom,tile", GEOMS)
def test_conv_wr_x3_forward(geom, tile):
    """Forward with bias and residual on fp32 rows (Cp = 192 holding 180 channels) vs float64 and vs the NT ring."""
    B, Hh, Ww = geom
    M = B * Hh * Ww
    assert H.conv3x3_wr_x3_tile(B, Hh, Ww, Cp, Cp) == tile
    g = torch.Generator().manual_seed(7)
    w, b = _weight(6)
    x, r = _padded_rows(torch.randn(M, C, generator=g)), _padded_rows(torch.randn(M, C, generator=g))
    bp = torch.zeros(Cp)
    bp[:C] = b
    xd, rd, bd = x.to(dev), r.to(dev), bp.to(dev)
    out = torch.full((M, Cp), float("nan"), device=dev)
    H.conv3x3_wr_x3(xd, Cp, 4, 0, _pack(w, 22, 2 * Cp * 9 * Cp), bd, rd, out, B, Hh, Ww, Cp, Cp)
    ring = torch.full((M, Cp), float("nan"), device=dev)
    Wf = _pack(w, 9, Cp * 2 * 9 * Cp).view(Cp, -1)
    A, Bo = H.im2col(xd, Hh, Ww, Cp), H.rows(Wf, w_split=True)
    A.x3_exp, Bo.x3_exp = 4, H.X3_WEXP
    H.gemm_nt(A, Bo, H.epilogue(ring, bias=bd, resid=rd), M, Cp, 9 * Cp, H.X3)
    ref = torch.nn.functional.conv2d(_nchw64(x, B, Hh, Ww), w.double(), b.double(), padding=1)
    ref = _rows_of(ref) + r[:, :C].double()
    torch.cuda.synchronize()
    e_ref, e_ring = rel(out[:, :C], ref), rel(out[:, :C], ring[:, :C])
    print(f"forward {geom}: vs float64 {e_ref:.2e}, vs ring {e_ring:.2e}, ring vs float64 {rel(ring[:, :C], ref):.2e}")
    assert e_ref < 2e-6 and e_ring < 2e-6
    assert torch.equal(out[:, C:].cpu(), r[:, C:])   # pad columns: zero weights and bias, the residual's pads


@pytest.mark.parametrize("backoff", [0, 6])
@pytest.mark.parametrize("geom,tile", [GEOMS[1], GEOMS[3], GEOMS[4]])
def test_conv_wr_x3_input_gradient(geom, tile, backoff):
    """The flipped form on a gradient image of ~1e-6 values at the exponent the engine picks for that loss
    normalisation (_x3_grad_exp, 24 here), and lowered by 6 as after a range back-off, vs float64 autograd."""
    B, Hh, Ww = geom
    M = B * Hh * Ww
    e_g = SwinIREngine._x3_grad_exp(types.SimpleNamespace(x3_gexp_off=4), 10 ** 6) - backoff
    assert e_g == int(round(math.log2(10 ** 6))) + 4 - backoff
    g = torch.Generator().manual_seed(9)
    w, _ = _weight(8)
    G = _padded_rows(torch.randn(M, C, generator=g) * 1e-6)
    Gd = G.to(dev)
    D = torch.full((M, Cp), float("nan"), device=dev)
    H.conv3x3_wr_x3(Gd, Cp, e_g, 1, _pack(w, 23, 2 * Cp * 9 * Cp), None, None, D, B, Hh, Ww, Cp, Cp)
    ring = torch.full((M, Cp), float("nan"), device=dev)
    Wd = _pack(w, 18, Cp * 2 * 9 * Cp).view(Cp, -1)
    A, Bo = H.im2col(Gd, Hh, Ww, Cp, flip=True), H.rows(Wd)
    A.x3_exp, Bo.x3_exp = e_g, H.X3_WEXP
    H.gemm_nt(A, Bo, H.epilogue(ring), M, Cp, 9 * Cp, H.X3)
    x = torch.zeros(B, C, Hh, Ww, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, w.double(), None, padding=1).backward(_nchw64(G, B, Hh, Ww))
    ref = _rows_of(x.grad)
    torch.cuda.synchronize()
    e_ref, e_ring = rel(D[:, :C], ref), rel(D[:, :C], ring[:, :C])
    print(f"input gradient {geom} e_g {e_g}: vs float64 {e_ref:.2e}, vs ring {e_ring:.2e}")
    assert e_ref < 2e-6 and e_ring < 2e-6
    assert (D[:, C:] == 0).all()


def test_conv_wr_x3_rejects():
    """Shapes the kernel has no form for are refused by the query and by the call (the ring runs them)."""
    assert H.conv3x3_wr_x3_tile(2, 6, 48, Cp, 64) == 0      # N <= 64: the narrow forms are not built for fp16 pairs
    assert H.conv3x3_wr_x3_tile(2, 7, 40, Cp, Cp) == 0      # no whole-row tiling
    assert H.conv3x3_wr_x3_tile(2, 6, 48, 256, Cp) == 0     # two 256-channel halos do not fit the LDS
    x, out = torch.zeros(2 * 7 * 40, Cp, device=dev), torch.zeros(2 * 7 * 40, Cp, device=dev)
    w = torch.zeros(2 * Cp * 9 * Cp, device=dev, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        H.conv3x3_wr_x3(x, Cp, 4, 0, w, None, None, out, 2, 7, 40, Cp, Cp)


def test_engine_routes_x3_convs_through_wr():
    """The fp32x3 engine plans the wr path at a batch with enough tiles, the ring below the threshold or with
    conv_wr off.  Both paths are the same fp32-class arithmetic: each meets the network-level fp32x3 bars against
    the oracle (outputs 1e-5, gradients 1e-3 relative: tests/test_x3_gpu.py), so they differ by at most twice that."""
    from kair_amd.models.network_swinir import SwinIR
    torch.manual_seed(0)
    net = SwinIR(upscale=2, in_chans=3, img_size=48, window_size=8, img_range=1.0, depths=[2], embed_dim=180,
                 num_heads=[6], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv", drop_path_rate=0.0,
                 compute_dtype="fp32x3").to(dev).train()
    eng = net.engine()
    assert eng.conv_wr and eng.rstb[0][1].wr and eng.rstb[0][1].Wf15.dtype == torch.float16
    x = torch.rand(2, 3, 48, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    res = {}
    for tag, min_tiles in (("wr", 0), ("ring", 10 ** 9)):
        eng.conv_wr_min_tiles = min_tiles
        eng.plans.clear()   # plans are cached per shape: rebuilt under the new rule
        net.zero_grad(set_to_none=True)
        E = net(x)
        assert bool(eng.cur["conv_wr"]) == (tag == "wr")
        E.square().mean().backward()
        torch.cuda.synchronize()
        res[tag] = (E.detach().clone(), net.layers[0].conv.weight.grad.clone(), net.conv_first.weight.grad.clone())
    assert rel(res["wr"][0], res["ring"][0]) < 2e-5
    for a, b in zip(res["wr"][1:], res["ring"][1:]):
        assert rel(a, b) < 2e-3
