"""Float64 statements of a dilated 3x3 conv (stride 1, padding = dilation = d) and of its two gradients, with the
magnitude sums S the elementwise bound of tests/convnet_forms_ref.py needs.  tests/test_dilconv_cpu.py pins the gradient
statements to torch's float64 autograd; tests/test_dilconv_gpu.py compares the kernels with them.

    forward   F.conv2d(x, w, b, padding=d, dilation=d)
    dgrad     the input gradient for an output gradient gy: F.conv_transpose2d(gy, w, padding=d, dilation=d)
    wgrad     dW[n][c][ky][kx] = sum_{b,y,x} gy[b][n][y][x] x[b][c][y + d (ky - 1)][x + d (kx - 1)]   (zero outside)
S is the same expression over |x|, |w|, |b|, |gy|."""
import torch
import torch.nn.functional as F

from convnet_forms_ref import bound, gen, pack_index, randn, ratio, to_nchw, to_rows  # noqa: F401  (re-exported)

DILS = (1, 2, 3, 4)
# (B, H, W, C, N): H < 2 d + 1 at d = 3, 4 in the first (whole tap rows fall outside); the second is M = 288 = 2 * 144,
# C = 64, aligned pointers -- the geometry the +-1-tap fast paths accept
GEMM_CASES = [(2, 5, 7, 16, 24), (2, 12, 12, 64, 64)]


def fwd(x, w, b, d):
    """(value, S) [B, N, H, W] of the dilated conv of x [B, C, H, W] with w [N, C, 3, 3] (+ bias b [N] or None)."""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    v = F.conv2d(x, w, b, padding=d, dilation=d)
    S = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), padding=d, dilation=d)
    return v, S


def dgrad(gy, w, d):
    """(value, S) [B, C, H, W]: the input gradient of fwd for the output gradient gy [B, N, H, W]."""
    gy, w = gy.double(), w.double()
    return (F.conv_transpose2d(gy, w, padding=d, dilation=d),
            F.conv_transpose2d(gy.abs(), w.abs(), padding=d, dilation=d))


def wgrad(gy, x, d):
    """(value, S) [N, C, 3, 3]: the weight gradient of fwd."""
    def one(g, xx):
        B, C = xx.shape[:2]
        N = g.shape[1]
        cols = F.unfold(xx, 3, dilation=d, padding=d)                 # [B, C 9, H W], row c 9 + tap
        return torch.einsum("bnp,bkp->nk", g.reshape(B, N, -1), cols).reshape(N, C, 3, 3)
    gy, x = gy.double(), x.double()
    return one(gy, x), one(gy.abs(), x.abs())


_CACHE = {}


def form(case, d):
    """Seeded bf16-exact inputs of a C -> N conv on the B x H x W grid and its three references, computed once:
    x rows [M, C], w [N, C, 3, 3], bias [N], the output gradient dy rows [M, N]; for the flipped product the same grid
    read the other way round: gy rows [M, C] (an output gradient of C channels) through wd [C, N, 3, 3] (a conv N -> C),
    whose input gradient has N channels -- so the GEMM of both products is M x N x 9 C."""
    key = (case, d)
    if key in _CACHE:
        return _CACHE[key]
    B, H, W, C, N = case
    g = gen(7000 + 10 * C + d + H)
    M = B * H * W
    r = dict(x=randn(g, M, C), w=randn(g, N, C, 3, 3, scale=0.1), bias=randn(g, N, scale=0.1), dy=randn(g, M, N),
             gy=randn(g, M, C), wd=randn(g, C, N, 3, 3, scale=0.1), M=M)
    v, S = fwd(to_nchw(r["x"], B, H, W), r["w"], r["bias"], d)
    r["fwd"] = to_rows(v), to_rows(S)
    r["relu"] = to_rows(torch.relu(v)), to_rows(S)                    # ReLU is 1-Lipschitz: S unchanged
    v, S = dgrad(to_nchw(r["gy"], B, H, W), r["wd"], d)
    r["dgrad"] = to_rows(v), to_rows(S)
    r["wgrad"] = wgrad(to_nchw(r["dy"], B, H, W), to_nchw(r["x"], B, H, W), d)
    _CACHE[key] = r
    return r
