"""Float64 statements of LayerNorm over the last dim (nn.LayerNorm(C): network_swinir.py:199,205,520,725) and of the
Swin window order, in plain torch on the CPU -- the reference of tests/test_layernorm_gpu.py, pinned to torch's own
layer_norm / autograd and to roll + window_partition by tests/test_layernorm_ref_cpu.py.  Nothing here imports the
kernel library or repeats its index arithmetic."""
import torch


def ln_fwd(x, gamma, beta, eps):
    """x [M, C] -> y, mean [M], rstd [M] in float64; rstd = 1 / sqrt(biased variance + eps)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd(x, dy, gamma, eps):
    """dx [M, C], dgamma [C], dbeta [C] in float64, in closed form:
    dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)),  g = dy gamma;  dgamma = sum_m dy xhat,  dbeta = sum_m dy."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def window_partition(x, ws):
    """[B, H, W, ...] -> [B * nWin, ws, ws, ...] (network_swinir.py:33-46, for any trailing dims)."""
    B, H, W = x.shape[:3]
    rest = x.shape[3:]
    x = x.reshape(B, H // ws, ws, W // ws, ws, *rest)
    perm = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return x.permute(*perm).reshape(-1, ws, ws, *rest)


def window_rows(B, H, W, ws, shift):
    """rows[r] = the token (row of the [B H W, C] token matrix) that window-order row r holds: an index image
    rolled by -shift as the shifted block rolls its input (network_swinir.py:250), then window-partitioned."""
    idx = torch.arange(B * H * W).view(B, H, W)
    if shift:
        idx = torch.roll(idx, (-shift, -shift), (1, 2))
    return window_partition(idx, ws).reshape(-1)
