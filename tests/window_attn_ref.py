"""A float64 statement of Swin window attention (WindowAttention.forward, network_swinir.py:114-145) in plain torch on
the CPU, and the packing of its operands into the kernels' layouts -- the reference of
tests/test_window_attn_shapes_gpu.py, pinned by tests/test_window_attn_ref_cpu.py.  Window size 7 or 8, any head
count / head dim, the shifted-window mask of calculate_mask (:216-237; any shift in 1..ws-1, any H, W that are
multiples of ws, H == ws included) or an explicit additive mask [mask_nw][T][T] applied to window w as
mask[w % mask_nw].  Nothing here imports the kernel library or repeats its index arithmetic."""
import torch


def rel_index(ws):
    """relative_position_index of network_swinir.py:92-102: [T, T] long, T = ws^2, values in [0, (2 ws - 1)^2)."""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)   # [2, T]
    r = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()                           # [T, T, 2]
    r[:, :, 0] += ws - 1
    r[:, :, 1] += ws - 1
    r[:, :, 0] *= 2 * ws - 1
    return r.sum(-1)


def shift_mask(H, W, ws, shift):
    """calculate_mask of network_swinir.py:216-237: [H/ws * W/ws, T, T] float64 of 0 / -100."""
    assert H % ws == 0 and W % ws == 0 and 0 < shift < ws
    img = torch.zeros(H, W)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    mw = img.view(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)   # window_partition
    d = mw[:, None, :] - mw[:, :, None]
    return torch.zeros(d.shape, dtype=torch.float64).masked_fill(d != 0, -100.0)


def scores(q, k, table, ws, scale, mask=None):
    """q, k [nWin, nh, T, hd], table [(2 ws - 1)^2, nh], mask [mask_nw, T, T] or None -> the softmax's argument
    [nWin, nh, T, T] in float64 (:124-136); window w takes mask[w % mask_nw]."""
    q, k, table = q.double(), k.double(), table.double()
    nWin, nh, T, _ = q.shape
    assert T == ws * ws and table.shape == ((2 * ws - 1) ** 2, nh)
    bias = table[rel_index(ws).view(-1)].view(T, T, nh).permute(2, 0, 1)
    s = (q * scale) @ k.transpose(-2, -1) + bias[None]
    if mask is not None:
        s = s + mask.double()[torch.arange(nWin) % mask.shape[0]][:, None]
    return s


def attention(q, k, v, table, ws, scale, mask=None):
    """-> O [nWin, nh, T, hd] = softmax(scores) @ v, lse [nWin, nh, T] = logsumexp(scores), float64."""
    s = scores(q, k, table, ws, scale, mask)
    return torch.softmax(s, -1) @ v.double(), torch.logsumexp(s, -1)


def reference(q, k, v, table, dO, ws, scale, mask=None):
    """O, lse and, by autograd on float64 leaves, dq, dk, dv, dtable for the output gradient dO [nWin, nh, T, hd]."""
    ql, kl, vl, tl = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v, table))
    O, lse = attention(ql, kl, vl, tl, ws, scale, mask)
    O.backward(dO.double())
    return dict(O=O.detach(), lse=lse.detach(), dq=ql.grad, dk=kl.grad, dv=vl.grad, dtable=tl.grad)


# ---------------------------------------------------------------------------------------------------------------
# the kernels' layouts (include/kair_hip.h: kair_window_attn_fwd / _bwd / _bwd_ex / _x3)
# ---------------------------------------------------------------------------------------------------------------
def pack_blocked(q, k, v, hp):
    """-> head-blocked [3][nWin][nh][T][hp] fp32, columns hd..hp-1 zero."""
    nWin, nh, T, hd = q.shape
    out = torch.zeros(3, nWin, nh, T, hp)
    out[0, ..., :hd], out[1, ..., :hd], out[2, ..., :hd] = q, k, v
    return out


def pack_rows(x, hp, ld, fill=0.0):
    """x [nWin, nh, T, hd] -> token rows [nWin*T, ld] in window order, head h at columns h*hp .. h*hp + hd - 1, the
    head's pad columns zero and columns nh*hp .. ld-1 set to `fill`."""
    nWin, nh, T, hd = x.shape
    out = torch.full((nWin * T, ld), float(fill))
    body = torch.zeros(nWin, T, nh, hp)
    body[..., :hd] = x.permute(0, 2, 1, 3)
    out[:, :nh * hp] = body.view(nWin * T, nh * hp)
    return out


def unpack_rows(rows, nWin, nh, T, hp):
    """Token rows [nWin*T, ld] -> ([nWin, nh, T, hp] head view of columns 0..nh*hp-1, the columns beyond)."""
    body = rows[:, :nh * hp].reshape(nWin, T, nh, hp).permute(0, 2, 1, 3)
    return body, rows[:, nh * hp:]


def hilo(x, e=0):
    """The fp16 pair planes of x * 2^e: [2, *x.shape] (hi = f16(x 2^e), lo = f16(x 2^e - hi))."""
    w = x * 2.0 ** e
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.stack([hi, lo])


def unhilo(p, e=0):
    """The float64 value (hi + lo) 2^-e of an fp16 pair [2, ...]."""
    return (p[0].double() + p[1].double()) * 2.0 ** -e


def dqkv_from_rows(d, nWin, nh, T, hp):
    """Token-row dqkv [nWin*T][3*nh*hp], column (part*nh + h)*hp + c -> the head-blocked form [3][nWin][nh][T][hp]
    (which needs no unpacking: dq, dk, dv are its planes)."""
    return d.reshape(nWin, T, 3, nh, hp).permute(2, 0, 3, 1, 4)
