"""tests/window_attn_ref.py against the module it restates, in float64 on the CPU.

kair_amd.models.network_swinir.WindowAttention runs on the HIP device only (it raises on a CPU tensor: no CPU
fallback), so the module compared here is oracle.swinir.WindowAttention, the CPU restatement of
network_swinir.py:65-145 that tests/test_oracle_golden.py pins to the reference's own golden vectors and that the
whole-network tests trust; from kair_amd's module file the pure-torch relative_position_index and calculate_mask are
compared exactly.  Both sides run in float64, so the differences are float64 rounding: bound 1e-12 relative L2.

The golden file tests/golden/window_attention.npz holds float32 arrays the reference computed in float32.  Its exact
parts (rel_index, mask) are compared exactly; the float64 reference on its weights and inputs is compared with the
float64 module at 1e-12; and its float32 outputs are compared at a bound from float32's precision (below)."""
import pytest
import torch

import window_attn_ref as R
from conftest import load_golden, sub_state
from oracle import swinir as osw


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _heads(x, nh):
    """[nWin, T, nh*hd] -> [nWin, nh, T, hd]"""
    n, T, C = x.shape
    return x.view(n, T, nh, C // nh).permute(0, 2, 1, 3)


def _module_run(m, x, gout, mask):
    """out, and the gradients of the q/k/v projection's output and of the bias table, of an oracle WindowAttention."""
    cap = {}

    def hook(mod, inp, out):
        out.retain_grad()
        cap["qkv"] = out

    h = m.qkv.register_forward_hook(hook)
    out = m(x, mask)
    h.remove()
    out.backward(gout)
    return out.detach(), cap["qkv"], m.relative_position_bias_table.grad


def _split_qkv(t, nh):
    """[nWin, T, 3C] -> q, k, v [nWin, nh, T, hd] (network_swinir.py:121-122)."""
    n, T, C3 = t.shape
    q, k, v = t.view(n, T, 3, nh, C3 // (3 * nh)).permute(2, 0, 3, 1, 4)
    return q, k, v


@pytest.mark.parametrize("ws,Hh,Ww,shift,nh,hd", [(8, 16, 24, 0, 6, 30), (8, 16, 24, 4, 6, 30), (8, 8, 24, 1, 3, 17),
                                                 (7, 14, 21, 0, 6, 30), (7, 14, 21, 3, 6, 30), (7, 7, 14, 6, 5, 10)])
def test_reference_matches_module(ws, Hh, Ww, shift, nh, hd):
    """Identity proj (so the module's output is O), a random q/k/v projection whose output feeds the reference; two
    images, with and without the module's own shift mask."""
    torch.manual_seed(ws * 100 + shift)
    T, C = ws * ws, nh * hd
    nWin = 2 * (Hh // ws) * (Ww // ws)
    m = osw.WindowAttention(C, ws, nh).double()
    with torch.no_grad():
        m.relative_position_bias_table.normal_(0, 0.5)
        m.proj.weight.copy_(torch.eye(C))
        m.proj.bias.zero_()
    x = torch.randn(nWin, T, C, dtype=torch.float64)
    gout = torch.randn(nWin, T, C, dtype=torch.float64)
    mask = osw.shift_region_mask(Hh, Ww, ws, shift).double() if shift else None
    out, qkv, dtab = _module_run(m, x, gout, mask)
    q, k, v = _split_qkv(qkv.detach(), nh)
    rmask = R.shift_mask(Hh, Ww, ws, shift) if shift else None
    r = R.reference(q, k, v, m.relative_position_bias_table.detach(), _heads(gout, nh), ws, m.scale, rmask)
    assert all(t.dtype == torch.float64 for t in r.values())
    gq, gk, gv = _split_qkv(qkv.grad, nh)
    errs = dict(O=_rel(r["O"], _heads(out, nh)), dq=_rel(r["dq"], gq), dk=_rel(r["dk"], gk), dv=_rel(r["dv"], gv),
                dtable=_rel(r["dtable"], dtab))
    print(errs)
    assert max(errs.values()) < 1e-12, errs
    # lse: the log of the softmax's normaliser, from scores assembled with the module's own index buffer
    bias = m.relative_position_bias_table.detach()[m.relative_position_index.view(-1)].view(T, T, nh).permute(2, 0, 1)
    s = (q * m.scale) @ k.transpose(-2, -1) + bias
    if shift:
        s = s + mask.repeat(2, 1, 1)[:, None]
    mx = s.max(-1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(s - mx).sum(-1, keepdim=True))).squeeze(-1)
    assert _rel(r["lse"], lse) < 1e-12
    assert torch.isfinite(r["lse"]).all()


@pytest.mark.parametrize("ws", [7, 8])
def test_index_and_shift_mask_are_the_modules(ws):
    from kair_amd.models import network_swinir as ksw
    assert torch.equal(R.rel_index(ws), osw.relative_position_index(ws))
    assert torch.equal(R.rel_index(ws), ksw._relative_position_index(ws))
    for Hh, Ww in ((2 * ws, 3 * ws), (ws, 2 * ws), (3 * ws, ws), (ws, ws)):
        for shift in range(1, ws):
            mine = R.shift_mask(Hh, Ww, ws, shift)
            assert mine.dtype == torch.float64 and mine.shape == ((Hh // ws) * (Ww // ws), ws * ws, ws * ws)
            assert torch.equal(mine, osw.shift_region_mask(Hh, Ww, ws, shift).double())
            assert torch.equal(mine, ksw._shift_mask(Hh, Ww, ws, shift).double())


def test_explicit_mask_wraps_by_window():
    """mask[w % mask_nw], and the analytic shift mask passed explicitly gives the same bits."""
    g = torch.Generator().manual_seed(5)
    nWin, nh, ws, hd = 7, 2, 7, 5
    q, k, v = (torch.randn(nWin, nh, 49, hd, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(169, nh, generator=g, dtype=torch.float64)
    mask = torch.randn(3, 49, 49, generator=g, dtype=torch.float64)
    O, lse = R.attention(q, k, v, table, ws, 0.4, mask)
    for w in range(nWin):
        Ow, lw = R.attention(q[w:w + 1], k[w:w + 1], v[w:w + 1], table, ws, 0.4, mask[w % 3][None])
        assert torch.equal(O[w], Ow[0]) and torch.equal(lse[w], lw[0])


def test_packing_round_trips():
    g = torch.Generator().manual_seed(6)
    nWin, nh, T, hd, hp = 3, 5, 49, 17, 32
    q, k, v = (torch.randn(nWin, nh, T, hd, generator=g) for _ in range(3))
    blk = R.pack_blocked(q, k, v, hp)
    assert blk.shape == (3, nWin, nh, T, hp) and torch.equal(blk[1, ..., :hd], k) and blk[..., hd:].abs().max() == 0
    rows = R.pack_rows(q, hp, nh * hp + 8, fill=-768.0)
    body, rest = R.unpack_rows(rows, nWin, nh, T, hp)
    assert torch.equal(body[..., :hd], q) and body[..., hd:].abs().max() == 0 and (rest == -768.0).all()
    assert rows[T + 2, 3 * hp + 4] == q[1, 3, 2, 4]   # window 1, token 2, head 3, channel 4
    # token-row dqkv: column (part*nh + h)*hp + c of row win*T + tok
    drows = blk.permute(1, 3, 0, 2, 4).reshape(nWin * T, 3 * nh * hp)
    assert drows[T + 2, (2 * nh + 3) * hp + 4] == v[1, 3, 2, 4]
    assert torch.equal(R.dqkv_from_rows(drows, nWin, nh, T, hp), blk)
    x = torch.randn(100, generator=g) * 3
    p = R.hilo(x, 4)
    assert p.dtype == torch.float16 and p.shape == (2, 100)
    assert ((R.unhilo(p, 4) - x.double()).abs() <= x.double().abs() * 2.0 ** -21 + 2.0 ** -28).all()


# float32 bound for the golden's outputs: each stage is a float32 dot product of length K whose rounding grows like
# sqrt(K) 2^-24 in relative L2 -- q/k/v projection (180), scores (30), the softmax normaliser (64), P V (64), proj
# (180): (13.4 + 5.5 + 8 + 8 + 13.4) 2^-24 = 2.9e-6 forward; the backward runs the same chain again on top: 6e-6.
GOLD_FWD, GOLD_BWD = 3e-6, 6e-6


@pytest.mark.parametrize("tag", ["nomask", "mask"])
def test_reference_matches_golden(tag):
    z = load_golden("window_attention")
    assert torch.equal(R.rel_index(8), torch.from_numpy(z["rel_index"]))
    assert torch.equal(R.shift_mask(16, 16, 8, 4), torch.from_numpy(z["mask"]).double())
    nh = 6
    m = osw.WindowAttention(180, 8, nh)
    m.load_state_dict(sub_state(z, ""), strict=True)
    m = m.double()
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    gout = torch.from_numpy(z[f"{tag}.gout"]).double()
    mask = torch.from_numpy(z["mask"]).double() if tag == "mask" else None
    out, qkv, dtab = _module_run(m, x, gout, mask)
    # the reference between the module's own projections (float64 torch Linear on the golden's weights)
    q, k, v = _split_qkv(qkv.detach(), nh)
    dO = _heads(gout @ m.proj.weight.detach(), nh)
    r = R.reference(q, k, v, m.relative_position_bias_table.detach(), dO, 8, m.scale,
                    R.shift_mask(16, 16, 8, 4) if tag == "mask" else None)
    O_rows = r["O"].permute(0, 2, 1, 3).reshape(4, 64, 180)
    mine = O_rows @ m.proj.weight.detach().t() + m.proj.bias.detach()
    gq, gk, gv = _split_qkv(qkv.grad, nh)
    e64 = dict(out=_rel(mine, out), dq=_rel(r["dq"], gq), dk=_rel(r["dk"], gk), dv=_rel(r["dv"], gv),
               dtable=_rel(r["dtable"], dtab))
    print("float64 module", e64)
    assert max(e64.values()) < 1e-12, e64
    # and the golden's float32 arrays
    dqkv = torch.stack([r["dq"], r["dk"], r["dv"]]).permute(1, 3, 0, 2, 4).reshape(4, 64, 540)
    dx = dqkv @ m.qkv.weight.detach()
    e32 = dict(out=_rel(mine, torch.from_numpy(z[f"{tag}.out"]).double()),
               dx=_rel(dx, torch.from_numpy(z[f"{tag}.dx"]).double()),
               dtable=_rel(r["dtable"], torch.from_numpy(z[f"{tag}.grad.relative_position_bias_table"]).double()))
    print("float32 golden", e32)
    assert e32["out"] < GOLD_FWD and e32["dx"] < GOLD_BWD and e32["dtable"] < GOLD_BWD, e32
