"""Window attention (csrc/window_attn.hip, csrc/attn_x3.hip) at the shapes its dispatch makes interesting, against
the float64 reference of tests/window_attn_ref.py: several windows per backward wave with a short last group, several
(window, head) tasks per bf16 forward wave with a clipped last wave, an idle wave in the fp32 backward, the explicit
additive mask, lse itself, the deferred / accumulated bias-table gradient and kair_attn_dtable_grouped, shifts 1 and
ws - 1, grids one window high, head dims 1 / 17 / 32, 1 / 3 / 5 heads, strided O / dO rows, the ones column, and the
KAIR_ATTN_BWD_NW=4 / KAIR_ATTN_FWD_TPW instantiations in a fresh child process.

Bars (relative L2 against float64; the project's own, tests/test_kernels_gpu.py::test_window_attention_fwd_bwd,
tests/test_x3_gpu.py::test_window_attention_x3): fp32 2e-5 forward / 5e-5 backward, bf16 1.5e-2 / 3e-2 on
bf16-rounded inputs, x3 2e-6 / 5e-6.  lse takes the forward bar.  Every output is pre-filled with NaN (the columns
past nh*hp of a strided row with a sentinel) and must come back finite, with zero pad columns and the sentinel intact.

The multi-window / multi-task shapes are searched for from the device's CU count by the dispatch rules restated in
_wpg_bf16 / _wpg_x3 / _tpw_bf16; the group counts are asserted against kair_window_attn_bwd_groups.  The fp32
backward needs nWin % 4 != 0, which four windows per image can never give, and a clipped two-task wave needs an odd
task count: those cases use a 2 x 3-window and a 1 x 3-window grid.

Measured on an MI355X (256 CUs), the largest relative L2 error of each case (every figure is printed, "MEASURED"):

  (a) backward, several windows per wave, short last group (forward O / lse, then dq dk dv / dtable)
      bf16 ws 8  hp 32 and 16, 344 windows, wpg 3 (115 groups, the last of 2): O 2.35e-3, lse 4.6e-8; 2.83e-3 / 1.08e-3;
                 token-row dqkv and its dtable bit-equal to the head-blocked launch
      bf16 ws 7  344 windows, wpg 3: O 2.35e-3, lse 4.6e-8; 2.72e-3 / 1.34e-3
      x3 ws 8    pair and fp32 outputs, 260 windows, wpg 3 (87 groups, the last of 2): O 2.23e-7, lse 4.63e-8;
                 3.32e-7 / 3.70e-7
      x3 ws 7    pair, 260 windows, wpg 3: O 2.16e-7, lse 4.74e-8; 3.23e-7 / 3.30e-7
      fp32 ws 8  18 windows, nh 5, WPG 4 (5 groups, the last of 2; 25 waves, one idle): O 2.37e-7, lse 4.62e-8;
                 3.42e-7 / 2.91e-7
      fp32 ws 7  the same geometry: O 2.18e-7, lse 4.73e-8; 3.21e-7 / 3.08e-7
  (b) bf16 forward, several tasks per wave, nh 5
      hp 32  411 windows, 2,055 tasks, tpw 2 (last wave 1 task): O 2.35e-3, lse 4.53e-8
      hp 16  615 windows, 3,075 tasks, tpw 2 (last wave 1 task): O 2.35e-3, lse 4.53e-8
  (c) explicit mask, 12 windows: the shift mask passed explicitly is bit-equal to the analytic launch (O, lse, dqkv,
      dtable; fp32 and bf16, ws 8 and 7) and as far from float64 (fp32 O 1.93e-7, backward 2.89e-7; bf16 2.35e-3,
      2.67e-3); random mask over window % 5: fp32 O 1.92e-7, lse 4.42e-8, backward 2.91e-7; bf16 2.36e-3, 2.72e-3
  (d) deferred dtable through kair_attn_dtable_grouped: bit-equal to the immediate form in all five jobs (fp32 ws 8
      nh 5, fp32 ws 7 nh 5 accumulating, bf16 ws 8 nh 6 wpg 3 accumulating, bf16 ws 7 nh 6, x3 ws 8 nh 3 accumulating);
      against float64 + prefill: fp32 2.86e-7, bf16 7.41e-4, x3 2.08e-7; the 32-job launch equals the single-job tables
  (e) geometry edges (1..12 windows), the worst case of each arithmetic: fp32 O 2.27e-7 (nh 1), lse 4.92e-8, backward
      5.34e-7 (ws 7, hd 1); bf16 O 2.40e-3, lse 4.79e-8, backward 7.82e-3 (dq, ws 7, hd 1); x3 O 2.16e-7, lse 5.42e-8,
      backward 4.78e-7 (ws 7, hd 1).  The largest absolute lse error anywhere: 1.72e-6 (x3, hd 1)
  child process, KAIR_ATTN_BWD_NW=4 and KAIR_ATTN_FWD_TPW=3: (a)'s bf16 ws 8 case 2.65e-3 / 8.13e-4; forward, 32
      windows, 160 tasks in waves of 3 (last wave 1 task): O 2.36e-3 (hp 32), 2.34e-3 (hp 16)
"""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_attn_ref as R  # noqa: E402
from kair_amd import _hip as H  # noqa: E402

dev = torch.device("cuda")
NAN = float("nan")
SENT = -768.0                      # exact in bf16, fp16 and fp32
E_ACT, E_GRAD, GS = 4, 26, 1e-7    # the x3 exponents and output-gradient scale of test_window_attention_x3
BARS = {"fp32": (2e-5, 5e-5), "bf16": (1.5e-2, 3e-2), "x3": (2e-6, 5e-6)}
CODE = {"fp32": H.F32, "bf16": H.BF16, "x3": H.X3}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
MEAS = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """A faulted device fails every later call: end the session there instead of launching on it again."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported a fault: {e}", returncode=3)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _note(name, **kw):
    MEAS[name] = kw
    print("MEASURED", name, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


# ---------------------------------------------------------------------------------------------------------------
# the dispatch rules of window_attn.hip / attn_x3.hip, restated
# ---------------------------------------------------------------------------------------------------------------
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wpg_bf16(nWin, nh):
    """bwd_wpg_bf16: windows per backward wave so that the (group, head) waves fill 4 wave slots per CU once."""
    return max(1, math.ceil(nWin / max(1, 4 * _ncu() // nh)))


def _wpg_x3(nWin, nh):
    """kair_attn_x3_wpg: the same at 3 workgroups per CU."""
    return max(1, math.ceil(nWin / max(1, 3 * _ncu() // nh)))


def _tpw_bf16(tasks, hp):
    """fwd_tpw_bf16: tasks per forward wave (occupancy 2 at head pad 32, 3 at 16), or KAIR_ATTN_FWD_TPW."""
    forced = int(os.environ.get("KAIR_ATTN_FWD_TPW", "0") or 0)
    if forced > 0:
        return forced
    return max(1, math.ceil(tasks / (4 * (3 if hp == 16 else 2) * _ncu())))


def _wpg(arith, nWin, nh):
    return {"fp32": 4, "bf16": _wpg_bf16(nWin, nh), "x3": _wpg_x3(nWin, nh)}[arith]


def _find_batch(per_image, cond, what, bmin=1):
    for B in range(bmin, 257):
        if cond(B * per_image):
            return B
    pytest.skip(f"{what}: no batch <= 256 meets the condition on {_ncu()} CUs")


def _assert_groups(nWin, nh):
    """The restated rules give kair_window_attn_bwd_groups' counts (a change of the dispatch fails here)."""
    L = H.lib()
    for arith in ("fp32", "bf16", "x3"):
        want = math.ceil(nWin / _wpg(arith, nWin, nh))
        got = L.kair_window_attn_bwd_groups(nWin, nh, CODE[arith])
        assert got == want, (arith, nWin, nh, got, want)


# ---------------------------------------------------------------------------------------------------------------
# cases (inputs + float64 reference, computed once, never modified) and the two runners
# ---------------------------------------------------------------------------------------------------------------
_CASES = {}


def make_case(ws, B, Hh, Ww, nh, hd, shift=0, bf=False, mask=None, grad=True, seed=19):
    """mask: None (the analytic shift mask of `shift`, if any) or "random": [5][T][T] of {0, -100} + 0.5 randn with a
    zero diagonal, applied as window % 5."""
    key = (ws, B, Hh, Ww, nh, hd, shift, bf, mask, grad, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(seed)
    T, nbin = ws * ws, (2 * ws - 1) ** 2
    nWin = B * (Hh // ws) * (Ww // ws)
    q, k, v = (torch.randn(nWin, nh, T, hd, generator=g) for _ in range(3))
    table = torch.randn(nbin, nh, generator=g) * 0.5
    go = torch.randn(nWin, nh, T, hd, generator=g)
    if bf:   # compare on the values the bf16 kernels read
        q, k, v, go = (t.bfloat16().float() for t in (q, k, v, go))
    m = None
    if mask == "random":
        assert shift == 0
        m = torch.where(torch.rand(5, T, T, generator=g) < 0.5, 0.0, -100.0) + 0.5 * torch.randn(5, T, T, generator=g)
        m[:, torch.arange(T), torch.arange(T)] = 0.0
        assert (m.diagonal(dim1=1, dim2=2) == 0).all()   # no fully masked row
    rmask = m.double() if m is not None else (R.shift_mask(Hh, Ww, ws, shift) if shift else None)
    scale = hd ** -0.5
    if grad:
        ref = R.reference(q, k, v, table, go, ws, scale, rmask)
    else:
        with torch.no_grad():
            O, lse = R.attention(q, k, v, table, ws, scale, rmask)
        ref = dict(O=O, lse=lse)
    assert torch.isfinite(ref["lse"]).all() and torch.isfinite(ref["O"]).all()
    c = SimpleNamespace(ws=ws, T=T, nbin=nbin, B=B, Hh=Hh, Ww=Ww, nWin=nWin, nh=nh, hd=hd, shift=shift, bf=bf, scale=scale,
                        q=q, k=k, v=v, table=table, go=go, mask=m, ref=ref)
    _CASES[key] = c
    return c


def _pads(t2d, nWin, nh, T, hp, hd, parts=1):
    """The pad columns [hd, hp) of every head of rows [nWin*T, >= parts*nh*hp]."""
    return t2d[:, :parts * nh * hp].reshape(nWin * T, parts * nh, hp)[..., hd:]


def run_fwd(c, arith, hp=32, extra=0, ones_col=-1, f32_out=False, mask=None, shift=None, name=None):
    """One forward launch on NaN / sentinel pre-filled outputs; asserts finiteness, pads, the sentinel, and O and lse
    against the reference at the forward bar.  Returns the launch state for run_bwd."""
    assert (arith == "bf16") == c.bf
    nWin, nh, T, hd, ws = c.nWin, c.nh, c.T, c.hd, c.ws
    M, ld = nWin * T, nh * hp + extra
    shift = c.shift if shift is None else shift
    blk = R.pack_blocked(c.q, c.k, c.v, hp)
    table = c.table.to(dev)
    lse = torch.full((nWin, nh, T), NAN, device=dev)
    pre = torch.full((M, ld), NAN)
    pre[:, nh * hp:] = SENT
    pair = arith == "x3" and not f32_out
    if arith == "x3":
        qkv = R.hilo(blk.to(dev), E_ACT)
        O = pre.to(dev) if f32_out else torch.stack([pre, pre]).to(dev, torch.float16)
        H.window_attn_fwd_x3(qkv, table, O, ld, lse, nWin, nh, hd, c.scale, c.Hh, c.Ww, shift, ones_col=ones_col,
                             e_in=E_ACT, e_out=E_ACT, ws=ws)
    else:
        qkv = blk.to(dev, TDT[arith]).contiguous()
        O = pre.to(dev, TDT[arith])
        H.window_attn_fwd(qkv, table, O, ld, lse, nWin, nh, hd, c.scale, c.Hh, c.Ww, shift, ones_col=ones_col,
                          mask=mask, head_pad=hp, ws=ws)
    torch.cuda.synchronize()
    Oc = O.cpu()
    planes = [Oc[0], Oc[1]] if pair else [Oc]
    val = R.unhilo(Oc, E_ACT) if pair else Oc.double()
    for p in planes:
        assert torch.isfinite(p[:, :nh * hp]).all()
        assert (p[:, nh * hp:] == SENT).all()            # past the heads of a strided row: untouched
    assert torch.isfinite(lse).all()
    if ones_col >= 0:   # 1.0 (the hi plane of a pair: 2^e_out, lo 0), then cleared for the zero check
        assert (val[:, ones_col] == 1.0).all()
        if pair:
            assert (planes[0][:, ones_col] == 2.0 ** E_ACT).all() and (planes[1][:, ones_col] == 0).all()
        planes = [p.clone() for p in planes]
        for p in planes:
            p[:, ones_col] = 0
    if hd < hp:
        for p in planes:
            assert _pads(p, nWin, nh, T, hp, hd).abs().max() == 0
    body, _ = R.unpack_rows(val, nWin, nh, T, hp)
    lse_c = lse.cpu().double()
    eO, eL = rel(body[..., :hd], c.ref["O"]), rel(lse_c, c.ref["lse"])
    if name:
        _note(name + ".fwd", nWin=nWin, O=eO, lse=eL, lse_maxabs=(lse_c - c.ref["lse"]).abs().max().item())
    assert eO < BARS[arith][0] and eL < BARS[arith][0], (name, eO, eL)
    return SimpleNamespace(qkv=qkv, O=O, lse=lse, ld=ld, hp=hp, f32_out=f32_out, mask=mask, shift=shift, table=table,
                           eO=eO, eL=eL)


def run_bwd(c, arith, st, rows=False, deferred=False, acc=False, prefill=None, name=None):
    """One backward launch on the forward's own O and lse.  dtable: immediate into a NaN table (acc: onto a copy of
    `prefill`), or deferred (the partials stay in the returned workspace).  Asserts finiteness, zero pads and
    dq / dk / dv / dtable against the reference at the backward bar.  Returns (raw dqkv, dtable or None, workspace)."""
    nWin, nh, T, hd, ws, hp, ld = c.nWin, c.nh, c.T, c.hd, c.ws, st.hp, st.ld
    M = nWin * T
    dO_rows = R.pack_rows(c.go, hp, ld, fill=NAN)       # NaN past the heads of a strided row: never to be read
    wsb = torch.full((H.window_attn_bwd_ws(nWin, nh, ws=ws),), NAN, device=dev)
    dtab = None
    if not deferred:
        dtab = prefill.clone().to(dev) if acc else torch.full((c.nbin, nh), NAN, device=dev)
    pair = arith == "x3" and not st.f32_out
    if arith == "x3":
        dO = R.hilo((dO_rows * GS).to(dev), E_GRAD)
        dqkv = torch.full((M, 3 * nh * 32), NAN, device=dev)
        if pair:
            dqkv = torch.stack([dqkv, dqkv]).to(torch.float16)
        H.window_attn_bwd_x3(st.qkv, st.O, ld, dO, ld, st.table, st.lse, dqkv, dtab, acc, wsb, nWin, nh, hd, c.scale, c.Hh,
                             c.Ww, st.shift, e_act=E_ACT, e_grad=E_GRAD, win_ws=ws)
    else:
        dO = dO_rows.to(dev, TDT[arith])
        shape = (M, 3 * nh * hp) if rows else tuple(st.qkv.shape)
        dqkv = torch.full(shape, NAN, device=dev, dtype=TDT[arith])
        H.window_attn_bwd(st.qkv, st.O, ld, dO, ld, st.table, st.lse, dqkv, dtab, acc, wsb, nWin, nh, hd, c.scale, c.Hh,
                          c.Ww, st.shift, mask=st.mask, dqkv_rows=rows, head_pad=hp, win_ws=ws)
    torch.cuda.synchronize()
    dc = dqkv.cpu()
    as_rows = rows or arith == "x3"
    for p in ([dc[0], dc[1]] if pair else [dc]):
        assert torch.isfinite(p).all()
        if hd < hp:
            pads = _pads(p, nWin, nh, T, hp, hd, parts=3) if as_rows else p[..., hd:]
            assert pads.abs().max() == 0
    val = R.unhilo(dc, E_GRAD) if pair else dc.double()
    if arith == "x3":
        val = val / GS
    d = R.dqkv_from_rows(val, nWin, nh, T, hp) if as_rows else val
    errs = dict(dq=rel(d[0, ..., :hd], c.ref["dq"]), dk=rel(d[1, ..., :hd], c.ref["dk"]), dv=rel(d[2, ..., :hd], c.ref["dv"]))
    if dtab is not None:
        assert torch.isfinite(dtab).all()
        gs = GS if arith == "x3" else 1.0
        want = c.ref["dtable"] * gs + (prefill.double() if acc else 0)
        errs["dtable"] = rel(dtab, want)
    if name:
        _note(name + ".bwd", nWin=nWin, wpg=_wpg(arith, nWin, nh), **errs)
    assert max(errs.values()) < BARS[arith][1], (name, errs)
    return dqkv, dtab, wsb


# ---------------------------------------------------------------------------------------------------------------
# (a) several windows per backward wave, a short last group, an idle fp32 wave
# ---------------------------------------------------------------------------------------------------------------
def bwd_multi_window_case(arith, ws, variant, shift):
    """variant: "hp32" / "hp16" (bf16), "pair" / "f32" (x3 output form), "" (fp32)."""
    nh = 5 if arith == "fp32" else 6
    hp, hd = (16, 10) if variant == "hp16" else (32, 30)
    if arith == "fp32":   # a short last group and an odd (group, head) count: the last workgroup's second wave idles
        Hh, Ww = 2 * ws, 3 * ws
        cond = lambda n: n % 4 != 0 and (math.ceil(n / 4) * nh) % 2 == 1
    else:
        Hh, Ww = 2 * ws, 2 * ws
        cond = lambda n: _wpg(arith, n, nh) >= 3 and n % _wpg(arith, n, nh) != 0
    B = _find_batch((Hh // ws) * (Ww // ws), cond, f"{arith} ws {ws} multi-window backward")
    nWin = B * (Hh // ws) * (Ww // ws)
    _assert_groups(nWin, nh)
    wpg = _wpg(arith, nWin, nh)
    groups = H.lib().kair_window_attn_bwd_groups(nWin, nh, CODE[arith])
    assert groups == math.ceil(nWin / wpg) and nWin % wpg != 0 and groups * wpg > nWin
    assert (wpg == 4 and (groups * nh) % 2 == 1) if arith == "fp32" else wpg >= 3
    c = make_case(ws, B, Hh, Ww, nh, hd, shift, bf=arith == "bf16")
    name = f"a.{arith}.ws{ws}.{variant or 'blocked'}.shift{shift}"
    st = run_fwd(c, arith, hp=hp, f32_out=variant == "f32", name=name)
    dqkv, dtab, _ = run_bwd(c, arith, st, name=name)
    if arith == "bf16" and ws == 8:   # token-row dqkv: the bits of the head-blocked launch on the same inputs
        dr, dtab_r, _ = run_bwd(c, arith, st, rows=True, name=name + ".rows")
        assert torch.equal(dr.cpu(), dqkv.cpu().permute(1, 3, 0, 2, 4).reshape(nWin * 64, 3 * nh * hp))
        assert torch.equal(dtab_r, dtab)
    return c, st


A_CASES = [("bf16", 8, "hp32"), ("bf16", 8, "hp16"), ("bf16", 7, "hp32"), ("x3", 8, "pair"), ("x3", 8, "f32"),
           ("x3", 7, "pair"), ("fp32", 8, ""), ("fp32", 7, "")]


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("arith,ws,variant", A_CASES)
def test_bwd_multi_window(arith, ws, variant, shifted):
    bwd_multi_window_case(arith, ws, variant, (3 if ws == 8 else 2) if shifted else 0)


# ---------------------------------------------------------------------------------------------------------------
# (b) several (window, head) tasks per bf16 forward wave, the last wave clipped
# ---------------------------------------------------------------------------------------------------------------
def fwd_multi_task_case(hp, shift, per_image_grid=(1, 3), bmin=1):
    """nh = 5 on a grid of 3 windows per image (an odd task count is reachable), ws 8: O, lse and the pads."""
    nh, hd, ws = 5, (10 if hp == 16 else 30), 8
    Hh, Ww = per_image_grid[0] * ws, per_image_grid[1] * ws
    per = per_image_grid[0] * per_image_grid[1]
    cond = lambda n: _tpw_bf16(n * nh, hp) >= 2 and (n * nh) % _tpw_bf16(n * nh, hp) != 0
    B = _find_batch(per, cond, f"bf16 head pad {hp} multi-task forward", bmin)
    nWin = B * per
    tpw = _tpw_bf16(nWin * nh, hp)
    assert tpw >= 2 and (nWin * nh) % tpw != 0
    c = make_case(ws, B, Hh, Ww, nh, hd, shift, bf=True, grad=False)
    name = f"b.bf16.hp{hp}.shift{shift}.tpw{tpw}"
    return run_fwd(c, "bf16", hp=hp, name=name)


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("hp", [32, 16])
def test_fwd_multi_task(hp, shift):
    fwd_multi_task_case(hp, shift)


# ---------------------------------------------------------------------------------------------------------------
# (c) the explicit additive mask
# ---------------------------------------------------------------------------------------------------------------
def _grid12(ws):
    return 2, 2 * ws, 3 * ws   # B, H, W: 12 windows


@pytest.mark.parametrize("ws", [8, 7])
@pytest.mark.parametrize("arith", ["fp32", "bf16"])
def test_explicit_shift_mask(arith, ws):
    """calculate_mask's mask for shift ws/2 passed explicitly with shift 0: the reference, and the analytic-shift
    launch on the same inputs."""
    B, Hh, Ww = _grid12(ws)
    c = make_case(ws, B, Hh, Ww, 6, 30, ws // 2, bf=arith == "bf16")
    m = R.shift_mask(Hh, Ww, ws, ws // 2).float().to(dev).contiguous()
    name = f"c.shiftmask.{arith}.ws{ws}"
    st_m = run_fwd(c, arith, mask=m, shift=0, name=name + ".explicit")
    d_m, t_m, _ = run_bwd(c, arith, st_m, name=name + ".explicit")
    st_a = run_fwd(c, arith, name=name + ".analytic")
    d_a, t_a, _ = run_bwd(c, arith, st_a, name=name + ".analytic")
    fbar, bbar = BARS[arith]
    errs = dict(O=rel(st_m.O, st_a.O), lse=rel(st_m.lse, st_a.lse), dqkv=rel(d_m, d_a), dtable=rel(t_m, t_a))
    equal = all(torch.equal(a, b) for a, b in ((st_m.O, st_a.O), (st_m.lse, st_a.lse), (d_m, d_a), (t_m, t_a)))
    _note(name + ".explicit_vs_analytic", bit_equal=equal, **errs)
    assert errs["O"] < fbar and errs["lse"] < fbar and errs["dqkv"] < bbar and errs["dtable"] < bbar


@pytest.mark.parametrize("ws", [8, 7])
@pytest.mark.parametrize("arith", ["fp32", "bf16"])
def test_random_mask_wraps(arith, ws):
    """mask_nw = 5 over 12 windows (window % 5 wraps), {0, -100} + 0.5 randn, zero diagonal."""
    B, Hh, Ww = _grid12(ws)
    c = make_case(ws, B, Hh, Ww, 6, 30, 0, bf=arith == "bf16", mask="random")
    assert c.nWin % 5 != 0
    name = f"c.randmask.{arith}.ws{ws}"
    st = run_fwd(c, arith, mask=c.mask.to(dev).contiguous(), name=name)
    run_bwd(c, arith, st, name=name)


@pytest.mark.parametrize("arith", ["fp32", "bf16"])
def test_mask_with_shift_is_rejected(arith):
    """No launch: the pre-filled outputs stay as they were."""
    ws = 8
    B, Hh, Ww = _grid12(ws)
    c = make_case(ws, B, Hh, Ww, 6, 30, 0, bf=arith == "bf16")
    st = run_fwd(c, arith)
    m = R.shift_mask(Hh, Ww, ws, 4).float().to(dev).contiguous()
    O = torch.full_like(st.O, NAN)
    lse = torch.full_like(st.lse, NAN)
    with pytest.raises(RuntimeError, match="explicit mask"):
        H.window_attn_fwd(st.qkv, st.table, O, st.ld, lse, c.nWin, c.nh, c.hd, c.scale, Hh, Ww, 4, mask=m, ws=ws)
    dqkv = torch.full_like(st.qkv, NAN)
    dtab = torch.full((c.nbin, c.nh), NAN, device=dev)
    wsb = torch.full((H.window_attn_bwd_ws(c.nWin, c.nh, ws=ws),), NAN, device=dev)
    dO = R.pack_rows(c.go, 32, st.ld).to(dev, TDT[arith])
    with pytest.raises(RuntimeError, match="explicit mask"):
        H.window_attn_bwd(st.qkv, st.O, st.ld, dO, st.ld, st.table, st.lse, dqkv, dtab, False, wsb, c.nWin, c.nh, c.hd,
                          c.scale, Hh, Ww, 4, mask=m, win_ws=ws)
    torch.cuda.synchronize()
    for t in (O, lse, dqkv, dtab, wsb):
        assert torch.isnan(t).all()


# ---------------------------------------------------------------------------------------------------------------
# (d) the deferred and the accumulated bias-table gradient
# ---------------------------------------------------------------------------------------------------------------
def _dtable_configs():
    """(arith, case, forward state, accumulate): 225- and 169-bin jobs mixed, nh in {5, 6, 3}."""
    out = []
    c, st = bwd_multi_window_case("fp32", 8, "", 0)          # nh 5, a short last group
    out.append(("fp32", c, st, False))
    c, st = bwd_multi_window_case("fp32", 7, "", 2)          # 169 bins
    out.append(("fp32", c, st, True))
    c, st = bwd_multi_window_case("bf16", 8, "hp32", 3)      # nh 6, >= 3 windows per wave
    assert _wpg_bf16(c.nWin, c.nh) >= 2
    out.append(("bf16", c, st, True))
    c, st = bwd_multi_window_case("bf16", 7, "hp32", 0)      # 169 bins
    out.append(("bf16", c, st, False))
    c = make_case(8, 2, 16, 24, 3, 30, 4)                    # nh 3
    out.append(("x3", c, run_fwd(c, "x3"), True))
    return out


def test_dtable_deferred_and_grouped():
    cfgs = _dtable_configs()
    g = torch.Generator().manual_seed(41)
    GAP = 64
    sizes = [c.nbin * c.nh for _, c, _, _ in cfgs]
    flat = torch.full((sum(sizes) + GAP * (len(sizes) + 1),), SENT, device=dev)
    jobs, views, imm, pre = [], [], [], []
    off = GAP
    for (arith, c, st, acc), n in zip(cfgs, sizes):
        # randn at the gradient's own RMS (x3's is in dO's 1e-7 units), so that neither term of the sum hides the other
        rms = c.ref["dtable"].norm().item() / math.sqrt(c.nbin * c.nh) * (GS if arith == "x3" else 1.0)
        p = torch.randn(c.nbin, c.nh, generator=g) * rms
        name = f"d.{arith}.ws{c.ws}.nh{c.nh}.acc{int(acc)}"
        _, t_imm, _ = run_bwd(c, arith, st, acc=acc, prefill=p, name=name + ".immediate")
        _, none, wsb = run_bwd(c, arith, st, deferred=True, name=name + ".deferred")
        assert none is None
        view = flat[off:off + n].view(c.nbin, c.nh)
        view.copy_(p.to(dev) if acc else torch.full_like(view, NAN))
        off += n + GAP
        jobs.append((wsb, c.nWin, c.nh, CODE[arith], view, acc, c.ws))
        views.append(view)
        imm.append(t_imm)
        pre.append(p)
    before = flat.clone()
    H.attn_dtable_grouped(jobs)
    torch.cuda.synchronize()
    keep = torch.ones_like(flat, dtype=torch.bool)
    for (arith, c, st, acc), view, t_imm, p in zip(cfgs, views, imm, pre):
        assert torch.equal(view, t_imm), (arith, c.ws)       # split_sum16 over the same partials
        want = c.ref["dtable"] * (GS if arith == "x3" else 1.0) + (p.double() if acc else 0)
        e = rel(view, want)
        _note(f"d.grouped.{arith}.ws{c.ws}.nh{c.nh}.acc{int(acc)}", dtable=e)
        assert e < BARS[arith][1]
        s = view.data_ptr() - flat.data_ptr()
        keep[s // 4:s // 4 + view.numel()] = False
    assert torch.equal(flat[keep], before[keep]) and (flat[keep] == SENT).all()   # nothing outside the jobs' tables
    # 32 jobs over the same partials, the two bin counts alternating, against single-job launches
    two = [jobs[0], jobs[1]]
    assert {cfgs[0][1].nbin, cfgs[1][1].nbin} == {225, 169}
    single = []
    for j in two:
        t = torch.full_like(j[4], NAN)
        H.attn_dtable_grouped([j[:4] + (t, False, j[6])])
        single.append(t)
    tabs = [torch.full_like(two[i % 2][4], NAN) for i in range(32)]
    H.attn_dtable_grouped([two[i % 2][:4] + (tabs[i], False, two[i % 2][6]) for i in range(32)])
    torch.cuda.synchronize()
    for i, t in enumerate(tabs):
        assert torch.equal(t, single[i % 2]), i
    # argument errors: no launch
    t = torch.full_like(two[0][4], NAN)
    with pytest.raises(RuntimeError, match="jobs"):
        H.attn_dtable_grouped([two[0][:4] + (t, False, 8)] * 33)
    with pytest.raises(RuntimeError, match="window size"):
        H.attn_dtable_grouped([two[0][:4] + (t, False, 5)])
    with pytest.raises(RuntimeError, match="job 1"):
        H.attn_dtable_grouped([two[0][:4] + (t, False, 8), two[0][:4] + (None, False, 8)])
    torch.cuda.synchronize()
    assert torch.isnan(t).all()


# ---------------------------------------------------------------------------------------------------------------
# (e) geometry edges, 1 to 12 windows
# ---------------------------------------------------------------------------------------------------------------
#        name          ws  B  H   W  nh  hd shift  extra ones
EDGES = [("s1", 8, 1, 16, 24, 6, 30, 1, 0, -1), ("s7", 8, 1, 16, 24, 6, 30, 7, 0, -1),
         ("flat.s1", 8, 2, 8, 24, 6, 30, 1, 0, -1), ("flat.s7", 8, 2, 8, 24, 6, 30, 7, 0, -1),
         ("w7.s1", 7, 1, 14, 21, 6, 30, 1, 0, -1), ("w7.s6", 7, 1, 14, 21, 6, 30, 6, 0, -1),
         ("w7.flat.s1", 7, 2, 7, 21, 6, 30, 1, 0, -1), ("w7.flat.s6", 7, 2, 7, 21, 6, 30, 6, 0, -1),
         ("hd32", 8, 1, 16, 16, 6, 32, 4, 0, -1), ("w7.hd32", 7, 1, 14, 14, 6, 32, 0, 0, -1),
         ("hd17", 8, 1, 16, 16, 6, 17, 4, 0, -1), ("w7.hd17", 7, 1, 14, 14, 6, 17, 3, 0, -1),
         ("hd1", 8, 1, 16, 16, 6, 1, 4, 0, -1), ("w7.hd1", 7, 1, 14, 14, 6, 1, 3, 0, -1),
         ("nh1", 8, 1, 8, 8, 1, 30, 0, 0, -1), ("w7.nh1", 7, 1, 14, 7, 1, 30, 3, 0, -1),
         ("nh3", 8, 1, 16, 24, 3, 30, 4, 0, -1), ("w7.nh3", 7, 1, 14, 21, 3, 30, 0, 0, -1),
         ("ld+8", 8, 1, 16, 24, 6, 30, 4, 8, -1), ("w7.ld+8", 7, 1, 14, 21, 5, 30, 3, 8, -1),
         ("ones", 8, 1, 16, 24, 6, 30, 4, 0, 6 * 32 - 2), ("w7.ones", 7, 1, 14, 21, 6, 30, 3, 8, 6 * 32 - 2)]


@pytest.mark.parametrize("arith", ["fp32", "bf16", "x3", "x3f"])
@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_geometry_edges(edge, arith):
    tag, ws, B, Hh, Ww, nh, hd, shift, extra, ones = edge
    f32_out = arith == "x3f"
    arith = "x3" if f32_out else arith
    c = make_case(ws, B, Hh, Ww, nh, hd, shift, bf=arith == "bf16")
    assert 1 <= c.nWin <= 12
    name = f"e.{tag}.{arith}{'.f32' if f32_out else ''}"
    st = run_fwd(c, arith, extra=extra, ones_col=ones, f32_out=f32_out, name=name)
    run_bwd(c, arith, st, name=name)
    if arith == "bf16" and hd <= 16 and ws == 8:   # the head pad 16 layout at the same edge
        st = run_fwd(c, arith, hp=16, extra=extra, name=name + ".hp16")
        run_bwd(c, arith, st, name=name + ".hp16")


@pytest.mark.parametrize("arith", ["fp32", "bf16", "x3", "x3f"])
def test_ones_column_at_hd32_is_rejected(arith):
    """hd = 32 leaves no pad column: no launch, outputs untouched."""
    f32_out = arith == "x3f"
    arith = "x3" if f32_out else arith
    c = make_case(8, 1, 16, 16, 6, 32, 4, bf=arith == "bf16")
    blk = R.pack_blocked(c.q, c.k, c.v, 32).to(dev)
    lse = torch.full((c.nWin, 6, 64), NAN, device=dev)
    with pytest.raises(RuntimeError, match="ones column"):
        if arith == "x3":
            O = torch.full((c.nWin * 64, 192) if f32_out else (2, c.nWin * 64, 192), NAN, device=dev,
                           dtype=torch.float32 if f32_out else torch.float16)
            H.window_attn_fwd_x3(R.hilo(blk, E_ACT), c.table.to(dev), O, 192, lse, c.nWin, 6, 32, c.scale, 16, 16, 4,
                                 ones_col=31, e_in=E_ACT, e_out=E_ACT)
        else:
            O = torch.full((c.nWin * 64, 192), NAN, device=dev, dtype=TDT[arith])
            H.window_attn_fwd(blk.to(TDT[arith]), c.table.to(dev), O, 192, lse, c.nWin, 6, 32, c.scale, 16, 16, 4,
                              ones_col=31)
    torch.cuda.synchronize()
    assert torch.isnan(O).all() and torch.isnan(lse).all()


# ---------------------------------------------------------------------------------------------------------------
# the A/B instantiations: read once per process, so a fresh child runs them
# ---------------------------------------------------------------------------------------------------------------
def child_main():
    """attn_bwd_bf16_kernel<4, 32> (KAIR_ATTN_BWD_NW=4) on (a)'s bf16 ws 8 case and a forced KAIR_ATTN_FWD_TPW on a
    (b) forward whose task count the forced value does not divide, at the same reference and bars."""
    assert os.environ.get("KAIR_ATTN_BWD_NW") == "4" and os.environ.get("KAIR_ATTN_FWD_TPW") == "3"
    bwd_multi_window_case("bf16", 8, "hp32", 3)
    for hp in (32, 16):
        st = fwd_multi_task_case(hp, 5, per_image_grid=(2, 2), bmin=8)
        assert st.eO < BARS["bf16"][0]
    print("CHILD OK")


def test_ab_instantiations_in_a_child_process():
    env = dict(os.environ, KAIR_ATTN_BWD_NW="4", KAIR_ATTN_FWD_TPW="3")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_window_attn_shapes_gpu as t; t.child_main()"
            % (here, os.path.dirname(here)))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(here), capture_output=True, text=True,
                       timeout=240)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "CHILD OK" in r.stdout
