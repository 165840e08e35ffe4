"""kair_amd/csrc/layernorm.hip end to end on the MI355X: kair_layernorm_fwd, kair_layernorm_fwd_x3, kair_layernorm_bwd,
its immediate parameter reducer and kair_ln_param_reduce_grouped against the float64 statements of
tests/layernorm_ref.py (pinned to torch by tests/test_layernorm_ref_cpu.py), on the exact fp32 / bf16-rounded values
the kernels are given (eps included: the float64 value of the fp32 1e-5 the C ABI passes).

Bars (L2-relative unless said otherwise): fp32 outputs, mean, rstd, dgamma, dbeta 2e-5 and bf16 outputs 2e-2 (TOL of
tests/test_kernels_gpu.py), the bf16 copy a quarter of that, pair forms 1e-6 (test_layernorm_x3_pair_forms).  dx is
an fp32 output whatever dy's dtype -- the reference takes the bf16-rounded dy -- so it is held to 2e-5 for both.
Per element, so that one wrong row cannot hide in a norm over 65k rows:
  fp32 forward   |y - ref| <= e32 = 16 2^-24 max|ref|
  bf16 forward   |y - ref| <= 2^-8 (|ref| + e32) + e32     (half a bf16 ulp of the fp32 result is <= 2^-8 |result|)
  backward dx    |dx - want| <= 16 2^-24 max|want|         (fewer than 8 fp32 operations per element on terms no
                 larger than the largest result, and two row means whose (log2 C + 4) roundings carry mean|g| <= that)
Every check prints its figure before it asserts.

The pair forward's "hi = fp16(ref32 2^e) within one fp16 ulp" cannot hold for elements where y nearly cancels to 0
(|y| ~ 1e-6 .. 1e-5 beside terms of order 1): there one fp32 rounding of the terms is several fp16 ulps of y 2^e, for
any fp32 evaluation.  Largest distance in fp16 ulps, M = 1000, e = 4, kernel on the MI355X / the reference formula
evaluated in fp32 on the CPU:  (C, ld) = (30, 32): 3 / 2;  (60, 60): 8 / 18;  (90, 96): 3 / 2;  (180, 180): 6 / 1;
(180, 192): 4 / 4;  1 / 1 at (4, 4), (60, 64), (64, 64), (68, 72).  A maximum over so few near-zero elements does not
scale from one evaluation to another, so the bar is per element: one fp16 ulp plus 4x the largest |y - ref| of that
CPU fp32 evaluation at the same shape (6.4e-7 .. 1.0e-6 at these shapes), times 2^e -- one ulp wherever y is not
tiny.

The reducers' bar 2^-22 sum|partials| per column assumed that fewer than ~4 roundings compound per element; the last
level of the tree adds its 32 row phases one after another, so an element passes through up to 32 adds on a growing
sum, and the kernel's figure in units of that bar is 1.00 .. 1.42 at 29 of the 60 (nb, C) shapes -- where
part.sum(0) in fp32 on the CPU loses 0.42 .. 1.04 itself.  At exactly those shapes the bar is 4x the CPU figure;
REDUCE_FP32_GAP lists each shape with both numbers (worst: nb = 289, C = 180: kernel 1.415, CPU 0.680; nb = 63,
C = 256: 1.361 / 0.635; nb = 255, C = 30: 1.114 / 1.040).  Every other shape keeps 2^-22 sum|partials|.

Which test reaches which path of the kernels:
  forward, two rows in flight and the 1024-block cap ........ test_fwd_row_counts (M = 16389, 32787)
  backward narrow form (C <= 64), its paired loop ........... test_bwd_row_counts[60-64-*], test_widths_bwd
  backward wide form's grid-stride loop (M > 32768) ......... test_bwd_row_counts[180-192-32773 / 65555]
  reducer regimes (8 in flight / pair loop / tail) .......... test_reduce_regimes, test_immediate_equals_deferred
  grouped block-to-job scan, mixed accumulate, 2C % 8 != 0 .. test_reduce_grouped_jobs, test_reduce_job_limit
  C % 4 != 0 (the straddling column group) .................. test_widths_fwd / test_widths_bwd (30, 32), (90, 96)
  window 7, H != W, shift 0 with a map ...................... test_window_maps, test_fwd_x3_pairs
  main map and a different copy map together ................ test_bwd_main_and_copy_maps
  dx_accumulate 0 / 1, dparam_accumulate 0 / 1, copies ...... test_bwd_options
  pad columns [C, ldy) written 0, ones column ............... test_widths_fwd
  the blocks * 2 * C workspace contract ..................... test_bwd_workspace_contract, test_bwd_blocks
  eps dominating, |mean| / sigma = 100 ...................... test_constant_rows, test_large_mean_rows
  argument checks ........................................... test_rejections, test_reduce_rejections
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import layernorm_ref as R  # noqa: E402
from kair_amd import _hip as H  # noqa: E402

dev = torch.device("cuda")
EPS = 1e-5
EPS32 = float(np.float32(EPS))   # what the kernel receives through the C ABI's float
TOL32, TOLBF, TOLPAIR = 2e-5, 2e-2, 1e-6
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
PADV = 1e3                       # pad columns of x and dy: finite, non-zero, must reach nothing
NAN = float("nan")
NOWIN = (0, 0, 0, 0)
U24 = 2.0 ** -24


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    if a.numel() == 0:
        return a.shape == b.shape and a.dtype == b.dtype
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def below(what, fig, bar):
    print(f"{what}: {fig:.3e} (bar {bar:.3e})")
    assert fig <= bar, f"{what}: {fig:.3e} > {bar:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# inputs and float64 references, computed once per shape and shared
# ---------------------------------------------------------------------------------------------------------------
def _finish_case(x, gamma, beta, dy, C, ld):
    M = x.shape[0]
    xp = torch.full((M, ld), PADV)
    xp[:, :C] = x
    y, mean, rstd = R.ln_fwd(x, gamma, beta, EPS32)
    return SimpleNamespace(M=M, C=C, ld=ld, x=x, gamma=gamma, beta=beta, dy=dy, y=y, mean=mean, rstd=rstd,
                           xd=xp.to(dev), gd=gamma.to(dev), bd=beta.to(dev), bwd={})


@functools.lru_cache(maxsize=8)
def _case(M, C, ld, dy_scale=1.0):
    g = torch.Generator().manual_seed(100003 * C + 1009 * ld + M)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(M, C, generator=g) * dy_scale
    return _finish_case(x, gamma, beta, dy, C, ld)


def _gap32(c):
    """max |y - ref| of the reference formula evaluated in fp32 on the CPU, on the case's inputs"""
    if "gap32" not in c.bwd:
        mu = c.x.mean(1, keepdim=True)
        var = ((c.x - mu) ** 2).mean(1, keepdim=True)
        y32 = (c.x - mu) * torch.rsqrt(var + EPS) * c.gamma + c.beta
        c.bwd["gap32"] = (y32.double() - c.y).abs().max().item()
    return c.bwd["gap32"]


def _bwd_ref(c, dt):
    """(the dy values the kernel is given in dtype dt, float64 dx, dgamma, dbeta), once per case and dtype"""
    if dt not in c.bwd:
        dyv = c.dy.to(DT[dt])
        c.bwd[dt] = (dyv,) + R.ln_bwd(c.x, dyv, c.gamma, EPS32)
    return c.bwd[dt]


# ---------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------
def run_fwd(c, kind, win=NOWIN, one_col=-1, ldy=None, x3_exp=0):
    """y (NaN-prefilled; kind 'x3': the [2, M, ldy] fp16 pair), mean, rstd"""
    ldy = ldy or c.ld
    mean, rstd = torch.full((c.M,), NAN, device=dev), torch.full((c.M,), NAN, device=dev)
    if kind == "x3":
        y = torch.full((2, c.M, ldy), NAN, device=dev, dtype=torch.float16)
        H.layernorm_fwd_x3(c.xd, c.ld, y, ldy, c.gd, c.bd, mean, rstd, c.M, c.C, EPS, win, one_col=one_col, x3_exp=x3_exp)
    else:
        y = torch.full((c.M, ldy), NAN, device=dev, dtype=DT[kind])
        H.layernorm_fwd(c.xd, c.ld, y, ldy, c.gd, c.bd, mean, rstd, c.M, c.C, EPS, win, one_col=one_col)
    torch.cuda.synchronize()
    return y, mean, rstd


def f16_ulp(v):
    """the fp16 ulp at |v| (float64 tensor): 2^(floor(log2 |v|) - 10), 2^-24 in the subnormal range"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(v), e - 11)


def check_fwd(c, kind, out, rows=None, one_col=-1, x3_exp=0, tag=""):
    y, mean, rstd = out
    C = c.C
    ref = c.y if rows is None else c.y[rows]
    below(f"{tag} mean", rel_err(mean, c.mean), TOL32)
    below(f"{tag} rstd", rel_err(rstd, c.rstd), TOL32)
    e32 = 16 * U24 * ref.abs().max().item()
    if kind == "x3":
        s = 2.0 ** x3_exp
        hi, lo = y[0].double().cpu(), y[1].double().cpu()
        full = hi + lo
        below(f"{tag} pair", rel_err(full[:, :C] / s, ref), TOLPAIR)
        want_hi = (ref.float() * s).to(torch.float16).double()
        d = (hi[:, :C] - want_hi).abs()
        ulp = torch.maximum(f16_ulp(want_hi), f16_ulp(hi[:, :C]))
        print(f"{tag} hi plane: {(d / ulp).max().item():.0f} fp16 ulps at most, fp32 formula gap {_gap32(c):.3e}")
        below(f"{tag} hi plane / (1 fp16 ulp + 4 x the fp32 gap)", (d / (ulp + 4 * _gap32(c) * s)).max().item(), 1.0)
        pads, one = full[:, C:], s
        assert (lo[:, C:] == 0).all()
    else:
        yc = y.double().cpu()
        below(f"{tag} y", rel_err(yc[:, :C], ref), TOL32 if kind == "f32" else TOLBF)
        err = (yc[:, :C] - ref).abs()
        if kind == "f32":
            below(f"{tag} y per element", err.max().item(), e32)
        else:
            below(f"{tag} y per element / bound", (err / (2.0 ** -8 * (ref.abs() + e32) + e32)).max().item(), 1.0)
        pads, one = yc[:, C:], 1.0
    want = torch.zeros_like(pads)
    if one_col >= 0:
        want[:, one_col - C] = one
    assert torch.equal(pads, want), f"{tag}: pad columns [C, ldy) are 0 but for the ones column"


def run_bwd(c, dt, win=NOWIN, rows=None, dx0=None, p0=None, p_acc=False, deferred=False, ws=None, copy=None, stats=None):
    """dx0 None: overwrite a NaN-filled dx; else accumulate onto dx0 [M, ld].  p0: the (dgamma, dbeta) prefill.
    rows: dy goes in window order (dy row r = token rows[r]).  Returns dx, dgamma, dbeta, ws."""
    M, C, ld = c.M, c.C, c.ld
    dyv = _bwd_ref(c, dt)[0]
    dyp = torch.full((M, ld), PADV, dtype=dyv.dtype)
    dyp[:, :C] = dyv if rows is None else dyv[rows]
    mean, rstd = stats if stats is not None else (c.mean.float().to(dev), c.rstd.float().to(dev))
    dx = torch.full((M, ld), NAN, device=dev) if dx0 is None else dx0.to(dev).clone()
    if deferred:
        dg = db = None
    elif p0 is not None:
        dg, db = p0[0].to(dev).clone(), p0[1].to(dev).clone()
    else:
        dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    if ws is None:
        ws = torch.empty(2 * 2048 * C, device=dev)
    H.layernorm_bwd(c.xd, ld, dyp.to(dev), ld, c.gd, mean, rstd, dx, ld, dx0 is not None, dg, db, p_acc, ws, M, C, win,
                    copy=copy)
    torch.cuda.synchronize()
    return dx, dg, db, ws


def check_bwd(c, dt, out, dx0=None, p0=None, p_acc=False, tag=""):
    dx, dg, db, _ = out
    C = c.C
    _, rdx, rdg, rdb = _bwd_ref(c, dt)
    want = rdx if dx0 is None else rdx + dx0[:, :C].double()
    got = dx[:, :C].double().cpu()
    below(f"{tag} dx", rel_err(got, want), TOL32)
    below(f"{tag} dx per element", (got - want).abs().max().item(), 16 * U24 * want.abs().max().item())
    if dx0 is not None:   # accumulating adds 0 to the pad columns of the straddling group and touches no other
        assert bits_equal(dx[:, C:].cpu(), dx0[:, C:])
    if dg is not None:
        wg, wb = (rdg + p0[0].double(), rdb + p0[1].double()) if p_acc else (rdg, rdb)
        below(f"{tag} dgamma", rel_err(dg, wg), TOL32)
        below(f"{tag} dbeta", rel_err(db, wb), TOL32)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# row-count regimes
# ---------------------------------------------------------------------------------------------------------------
FWD_M = [1, 5, 17, 512, 16384 + 5, 32768 + 16 + 3]
BWD_M = [5, 512, 32768 + 5, 65536 + 19]


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("M", FWD_M)
@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_fwd_row_counts(C, ld, M, kind):
    """The single-row tail alone (M <= 16 blocks), the paired loop (M > 16 x blocks), and past the 1024-block cap:
    one paired pass + a tail (16389) and two passes + a tail in two blocks (32787)."""
    c = _case(M, C, ld)
    out = run_fwd(c, kind, one_col=C)
    check_fwd(c, kind, out, one_col=C, tag=f"fwd {kind} M={M} C={C}")
    if M == FWD_M[-1]:
        again = run_fwd(c, kind, one_col=C)
        assert all(bits_equal(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M", BWD_M)
@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_bwd_row_counts(C, ld, M, dt):
    """Narrow form (C = 60): tail only, the paired loop (M > 16 x blocks happens past the 2048-block cap: 32773),
    two paired passes + tail (65555).  Wide form (C = 180): one, two and three trips of the grid-stride loop."""
    c = _case(M, C, ld)
    dx0 = _rand((M, ld), M + C)
    out = run_bwd(c, dt, dx0=dx0)
    check_bwd(c, dt, out, dx0=dx0, tag=f"bwd {dt} M={M} C={C}")
    if M == BWD_M[-1]:
        again = run_bwd(c, dt, dx0=dx0)
        nw = H.layernorm_bwd_blocks(M) * 2 * C
        assert all(bits_equal(a, b) for a, b in zip(out[:3], again[:3])) and bits_equal(out[3][:nw], again[3][:nw])


# ---------------------------------------------------------------------------------------------------------------
# widths
# ---------------------------------------------------------------------------------------------------------------
WIDTHS = [(4, 4), (30, 32), (60, 60), (60, 64), (64, 64), (68, 72), (90, 96), (180, 180), (180, 192), (180, 256), (256, 256)]


@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("C,ld", WIDTHS)
def test_widths_fwd(C, ld, kind):
    """x's pad columns hold 1e3 and reach no statistic; y's come back 0 from a NaN prefill, the ones column 1 (2^e)
    at C and at ldy - 1."""
    c = _case(1000, C, ld)
    e = 4 if kind == "x3" else 0
    for one_col in sorted({-1, C, ld - 1} if ld > C else {-1}):
        out = run_fwd(c, kind, one_col=one_col, x3_exp=e)
        check_fwd(c, kind, out, one_col=one_col, x3_exp=e, tag=f"fwd {kind} C={C} ld={ld} one_col={one_col}")


def test_fwd_distinct_strides():
    """ldx != ldy: the output's pad columns past x's stride are written too."""
    c = _case(1000, 180, 192)
    out = run_fwd(c, "f32", one_col=255, ldy=256)
    check_fwd(c, "f32", out, one_col=255, tag="fwd ldx=192 ldy=256")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,ld", WIDTHS)
def test_widths_bwd(C, ld, dt):
    """(64, 64) is the last narrow form, (68, 72) the first wide one; (30, 32) and (90, 96) have a column group
    straddling C.  Pad columns of x and dy hold 1e3."""
    c = _case(1000, C, ld)
    dx0 = _rand((1000, ld), 7 * C + ld)
    out = run_bwd(c, dt, dx0=dx0)
    check_bwd(c, dt, out, dx0=dx0, tag=f"bwd {dt} C={C} ld={ld}")


# ---------------------------------------------------------------------------------------------------------------
# window maps
# ---------------------------------------------------------------------------------------------------------------
MAPS = [(3, 16, 24, 8, 4), (3, 16, 24, 8, 0), (2, 14, 21, 7, 3), (1, 8, 8, 8, 0)]


@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
@pytest.mark.parametrize("geo", MAPS)
def test_window_maps(geo, C, ld):
    """Forward row r holds token window_rows[r] (mean / rstd by token); the backward reads dy in window order and
    writes dx by token, here on the forward kernel's own mean / rstd as the engine runs it."""
    B, Hh, Ww, ws, shift = geo
    rows = R.window_rows(*geo)
    c = _case(B * Hh * Ww, C, ld)
    win = (Hh, Ww, ws, shift)
    stats = None
    for kind in ("f32", "bf16"):
        out = run_fwd(c, kind, win=win, one_col=C)
        check_fwd(c, kind, out, rows=rows, one_col=C, tag=f"fwd {kind} {geo} C={C}")
        stats = stats or out[1:]
    for dt in ("f32", "bf16"):
        out = run_bwd(c, dt, win=win, rows=rows, stats=stats)
        check_bwd(c, dt, out, tag=f"bwd {dt} {geo} C={C}")


@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_bwd_main_and_copy_maps(C, ld):
    """dy through the shift-4 map, the copy through the shift-0 map of the same geometry, a scale per image."""
    B, Hh, Ww, ws = 3, 16, 24, 8
    M = B * Hh * Ww
    rows4, rows0 = R.window_rows(B, Hh, Ww, ws, 4), R.window_rows(B, Hh, Ww, ws, 0)
    c = _case(M, C, ld)
    sc = torch.tensor([0.5, 2.0, 1.25])
    cp = torch.zeros(M, ld, device=dev)
    dx0 = _rand((M, ld), 11 + C)
    out = run_bwd(c, "f32", win=(Hh, Ww, ws, 4), rows=rows4, dx0=dx0,
                  copy=H.copy_desc(cp, rowscale=sc.to(dev), rows_per_scale=Hh * Ww, win=(Hh, Ww, ws, 0)))
    check_bwd(c, "f32", out, dx0=dx0, tag=f"bwd two maps C={C}")
    want = (out[0].cpu() * sc.repeat_interleave(Hh * Ww)[:, None])[rows0]
    assert bits_equal(cp.cpu()[:, :C], want[:, :C])
    assert (cp[:, C:] == 0).all()   # the copy writes the C real columns only


@pytest.mark.parametrize("e", [0, 4])
@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192), (256, 256)])
@pytest.mark.parametrize("geo", MAPS)
def test_fwd_x3_pairs(geo, C, ld, e):
    """The fp16-pair forward against the float64 reference through window_rows (not through the fp32 kernel's map):
    (hi + lo) 2^-e at 1e-6, hi = fp16(y 2^e) within one fp16 ulp, the ones column 2^e."""
    B, Hh, Ww, ws, shift = geo
    c = _case(B * Hh * Ww, C, ld)
    one_col = C if ld > C else -1
    out = run_fwd(c, "x3", win=(Hh, Ww, ws, shift), one_col=one_col, x3_exp=e)
    check_fwd(c, "x3", out, rows=R.window_rows(*geo), one_col=one_col, x3_exp=e, tag=f"x3 {geo} C={C} e={e}")


# ---------------------------------------------------------------------------------------------------------------
# backward options
# ---------------------------------------------------------------------------------------------------------------
OPT_SHAPES = [(1000, 60, 64), (1000, 180, 192)]


@pytest.mark.parametrize("M,C,ld", OPT_SHAPES)
def test_bwd_options(M, C, ld):
    c = _case(M, C, ld)
    # dx_accumulate = 0 overwrites NaN; dparam_accumulate = 0 overwrites random values
    p0 = (_rand((C,), 1), _rand((C,), 2))
    out = run_bwd(c, "f32", p0=p0, p_acc=False)
    check_bwd(c, "f32", out, p0=p0, p_acc=False, tag=f"overwrite C={C}")
    assert out[0][:, C:].isnan().all()   # C % 4 == 0: no pad column of dx is written
    # dx_accumulate = 1 adds to random values; dparam_accumulate = 1 adds
    dx0 = _rand((M, ld), 3)
    out = run_bwd(c, "f32", dx0=dx0, p0=p0, p_acc=True)
    check_bwd(c, "f32", out, dx0=dx0, p0=p0, p_acc=True, tag=f"accumulate C={C}")
    # copies of the finished row, a scale per 250 rows (it changes inside a block's 16 rows)
    sc = torch.tensor([0.5, 2.0, -1.5, 0.75])
    scr = sc.repeat_interleave(250)[:, None]
    for cdt in (torch.float32, torch.bfloat16):
        cp = torch.zeros(M, ld, device=dev, dtype=cdt)
        out = run_bwd(c, "f32", dx0=dx0, copy=H.copy_desc(cp, rowscale=sc.to(dev), rows_per_scale=250))
        check_bwd(c, "f32", out, dx0=dx0, tag=f"copy {cdt} C={C}")
        fin = out[0].cpu()[:, :C]
        if cdt == torch.float32:
            assert bits_equal(cp.cpu()[:, :C], fin * scr)
        else:
            below(f"bf16 copy C={C}", rel_err(cp[:, :C], fin.double() * scr.double()), TOLBF / 4)
        assert (cp[:, C:] == 0).all()


@pytest.mark.parametrize("M,C,ld", OPT_SHAPES)
def test_bwd_pair_copy(M, C, ld):
    """The fp16-pair copy at exponent 20 of a gradient-sized dx (dy ~ 1e-5), overwriting dx."""
    c = _case(M, C, ld, 1e-5)
    sc = torch.tensor([0.5, 2.0, -1.5, 0.75])
    cp = torch.zeros(2, M, ld, device=dev, dtype=torch.float16)
    out = run_bwd(c, "f32", copy=H.copy_desc(cp, rowscale=sc.to(dev), rows_per_scale=250, x3_exp=20))
    check_bwd(c, "f32", out, tag=f"pair copy C={C}")
    want = out[0].double().cpu()[:, :C] * sc.double().repeat_interleave(250)[:, None]
    got = (cp[0].double() + cp[1].double()).cpu() * 2.0 ** -20
    assert torch.isfinite(got).all()
    below(f"pair copy C={C}", rel_err(got[:, :C], want), TOLPAIR)
    assert (got[:, C:] == 0).all()


def test_bwd_blocks():
    for M in (1, 16, 17, 32768, 32769, 10 ** 6):
        assert H.layernorm_bwd_blocks(M) == min(-(-M // 16), 2048)


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("M,C,ld", [(1000, 60, 64), (1000, 180, 192), (32768 + 5, 60, 64)])
def test_bwd_workspace_contract(M, C, ld, deferred):
    """kair_layernorm_bwd_blocks(M) * 2 * C floats of workspace are enough: the same bits as with 2 * 2048 * C, and
    the NaN guard behind them in the same allocation keeps every bit."""
    c = _case(M, C, ld)
    n = H.layernorm_bwd_blocks(M) * 2 * C
    big = run_bwd(c, "f32", deferred=deferred)
    buf = torch.full((n + 4096,), NAN, device=dev)
    guard = buf[n:].clone()
    out = run_bwd(c, "f32", deferred=deferred, ws=buf[:n])
    check_bwd(c, "f32", out, tag=f"exact ws M={M} C={C}")
    assert bits_equal(out[0], big[0]) and bits_equal(buf[:n], big[3][:n])
    assert not buf[:n].isnan().any()   # every partial the reducers read was written
    if not deferred:
        assert bits_equal(out[1], big[1]) and bits_equal(out[2], big[2])
    assert bits_equal(buf[n:], guard)


# ---------------------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_constant_rows(C, ld):
    """Variance 0: rstd = eps^-1/2 and y = beta.  The constants are small multiples of 1/4, so every fp32 partial sum
    and the mean are exact and y equals beta up to the final rounding (2^-24 |beta|; in fact bit for bit)."""
    M = 1000
    g = torch.Generator().manual_seed(5 + C)
    x = (((torch.arange(M) % 17) - 8) / 4.0)[:, None].expand(M, C).contiguous()
    c = _finish_case(x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1,
                     torch.randn(M, C, generator=g), C, ld)
    y, mean, rstd = run_fwd(c, "f32")
    assert torch.equal(mean.cpu(), x[:, 0])
    below("constant rows rstd", rel_err(rstd, c.rstd), TOL32)
    d = (y[:, :C].double().cpu() - c.beta.double()).abs() / c.beta.double().abs()
    below("constant rows |y - beta| / |beta|", d.max().item(), U24)
    out = run_bwd(c, "f32", stats=(mean, rstd))
    assert torch.isfinite(out[0][:, :C]).all()
    check_bwd(c, "f32", out, tag=f"constant rows C={C}")


K_COND = {60: 11.3, 180: 13.2}


@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_large_mean_rows(C, ld):
    """Rows with |mean| / sigma ~ 100 (mean 10, sigma 0.1).  An fp32 mean is off by ~2^-24 |mean|, which moves xhat by
    that over sigma, so per element  |y - ref| <= k 2^-24 (|mean| / sigma + sqrt C) max|gamma|  with the row's own
    |mean| rstd for |mean| / sigma.  k is 4x what torch.nn.functional.layer_norm in fp32 on the CPU loses against the
    float64 reference on these same inputs, in the same units: it loses 2.82 (C = 60) and 3.30 (C = 180), so
    k = 11.3 and 13.2 (a different, valid summation order may lose that much more).  The plain formula evaluated in
    fp32 on the CPU loses 3.19 and 2.84; the kernel measured 2.40 (C = 60) and 1.79 (C = 180) on the MI355X."""
    M = 1000
    g = torch.Generator().manual_seed(900 + C)
    x = 10 + 0.1 * torch.randn(M, C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    c = _finish_case(x, gamma, beta, torch.randn(M, C, generator=g), C, ld)
    y, mean, rstd = run_fwd(c, "f32")
    unit = U24 * (c.mean.abs() * c.rstd + math.sqrt(C)) * gamma.max().double()
    fig = ((y[:, :C].double().cpu() - c.y).abs() / unit[:, None]).max().item()
    below(f"|mean|/sigma = 100, C={C}: |y - ref| in units of 2^-24 (|mean|/sigma + sqrt C) max|gamma|", fig, K_COND[C])
    below("mean", rel_err(mean, c.mean), TOL32)


# ---------------------------------------------------------------------------------------------------------------
# parameter reducers
# ---------------------------------------------------------------------------------------------------------------
def _partials(nb, C, seed):
    """[nb, 2C] fp32 with mean 3: a dropped or doubled row moves a column sum by ~3, far beyond rounding"""
    return _rand((nb, 2 * C), seed) + 3.0


def _reduce_figure(part, C, dg, db, dg0=None, db0=None):
    """max over the 2C columns ([0, C) -> dgamma, [C, 2C) -> dbeta) of |got - float64 sum| / (2^-22 sum|partials|),
    an accumulated prefill counted as one more partial"""
    p = part.double()
    want, mag = p.sum(0), p.abs().sum(0)
    if dg0 is not None:
        pre = torch.cat([dg0, db0]).double()
        want, mag = want + pre, mag + pre.abs()
    got = torch.cat([dg, db]).double().cpu()
    return ((got - want).abs() / (2.0 ** -22 * mag)).max().item()


def _check_reduce(part, C, dg, db, dg0=None, db0=None, tag=""):
    """For the grouped-launch tests, whose shapes are not test_reduce_regimes' grid: the rigorous bound of a fixed summation
    tree, height x 2^-24 x sum|partials| -- an element passes through at most ceil(nb / 64) adds in its thread, one
    s0 + s1, 32 adds over the row phases and one for an accumulated prefill.  A dropped or doubled partial row moves
    the sum by ~1 / nb of sum|partials|, over 100x this bound even at nb = 2048."""
    height = -(-part.shape[0] // 64) + 34
    below(f"{tag} column sums / (2^-22 sum|partials|)", _reduce_figure(part, C, dg, db, dg0, db0), height / 4)


NBS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 289, 2048]
# Shapes at which the kernel's fixed-order fp32 sum misses 2^-22 sum|partials|: (nb, C) -> (the kernel's figure on the
# MI355X, the figure of part.sum(0) in fp32 on the CPU against the same float64 sums), both in units of that bar.
# Their bar is 4x the CPU figure (module docstring).
REDUCE_FP32_GAP = {
    (31, 60): (1.044, 0.510), (31, 180): (1.131, 0.698), (31, 256): (1.113, 0.680),
    (32, 30): (1.076, 0.583), (32, 60): (1.009, 0.530), (32, 180): (1.179, 0.634), (32, 256): (1.184, 0.678),
    (33, 256): (1.144, 0.830),
    (63, 60): (1.004, 0.491), (63, 180): (1.265, 0.675), (63, 256): (1.361, 0.635),
    (64, 60): (1.068, 0.419), (64, 256): (1.195, 0.680),
    (65, 60): (1.028, 0.621), (65, 180): (1.152, 0.635), (65, 256): (1.137, 0.755),
    (255, 30): (1.114, 1.040), (255, 60): (1.230, 0.814), (255, 180): (1.159, 0.861), (255, 256): (1.173, 0.727),
    (256, 60): (1.074, 0.949), (256, 180): (1.183, 0.886), (256, 256): (1.218, 0.840),
    (257, 60): (1.059, 0.719), (257, 180): (1.066, 0.898),
    (289, 180): (1.415, 0.680),
    (2048, 60): (1.045, 0.550), (2048, 180): (1.087, 0.697), (2048, 256): (1.028, 0.609),
}


@pytest.mark.parametrize("C", [1, 30, 60, 180, 256])
@pytest.mark.parametrize("nb", NBS)
def test_reduce_regimes(nb, C):
    """The single-load tail (nb <= 32), the pair loop (33 .. 256), the 8-in-flight loop (> 256) and their seams, each
    column sum within 2^-22 sum|partials| of the float64 sum (4x the CPU fp32 figure at the REDUCE_FP32_GAP shapes)."""
    part = _partials(nb, C, 31 * nb + C)
    dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    H.ln_param_reduce_grouped([(part.to(dev), 0, C, dg, db, False, nb)])
    torch.cuda.synchronize()
    bar = 4 * REDUCE_FP32_GAP[nb, C][1] if (nb, C) in REDUCE_FP32_GAP else 1.0
    below(f"nb={nb} C={C} column sums / (2^-22 sum|partials|)", _reduce_figure(part, C, dg, db), bar)


def _job_buffers(C, seed):
    """dgamma / dbeta as views into random-filled allocations with 8 floats of guard on either side"""
    buf = _rand((2, C + 16), seed).to(dev)
    return buf, buf[0, 8:8 + C], buf[1, 8:8 + C]


def test_reduce_grouped_jobs():
    """Five jobs of different (C, nb) and mixed accumulate flags in one launch: each equals its own single-job launch
    bit for bit (a wrong block-to-job scan reads another job's partials), and nothing outside [0, C) is written."""
    spec = [(180, 289, True), (60, 33, False), (1, 2048, True), (30, 257, False), (256, 5, True)]
    parts = [_partials(nb, C, 77 + i).to(dev) for i, (C, nb, _) in enumerate(spec)]
    grouped = [_job_buffers(C, 500 + i) for i, (C, _, _) in enumerate(spec)]
    single = [_job_buffers(C, 500 + i) for i, (C, _, _) in enumerate(spec)]
    H.ln_param_reduce_grouped([(p, 0, C, b[1], b[2], acc, nb) for p, (C, nb, acc), b in zip(parts, spec, grouped)])
    for p, (C, nb, acc), b in zip(parts, spec, single):
        H.ln_param_reduce_grouped([(p, 0, C, b[1], b[2], acc, nb)])
    torch.cuda.synchronize()
    for i, ((C, nb, acc), p, gb, sb) in enumerate(zip(spec, parts, grouped, single)):
        pre = _rand((2, C + 16), 500 + i)
        assert bits_equal(gb[0], sb[0]), f"job {i}"
        for t in (0, 1):
            assert bits_equal(gb[0][t, :8].cpu(), pre[t, :8]) and bits_equal(gb[0][t, 8 + C:].cpu(), pre[t, 8 + C:])
        pg, pb = (pre[0, 8:8 + C], pre[1, 8:8 + C]) if acc else (None, None)
        _check_reduce(p.cpu(), C, gb[1], gb[2], pg, pb, tag=f"job {i}")


def test_reduce_job_limit():
    """32 jobs in one launch pass; 33 are refused before anything is launched."""
    Cs, nbs = [1, 30, 60, 180, 256, 7], [1, 33, 257, 64, 300]
    spec = [(Cs[i % len(Cs)], nbs[i % len(nbs)]) for i in range(33)]
    parts = [_partials(nb, C, 900 + i) for i, (C, nb) in enumerate(spec)]
    outs = [(torch.full((C,), 7.0, device=dev), torch.full((C,), 7.0, device=dev)) for C, _ in spec]
    jobs = [(p.to(dev), 0, C, o[0], o[1], False, nb) for p, (C, nb), o in zip(parts, spec, outs)]
    H.ktime_begin(8)
    try:
        with pytest.raises(RuntimeError, match="ln_param_reduce_grouped"):
            H.ln_param_reduce_grouped(jobs)
    finally:
        n = H.ktime_end()
    torch.cuda.synchronize()
    assert n == 0 and all((o[0] == 7).all() and (o[1] == 7).all() for o in outs)
    H.ln_param_reduce_grouped(jobs[:32])
    torch.cuda.synchronize()
    for i in range(32):
        _check_reduce(parts[i], spec[i][0], *outs[i], tag=f"job {i} of 32")
    assert (outs[32][0] == 7).all() and (outs[32][1] == 7).all()


@pytest.mark.parametrize("M", [1000, 65536 + 19])
@pytest.mark.parametrize("C,ld", [(60, 64), (180, 192)])
def test_immediate_equals_deferred(C, ld, M):
    """dgamma / dbeta from kair_layernorm_bwd itself, and from the same call with NULL + a grouped reduce of its
    partials: the header promises the same sums."""
    c = _case(M, C, ld)
    now = run_bwd(c, "f32")
    later = run_bwd(c, "f32", deferred=True)
    dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    H.ln_param_reduce_grouped([(later[3], M, C, dg, db, False)])
    torch.cuda.synchronize()
    assert bits_equal(now[0], later[0]) and bits_equal(dg, now[1]) and bits_equal(db, now[2])
    _, _, rdg, rdb = _bwd_ref(c, "f32")
    below("dgamma", rel_err(dg, rdg), TOL32)
    below("dbeta", rel_err(db, rdb), TOL32)


# ---------------------------------------------------------------------------------------------------------------
# rejections: an error, no launch, every output as it was
# ---------------------------------------------------------------------------------------------------------------
class _Reject:
    """Buffers for M = 1000 rows allocated as 1152 x 260 (three whole 16 x 24 images, the widest stride any case
    names), so that no case could leave its allocations even if a check were missing."""
    ROWS, LD = 1152, 260

    def __init__(self):
        z = lambda dt=torch.float32: torch.full((self.ROWS, self.LD), 3.0, device=dev, dtype=dt)
        self.x, self.dy = _rand((self.ROWS, self.LD), 1).to(dev), _rand((self.ROWS, self.LD), 2).to(dev)
        self.gamma, self.beta = torch.ones(256, device=dev), torch.zeros(256, device=dev)
        self.out = dict(y=z(), ybf=z(torch.bfloat16), yhi=torch.full((2, self.ROWS, self.LD), 3.0, device=dev, dtype=torch.float16),
                        mean=torch.full((self.ROWS,), 3.0, device=dev), rstd=torch.full((self.ROWS,), 3.0, device=dev),
                        dx=z(), dg=torch.full((256,), 3.0, device=dev), db=torch.full((256,), 3.0, device=dev),
                        ws=torch.full((2 * 2048 * 256,), 3.0, device=dev), cp=z(), cph=torch.full((2, self.ROWS, self.LD), 3.0, device=dev, dtype=torch.float16))

    def fwd(self, C=180, ldx=192, ldy=192, M=1000, win=NOWIN, one_col=-1, x3=False, x3_exp=0, bf=False):
        o = self.out
        if x3:
            H.layernorm_fwd_x3(self.x, ldx, o["yhi"], ldy, self.gamma, self.beta, o["mean"], o["rstd"], M, C, EPS, win,
                               one_col=one_col, x3_exp=x3_exp)
        else:
            H.layernorm_fwd(self.x, ldx, o["ybf"] if bf else o["y"], ldy, self.gamma, self.beta, o["mean"], o["rstd"], M, C,
                            EPS, win, one_col=one_col)

    def bwd(self, C=180, ldx=192, ldy=192, ld_dx=192, M=1000, win=NOWIN, dg=True, db=True, copy=None):
        o = self.out
        H.layernorm_bwd(self.x, ldx, self.dy, ldy, self.gamma, o["mean"], o["rstd"], o["dx"], ld_dx, True,
                        o["dg"] if dg else None, o["db"] if db else None, False, o["ws"], M, C, win, copy=copy)

    def pair_copy_without_lo(self):
        d = H.copy_desc(self.out["cph"], ld=192, x3_exp=20)
        d.out_lo = None
        return d


REJECT = {
    # sizes and pointers the entry points already refused
    "fwd C=0": lambda r: r.fwd(C=0),
    "fwd C=257": lambda r: r.fwd(C=257, ldx=260, ldy=260),
    "fwd ldy=260": lambda r: r.fwd(ldy=260),
    "fwd ldx%4": lambda r: r.fwd(ldx=190),
    "fwd ldy%4": lambda r: r.fwd(ldy=190, bf=True),
    "fwd one_col<C": lambda r: r.fwd(one_col=179),
    "fwd one_col>=ldy": lambda r: r.fwd(one_col=192),
    "fwd_x3 one_col<C": lambda r: r.fwd(one_col=100, x3=True),
    "fwd_x3 C=0": lambda r: r.fwd(C=0, x3=True),
    "fwd_x3 ldy=260": lambda r: r.fwd(ldy=260, x3=True),
    "fwd_x3 x3_exp=100": lambda r: r.fwd(x3=True, x3_exp=100),
    "fwd window geometry": lambda r: r.fwd(M=960, win=(20, 24, 8, 4)),
    "bwd C=0": lambda r: r.bwd(C=0),
    "bwd C=257": lambda r: r.bwd(C=257, ldx=260, ldy=260, ld_dx=260),
    "bwd ldx%4": lambda r: r.bwd(ldx=190),
    "bwd dgamma without dbeta": lambda r: r.bwd(db=False),
    "bwd dbeta without dgamma": lambda r: r.bwd(dg=False),
    "bwd copy stride<C": lambda r: r.bwd(copy=H.copy_desc(r.out["cp"], ld=176)),
    "bwd copy stride%4": lambda r: r.bwd(copy=H.copy_desc(r.out["cp"], ld=190)),
    "bwd pair copy without out_lo": lambda r: r.bwd(copy=r.pair_copy_without_lo()),
    "bwd copy window geometry": lambda r: r.bwd(M=960, copy=H.copy_desc(r.out["cp"], ld=192, win=(20, 24, 8, 0))),
    # the checks added to layernorm.hip together with this file
    "bwd ldx<C": lambda r: r.bwd(ldx=176),
    "bwd ldy<C": lambda r: r.bwd(ldy=176),
    "bwd ld_dx<C": lambda r: r.bwd(ld_dx=176),
    "bwd window geometry": lambda r: r.bwd(M=960, win=(20, 24, 8, 4)),
    "fwd M%(H W)": lambda r: r.fwd(win=(16, 24, 8, 4)),
    "fwd_x3 M%(H W)": lambda r: r.fwd(win=(16, 24, 8, 0), x3=True),
    "bwd M%(H W)": lambda r: r.bwd(win=(16, 24, 8, 4)),
    "bwd copy M%(H W)": lambda r: r.bwd(copy=H.copy_desc(r.out["cp"], ld=192, win=(16, 24, 8, 0))),
    "fwd map with H=0": lambda r: r.fwd(win=(0, 24, 8, 0)),
}


@pytest.fixture(scope="module")
def rejector():
    return _Reject()


@pytest.mark.parametrize("name", list(REJECT))
def test_rejections(rejector, name):
    H.ktime_begin(8)
    try:
        with pytest.raises(RuntimeError, match="layernorm_(fwd|fwd_x3|bwd)"):
            REJECT[name](rejector)
    finally:
        n = H.ktime_end()
    torch.cuda.synchronize()
    assert n == 0
    for k, t in rejector.out.items():
        assert (t == 3).all(), f"{name}: {k} was written"


def test_rejector_accepts_good_calls():
    """The rejection cases' base calls are valid: each case is refused for the one thing it changes."""
    r = _Reject()
    r.fwd(M=1152, win=(16, 24, 8, 4), one_col=180)
    r.fwd(M=1152, win=(16, 24, 8, 4), one_col=180, x3=True, x3_exp=4)
    r.fwd(bf=True)
    r.bwd(M=1152, win=(16, 24, 8, 4), copy=H.copy_desc(r.out["cp"], ld=192, win=(16, 24, 8, 0)))
    r.bwd(copy=H.copy_desc(r.out["cph"], ld=192, x3_exp=4))
    torch.cuda.synchronize()
    assert not (r.out["y"][:1000, :180] == 3).all() and not (r.out["dx"][:1000, :180] == 3).all()


@pytest.mark.parametrize("bad", ["njobs=0", "C=300", "nb=0", "C=0"])
def test_reduce_rejections(bad):
    part = torch.full((64, 600), 3.0, device=dev)
    dg, db = torch.full((300,), 3.0, device=dev), torch.full((300,), 3.0, device=dev)
    good = (part, 0, 60, dg, db, False, 64)
    jobs = {"njobs=0": [], "C=300": [good, (part, 0, 300, dg, db, False, 64)], "nb=0": [good, (part, 0, 60, dg, db, False, 0)],
            "C=0": [(part, 0, 0, dg, db, False, 64)]}[bad]
    H.ktime_begin(8)
    try:
        with pytest.raises(RuntimeError, match="ln_param_reduce_grouped"):
            H.ln_param_reduce_grouped(jobs)
    finally:
        n = H.ktime_end()
    torch.cuda.synchronize()
    assert n == 0 and (dg == 3).all() and (db == 3).all()
