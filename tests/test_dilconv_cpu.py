"""tests/dilconv_ref.py pinned to torch's float64 autograd, and the host side of kair_operand.im_dil: H.im2col(dil=)
sets the field, and a dilation outside 0..4 is an argument error of kair_gemm_nt / kair_gemm_tn raised on the host,
before any launch (no GPU needed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import dilconv_ref as D
from kair_amd import _hip as H


@pytest.mark.parametrize("d", D.DILS)
def test_gradient_statements_match_autograd(d):
    """Input and weight gradient of a dilated conv on a 2 x 5 x 7 x 6 input (taps leave the grid on every side; at
    d = 3, 4 whole tap rows do)."""
    g = D.gen(40 + d)
    x = torch.randn(2, 5, 7, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 4, 7, 6, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, padding=d, dilation=d)
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    assert torch.equal(D.fwd(x.detach(), w.detach(), b, d)[0], y.detach())
    torch.testing.assert_close(D.dgrad(gy, w.detach(), d)[0], gx, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(D.wgrad(gy, x.detach(), d)[0], gw, rtol=1e-12, atol=1e-12)
    # the magnitude sums bound the values
    for (v, S) in (D.fwd(x.detach(), w.detach(), b, d), D.dgrad(gy, w.detach(), d), D.wgrad(gy, x.detach(), d)):
        assert bool((S + 1e-12 >= v.abs()).all())


def test_im2col_sets_the_field():
    t = torch.zeros(4 * 4, 8)
    assert H.im2col(t, 4, 4, 8).im_dil == 0
    assert H.im2col(t, 4, 4, 8, dil=1).im_dil == 0          # the bytes every earlier caller passed
    assert bytes(H.im2col(t, 4, 4, 8, dil=1)) == bytes(H.im2col(t, 4, 4, 8))
    for d in (2, 3, 4):
        o = H.im2col(t, 4, 4, 8, flip=True, dil=d)
        assert (o.im_dil, o.im_flip, o.im_H, o.im_W, o.im_C) == (d, 1, 4, 4, 8)
    assert H.Operand._fields_[-1] == ("im_dil", ctypes.c_int)


@pytest.mark.parametrize("dil", [5, -1, -3, 17])
def test_bad_dilation_is_an_argument_error_on_the_host(dil):
    """No device pointer is ever dereferenced: the operands are host tensors and the call must return KAIR_ERR_ARG from
    kair_check_operand."""
    L = H.lib()
    x, w, out, ws = torch.zeros(16, 8), torch.zeros(8, 72), torch.zeros(16, 8), torch.zeros(8 * 72)
    A = H.im2col(x, 4, 4, 8, dil=dil)
    rc = L.kair_gemm_nt(ctypes.byref(A), ctypes.byref(H.rows(w)), ctypes.byref(H.epilogue(out)), 16, 8, 72, H.F32, None)
    assert rc == -1, rc     # KAIR_ERR_ARG
    assert b"dilation" in L.kair_last_error()
    rc = L.kair_gemm_tn(ctypes.byref(H.rows(out)), ctypes.byref(A), ws.data_ptr(), 1, 16, 8, 72, H.F32, None)
    assert rc == -1, rc
    assert b"dilation" in L.kair_last_error()


def test_dilation_with_upsample_or_x3_is_an_argument_error():
    L = H.lib()
    x, w, out = torch.zeros(16, 8), torch.zeros(8, 72), torch.zeros(16, 8)
    A = H.im2col(x, 4, 4, 8, dil=2, up=2)
    assert L.kair_gemm_nt(ctypes.byref(A), ctypes.byref(H.rows(w)), ctypes.byref(H.epilogue(out)), 16, 8, 72, H.F32, None) == -1
    assert b"upsample" in L.kair_last_error()
    A = H.im2col(x, 4, 4, 8, dil=2)
    assert L.kair_gemm_nt(ctypes.byref(A), ctypes.byref(H.rows(w)), ctypes.byref(H.epilogue(out)), 16, 8, 72, H.X3, None) == -1
    assert b"fp32x3" in L.kair_last_error()


def test_conv3x3_dil_contract_on_the_host():
    assert [H.conv3x3_dil_ok(d, 64, 64) for d in (1, 2, 3, 4, 5)] == [False, True, True, True, False]
    assert not H.conv3x3_dil_ok(2, 32, 64) and not H.conv3x3_dil_ok(2, 64, 48)
