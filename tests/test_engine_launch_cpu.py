"""The GEMM launch layer of EngineBase (_nt, _wgrad): which compute enum and which fp32x3 exponents reach
kair_gemm_nt / kair_gemm_tn / kair_wgrad_finalize.  No GPU and no library: the _hip entry points are replaced by
recorders, operands and epilogues are plain namespaces."""
import types

import pytest
import torch.nn as nn

from kair_amd import _hip as H
from kair_amd.engine.base import EngineBase

CD = 77     # a compute enum no kernel has: whatever _nt passes on must be the engine's own `cd`
UNSET = "unset"


class _Trivial(EngineBase):
    COMPUTE_DTYPES = ("bf16", "fp32", "fp32x3")

    def __init__(self, compute_dtype):
        self.net = nn.Linear(2, 2)      # (EngineBase keeps a weak reference)
        super().__init__(self.net, compute_dtype)
        self.cd = CD


def op(dtype=H.F32, lo_ptr=None, ones_col=-1):
    return types.SimpleNamespace(dtype=dtype, lo_ptr=lo_ptr, ones_col=ones_col, x3_exp=UNSET)


def epi(out_dtype=H.F32):
    return types.SimpleNamespace(out_dtype=out_dtype, x3_out_exp=UNSET)


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(H, "gemm_nt", lambda *a: rec.append(("nt",) + a))
    monkeypatch.setattr(H, "gemm_tn", lambda *a: rec.append(("tn",) + a))
    monkeypatch.setattr(H, "wgrad_finalize", lambda *a, **kw: rec.append(("fin", a, kw)))
    monkeypatch.setattr(H, "wgrad_splits", lambda M, N, K: 8)
    monkeypatch.setattr(H, "wgrad_tiles", lambda N, K: 2)
    return rec


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_nt_launches_in_cd_and_leaves_the_exponents(calls, dt):
    eng = _Trivial(dt)
    A, B, E = op(H.F16), op(), epi(H.F16)     # (no check is made off fp32x3)
    eng._nt(A, B, E, 5, 6, 7)
    assert calls == [("nt", A, B, E, 5, 6, 7, CD)]
    assert (A.x3_exp, B.x3_exp, E.x3_out_exp) == (UNSET, UNSET, UNSET)
    assert eng.tn_cd == CD


def test_nt_x3_sets_exponents_and_launches_in_x3(calls):
    eng = _Trivial("fp32x3")
    eng._ax = 11
    A, B, E = op(), op(), epi(H.F32)
    eng._nt(A, B, E, 5, 6, 7)
    assert calls == [("nt", A, B, E, 5, 6, 7, H.X3)]
    assert (A.x3_exp, B.x3_exp, E.x3_out_exp) == (11, H.X3_WEXP, UNSET)     # an fp32 output carries no exponent
    A, E = op(H.F16, lo_ptr=1234), epi(H.F16)
    eng._nt(A, B, E, 5, 6, 7)
    assert (A.x3_exp, E.x3_out_exp) == (11, 11)
    assert eng.tn_cd == H.X3


def test_nt_x3_refuses_an_unpaired_fp16_operand_and_a_ones_column(calls):
    eng = _Trivial("fp32x3")
    with pytest.raises(RuntimeError, match="lo plane"):
        eng._nt(op(H.F16), op(), epi(), 5, 6, 7)
    with pytest.raises(RuntimeError, match="ones column"):
        eng._nt(op(ones_col=3), op(), epi(), 5, 6, 7)
    assert calls == []


def test_wgrad_exponents_and_the_act_rows_swap(calls):
    eng = _Trivial("fp32x3")
    P = {"wg_ws": "ws", "e_g": 21}
    A, Bop = op(), op()
    eng._wgrad(P, A, Bop, 100, 16, 32, "map", "grad")
    assert (A.x3_exp, Bop.x3_exp) == (21, eng.X3_AEXP)               # (gradient, activation)
    assert calls[0] == ("tn", A, Bop, "ws", 8, 100, 16, 32, H.X3)
    assert calls[1] == ("fin", ("ws", 8, "map", "grad", None, -1), {"accumulate": False})
    eng._wgrad(P, A, Bop, 100, 16, 32, "map", "grad", act_rows=True)
    assert (A.x3_exp, Bop.x3_exp) == (eng.X3_AEXP, 21)               # the transposed conv: (activation, gradient)
    A, Bop = op(), op()
    eng._wgrad({"wg_ws": "ws"}, A, Bop, 100, 16, 32, "map", "grad")  # a plan without an exponent yet
    assert (A.x3_exp, Bop.x3_exp) == (0, eng.X3_AEXP)
    off = _Trivial("bf16")
    A, Bop = op(), op()
    off._wgrad(P, A, Bop, 100, 16, 32, "map", "grad")
    assert (A.x3_exp, Bop.x3_exp) == (UNSET, UNSET) and calls[-2][-1] == CD


@pytest.mark.parametrize("max_ctas,M,splits", [(0, 100, 8), (6, 100, 3), (1, 100, 1), (-2, 100, 4), (-2, 10 ** 6, 16)])
def test_wgrad_split_count(calls, max_ctas, M, splits):
    """8 splits of 2 tiles each: a cap of 6 workgroups leaves 3 splits (never fewer than 1); -2 doubles them, but no
    split is shorter than 32 rows (M = 100: 4 splits)."""
    _Trivial("fp32")._wgrad({"wg_ws": "ws"}, op(), op(), M, 16, 32, "map", "grad", max_ctas=max_ctas)
    assert calls[0][4] == splits and calls[1][1][1] == splits


def test_wgrad_forwards_workspace_bias_and_accumulate(calls):
    eng = _Trivial("fp32")
    eng._wgrad({"wg_ws": "ws"}, op(), op(), 100, 16, 32, "map", "grad", "bgrad", 5, ws="side", acc=True)
    assert calls[0][3] == "side"
    assert calls[1] == ("fin", ("side", 8, "map", "grad", "bgrad", 5), {"accumulate": True})
