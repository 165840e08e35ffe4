"""The engine protocol is single-sourced in kair_amd/engine/base.py: the four step programs derive from EngineBase,
the fp32x3 exponent state / range-guard reaction / pack() exist once, and the conv engines do not import the SwinIR
module.  No GPU: EngineBase.__init__ does no device work."""
import math
import os
import re
import subprocess
import sys
import types

import pytest
import torch.nn as nn

from kair_amd.engine.base import ConvEngineBase, EngineBase
from kair_amd.engine.dncnn_engine import DnCNNEngine, FFDNetEngine
from kair_amd.engine.drunet_engine import DRUNetEngine
from kair_amd.engine.resunet import ResUNetProgram
from kair_amd.engine.rrdbnet_engine import RRDBNetEngine
from kair_amd.engine.swinir_engine import SwinIREngine
from kair_amd.engine.usrnet_engine import USRNetEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = (SwinIREngine, RRDBNetEngine, DnCNNEngine, USRNetEngine)
X3_ALL = ("bf16", "fp32", "fp32x3")


class _Trivial(EngineBase):
    COMPUTE_DTYPES = X3_ALL

    def convs(self):
        return []

    def _build_plan(self, key, infer):
        return {"key": key, "infer": infer}


def test_inheritance_and_single_definitions():
    for cls in ENGINES:
        assert issubclass(cls, EngineBase)
        for name in ("x3_backoff", "_x3_grad_exp", "pack", "_e", "X3_BACKOFF_STEP", "X3_BACKOFF_MAX"):
            assert name not in vars(cls), (cls.__name__, name)
    for cls in (RRDBNetEngine, DnCNNEngine, USRNetEngine):
        assert issubclass(cls, ConvEngineBase)
    assert not issubclass(SwinIREngine, ConvEngineBase)
    for cls in ENGINES + (ConvEngineBase, ResUNetProgram, FFDNetEngine, DRUNetEngine):   # the launch layer: base.py only
        for name in ("_nt", "_wgrad"):
            assert name in vars(EngineBase) and name not in vars(cls), (cls.__name__, name)
        assert ("conv_wgrad" in vars(cls)) == (cls is ConvEngineBase), cls.__name__
    assert "conv_wgrad" not in vars(EngineBase)
    assert [cls.COMPUTE_DTYPES for cls in ENGINES] == [X3_ALL, X3_ALL, ("bf16", "fp32"), X3_ALL]
    assert (EngineBase.X3_AEXP, EngineBase.X3_BACKOFF_STEP, EngineBase.X3_BACKOFF_MAX) == (4, 6, 4)


def test_base_init_state_and_plan():
    net = nn.Linear(2, 2)
    eng = _Trivial(net, "bf16")
    assert eng.net_ref() is net and not eng.x3
    assert eng.blocks == [] and eng.seg_hook is None and eng.repack_always is False
    assert eng.plan_mode == "primary" and eng._packed_version is None and eng._pack_table is None
    assert eng.pack_jobs() == []
    P = eng.plan(2, 3, 4, 5, 6, 7)   # a key of any length (USRNet's has six parts)
    assert P == {"key": (2, 3, 4, 5, 6, 7), "infer": False} and eng.plan(2, 3, 4, 5, 6, 7) is P
    with pytest.raises(ValueError):
        _Trivial(net, "fp16")
    with pytest.raises(ValueError):
        EngineBase(net, "fp32")      # an engine declares what it implements


def test_x3_exponent_state_and_backoff():
    net = nn.Linear(2, 2)
    eng = _Trivial(net, "fp32x3")
    assert eng.x3
    assert (eng.X3_AEXP, eng.x3_gexp_off, eng.x3_backoffs) == (4, 4, 0)
    assert eng._x3_grad_exp(10 ** 6) == 24
    assert eng._x3_grad_exp(10 ** 6, 0.5) == 25
    assert eng.x3_backoff(act=True, grad=False) == (-2, 4)
    assert eng.x3_backoff(step=2, act=False, grad=True) == (-2, 2)
    assert eng._x3_grad_exp(10 ** 6) == 22
    eng.x3_backoff()
    eng.x3_backoff()
    assert eng.x3_backoffs == 4
    with pytest.raises(RuntimeError, match="range guard") as ei:
        eng.x3_backoff()
    assert "activation 2^-14" in str(ei.value) and "gradient offset 2^-10" in str(ei.value)   # names the exponents
    assert _Trivial.X3_AEXP == 4 and _Trivial(net, "fp32x3").X3_AEXP == 4                      # per-instance state
    with pytest.raises(RuntimeError, match="not an fp32x3 engine"):
        _Trivial(net, "fp32").x3_backoff()
    # an ordinary method that reads only x3_gexp_off (tests/test_conv_wr_x3_gpu.py calls it unbound)
    assert SwinIREngine._x3_grad_exp(types.SimpleNamespace(x3_gexp_off=4), 10 ** 6) == 24


@pytest.mark.parametrize("mx,exp", [(1.0, 8), (300.0, -1), (2.0 ** -20, 28), (0.0, 0), (math.inf, 0), (math.nan, 0)])
def test_x3_upstream_grad_exp(mx, exp):
    assert EngineBase.x3_upstream_grad_exp(mx) == exp
    assert _Trivial(nn.Linear(2, 2), "fp32x3").x3_upstream_grad_exp(mx) == exp


def test_dncnn_declares_no_fp32x3():
    from kair_amd.models.select_network import compute_dtype_of
    with pytest.raises(ValueError):
        DnCNNEngine(object(), "fp32x3")    # before anything else: the network is not even looked at
    with pytest.raises(ValueError):
        compute_dtype_of({"netG": {"net_type": "dncnn", "compute_dtype": "fp32x3"}})
    assert compute_dtype_of({"netG": {"net_type": "dncnn"}}) == "fp32"
    assert compute_dtype_of({"netG": {"net_type": "rrdbnet"}}) == "fp32x3"
    assert compute_dtype_of({"netG": {"net_type": "usrnet", "compute_dtype": "fp32x3"}}) == "fp32x3"


def test_conv_engines_do_not_import_swinir_engine():
    code = ("import sys, kair_amd.engine.dncnn_engine, kair_amd.engine.rrdbnet_engine; "
            "sys.exit(int('kair_amd.engine.swinir_engine' in sys.modules))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]


FUNCTION_NODE = r"class \w+Function\(torch\.autograd\.Function\)"   # one for the conv programs, SwinIR's own


@pytest.mark.parametrize("pattern", [r"def x3_backoff\b", r"def _x3_grad_exp\b", r"math\.ceil\(math\.log2", r"def _nt\b",
                                     r"def _wgrad\b", FUNCTION_NODE])
def test_defined_once_under_engine(pattern):
    d = os.path.join(ROOT, "kair_amd", "engine")
    hits = []
    for f in sorted(os.listdir(d)):
        if f.endswith(".py"):
            with open(os.path.join(d, f)) as fh:
                hits += [f] * len(re.findall(pattern, fh.read()))
    assert hits == (["base.py", "swinir_engine.py"] if pattern == FUNCTION_NODE else ["base.py"]), hits


def test_swinir_tail_and_conv_wr_rule_single_sourced():
    """The SwinIR engine neither branches on the upsampler (swinir_tail.py's classes do) nor reads the environment, and
    the register-streamed conv's eligibility rule is written in one function of the engine package."""
    d = os.path.join(ROOT, "kair_amd", "engine")
    with open(os.path.join(d, "swinir_engine.py")) as fh:
        src = fh.read()
    assert "self.upsampler ==" not in src and "os.environ" not in src
    callers = []
    for f in sorted(os.listdir(d)):
        if f.endswith(".py"):
            with open(os.path.join(d, f)) as fh:
                for fn in re.split(r"\n(?= *def )", fh.read()):   # one piece per function (nested ones included)
                    if "conv3x3_wr_tile(" in fn:
                        callers.append((f, re.match(r" *def (\w+)", fn).group(1)))
    assert callers == [("swinir_engine.py", "_wr_ok")], callers
