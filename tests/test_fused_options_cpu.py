"""The fused trainer's l2 / l2sum losses and gradient-norm clipping, the parts that need no GPU: the C boundary of
kair_l2_loss / kair_grad_norm / kair_adam_ema_clip (declared, bound, exported; argument errors return before any
launch), ModelPlain's fused_step_supported truth table, and the fp32x3 gradient exponents of the new losses."""
import ctypes
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kair_l2_loss", "kair_grad_norm", "kair_adam_ema_clip")


def test_header_binding_and_library_carry_the_new_functions():
    from kair_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kair_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW + ("kair_grad_norm_ws",):
        assert re.search(r"^\s*(?:int|long)\s+%s\s*\(" % name, src, flags=re.M), name
        assert name in _hip._SIGS, name
        assert hasattr(L, name), name
    # the declared parameter counts are the bound ones
    for name in NEW:
        decl = re.search(r"%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGS[name]), name


def test_grad_norm_geometry_query():
    """Fixed launch geometry and the workspace size, one partial per workgroup; at the largest gradient buffers of the
    project (SwinIR classical, 11.9 M parameters) the fp32 addition chain stays short."""
    from kair_amd import _hip
    grid, block, ws = _hip.grad_norm_geometry()
    assert grid > 0 and block > 0 and block & (block - 1) == 0 and ws == grid
    assert _hip.lib().kair_grad_norm_ws(None, None) == ws


def test_argument_errors_name_the_function_and_launch_nothing():
    """Null pointers and bad sizes: every check is on the host, before the first launch (there is no device here)."""
    from kair_amd import _hip
    L = _hip.lib()
    one = ctypes.c_float(0.0)
    p = ctypes.addressof(one)   # a non-null pointer no check dereferences

    def err(rc, word):
        assert rc != 0
        msg = L.kair_last_error()
        assert word in msg, msg

    err(L.kair_l2_loss(None, None, None, None, _hip.F32, 16, 1, 1.0, 0, 1, 1, 8, 8, None, None), b"l2_loss")
    err(L.kair_l2_loss(p, p, p, p, _hip.F32, 16, 2, 1.0, 0, 1, 1, 7, 8, p, None), b"l2_loss")    # Hh % ps_r
    err(L.kair_l2_loss(p, p, p, p, _hip.F32, 16, 2, 1.0, 1, 1, 1, 8, 7, p, None), b"l2_loss")    # Ww % ps_r
    err(L.kair_l2_loss(p, p, p, p, _hip.F32, 3, 2, 1.0, 0, 1, 1, 8, 8, p, None), b"l2_loss")     # C r^2 > ldc
    err(L.kair_grad_norm(p, 0, p, p, None), b"grad_norm")
    err(L.kair_grad_norm(p, -5, p, p, None), b"grad_norm")
    err(L.kair_grad_norm(None, 8, p, p, None), b"grad_norm")
    adam = lambda gnorm, mx: L.kair_adam_ema_clip(p, p, p, p, None, 1, p, 0.9, 0.999, 1e-8, 0.0, 0.0, None, gnorm, mx, None)
    err(adam(p, 0.0), b"adam_ema_clip")
    err(adam(p, -1.0), b"adam_ema_clip")
    err(adam(None, 1.0), b"adam_ema_clip")


BASE = {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
        "G_optimizer_clipgrad": None, "G_regularizer_orthstep": None, "G_regularizer_clipstep": None}


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("loss", ["l1", "l2", "l2sum", "charbonnier", "ssim"])
def test_fused_step_supported_says_yes(loss, clip):
    from kair_amd.models.model_plain import fused_step_supported
    ok, reason = fused_step_supported({**BASE, "G_lossfn_type": loss, "G_optimizer_clipgrad": clip})
    assert ok is True and reason == ""
    ok, _ = fused_step_supported({**BASE, "G_lossfn_type": loss, "G_optimizer_clipgrad": clip, "use_fused_trainer": True})
    assert ok is True


@pytest.mark.parametrize("change", [{"G_regularizer_clipstep": 10}, {"G_regularizer_orthstep": 10},
                                    {"G_optimizer_type": "sgd"}, {"use_fused_trainer": False}])
def test_fused_step_supported_says_no_with_a_reason(change):
    from kair_amd.models.model_plain import fused_step_supported
    for loss in ("l1", "l2"):
        ok, reason = fused_step_supported({**BASE, "G_lossfn_type": loss, **change})
        assert ok is False and isinstance(reason, str) and reason.strip()
        assert list(change)[0] in reason or str(list(change.values())[0]) in reason, reason


def test_fused_step_supported_reads_a_nonedict_and_is_pure():
    from kair_amd.models.model_plain import fused_step_supported
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = dict_to_nonedict({"G_lossfn_type": "l2sum", "G_optimizer_type": "adam", "G_optimizer_clipgrad": 0.1})
    before = dict(opt)
    assert fused_step_supported(opt) == (True, "")
    assert dict(opt) == before


def test_x3_gradient_exponents_of_the_l2_losses():
    """_x3_grad_exp: 'l2' one binade below 'l1' (the gradient bound 2 |w| / numel is twice L1's |w| / numel), 'l2sum'
    = 'l2' at numel 1 (no division by numel); the 'l1' / 'ssim' exponents are what they were."""
    from kair_amd.engine.base import EngineBase
    eng = types.SimpleNamespace(x3_gexp_off=4, X3_SSIM_HEADROOM=EngineBase.X3_SSIM_HEADROOM)
    f = lambda *a: EngineBase._x3_grad_exp(eng, *a)
    for numel in (1, 2 * 3 * 32 * 32, 32 * 3 * 192 * 192, 5 * 7 * 9):
        for w in (1.0, -0.5, 1e3, 1.0 / 255):
            assert f(numel, w, "l2") == f(numel, w, "l1") - 1 == f(numel, w, None) - 1
            assert f(numel, w, "l2sum") == f(1, w, "l2")
            assert f(numel, w, "ssim") == f(numel, w, "l1") - 6
    assert f(2 ** 20, 1.0, None) == f(2 ** 20, 1.0, "l1") == f(2 ** 20, 1.0, "charbonnier") == 24
    assert f(2 ** 20, 0.25, "l1") == 26 and f(2 ** 20, 1.0, "ssim") == 18
    assert f(2 ** 20, 1.0, "l2") == 23 and f(2 ** 20, 1.0, "l2sum") == 3 and f(2 ** 20, 4.0, "l2sum") == 1
    eng.x3_gexp_off = 2   # after a back-off every loss follows
    assert f(2 ** 20, 1.0, "l2") == 21 and f(2 ** 20, 1.0, "l1") == 22
