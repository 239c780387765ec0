"""CPU: the differentiable attention surface exists — omh_flash_attn_bwd_varlen_d128 is declared, exported and bound,
ops.flash_attn_func exists, ops.flash_attn_bwd takes q_lens — and the new entry rejects bad arguments before it touches
the device."""
import ctypes as C
import importlib
import inspect
import os
import re

from conftest import PKG, ROOT

OMH_E_BADARG, OMH_E_ALIGN = -1, -2


def test_varlen_backward_is_declared_and_bound(omh):
    src = open(os.path.join(ROOT, "include", "omh.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+omh_flash_attn_bwd_varlen_d128\s*\(([^)]*)\)", decl)
    assert m, "omh_flash_attn_bwd_varlen_d128 is not declared in include/omh.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 5 and "omh_attn_bwd_args" in params[0] and "q_lens" in params[1]
    assert re.search(r"#define\s+OMH_ABI_VERSION\s+12\b", src)      # additive: the version stays
    binding = importlib.import_module(PKG + "._lib")
    assert "omh_flash_attn_bwd_varlen_d128" in binding.EXPORTED
    fn = binding.lib.omh_flash_attn_bwd_varlen_d128
    assert len(fn.argtypes) == 5


def test_ops_surface(omh):
    ops = importlib.import_module(PKG + ".ops")
    assert callable(ops.flash_attn_func) and "flash_attn_func" in ops.__all__
    sig = inspect.signature(ops.flash_attn_func)
    assert list(sig.parameters)[:3] == ["q", "k", "v"]
    for name in ("k_lens", "q_lens", "scale", "window"):
        assert name in sig.parameters
    assert sig.parameters["window"].default == (-1, -1)
    bwd = inspect.signature(ops.flash_attn_bwd).parameters
    assert "q_lens" in bwd and bwd["q_lens"].default is None


def _args(binding, o32=True):
    a = binding.AttnBwdArgs()
    for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv"):
        setattr(a, name, C.c_void_p(4096))
    a.o32 = C.c_void_p(4096) if o32 else None
    a.B, a.H, a.Lq, a.Lk = 1, 2, 100, 100
    a.q_rs = a.k_rs = a.o_rs = a.dq_rs = a.dk_rs = 256
    a.q_bs = a.k_bs = a.o_bs = a.dq_bs = a.dk_bs = 256 * 100
    return a


def test_varlen_backward_argument_validation(omh):
    binding = importlib.import_module(PKG + "._lib")
    fn = binding.lib.omh_flash_attn_bwd_varlen_d128
    ql = C.c_void_p(4096)
    assert fn(None, ql, -1, 0, None) == OMH_E_BADARG
    assert fn(C.byref(_args(binding, o32=False)), ql, -1, 0, None) == OMH_E_BADARG          # o32 required
    assert fn(C.byref(_args(binding, o32=False)), None, -1, -1, None) == OMH_E_BADARG
    for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv"):
        a = _args(binding)
        setattr(a, name, None)
        assert fn(C.byref(a), ql, 8, 8, None) == OMH_E_BADARG, name
    a = _args(binding)
    a.Lk = 0
    assert fn(C.byref(a), ql, 8, 8, None) == OMH_E_BADARG
    a = _args(binding)
    a.o_rs = 250
    assert fn(C.byref(a), ql, 8, 8, None) == OMH_E_ALIGN
    assert fn(C.byref(_args(binding)), C.c_void_p(4098), 8, 8, None) == OMH_E_ALIGN      # int32 q_lens
