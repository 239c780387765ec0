"""CPU: omh_flash_attn_bwd_band_d128 (the band backward, additive to ABI v12) rejects bad arguments before it touches
the device."""
import ctypes as C
import importlib

from conftest import PKG

OMH_E_BADARG, OMH_E_ALIGN = -1, -2


def _args(binding, o32=True):
    a = binding.AttnBwdArgs()
    for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv"):
        setattr(a, name, C.c_void_p(4096))
    a.o32 = C.c_void_p(4096) if o32 else None
    a.B, a.H, a.Lq, a.Lk = 1, 2, 100, 100
    a.q_rs = a.k_rs = a.o_rs = a.dq_rs = a.dk_rs = 256
    a.q_bs = a.k_bs = a.o_bs = a.dq_bs = a.dk_bs = 256 * 100
    return a


def test_band_backward_argument_validation(omh):
    binding = importlib.import_module(PKG + "._lib")
    lib = binding.lib
    assert lib.omh_flash_attn_bwd_band_d128(None, 8, 8, None) == OMH_E_BADARG
    assert lib.omh_flash_attn_bwd_band_d128(C.byref(_args(binding, o32=False)), 8, 8, None) == OMH_E_BADARG   # o32 required
    assert lib.omh_flash_attn_bwd_band_d128(C.byref(_args(binding, o32=False)), -1, -1, None) == OMH_E_BADARG
    for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv"):
        a = _args(binding)
        setattr(a, name, None)
        assert lib.omh_flash_attn_bwd_band_d128(C.byref(a), 8, 8, None) == OMH_E_BADARG, name
    a = _args(binding)
    a.Lq = 0
    assert lib.omh_flash_attn_bwd_band_d128(C.byref(a), 8, 8, None) == OMH_E_BADARG
    a = _args(binding)
    a.q_rs = 250                                                     # rows of 16 bytes: the same rule as the full entry
    assert lib.omh_flash_attn_bwd_band_d128(C.byref(a), 8, 8, None) == OMH_E_ALIGN
    a = _args(binding)
    a.dq = C.c_void_p(4100)
    assert lib.omh_flash_attn_bwd_band_d128(C.byref(a), 8, 8, None) == OMH_E_ALIGN
