"""The DMD rule of include/omh.h (omh_dmd_grad) evaluated in fp64 from fp32 inputs, and the bounds the GPU tests hold the
kernels to (derived in tests/test_gpu_dmd_kernel.py).  Test infrastructure, not a test module."""
import torch

FLT_MAX = 3.4028234663852886e+38
TOL_NORM, TOL_RMS, TOL_MAX, TOL_LOSS = 2e-6, 2e-6, 4e-6, 1e-12


def rule(x, xt, vc, vu, vf, sigma, guide):
    """(grad, norm) in fp64 for [B, n] inputs; ``vu`` None: no guidance."""
    x, xt, vc, vf = (t.double() for t in (x, xt, vc, vf))
    s = sigma.double().view(-1, 1)
    vr = vc if vu is None else vu.double() + guide * (vc - vu.double())
    nb = ((x - xt) + s * vr).abs().mean(1)
    with torch.no_grad():
        grad = torch.nan_to_num(s * (vr - vf) / nb.view(-1, 1), nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
    return grad, nb
