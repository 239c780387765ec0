"""A CPU restatement of AdamW with FP8 block-scaled moments (include/omh.h states the format): plain torch, fp32
arithmetic in the order the header gives, ``torch.float8_e4m3fn`` for the rounding.  The reference of
tests/test_gpu_adamw8.py and, on its own, of the host test that shows the format trains.

A moment of a weight viewed as [rows, cols]: uint8 e4m3fn codes [rows, cols] + one fp32 scale per 64 columns of a row;
the second moment is kept as its root r = sqrt(v)."""
import numpy as np
import torch

E4M3_MAX = 448.0
BLOCK = 64
f32 = np.float32


def encode(q):
    """fp32 in [-448, 448] -> e4m3fn bit patterns (uint8), round to nearest even: torch's cast."""
    return q.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


def decode(codes):
    return codes.view(torch.float8_e4m3fn).to(torch.float32)


def n_blocks(cols):
    return (cols + BLOCK - 1) // BLOCK


def _blocked(x):
    """[rows, cols] -> [rows, blocks, 64], zero behind the end of a row."""
    rows, cols = x.shape
    nb = n_blocks(cols)
    out = torch.zeros(rows, nb * BLOCK, dtype=x.dtype)
    out[:, :cols] = x
    return out.view(rows, nb, BLOCK)


def quantize(x, root=False, with_pre=False):
    """fp32 [rows, cols] -> (codes uint8 [rows, cols], scales fp32 [rows, blocks]); ``root``: x is v, the codes hold
    sqrt(v) and a positive value never gets code 0.  ``with_pre``: also the values x / scale that were rounded."""
    x = x.to(torch.float32)
    rows, cols = x.shape
    xb = _blocked(torch.sqrt(x) if root else x)
    scale = xb.abs().amax(-1) / f32(E4M3_MAX).item()
    s = scale[..., None]
    pre = torch.where(s > 0, xb / s, torch.zeros_like(xb)).clamp(-E4M3_MAX, E4M3_MAX)
    codes = encode(pre)
    if root:
        codes = torch.where((xb > 0) & (codes == 0), torch.ones_like(codes), codes)
    codes = codes.view(rows, -1)[:, :cols].contiguous()
    if with_pre:
        return codes, scale, pre.view(rows, -1)[:, :cols].contiguous()
    return codes, scale


def dequantize(codes, scale, root=False):
    """-> fp32 [rows, cols]: m, or v = (decode * scale)^2 with ``root``."""
    rows, cols = codes.shape
    x = decode(codes) * scale.to(torch.float32).repeat_interleave(BLOCK, dim=1)[:, :cols]
    return x * x if root else x


def adamw_update(p, g, m_old, v_old, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, coef=None):
    """One AdamW step in fp32 on unquantised moments, in the kernels' association: -> (p_new, m, v)."""
    b1, b2, lr_, eps_, wd_ = f32(beta1), f32(beta2), f32(lr), f32(eps), f32(wd)
    bc1 = f32(1) - np.power(b1, f32(step), dtype=f32)
    bc2 = np.sqrt(f32(1) - np.power(b2, f32(step), dtype=f32), dtype=f32)
    gi = g.to(torch.float32) * (f32(1) / f32(grad_scale)).item()
    if coef is not None:
        gi = gi * f32(coef).item()
    m = m_old * b1.item() + gi * (f32(1) - b1).item()
    v = v_old * b2.item() + (gi * (f32(1) - b2).item()) * gi
    denom = torch.sqrt(v) / bc2.item() + eps_.item()
    p_new = p * (f32(1) - lr_ * wd_).item() - (m / denom) * (lr_ / bc1).item()
    return p_new, m, v


def step8(p, g, state, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, coef=None, with_pre=False):
    """One step on 8-bit state ``state`` = (m codes, m scales, r codes, r scales) of a [rows, cols] weight: decode,
    update on the fresh unquantised moments, quantise.  -> (p_new, new state[, (m pre, r pre)])."""
    mq, ms, rq, rs = state
    p_new, m, v = adamw_update(p, g, dequantize(mq, ms), dequantize(rq, rs, root=True), lr, beta1, beta2, eps, wd, step,
                               grad_scale, coef)
    qm = quantize(m, with_pre=with_pre)
    qr = quantize(v, root=True, with_pre=with_pre)
    if with_pre:
        return p_new, (qm[0], qm[1], qr[0], qr[1]), (qm[2], qr[2])
    return p_new, (qm[0], qm[1], qr[0], qr[1])


def zero_state(rows, cols):
    nb = n_blocks(cols)
    return (torch.zeros(rows, cols, dtype=torch.uint8), torch.zeros(rows, nb), torch.zeros(rows, cols, dtype=torch.uint8),
            torch.zeros(rows, nb))


# every code's value, ascending by magnitude: index = code & 0x7f (0x7f itself is NaN)
MAGNITUDES = decode(torch.arange(0, 127, dtype=torch.uint8))


def tie_distance(pre, code_a, code_b):
    """For codes that differ: |pre - boundary| / |boundary| where boundary is the midpoint between the two codes' values
    (inf where the two are not neighbours of equal sign, or a NaN code is involved).  A genuine tie under reordered fp32
    arithmetic has a distance of a few 2^-24."""
    a, b = code_a.to(torch.int32), code_b.to(torch.int32)
    ma, mb = a & 0x7f, b & 0x7f
    ok = ((a & 0x80) == (b & 0x80)) & ((ma - mb).abs() == 1) & (ma < 127) & (mb < 127)
    va = MAGNITUDES[ma.clamp(max=126).long()]
    vb = MAGNITUDES[mb.clamp(max=126).long()]
    bound = 0.5 * (va.double() + vb.double())
    dist = (pre.double().abs() - bound).abs() / bound
    return torch.where(ok, dist, torch.full_like(dist, float("inf")))
