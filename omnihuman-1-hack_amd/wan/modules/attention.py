"""``flash_attention`` with the reference's signature
(seaweed_apt/wan/modules/attention.py:24-130) on the gfx950 kernel
``omh_flash_attn_fwd_d128``.

The reference packs variable-length sequences and calls flash-attn's varlen
kernel; the result is softmax(q k^T * scale) v per head over the first
``k_lens[b]`` keys of each sample, for every one of the first ``q_lens[b]``
query rows (rows past it are zero; ``q_lens`` is never passed by model.py).  This wrapper keeps that contract
for head_dim 128, including flash-attn's ``causal`` / ``window_size`` band (bottom-right aligned: query i sees key j
iff i + klen - qlen - left <= j <= i + klen - qlen + right; rows with an empty band are zero), on the
short-sequence kernel; ``dropout_p`` > 0 is rejected (a random mask has no parity to hold).  The DiT blocks do not go through it (they hand the kernel
pre-laid-out q / k / V^T buffers); it exists for callers of the reference API.

The call is differentiable, as the reference's is through flash-attn: with grad enabled and an input that requires it,
full attention (``q_lens`` / ``k_lens`` honoured) goes through ``ops.flash_attn_func`` and the gradients come back in
each input's own dtype and shape.  The band's backward exists too (``ops.flash_attn_func(window=)``); through this
wrapper a bounded window with a grad-requiring input is still refused — see ``flash_attention``.
"""
import importlib
import math

import torch

from .._backend import ops

_sparse = importlib.import_module(ops.__package__ + ".sparse")

__all__ = ["flash_attention", "attention"]


def flash_attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None,
                    causal=False, window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None,
                    chunk_causal=None, interval_mask=None, block_mask=None):
    """q [B, Lq, N, 128], k/v [B, Lk, N, 128]; returns [B, Lq, N, 128] in q's dtype.

    ``interval_mask`` (not in the reference): a ``causal.IntervalMask`` — query i sees key j < k_lens[b] iff the mask's
    bool matrix holds True at [i // group, j // group] (at most two runs of True per row and per column: teacher forcing,
    the staircase, sink + window); absolute positions; rows that see no key are zero.  Differentiable through this wrapper
    like the unmasked call.  Together with ``causal``, a bounded ``window_size``, ``block_mask`` or ``chunk_causal`` it
    raises ValueError.

    ``chunk_causal`` = (chunk, left_chunks, q_offset) (not in the reference): the chunk-causal staircase of
    ``ops.flash_attn(chunk_causal=)`` — query i, at position q_offset + i, sees key j < k_lens[b] iff j // chunk <=
    (q_offset + i) // chunk and, for left_chunks >= 0, j // chunk >= (q_offset + i) // chunk - left_chunks; absolute
    positions, no bottom-right shift; rows that see no key are zero.  Differentiable through this wrapper like the
    unmasked call.  Together with ``causal``, a bounded ``window_size`` or ``block_mask`` it raises ValueError.

    ``block_mask`` (not in the reference: flash-attn takes no mask): a ``sparse.BlockMask`` or a bool tensor
    [nQb, nKb] / [N, nQb, nKb] over 128 x 128 blocks of the padded sequence — query i sees key j iff its block is kept,
    j < k_lens[b] and i < q_lens[b]; rows that see no key are zero.  Differentiable like the unmasked call.  Together
    with ``causal`` or a bounded ``window_size`` it raises ValueError (a mask is not intersected with a band).
    A ``sparse.DynamicBlockPolicy`` in its place lets the call choose the mask itself (``sparse.block_mask_from_qk`` on
    ``q * q_scale`` and ``k`` as bf16, ``q_lens`` / ``k_lens`` honoured): built on the device with no host synchronisation,
    shared by the samples of the batch (the union of their selections), and no gradient flows through the selection — the
    call stays differentiable exactly as with that mask handed in.

    With grad enabled and q, k or v requiring it the result carries a ``grad_fn`` (``ops.flash_attn_func``; the casts
    to bf16 and ``q * q_scale`` stay torch ops in front of it, so fp32 inputs — the reference's own call pattern — get
    fp32 gradients of their own shape).  Under ``torch.no_grad()`` or with no input requiring grad the call is the
    forward-only path.  The grad path pins the short-sequence kernel (its backward needs that kernel's lse and fp32
    output), so the two give the same output bits whenever the forward-only call takes the short-sequence kernel too —
    every call with ``q_lens`` or a band, and full attention below the long-sequence dispatch (>= 512 tiles of 256 rows
    and Lk >= 1024); beyond it the forward-only call runs the long-sequence stream: other bits, and a faster forward.
    ``causal`` / a bounded ``window_size`` with an input that requires grad raises NotImplementedError: the refusal is
    kept because tests/test_gpu_kernels.py pins it (test_flash_attention_causal_and_window) and can be lifted when that
    test is revisited — the differentiable band is ``ops.flash_attn_func(window=)``.
    ``deterministic`` is accepted and changes nothing: the backward kernels use no atomics and repeat bit for bit either
    way."""
    assert dtype in (torch.float16, torch.bfloat16)
    assert q.device.type == "cuda" and q.size(-1) <= 256
    if dropout_p != 0.:
        # the reference forwards it to flash-attn (attention.py:96-127); no caller in the repository sets it
        # (model.py:151-156,181,221-223) and a random mask cannot be held to parity: rejected, not silently ignored
        raise NotImplementedError("flash_attention on gfx950: dropout_p > 0 is not built (no caller in the reference "
                                  "uses it); q_lens, k_lens, causal and window_size are")
    # flash-attn's window (attention.py:121-126): causal bounds the right side at 0 (flash_attn_varlen_func sets
    # window_size = (left, 0) for causal=True); a negative side is unbounded
    wl, wr = int(window_size[0]), int(window_size[1])
    if causal:
        wr = 0
    window = (wl if wl >= 0 else -1, wr if wr >= 0 else -1)
    # one of the five kinds, or a ValueError before anything touches a device (ops.attn_mask); a block policy stands in for
    # the mask it chooses below, from q and k
    policy = block_mask if isinstance(block_mask, _sparse.DynamicBlockPolicy) else None
    resolve = lambda bm: ops.attn_mask(window, bm, chunk_causal, interval_mask, H=q.shape[2], Lq=q.shape[1], Lk=k.shape[1],
                                       device=q.device)
    mask = resolve(None if policy is not None else block_mask)
    if policy is not None and mask.kind != "full":
        raise ValueError("flash_attention: block_mask excludes causal / a bounded window_size / chunk_causal / interval_mask")
    if mask.kind == "band" and torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise NotImplementedError("flash_attention on gfx950: causal / window_size are forward-only through this wrapper; "
                                  "the differentiable band is ops.flash_attn_func(window=)")
    B, Lq, N, D = q.shape
    Lk = k.shape[1]
    if D != 128:
        raise NotImplementedError("the gfx950 attention kernel is built for head_dim 128")
    out_dtype = q.dtype
    if q_scale is not None:
        q = q * q_scale
    kl = None if k_lens is None else k_lens.to(device=q.device, dtype=torch.int32).contiguous()
    ql = None if q_lens is None else q_lens.to(device=q.device, dtype=torch.int32).contiguous()
    if policy is not None:
        mask = resolve(_sparse.block_mask_from_qk(q.detach().to(torch.bfloat16), k.detach().to(torch.bfloat16), policy, ql, kl,
                                                  (softmax_scale if softmax_scale is not None else D ** -0.5) * math.log2(math.e)))
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        o = ops.flash_attn_func(q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), kl, ql,
                                scale=softmax_scale, mask=mask)
        return o.type(out_dtype)
    qb = q.to(torch.bfloat16).contiguous()
    kb = k.to(torch.bfloat16).contiguous()
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, N * D, Lp, dtype=torch.bfloat16, device=q.device)
    vt[:, :, :Lk] = v.to(torch.bfloat16).reshape(B, Lk, N * D).transpose(1, 2)   # layout change only
    # q_lens (attention.py:55-60,79): the reference cuts the queries past q_lens[b] out of the packed batch — and can only
    # un-flatten the result when every q_lens[b] == Lq (attention.py:110); here those rows come back as zeros
    o = ops.flash_attn(qb, kb, vt, kl, scale=softmax_scale, q_lens=ql, mask=mask)
    return o.type(out_dtype)


def attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
              window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, fa_version=None,
              chunk_causal=None, interval_mask=None, block_mask=None):
    """attention.py:133-179 — same kernel; the reference's SDPA fallback is not needed here."""
    return flash_attention(q, k, v, q_lens, k_lens, dropout_p, softmax_scale, q_scale, causal, window_size,
                           deterministic, dtype, fa_version, block_mask=block_mask, chunk_causal=chunk_causal,
                           interval_mask=interval_mask)
