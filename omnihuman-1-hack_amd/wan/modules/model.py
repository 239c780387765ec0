"""Wan2.1 DiT backbone on hand-written gfx950 kernels — drop-in for the
reference's ``wan.modules.model`` (seaweed_apt/wan/modules/model.py).

Same constructor, attributes, module tree and state-dict keys as the
reference ``WanModel`` (model.py:377-499) so checkpoints, EMA
zips, forward hooks on ``model.blocks[i]`` and ``copy.deepcopy`` keep working;
``forward(x, t, context, seq_len, clip_fea=None, y=None)`` returns the same
list of fp32 ``[C_out, F, H, W]`` tensors.  The parameters stay ordinary fp32
``nn.Parameter``s; the arithmetic runs on bf16 copies packed once per weight
version, through the C ABI of libomh.so (include/omh.h):

  patch embed  -> omh_patchify + omh_gemm_bf16(EPI_F32)            model.py:515-522
  time embed   -> omh_sinusoidal_embedding + omh_dense_f32          model.py:526-528
  text embed   -> omh_cast + omh_gemm(GELU) + omh_gemm              model.py:531-532
  block        -> omh_layernorm_modulate, omh_gemm (q|k fp32, V^T bf16),
                  omh_rmsnorm_rope, omh_flash_attn_fwd_d128,
                  omh_gemm(EPI_RESID: x += (o W^T + b) * gate), ... model.py:279-330
  head         -> omh_layernorm_modulate + omh_gemm + omh_unpatchify model.py:349-359,565-588

Deliberate differences from the reference: the
reference's per-call ``empty_cache()``, FFN->CPU offload of blocks > 10 and
forced fp16 autocast are execution mechanics, not math, and are not
reproduced; compute is bf16 MFMA with fp32 accumulation, fp32 residual
stream, fp32 norm statistics (tolerance stated in tests/ and DESIGN.md).
"""
import math
from typing import List, Optional

import torch
import torch.nn as nn

from .._backend import ops

BIAS_M, BIAS_N, BIAS_NONE = ops.BIAS_M, ops.BIAS_N, ops.BIAS_NONE
EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID = ops.EPI_BF16, ops.EPI_F32, ops.EPI_GELU_BF16, ops.EPI_RESID
EPI_BF16_SPLIT_T = ops.EPI_BF16_SPLIT_T
ptr = ops.ptr

__all__ = ["WanModel"]


def _sparse():
    import importlib
    return importlib.import_module(ops.__package__ + ".sparse")


# ----------------------------------------------------------------------------
# reference-compatible helpers
# ----------------------------------------------------------------------------
def sinusoidal_embedding_1d(dim, position):
    """model.py:17-27 (host fp64 version, kept for API parity)."""
    assert dim % 2 == 0
    half = dim // 2
    position = position.type(torch.float64)
    sinusoid = torch.outer(position, torch.pow(10000, -torch.arange(half).to(position).div(half)))
    return torch.cat([torch.cos(sinusoid), torch.sin(sinusoid)], dim=1)


def rope_params(max_seq_len, dim, theta=10000):
    """model.py:31-38 — complex128 rotary table."""
    assert dim % 2 == 0
    freqs = torch.outer(torch.arange(max_seq_len),
                        1.0 / torch.pow(theta, torch.arange(0, dim, 2).to(torch.float64).div(dim)))
    return torch.polar(torch.ones_like(freqs), freqs)


class _Packed:
    """bf16 copies of weights, rebuilt when the source parameter changes."""

    def __init__(self):
        self.store = {}

    def get(self, key, params, builder, extra=()):
        """``extra``: what else the copy depends on (the adapters of ``_lora_sig``); () leaves the signature as it was."""
        sig = tuple((p.data_ptr(), p._version, str(p.device)) for p in params) + extra
        ent = self.store.get(key)
        if ent is None or ent[0] != sig:
            with torch.no_grad():
                ent = (sig, builder())
            self.store[key] = ent
        return ent[1]

    def __deepcopy__(self, memo):
        return _Packed()


def _bf16(w: torch.Tensor) -> torch.Tensor:
    w = w.detach()
    if w.dtype == torch.bfloat16:
        return w.contiguous()
    return ops.cast_bf16(w.float().contiguous())


def lora_of(lin):
    """(A, B, scale) of a Linear that carries a low-rank adapter (lora.add_lora: parameters ``lora_A`` [rank, in] and
    ``lora_B`` [out, rank], scale = alpha / rank unless lora.set_lora_scale overrode it), else None."""
    A = lin._parameters.get("lora_A")
    if A is None:
        return None
    ov = lin.__dict__.get("lora_scale_override")
    return A, lin._parameters["lora_B"], float(ov) if ov is not None else float(lin.lora_alpha) / A.shape[0]


def _lora_sig(*lins):
    """Signature of the adapters of ``lins`` for _Packed.get: () when there is none."""
    out = ()
    for lin in lins:
        lo = lora_of(lin)
        if lo is not None:
            A, B, s = lo
            out += ((A.data_ptr(), A._version, B.data_ptr(), B._version, s),)
    return out


def lora_pack_row(w, dst, dstT, ld_dst, ld_t, lo):
    """One entry of the adapter pack table (include/omh.h: omh_pack_weights_lora_multi) for the fp32 weight ``w``;
    ``lo``: lora_of()'s triple or None.  Column 7 (first tile) is filled by the caller."""
    r, c = w.shape
    row = [w.data_ptr(), dst.data_ptr() if dst is not None else 0, dstT.data_ptr() if dstT is not None else 0, r, c,
           ld_dst, ld_t, 0, 0]
    if lo is None:
        return row + [0, 0, 0, 0]
    A, B, s = lo
    if not (A.dtype == B.dtype == w.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous()
            and w.is_contiguous() and A.device == B.device == w.device):
        raise ops.OmhError("a low-rank adapter needs contiguous fp32 weight, lora_A and lora_B on one device")
    if A.shape[1] != c or B.shape[0] != r or B.shape[1] != A.shape[0] or not 1 <= A.shape[0] <= 128:
        raise ops.OmhError(f"adapter shapes {tuple(A.shape)}, {tuple(B.shape)} do not fit the weight {tuple(w.shape)}")
    return row + [A.data_ptr(), B.data_ptr(), A.shape[0], ops.f32_bits(s)]


def _weight_bf16(lin):
    """bf16 operand copy of a Linear's weight: bf16(W), or bf16(W + s B A) with an adapter (one launch of the fused
    pack kernel — the training step's, so both paths read the same bits)."""
    lo = lora_of(lin)
    if lo is None:
        return _bf16(lin.weight)
    w = lin.weight.detach()
    out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    row = lora_pack_row(w, out, None, w.shape[1], 0, (lo[0].detach(), lo[1].detach(), lo[2]))
    table = torch.tensor([row], dtype=torch.int64).to(w.device)
    ops.pack_weights_lora_multi(table, 1, ((w.shape[0] + 63) // 64) * ((w.shape[1] + 63) // 64))
    return out


def _cat_bf16(*lins):
    """bf16 copy of the row-wise concatenation of the Linears' (effective) weights."""
    if not any(lora_of(lin) is not None for lin in lins):
        return _bf16(torch.cat([lin.weight.detach() for lin in lins], 0))
    return torch.cat([_weight_bf16(lin) for lin in lins], 0)


def _round_up(a, b):
    return (a + b - 1) // b * b


LOG2E = 1.4426950408889634        # log2(e): folded into q with softmax_scale, so that the attention kernels take exp2
N_IMG = 257                       # CLIP image tokens in front of the text in an i2v context (model.py:189-230)


_CONST_CACHE = {}


def _dev_ints(values, dtype, device):
    """Small integer table (sequence lengths, grids) as a device tensor, cached by value: the forward issues no
    host-to-device copy after the first call with a given geometry (each one is a synchronous pageable copy, and
    none is allowed while a hipGraph is being captured).  Read-only by convention."""
    key = (str(device), dtype, tuple(tuple(v) if isinstance(v, (tuple, list)) else v for v in values))
    t = _CONST_CACHE.get(key)
    if t is None:
        if len(_CONST_CACHE) > 4096:
            _CONST_CACHE.clear()
        t = _CONST_CACHE[key] = torch.tensor(values, dtype=dtype, device=device)
    return t


class _FwdCtx:
    """Per-forward shared state handed to every block."""
    __slots__ = ("B", "S", "dim", "e0", "seq_lens32", "ctx_lens32", "grid32", "rope_cos", "rope_sin", "ctx",
                 "Lc", "n_img", "seq_lens_host", "ctx_lens_host", "kv", "split_k",
                 # chunk: (tokens per chunk, left_chunks, 0) under WanModel.set_causal_chunks, else None;
                 # cache, cache_layer, cache_lo: WanModel.forward_chunk (a causal.KVCache, the running block, first key)
                 "chunk", "cache", "cache_layer", "cache_lo",
                 # rpb: rows of the sequence that share one row of e0 (seq_len, or h * w with a per-frame t);
                 # interval: a causal.IntervalMask every self-attention runs under (forward_teacher_forcing), else None
                 "rpb", "interval",
                 # cache_pos, cache_hi, cache_mask: forward_chunk on a causal.RollingKVCache (the chunk's slot, the end of
                 # the filled slots, the resolved ops.AttnMask over stale keys of a short last chunk), else None
                 "cache_pos", "cache_hi", "cache_mask",
                 # grids: the (f, h, w) of the samples (host); ctx_mask: the resolved ops.AttnMask every cross-attention runs
                 # under (frame-aligned condition tokens: WanModel._condition_mask), else None
                 "grids", "ctx_mask",
                 # bounds: where the self-attention calls of this forward take their zeroed score-bound buffers from
                 "bounds",
                 # sink_fan: forward_teacher_forcing(pin_sink=True) on a clip that outlasts the ring — (device table of
                 # ops.rope_shift_table, copies, sink rows): every self-attention appends that many rotated images of its
                 # sink keys (and copies of their V^T columns) to the key axis; else None
                 "sink_fan")

    def __init__(self):
        self.kv = self.chunk = self.cache = self.cache_layer = self.cache_lo = self.rpb = self.interval = None
        self.cache_pos = self.cache_hi = self.cache_mask = None
        self.grids = self.ctx_mask = self.sink_fan = None
        self.bounds = _BoundPool()


class _BoundPool:
    """Zeroed float [B, heads, 2] buffers for ops.rmsnorm_rope_bf16_pair_bound_raw, cut from one [SLICES, B, heads, 2] tensor:
    one fill launch per forward instead of one per block (59 in a CFG step).  Every slice is handed out once; the two branches
    of a CFG pair share the pool by reference, so neither sees the other's maxima."""
    SLICES = 64

    def __init__(self):
        self.buf, self.used = None, 0

    def take(self, B, heads, device):
        if self.buf is None or self.used == self.buf.shape[0] or self.buf.shape[1:] != (B, heads, 2) or self.buf.device != device:
            self.buf, self.used = torch.zeros(self.SLICES, B, heads, 2, dtype=torch.float32, device=device), 0
        self.used += 1
        return self.buf[self.used - 1]


class ContextState:
    """Everything a forward derives from (context, clip_fea) alone — the text/image embedding output and every
    block's cross-attention K (normalised) and V^T — computed once by ``WanModel.encode_context`` and accepted by
    ``WanModel.forward`` in place of ``context``.  The reference recomputes these on each of the 100 forwards
    of a 50-step CFG sample (model.py:531-537,176-178,216-220); they do not depend on x or t, so reusing them
    changes no value.  ``cond``: the frames and the window of frame-aligned condition
    tokens (the normal form of ``extra_conditions``, without the tokens), or None."""
    __slots__ = ("ctx", "ctx_lens", "kv", "B", "model_id", "version", "cond")


# ----------------------------------------------------------------------------
# the block forward, stated once: the steps below and the ``_attend`` / ``_query`` / ``_attend_rows`` methods of the
# attention modules hold every launch of a WanAttentionBlock's forward; the inference block (WanAttentionBlock.forward)
# and the training node (model_train._block_forward) are sequences of these calls.  What the backward wants on top
# (branch outputs, FFN pre-activation, log-sum-exp, fp32 attention output, fp32 pre-norm K) is an optional output of the
# producing step.
# ----------------------------------------------------------------------------
class BlockWeights:
    """The operands one block's forward reads: bf16 weights [out, in] and fp32 biases — plain attributes, None where a
    caller has nothing (``_c``: cross-attention, ``_i``: its i2v image branch).  Inference fills it from the ``_Packed``
    copies (WanAttentionBlock._operands), training with views into its ``TrainPacks`` buffers and the fp32 master biases
    (model_train._operands); either way it is cached with the copies it points into.  The self-attention projections come
    as q | k and v, or as ``wqkv`` (the one-launch product of long sequences, inference only): no unused copy is built."""
    wqk = bqk = wv = bv = wqkv = bqkv = wo = bo = wq_c = bq_c = wk_c = bk_c = wv_c = bv_c = wo_c = bo_c = None
    wk_i = bk_i = wv_i = bv_i = w1 = b1 = w2 = b2 = n3w = n3b = None

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _vt_fresh(B, d, Lp, L, device):
    """V^T [B, d, Lp] bf16 for a product that writes columns [0, L): only the pad columns are zeroed (0 x P = 0 needs
    them finite)."""
    vt = torch.empty(B, d, Lp, dtype=torch.bfloat16, device=device)
    if Lp != L:
        vt[:, :, L:].zero_()
    return vt


def _ln_mod(x, fc, mod, eps, shift_i, scale_i):
    """bf16 [R, dim] = LN(x) (1 + e[scale_i]) + e[shift_i], e = mod + fc.e0 (mod: the block's fp32 modulation)."""
    S, d = x.shape[1], x.shape[2]
    R = x.shape[0] * S
    h = torch.empty(R, d, dtype=torch.bfloat16, device=x.device)
    # (rows per row of e0: the sequence, or a frame with a per-frame t)
    ops.layernorm_modulate_raw(ptr(x), ptr(h), R, d, eps, 1.0, ptr(mod, scale_i * d), ptr(fc.e0, scale_i * d), 6 * d,
                               ptr(mod, shift_i * d), ptr(fc.e0, shift_i * d), 6 * d, fc.rpb or S)
    return h


def _resid(x, a, w, b, fc, mod=None, gate_i=None, out=None, y=None):
    """out = x + (a w^T + b) * gate, gate = mod[gate_i] + e0[:, gate_i] (``gate_i`` None: 1); fp32 [B, S, dim].
    ``out`` None: x is updated in place (the inference block); else written out of place (the training node).
    ``y``: optional bf16 [R, dim] output, the branch a w^T + b before the gate (the gate's gradient needs it)."""
    S, d = x.shape[1], x.shape[2]
    M, K = a.shape
    kw = dict(c_in=ptr(x) if out is not None and out.data_ptr() != x.data_ptr() else None,
              aux=ptr(y) if y is not None else None, ldaux=d if y is not None else 0, split_k=fc.split_k)
    xo = ptr(x if out is None else out)
    if gate_i is None:
        ops.gemm_raw(ptr(a), ptr(w), xo, M, d, K, a.stride(0), w.stride(0), d, EPI_RESID,
                     bias=ptr(b) if b is not None else None,
                     bias_mode=BIAS_N if b is not None else BIAS_NONE, gate_const=1.0, **kw)
    else:
        # (split_k: at one or two [16,1,60,104] clips the FFN-down contraction, K = ffn_dim over 56 / 104 tiles,
        # runs in slices — ABI v9; nothing is split at the sampling sizes)
        ops.gemm_raw(ptr(a), ptr(w), xo, M, d, K, a.stride(0), w.stride(0), d, EPI_RESID, bias=ptr(b), bias_mode=BIAS_N,
                     gate0=ptr(mod, gate_i * d), gate1=ptr(fc.e0, gate_i * d), gate1_stride=6 * d, gate_rows=fc.rpb or S,
                     gate_const=0.0, **kw)
    return x if out is None else out


def _cross_input(x, W, eps):
    """bf16 [R, dim] input of the cross-attention: norm3(x) (``W.n3w`` / ``W.n3b``, cross_attn_norm) or the plain cast."""
    d = x.shape[2]
    R = x.shape[0] * x.shape[1]
    h = torch.empty(R, d, dtype=torch.bfloat16, device=x.device)
    if W.n3w is not None:
        ops.layernorm_modulate_raw(ptr(x), ptr(h), R, d, eps, 0.0, ptr(W.n3w), None, 0, ptr(W.n3b), None, 0, R)
    else:
        ops.cast_bf16(x.view(R, d), out=h)
    return h


def _ffn_up(h, W, pre=False):
    """bf16 [R, ffn_dim] = gelu(h W1^T + b1).  ``pre``: also the pre-activation (GELU'), an optional output: (u, pre)."""
    R, d = h.shape
    f = W.w1.shape[0]
    u = torch.empty(R, f, dtype=torch.bfloat16, device=h.device)
    u_pre = torch.empty_like(u) if pre else None
    ops.gemm_raw(ptr(h), ptr(W.w1), ptr(u), R, f, d, d, d, f, EPI_GELU_BF16, bias=ptr(W.b1), bias_mode=BIAS_N,
                 aux=ptr(u_pre) if pre else None, ldaux=f if pre else 0)
    return (u, u_pre) if pre else u


# ----------------------------------------------------------------------------
# modules (same tree / parameter names as the reference)
# ----------------------------------------------------------------------------
class WanRMSNorm(nn.Module):
    """model.py:72-88 (parameters only; fused into omh_rmsnorm_rope)."""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1]).float().contiguous()
        return ops.rmsnorm_rope(x2, self.weight.detach(), self.eps).reshape(x.shape)


class WanLayerNorm(nn.LayerNorm):
    """model.py:91-104 (fused into omh_layernorm_modulate)."""

    def __init__(self, dim, eps=1e-6, elementwise_affine=False):
        super().__init__(dim, elementwise_affine=elementwise_affine, eps=eps)

    def forward(self, x):
        x2 = x.float().contiguous()
        w = self.weight.detach() if self.elementwise_affine else None
        b = self.bias.detach() if self.elementwise_affine else None
        return ops.layernorm_modulate(x2, self.eps, 0.0 if w is not None else 1.0, mul0=w, add0=b)


class WanSelfAttention(nn.Module):
    """model.py:107-161."""

    def __init__(self, dim, num_heads, window_size=(-1, -1), qk_norm=True, eps=1e-6):
        assert dim % num_heads == 0
        super().__init__()
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.window_size, self.qk_norm, self.eps = window_size, qk_norm, eps
        self.q = nn.Linear(dim, dim)
        self.k = nn.Linear(dim, dim)
        self.v = nn.Linear(dim, dim)
        self.o = nn.Linear(dim, dim)
        self.norm_q = WanRMSNorm(dim, eps=eps) if qk_norm else nn.Identity()
        self.norm_k = WanRMSNorm(dim, eps=eps) if qk_norm else nn.Identity()
        self._packed = _Packed()
        # WanModel.set_attention_block_mask: a sparse.BlockMask or None — a plain attribute (no parameter, no buffer,
        # not in the state_dict); read by the self-attention only (_attend / the training block), never by _attend_ctx
        self._block_mask = None
        # WanModel.set_attention_block_policy: a sparse.DynamicBlockPolicy or None, kept the same way; the mask the last
        # self-attention call built under it is left in last_block_mask for inspection
        self._block_policy = None
        self.last_block_mask = None

    def _dynamic_mask(self, q, k, B, S, lens32):
        """The block mask the layer's policy chooses for this call's q and k (bf16 [B*S, dim], q already carrying
        softmax_scale * log2(e)), built on the device: sparse.block_mask_from_rows."""
        bm = _sparse().block_mask_from_rows(q, k, B, self.num_heads, S, S, self.dim, self.dim, self._block_policy, 1.0, None,
                                            lens32)
        self.last_block_mask = bm
        return bm

    def _call_mask(self, fc, device, chosen=None):
        """The ``ops.AttnMask`` of a self-attention over fc.S (padded) positions, resolved on ``device``: the layer's band,
        its block mask, or the context's staircase / interval mask.  Under a block policy the mask is chosen after q and k
        exist: None then, and the call again with ``chosen`` = ``_dynamic_mask``'s BlockMask resolves it.  ValueError for
        two restrictions at once (they are not intersected) and for a block mask of other block or head counts."""
        window, bm, policy = tuple(self.window_size), self._block_mask, self._block_policy
        if bm is not None and policy is not None:
            raise ValueError("the layer has both a static block mask and a block policy")
        blocks, banded = bm is not None or policy is not None, window[0] >= 0 or window[1] >= 0
        if blocks and banded:
            raise ValueError(f"a block mask / policy excludes window_size={window} (it is not an intersection)")
        if (blocks or banded) and (fc.chunk is not None or fc.interval is not None):
            raise ValueError(f"{'causal chunks' if fc.chunk is not None else 'teacher forcing'} exclude(s) a block mask, a "
                             "block policy and a bounded window_size")
        if policy is not None and chosen is None:
            return None
        ext = 0 if fc.sink_fan is None else fc.sink_fan[1] * fc.sink_fan[2]        # (rotated sink copies behind the sequence)
        return ops.attn_mask(window, bm if chosen is None else chosen, fc.chunk, fc.interval, H=self.num_heads, Lq=fc.S,
                             Lk=fc.S + ext, device=device)

    # packed weights ---------------------------------------------------------
    def _w_qk(self):
        return self._packed.get("qk", (self.q.weight, self.k.weight, self.q.bias, self.k.bias), lambda: (
            _cat_bf16(self.q, self.k),
            torch.cat([self.q.bias.detach(), self.k.bias.detach()], 0).float().contiguous()), _lora_sig(self.q, self.k))

    def _w_qkv(self):
        return self._packed.get("qkv", (self.q.weight, self.k.weight, self.v.weight, self.q.bias, self.k.bias, self.v.bias),
                                lambda: (_cat_bf16(self.q, self.k, self.v),
                                         torch.cat([self.q.bias.detach(), self.k.bias.detach(), self.v.bias.detach()],
                                                   0).float().contiguous()), _lora_sig(self.q, self.k, self.v))

    def _w(self, name):
        lin = getattr(self, name)
        return self._packed.get(name, (lin.weight, lin.bias),
                                lambda: (_weight_bf16(lin), lin.bias.detach().float().contiguous()), _lora_sig(lin))

    def _norm_w(self, name):
        m = getattr(self, name)
        return m.weight.detach() if isinstance(m, WanRMSNorm) else None

    def _takes_fused(self, S):
        """Does a sequence of S rows per clip take q | k | v as ONE product per clip over the concatenated weights
        (ABI v10)?  h is read once and the V third leaves the kernel transposed (V^T [dim, Sp], what the attention kernel reads); the
        same bits as the two products, which short sequences / batches keep (their rows fill the chip only together).
        (tried at S = 1 560 in round 5: one launch instead of two is the same 19.7 ms per single-frame forward, and the
        batched CFG pair gets slower, 14.8 -> 15.4 ms: one launch per clip against two over both clips)
        (the library takes the one-launch form only when the q|k part is whole 384-column tiles: true at dim 1 536, not
        at dim 5 120, where asking for it would cost B launches and a third weight copy for nothing — ADVICE round 5)"""
        return S >= 8192 and S % 8 == 0 and (2 * self.dim) % 384 == 0

    def _operands(self, fused=False, W=None):
        """This layer's part of a ``BlockWeights``: q | k | v in one piece for the one-launch product (``fused``),
        else q | k and v; the o projection."""
        W = BlockWeights() if W is None else W
        if fused:
            W.wqkv, W.bqkv = self._w_qkv()
        else:
            (W.wqk, W.bqk), (W.wv, W.bv) = self._w_qk(), self._w("v")
        W.wo, W.bo = self._w("o")
        return W

    def _attend(self, h, fc: "_FwdCtx", W, extras=False, lse=False, o32=False, flags=0, vt_alloc=_vt_fresh, mask=None):
        """h bf16 [B*S, dim] -> attention output bf16 [B*S, dim] (before o-proj).  ``W``: a ``BlockWeights``.
        ``lse`` (fp32 [B, heads, S]) and ``o32`` (fp32 [B*S, dim], the output before its rounding): optional outputs;
        ``flags``: ops.flash_attn_raw's (the training node pins the short-sequence kernel); ``vt_alloc``: where V^T comes
        from; ``mask``: the resolved mask of an earlier call on the same input (a checkpoint re-run), else resolved here.
        The one-launch q | k | v product and the bounded long-sequence stream need ``flags == 0`` and no ``extras``.
        ``fc.sink_fan`` (teacher forcing under a pinned sink): k and V^T get ``copies * sink_rows`` more rows / columns per
        sample behind the S of the sequence; the norm + RoPE kernel and the V^T product write the first S as ever (only
        pitches change, k one launch per sample), ``ops.rope_shift_fan`` fills the k rows with the rotated sink keys, one
        device copy the V^T columns, and the attention runs with Lk = S + copies * sink_rows under the extended mask.
        Returns o; with ``extras`` (o, qk, q, k, vt, mask, lse, o32) — what the backward reads (k: [B * Lk, dim])."""
        if fc.cache is not None:
            return self._attend_cached(h, fc, W, extras)
        B, S, d, N, D = fc.B, fc.S, self.dim, self.num_heads, self.head_dim
        R = B * S
        fan = fc.sink_fan
        Lk = S if fan is None else S + fan[1] * fan[2]
        if mask is None:
            mask = self._call_mask(fc, h.device)           # None: a block policy, which chooses below
        # q|k projection kept in bf16 (fp32 accumulate): the normalisation statistics are taken in fp32 from
        # it; measured effect on the 30-layer output < 1e-3 relative RMS, and it halves this step's traffic
        qk = torch.empty(R, 2 * d, dtype=torch.bfloat16, device=h.device)
        Sp = _round_up(Lk, 64)
        fused = W.wqkv is not None and flags == 0 and not extras          # (see _takes_fused)
        assert fused or W.wqk is not None, "a q | k | v record serves only a call without flags and extras"
        if fused:
            vt = vt_alloc(B, d, Sp, Lk, h.device)          # (pad columns zero; the GEMM writes the rest)
            for b in range(B):                         # one launch per clip: V^T is [B, dim, Sp], a clip's rows fill the chip
                ops.gemm_raw(ptr(h, b * S * d), ptr(W.wqkv), ptr(qk, b * S * 2 * d), S, 3 * d, d, d, d, 2 * d,
                             EPI_BF16_SPLIT_T, bias=ptr(W.bqkv), bias_mode=BIAS_N, aux=ptr(vt, b * d * Sp), ldaux=Sp,
                             n_split=2 * d)
        else:
            ops.gemm_raw(ptr(h), ptr(W.wqk), ptr(qk), R, 2 * d, d, d, d, 2 * d, EPI_BF16, bias=ptr(W.bqk),
                         bias_mode=BIAS_N)
        q = torch.empty(R, d, dtype=torch.bfloat16, device=h.device)
        k = torch.empty(B * Lk, d, dtype=torch.bfloat16, device=h.device)
        # q leaves the norm kernel already multiplied by softmax_scale * log2(e) (attention.py:96-127), in fp32
        # before its one rounding to bf16: the attention kernel's exponentials then need no per-score multiply
        q_scale = D ** -0.5 * LOG2E
        wq, wk = self._norm_w("norm_q"), self._norm_w("norm_k")          # q and k: one launch (two column segments)
        # where the long-sequence attention stream runs, the norm kernel also emits max |q|^2, |k|^2 per (sample, head): the
        # stream then needs no running max (a bound on this call's scores: ops.flash_attn_raw, qk_norm2_max)
        nmax = None
        if flags == 0 and not extras:
            # (a block, staircase or interval mask runs the short-sequence kernel: no long-sequence stream, no bound)
            if mask is not None and mask.rule is None and D == 128 and d <= 5120 and \
                    ops.flash_attn_takes_bounded(B, N, S, S, d, d, d, Sp, mask.window):
                nmax = fc.bounds.take(B, N, h.device)                    # zeroed float [B, N, 2]
            self.last_qk_norm2_max = nmax                                # (read by tools/attn_bound_values.py)
        norm_args = (ptr(qk), 2 * d, d, ptr(q), ptr(k), R, d, ptr(wq) if wq is not None else None,
                     ptr(wk) if wk is not None else None, self.eps, int(self.qk_norm), ptr(fc.rope_cos), ptr(fc.rope_sin),
                     fc.rope_cos.shape[0], D, ptr(fc.grid32), S)
        if nmax is not None:
            ops.rmsnorm_rope_bf16_pair_bound_raw(*norm_args, ptr(nmax), out_scale0=q_scale, out_scale1=1.0)
        elif fan is None or B == 1:
            ops.rmsnorm_rope_bf16_pair_raw(*norm_args, out_scale0=q_scale, out_scale1=1.0)
        else:
            for b in range(B):                             # a sample's k rows start Lk rows behind the last one's
                ops.rmsnorm_rope_bf16_pair_raw(ptr(qk, b * S * 2 * d), 2 * d, d, ptr(q, b * S * d), ptr(k, b * Lk * d), S, d,
                                               *norm_args[7:15], ptr(fc.grid32, 3 * b), S, out_scale0=q_scale, out_scale1=1.0)
        if fan is not None:
            # the sink keys as the pinned rollout holds them for every later chunk: image c = rows [S + c sr, S + (c + 1) sr)
            tab, copies, sr = fan
            ops.rope_shift_fan(k.view(B, Lk, d)[:, :sr], torch.as_strided(k, (B, copies, sr, d), (Lk * d, sr * d, d, 1), S * d),
                               tab, D)
        if not extras:
            del qk
        if mask is None:                               # the mask is chosen from the q and k this call attends with
            mask = self._call_mask(fc, h.device, self._dynamic_mask(q, k, B, S, fc.seq_lens32))
        if not fused:
            # V^T[b] = Wv h_b^T + bv  ->  [B, dim, Sp]   (pad columns stay zero)
            vt = vt_alloc(B, d, Sp, Lk, h.device)
            ops.gemm_raw(ptr(W.wv), ptr(h), ptr(vt), d, S, d, d, d, Sp, EPI_BF16, bias=ptr(W.bv), bias_mode=BIAS_M,
                         batch=B,
                         strideA=0, strideB=S * d, strideC=d * Sp)
        if fan is not None:                            # V has no rotary position: the copies' columns are the sink's
            vt[:, :, S:Lk].unflatten(2, (fan[1], fan[2])).copy_(vt[:, :, None, :fan[2]].expand(-1, -1, fan[1], -1))
        o = torch.empty(R, d, dtype=torch.bfloat16, device=h.device)
        lse = torch.empty(B, N, S, dtype=torch.float32, device=h.device) if lse else None
        o32 = torch.empty(R, d, dtype=torch.float32, device=h.device) if o32 else None
        # window_size: flash-attn's bottom-right aligned band (model.py:151-156); a bounded one takes the short kernel
        # (under a sink fan-out every clip fills the sequence — forward_teacher_forcing — and every key row is live)
        ops.flash_attn_raw(ptr(q), ptr(k), ptr(vt), ptr(o), ptr(fc.seq_lens32) if fan is None else None, B, N, S, Lk, S * d, d,
                           Lk * d, d, d * Sp, S * d, d, Sp, D ** -0.5, lse=ptr(lse) if lse is not None else None, q_prescaled=1,
                           o32=ptr(o32) if o32 is not None else None, flags=flags,
                           qk_norm2_max=ptr(nmax) if nmax is not None else None, mask=mask)
        return (o, qk, q, k, vt, mask, lse, o32) if extras else o

    def _attend_cached(self, h, fc: "_FwdCtx", W, extras=False):
        """``_attend`` for WanModel.forward_chunk: h holds the rows of ONE chunk per sample.  q, k, v are projected for
        these rows only (``W``: the caller's ``BlockWeights``, its two-product form); k (normalised, rotated) lands in
        rows [length, length + C) of this layer's cache and V^T in the same columns, straight from the V^T product (ldc = the cache pitch); plain attention then runs with Lq = C over the
        keys [lo, length + C) of the cache — a pointer offset, no copy.  The launches of ``_attend`` at seq_len = C
        otherwise, so on an empty cache the result has its bits.
        A ``causal.RollingKVCache``: the chunk's rows go to ``fc.cache_pos`` (its slot) and the keys are [0, fc.cache_hi) —
        every filled slot; softmax attention does not depend on the order of its keys, and they carry absolute rotary
        positions (a cache with ``pin_sink`` has moved its sink rows behind the window before the blocks run:
        ``RollingKVCache.pin``).  ``fc.cache_mask`` (a short last chunk in a wrapped ring): the interval kernel skips the stale keys
        behind the chunk in its slot.
        ``extras`` (forward_chunk(grad=True), model_train.py): ``lse`` and ``o32`` are asked for on top (the choice of the
        kernel does not depend on them), and the chunk's own k rows and V (row-major, what the backward reads) are copied
        out: the next denoising step and the commit pass overwrite them in the cache.
        Returns o; with ``extras`` (o, qk, q, k_own, v_own, lse, o32)."""
        B, C, d, N, D = fc.B, fc.S, self.dim, self.num_heads, self.head_dim
        cache, lo = fc.cache, fc.cache_lo
        kc, vtc = cache.k[fc.cache_layer], cache.vt[fc.cache_layer]
        L0, cap, pitch = cache.length, cache.cap, cache.pitch
        hi = L0 + C
        if fc.cache_pos is not None:
            L0, hi = fc.cache_pos, fc.cache_hi             # (L0: where this chunk's rows go)
        R = B * C
        qk = torch.empty(R, 2 * d, dtype=torch.bfloat16, device=h.device)
        ops.gemm_raw(ptr(h), ptr(W.wqk), ptr(qk), R, 2 * d, d, d, d, 2 * d, EPI_BF16, bias=ptr(W.bqk), bias_mode=BIAS_N)
        q = torch.empty(R, d, dtype=torch.bfloat16, device=h.device)
        wq, wk = self._norm_w("norm_q"), self._norm_w("norm_k")
        for b in range(B):                                 # one launch per sample: its k rows sit at their own place in the cache
            ops.rmsnorm_rope_bf16_pair_raw(ptr(qk, b * C * 2 * d), 2 * d, d, ptr(q, b * C * d), ptr(kc, (b * cap + L0) * d), C, d,
                                           ptr(wq) if wq is not None else None, ptr(wk) if wk is not None else None,
                                           self.eps, int(self.qk_norm), ptr(fc.rope_cos), ptr(fc.rope_sin),
                                           fc.rope_cos.shape[0], D, ptr(fc.grid32, 3 * b), C,
                                           out_scale0=D ** -0.5 * LOG2E, out_scale1=1.0)
        ops.gemm_raw(ptr(W.wv), ptr(h), ptr(vtc, L0), d, C, d, d, d, pitch, EPI_BF16, bias=ptr(W.bv), bias_mode=BIAS_M,
                     batch=B,
                     strideA=0, strideB=C * d, strideC=d * pitch)
        o = torch.empty(R, d, dtype=torch.bfloat16, device=h.device)
        lse = torch.empty(B, N, C, dtype=torch.float32, device=h.device) if extras else None
        o32 = torch.empty(R, d, dtype=torch.float32, device=h.device) if extras else None
        # without a mask, pinned to the short-sequence kernel: its V^T reads end at most 63 columns past the last key (the
        # cache keeps that much slack behind its last row); a chunk of queries does not reach the long-sequence dispatch at
        # 12 heads
        ops.flash_attn_raw(ptr(q), ptr(kc, lo * d), ptr(vtc, lo), ptr(o), None, B, N, C, hi - lo, C * d, d, cap * d, d,
                           d * pitch, C * d, d, pitch, D ** -0.5, lse=ptr(lse) if extras else None, q_prescaled=1,
                           o32=ptr(o32) if extras else None, flags=0 if fc.cache_mask is not None else ops.ATTN_SHORT_KERNEL,
                           mask=fc.cache_mask)
        if not extras:
            return o
        k_own = kc[:, L0:L0 + C].clone()                   # [B, C, d]
        v_own = torch.empty(B, C, d, dtype=torch.bfloat16, device=h.device)
        ops.transpose_bf16_raw(ptr(vtc, L0), ptr(v_own), d, C, pitch, d, batch=B, bs_in=d * pitch, bs_out=C * d)
        return o, qk, q, k_own.view(R, d), v_own.view(R, d), lse, o32

    def forward(self, x, seq_lens, grid_sizes, freqs, _fc: Optional["_FwdCtx"] = None):
        """Reference signature (model.py:132): x [B, L, C] -> [B, L, C] fp32."""
        B, S, d = x.shape
        fc = _fc or _make_ctx_for_attention(self, x, seq_lens, grid_sizes, freqs)
        h = x.reshape(B * S, d)
        h = h if h.dtype == torch.bfloat16 else ops.cast_bf16(h.float().contiguous())
        W = self._operands(fc.cache is None and self._takes_fused(S))
        o = self._attend(h.contiguous(), fc, W)
        return ops.gemm(o, W.wo, bias=W.bo, epilogue=EPI_F32).view(B, S, d)


class WanT2VCrossAttention(WanSelfAttention):
    """model.py:164-186."""

    n_img = 0                                          # context rows in front of the text (the i2v image tokens)

    def _operands(self, W=None):
        """This layer's part of a ``BlockWeights``."""
        W = BlockWeights() if W is None else W
        (W.wq_c, W.bq_c), (W.wk_c, W.bk_c), (W.wv_c, W.bv_c), (W.wo_c, W.bo_c) = (self._w(n) for n in "qkvo")
        return W

    def _context_kv(self, fc: "_FwdCtx", W, img=False, extras=False, vt_alloc=None):
        """K (normalised, bf16 [B*L, dim]) and V^T ([B, dim, Lp]) of the text rows of the context (``img``: of its
        N_IMG image rows): (kn, vt, L, Lp), kept in ``fc.kv`` (a ContextState's cache).  ``vt_alloc``: where V^T comes
        from (``_vt_fresh``'s signature; None: a zeroed tensor).  With ``extras`` (kn, vt, L, Lp, kf): the fp32 K before
        its norm on top."""
        if img:
            wk, bk, wv, bv, nname, key, lo, hi = W.wk_i, W.bk_i, W.wv_i, W.bv_i, "norm_k_img", "k_img", 0, N_IMG
        else:
            wk, bk, wv, bv, nname, key, lo, hi = W.wk_c, W.bk_c, W.wv_c, W.bv_c, "norm_k", "k", self.n_img, fc.Lc
        kv = fc.kv
        if kv is not None and not extras and (id(self), key) in kv:
            return kv[(id(self), key)]
        B, d = fc.B, self.dim
        ctx = fc.ctx                                    # bf16 [B, Lc, dim]
        L = hi - lo
        Lp = _round_up(L, 64)
        kf = torch.empty(B, L, d, dtype=torch.float32, device=ctx.device)
        ops.gemm_raw(ptr(ctx, lo * d), ptr(wk), ptr(kf), L, d, d, d, d, d, EPI_F32, bias=ptr(bk), bias_mode=BIAS_N,
                     batch=B, strideA=fc.Lc * d, strideB=0, strideC=L * d)
        kn = ops.rmsnorm_rope(kf.view(B * L, d), self._norm_w(nname), self.eps, do_norm=self.qk_norm)
        if vt_alloc is None:
            vt = torch.zeros(B, d, Lp, dtype=torch.bfloat16, device=ctx.device)
        else:
            vt = vt_alloc(B, d, Lp, L, ctx.device)
        ops.gemm_raw(ptr(wv), ptr(ctx, lo * d), ptr(vt), d, L, d, d, d, Lp, EPI_BF16, bias=ptr(bv), bias_mode=BIAS_M,
                     batch=B, strideA=0, strideB=fc.Lc * d, strideC=d * Lp)
        if kv is not None:
            kv[(id(self), key)] = (kn, vt, L, Lp)
        return (kn, vt, L, Lp, kf) if extras else (kn, vt, L, Lp)

    def _query(self, h, fc, W, extras=False):
        """The normalised query bf16 [R, dim]; with ``extras`` (q, its pre-norm projection)."""
        R, d = h.shape
        # as the self-attention's q|k: the projection leaves the GEMM in bf16 (fp32 accumulate), the norm takes its
        # statistics in fp32 from it — half the traffic of an fp32 q between the two kernels
        qb = ops.gemm(h, W.wq_c, bias=W.bq_c, epilogue=EPI_BF16)
        q = torch.empty(R, d, dtype=torch.bfloat16, device=h.device)
        w = self._norm_w("norm_q")
        ops.rmsnorm_rope_bf16_raw(ptr(qb), d, ptr(q), R, d, ptr(w) if w is not None else None, self.eps,
                                  int(self.qk_norm), None, None, 0, self.head_dim, None, fc.S)
        return (q, qb) if extras else q

    def _attend_rows(self, q, fc, W, img=False, extras=False, lse=False, o32=False, flags=0, vt_alloc=None):
        """Attention of q over the text rows of the context (``img``: over its image rows): bf16 [B*S, dim].
        ``lse`` / ``o32`` / ``flags``: as in ``WanSelfAttention._attend``.  With ``extras`` (o, kf, kn, vt, lse, o32)."""
        B, S, d, N, D = fc.B, fc.S, self.dim, self.num_heads, self.head_dim
        kn, vt, L, Lp, *kf = self._context_kv(fc, W, img, extras, vt_alloc)
        o = torch.empty(B * S, d, dtype=torch.bfloat16, device=q.device)
        lse = torch.empty(B, N, S, dtype=torch.float32, device=q.device) if lse else None
        o32 = torch.empty(B * S, d, dtype=torch.float32, device=q.device) if o32 else None
        # text rows: under fc.ctx_mask (frame-aligned condition tokens — the interval kernels with one group size per
        # axis; None: as ever) and the context lengths — for i2v the reference passes the (text + 257) lengths here
        # (model.py:223,537); keys are clipped to the text rows.  Image rows: every one of them, no lengths, no mask
        ops.flash_attn_raw(ptr(q), ptr(kn), ptr(vt), ptr(o), None if img else ptr(fc.ctx_lens32), B, N, S, L, S * d, d,
                           L * d, d, d * Lp, S * d, d, Lp, D ** -0.5, lse=ptr(lse) if lse is not None else None,
                           o32=ptr(o32) if o32 is not None else None, flags=flags,
                           mask=None if img else fc.ctx_mask)
        return (o, kf[0], kn, vt, lse, o32) if extras else o

    def _attend_ctx(self, h, fc: "_FwdCtx", W):
        """Returns the list of attention outputs (bf16 [B*S, dim]) whose sum feeds the o-projection: over the text,
        and for i2v over the image tokens too."""
        q = self._query(h, fc, W)
        return [self._attend_rows(q, fc, W, img) for img in ((False, True) if self.n_img else (False,))]

    def forward(self, x, context, context_lens, _fc: Optional["_FwdCtx"] = None, interval_mask=None):
        """Reference signature (model.py:166): returns [B, L1, C] fp32.  ``interval_mask``: a ``causal.IntervalMask`` over
        (queries, context rows) the attention runs under (a stand-alone call; inside a model the shared state carries it)."""
        B, S, d = x.shape
        fc = _fc or _make_ctx_for_cross(self, x, context, context_lens)
        if interval_mask is not None:
            fc.ctx_mask = ops.attn_mask(interval_mask=interval_mask, H=self.num_heads, Lq=S, Lk=fc.Lc, device=x.device)
        h = x.reshape(B * S, d)
        h = h if h.dtype == torch.bfloat16 else ops.cast_bf16(h.float().contiguous())
        W = self._operands()
        outs = self._attend_ctx(h.contiguous(), fc, W)
        y = ops.gemm(outs[0], W.wo_c, bias=W.bo_c, epilogue=EPI_F32)
        for extra in outs[1:]:
            ops.gemm(extra, W.wo_c, out=y, epilogue=ops.EPI_F32_ACCUM)
        return y.view(B, S, d)


class WanI2VCrossAttention(WanT2VCrossAttention):
    """model.py:189-230 — extra attention over the first N_IMG (CLIP image) context tokens."""

    def __init__(self, dim, num_heads, window_size=(-1, -1), qk_norm=True, eps=1e-6):
        super().__init__(dim, num_heads, window_size, qk_norm, eps)
        self.k_img = nn.Linear(dim, dim)
        self.v_img = nn.Linear(dim, dim)
        self.norm_k_img = WanRMSNorm(dim, eps=eps) if qk_norm else nn.Identity()

    n_img = N_IMG

    def _operands(self, W=None):
        W = super()._operands(W)
        (W.wk_i, W.bk_i), (W.wv_i, W.bv_i) = self._w("k_img"), self._w("v_img")
        return W


WAN_CROSSATTENTION_CLASSES = {"t2v_cross_attn": WanT2VCrossAttention, "i2v_cross_attn": WanI2VCrossAttention}


class WanAttentionBlock(nn.Module):
    """model.py:239-330."""

    def __init__(self, cross_attn_type, dim, ffn_dim, num_heads, window_size=(-1, -1), qk_norm=True,
                 cross_attn_norm=False, eps=1e-6):
        super().__init__()
        self.dim, self.ffn_dim, self.num_heads = dim, ffn_dim, num_heads
        self.window_size, self.qk_norm, self.cross_attn_norm, self.eps = window_size, qk_norm, cross_attn_norm, eps
        self.norm1 = WanLayerNorm(dim, eps)
        self.self_attn = WanSelfAttention(dim, num_heads, window_size, qk_norm, eps)
        self.norm3 = WanLayerNorm(dim, eps, elementwise_affine=True) if cross_attn_norm else nn.Identity()
        self.cross_attn = WAN_CROSSATTENTION_CLASSES[cross_attn_type](dim, num_heads, (-1, -1), qk_norm, eps)
        self.norm2 = WanLayerNorm(dim, eps)
        self.ffn = nn.Sequential(nn.Linear(dim, ffn_dim), nn.GELU(approximate="tanh"), nn.Linear(ffn_dim, dim))
        self.modulation = nn.Parameter(torch.randn(1, 6, dim) / dim ** 0.5)
        self._packed = _Packed()

    def _ffn_w(self, i):
        lin = self.ffn[i]
        return self._packed.get(f"ffn{i}", (lin.weight, lin.bias),
                                lambda: (_weight_bf16(lin), lin.bias.detach().float().contiguous()), _lora_sig(lin))

    def _operands(self, fused=False):
        """The ``BlockWeights`` of this block from the ``_Packed`` copies (``fused``: WanSelfAttention._operands), rebuilt
        when a parameter or an adapter behind it changed."""
        sa, ca = self.self_attn, self.cross_attn
        lins = [sa.q, sa.k, sa.v, sa.o, ca.q, ca.k, ca.v, ca.o, self.ffn[0], self.ffn[2]]
        if ca.n_img:
            lins += [ca.k_img, ca.v_img]
        params = [p for lin in lins for p in (lin.weight, lin.bias)]
        if self.cross_attn_norm:
            params += [self.norm3.weight, self.norm3.bias]

        def build():
            W = ca._operands(sa._operands(fused))
            (W.w1, W.b1), (W.w2, W.b2) = self._ffn_w(0), self._ffn_w(2)
            if self.cross_attn_norm:
                W.n3w, W.n3b = self.norm3.weight.detach().float(), self.norm3.bias.detach().float()
            return W
        return self._packed.get(("W", fused), params, build, _lora_sig(*lins))

    def forward(self, x, e, seq_lens, grid_sizes, freqs, context, context_lens, block_idx=0,
                _fc: Optional["_FwdCtx"] = None, _part: str = "all"):
        """x fp32 [B, L, C] residual stream (updated and returned), e fp32 [B, 6, C].
        ``_part`` (WanModel.forward_cfg_pair): "self" = the self-attention sub-layer only, "rest" = what follows it.
        The launches are the steps above (the training node's too: model_train._block_forward), here in place on x."""
        assert e.dtype == torch.float32
        fc = _fc or _make_ctx_for_block(self, x, e, seq_lens, grid_sizes, freqs, context, context_lens)
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.float().contiguous()
        mod = self.modulation.detach()
        if mod.dtype != torch.float32:
            mod = mod.float()
        sa, ca = self.self_attn, self.cross_attn
        W = self._operands(fc.cache is None and sa._takes_fused(x.shape[1]))
        # ---- self-attention: x += o(attn(LN(x)(1+e1)+e0)) * e2        model.py:292-296
        if _part != "rest":
            h = _ln_mod(x, fc, mod, self.eps, 0, 1)
            o = sa._attend(h, fc, W)
            _resid(x, o, W.wo, W.bo, fc, mod, 2)
            del h, o
            if _part == "self":
                return x
        # ---- cross-attention: x += o(attn(norm3(x), context))          model.py:313
        h = _cross_input(x, W, getattr(self.norm3, "eps", self.eps))
        outs = ca._attend_ctx(h, fc, W)
        _resid(x, outs[0], W.wo_c, W.bo_c, fc)
        for extra in outs[1:]:
            _resid(x, extra, W.wo_c, None, fc)
        del h, outs
        # ---- FFN: x += (W2 gelu(W1 (LN(x)(1+e4)+e3) + b1) + b2) * e5    model.py:314-328
        u = _ffn_up(_ln_mod(x, fc, mod, self.eps, 3, 4), W)
        _resid(x, u, W.w2, W.b2, fc, mod, 5)
        return x

    def cross_attn_ffn(self, x, context, context_lens, e, block_idx):  # pragma: no cover - API parity
        raise NotImplementedError("cross_attn_ffn is fused into WanAttentionBlock.forward in this build")


class Head(nn.Module):
    """model.py:332-359."""

    def __init__(self, dim, out_dim, patch_size, eps=1e-6):
        super().__init__()
        self.dim, self.out_dim, self.patch_size, self.eps = dim, out_dim, patch_size, eps
        out_dim = math.prod(patch_size) * out_dim
        self.norm = WanLayerNorm(dim, eps)
        self.head = nn.Linear(dim, out_dim)
        self.modulation = nn.Parameter(torch.randn(1, 2, dim) / dim ** 0.5)
        self._packed = _Packed()

    def forward(self, x, e, rows_per_batch=None):
        """x fp32 [B, L, C], e fp32 [B, C] -> fp32 [B, L, prod(patch)*out_dim].  ``rows_per_batch``: rows of x that share
        one row of e (default L; h * w with a per-frame t, e then [B * L / (h w), C])."""
        assert e.dtype == torch.float32
        B, S, d = x.shape
        R = B * S
        x = x.float().contiguous()
        e = e.contiguous()
        mod = self.modulation.detach().float()
        h = torch.empty(R, d, dtype=torch.bfloat16, device=x.device)
        ops.layernorm_modulate_raw(ptr(x), ptr(h), R, d, self.eps, 1.0, ptr(mod, d), ptr(e), d, ptr(mod, 0), ptr(e), d,
                                   rows_per_batch or S)
        w, b = self._packed.get("head", (self.head.weight, self.head.bias), lambda: (
            _bf16(self.head.weight), self.head.bias.detach().float().contiguous()))
        return ops.gemm(h, w, bias=b, epilogue=EPI_F32).view(B, S, -1)


class MLPProj(nn.Module):
    """model.py:362-374 (CLIP image tokens -> model dim, i2v only)."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.proj = nn.Sequential(nn.LayerNorm(in_dim), nn.Linear(in_dim, in_dim), nn.GELU(),
                                  nn.Linear(in_dim, out_dim), nn.LayerNorm(out_dim))
        self._packed = _Packed()

    def _w(self, i):
        lin = self.proj[i]
        return self._packed.get(f"l{i}", (lin.weight, lin.bias),
                                lambda: (_bf16(lin.weight), lin.bias.detach().float().contiguous()))

    def forward(self, image_embeds):
        """[B, 257, 1280] CLIP tokens -> bf16 [B, 257, out_dim]  (LayerNorm, Linear, GELU(erf), Linear, LayerNorm)."""
        B, L, Cin = image_embeds.shape
        x = image_embeds.float().contiguous().view(B * L, Cin)
        ln0, ln4 = self.proj[0], self.proj[4]
        h = ops.layernorm_modulate(x, ln0.eps, 0.0, mul0=ln0.weight.detach().float(), add0=ln0.bias.detach().float())
        w1, b1 = self._w(1)
        w3, b3 = self._w(3)
        h = ops.gemm(h, w1, bias=b1, epilogue=ops.EPI_GELU_ERF_BF16)
        h = ops.gemm(h, w3, bias=b3, epilogue=EPI_F32)
        out = ops.layernorm_modulate(h, ln4.eps, 0.0, mul0=ln4.weight.detach().float(),
                                     add0=ln4.bias.detach().float())
        return out.view(B, L, -1)


def _rope_tables(freqs: torch.Tensor, device):
    """fp32 cos/sin of the reference's complex rotary table."""
    return (freqs.real.to(torch.float32).contiguous().to(device),
            freqs.imag.to(torch.float32).contiguous().to(device))


def _make_ctx_for_block(block, x, e, seq_lens, grid_sizes, freqs, context, context_lens):
    """Build the per-forward context when a block is called stand-alone with
    the reference's positional arguments (e.g. from a test or a hook)."""
    B, S, d = x.shape
    fc = _FwdCtx()
    fc.B, fc.S, fc.dim = B, S, d
    fc.split_k = True
    fc.e0 = e.contiguous()
    fc.seq_lens32 = seq_lens.to(device=x.device, dtype=torch.int32).contiguous()
    fc.grid32 = grid_sizes.to(device=x.device, dtype=torch.int32).contiguous()
    fc.rope_cos, fc.rope_sin = freqs if isinstance(freqs, tuple) else _rope_tables(freqs, x.device)
    ctx = context
    fc.ctx = ctx if ctx.dtype == torch.bfloat16 else ops.cast_bf16(ctx.float().contiguous())
    fc.Lc = ctx.shape[1]
    fc.ctx_lens32 = (context_lens.to(device=x.device, dtype=torch.int32).contiguous()
                     if context_lens is not None else None)
    return fc


def _make_ctx_for_attention(attn, x, seq_lens, grid_sizes, freqs):
    B, S, d = x.shape
    fc = _FwdCtx()
    fc.B, fc.S, fc.dim = B, S, d
    fc.seq_lens32 = seq_lens.to(device=x.device, dtype=torch.int32).contiguous()
    fc.grid32 = grid_sizes.to(device=x.device, dtype=torch.int32).contiguous()
    fc.rope_cos, fc.rope_sin = freqs if isinstance(freqs, tuple) else _rope_tables(freqs, x.device)
    return fc


def _make_ctx_for_cross(attn, x, context, context_lens):
    B, S, d = x.shape
    fc = _FwdCtx()
    fc.B, fc.S, fc.dim = B, S, d
    fc.ctx = context if context.dtype == torch.bfloat16 else ops.cast_bf16(context.float().contiguous())
    fc.Lc = context.shape[1]
    fc.ctx_lens32 = (context_lens.to(device=x.device, dtype=torch.int32).contiguous()
                     if context_lens is not None else None)
    return fc


class WanModel(nn.Module):
    r"""Wan diffusion backbone (t2v / i2v) — reference model.py:377-612."""

    ignore_for_config = ["patch_size", "cross_attn_norm", "qk_norm", "text_dim", "window_size"]
    _no_split_modules = ["WanAttentionBlock"]

    def __init__(self, model_type="t2v", patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=2048, ffn_dim=8192,
                 freq_dim=256, text_dim=4096, out_dim=16, num_heads=16, num_layers=32, window_size=(-1, -1),
                 qk_norm=True, cross_attn_norm=True, eps=1e-6, use_checkpoint=True):
        super().__init__()
        assert model_type in ["t2v", "i2v"]
        self.config = dict(model_type=model_type, patch_size=tuple(patch_size), text_len=text_len, in_dim=in_dim,
                           dim=dim, ffn_dim=ffn_dim, freq_dim=freq_dim, text_dim=text_dim, out_dim=out_dim,
                           num_heads=num_heads, num_layers=num_layers, window_size=tuple(window_size),
                           qk_norm=qk_norm, cross_attn_norm=cross_attn_norm, eps=eps)
        self.model_type = model_type
        self.use_checkpoint = use_checkpoint
        # how a True flag is honoured (model_train.py): "auto" keeps the activations when a step's worth of them fits in
        # half of the free HBM (same gradients, no second forward pass), "always" re-runs every block in the backward
        self.checkpoint_policy = "auto"
        # reference quirk (model.py:317-324): FFNs of blocks > 10 receive no gradient; False = full gradients
        self.reference_ffn_freeze = True
        # False (default): products with few rows and a long contraction — the FFN-down projection at one or two
        # [16,1,60,104] clips — are summed in 2-4 k slices (ABI v9), so a sample's last bits depend on how many samples
        # share its forward (a clip alone, in a CFG pair, in a batch of four: 4 / 2 / no slices; 9e-3 between the
        # guided velocities, where each is 1e-2 from the fp32 arithmetic).  True: every product keeps one summation order
        # whatever the batch — bit-identical outputs for a sample alone and inside any batch, at the price of the
        # small-M speed-up (15.3 -> 16.1 ms per single-frame CFG pair).  Nothing is split at the sampling sizes
        # (S = 32 760) either way.  ADVICE round 4; pinned by test_batch_invariant_flag_pins_the_summation_order.
        self.batch_invariant = False
        self.patch_size = tuple(patch_size)
        self.text_len, self.in_dim, self.dim, self.ffn_dim = text_len, in_dim, dim, ffn_dim
        self.freq_dim, self.text_dim, self.out_dim = freq_dim, text_dim, out_dim
        self.num_heads, self.num_layers, self.window_size = num_heads, num_layers, window_size
        self.qk_norm, self.cross_attn_norm, self.eps = qk_norm, cross_attn_norm, eps

        self.patch_embedding = nn.Conv3d(in_dim, dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.text_embedding = nn.Sequential(nn.Linear(text_dim, dim), nn.GELU(approximate="tanh"),
                                            nn.Linear(dim, dim))
        self.time_embedding = nn.Sequential(nn.Linear(freq_dim, dim), nn.SiLU(), nn.Linear(dim, dim))
        self.time_projection = nn.Sequential(nn.SiLU(), nn.Linear(dim, dim * 6))

        cross_attn_type = "t2v_cross_attn" if model_type == "t2v" else "i2v_cross_attn"
        self.blocks = nn.ModuleList([
            WanAttentionBlock(cross_attn_type, dim, ffn_dim, num_heads, window_size, qk_norm, cross_attn_norm, eps)
            for _ in range(num_layers)])
        self.head = Head(dim, out_dim, self.patch_size, eps)

        assert (dim % num_heads) == 0 and (dim // num_heads) % 2 == 0
        d = dim // num_heads
        if d != 128:
            raise NotImplementedError(f"head_dim {d}: the gfx950 attention kernel is built for head_dim 128 "
                                      "(every Wan2.1 checkpoint)")
        # not a buffer, as in the reference (model.py:484-492)
        self.freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)),
                                rope_params(1024, 2 * (d // 6))], dim=1)
        if model_type == "i2v":
            self.img_emb = MLPProj(1280, dim)
        self._packed = _Packed()
        self._rope_dev = None
        self._causal_chunks = None                  # set_causal_chunks: (frames per chunk, left_chunks[, sink_chunks > 0]) or None
        self.init_weights()

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_config(cls, config: dict, **kw):
        cfg = {k: v for k, v in config.items() if not k.startswith("_")}
        cfg.update(kw)
        return cls(**cfg)

    @classmethod
    def from_pretrained(cls, checkpoint_dir: str, **kw):
        """diffusers-layout loader: ``config.json`` + ``diffusion_pytorch_model*.safetensors``
        (what the reference gets from diffusers' ModelMixin, text2video.py:86)."""
        import glob
        import json
        import os
        from safetensors.torch import load_file
        with open(os.path.join(checkpoint_dir, "config.json")) as fh:
            config = json.load(fh)
        allowed = set(cls.__init__.__code__.co_varnames)
        model = cls(**{k: v for k, v in config.items() if k in allowed}, **kw)
        sd = {}
        for f in sorted(glob.glob(os.path.join(checkpoint_dir, "diffusion_pytorch_model*.safetensors"))):
            sd.update(load_file(f))
        model.load_state_dict(sd, strict=True)
        return model

    # ------------------------------------------------------------------ sparsity
    def set_attention_block_mask(self, mask, layers=None):
        """Restrict the SELF-attention of ``layers`` (None: every block; else an iterable of block indices) to the kept
        128 x 128 blocks of ``mask``: a bool tensor ``[nb, nb]`` (all heads) or ``[num_heads, nb, nb]``, a
        ``sparse.BlockMask``, or None to clear.  nb = ceil(seq_len / 128) for the ``seq_len`` later passed to ``forward``
        (checked there: ValueError); the mask is in padded-sequence coordinates, shared by the samples of a batch, and
        ``seq_lens`` still limits the keys.  Honoured by ``forward`` (inference and training), ``forward_cfg_pair`` and
        the LoRA paths; cross-attention is never masked.  The mask is no parameter or buffer and is in neither ``config``
        nor the ``state_dict``.  A model built with a bounded ``window_size`` refuses a mask (ValueError)."""
        import importlib
        sparse = importlib.import_module(ops.__package__ + ".sparse")
        idx = list(range(len(self.blocks))) if layers is None else [int(i) for i in layers]
        for i in idx:
            if not 0 <= i < len(self.blocks):
                raise ValueError(f"set_attention_block_mask: no block {i} (the model has {len(self.blocks)})")
        bm = None
        if mask is not None:
            if self.window_size[0] >= 0 or self.window_size[1] >= 0:
                raise ValueError(f"set_attention_block_mask: the model has window_size={tuple(self.window_size)}; a block "
                                 "mask excludes a bounded window (it is not an intersection)")
            if isinstance(mask, sparse.BlockMask):
                bm = mask
            else:
                if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() not in (2, 3):
                    raise ValueError("set_attention_block_mask: a bool tensor [nb, nb] or [num_heads, nb, nb] is expected")
                if mask.shape[-1] != mask.shape[-2]:
                    raise ValueError(f"set_attention_block_mask: self-attention needs a square mask, got {tuple(mask.shape)}")
                L = int(mask.shape[-1]) * sparse.BLOCK
                bm = sparse.BlockMask(mask, L, L)
            if bm.q_blocks != bm.k_blocks:
                raise ValueError("set_attention_block_mask: self-attention needs a square mask")
            if bm.heads not in (1, self.num_heads):
                raise ValueError(f"set_attention_block_mask: {bm.heads} heads in the mask, 1 or {self.num_heads} expected")
        if bm is not None:
            for i in idx:
                if self.blocks[i].self_attn._block_policy is not None:
                    raise ValueError(f"set_attention_block_mask: block {i} has a block policy; clear it first "
                                     "(set_attention_block_policy(None))")
        for i in idx:
            self.blocks[i].self_attn._block_mask = bm

    def set_attention_block_policy(self, policy, layers=None):
        """Let the SELF-attention of ``layers`` (None: every block; else an iterable of block indices) choose its own
        block mask per call, per head, from the q and k it is about to attend with: ``policy`` is a
        ``sparse.DynamicBlockPolicy`` (top-p over block-pooled scores; the rule: include/omh.h), or None to clear.  The
        mask is built on the device after the norm / RoPE kernel, with no host synchronisation, and handed to the
        block-list kernels; the layer keeps it in ``self_attn.last_block_mask``.  It is shared by the samples of a batch
        (the union of their selections; at batch 1 the sample's own) and ``seq_lens`` limits the keys it is chosen from.
        Honoured by ``forward`` (inference and training: a block's backward and its checkpoint re-run use the mask its
        forward built), ``forward_cfg_pair`` (block 0's shared mask is built once) and the LoRA paths; cross-attention
        never is.  No parameter, no buffer, not in ``config`` or the ``state_dict``.  Raises ValueError for a layer that
        has a static mask (``set_attention_block_mask``), a model with a bounded ``window_size``, and an ``always``
        whose block count the ``seq_len`` of a later ``forward`` does not match (raised there)."""
        sparse = _sparse()
        idx = list(range(len(self.blocks))) if layers is None else [int(i) for i in layers]
        for i in idx:
            if not 0 <= i < len(self.blocks):
                raise ValueError(f"set_attention_block_policy: no block {i} (the model has {len(self.blocks)})")
        if policy is not None:
            if not isinstance(policy, sparse.DynamicBlockPolicy):
                raise ValueError("set_attention_block_policy: a sparse.DynamicBlockPolicy (or None) is expected")
            if self.window_size[0] >= 0 or self.window_size[1] >= 0:
                raise ValueError(f"set_attention_block_policy: the model has window_size={tuple(self.window_size)}; a "
                                 "block policy excludes a bounded window (it is not an intersection)")
            a = policy.always
            if a is not None:
                if a.shape[-1] != a.shape[-2]:
                    raise ValueError(f"set_attention_block_policy: self-attention needs a square always, got {tuple(a.shape)}")
                if a.dim() == 3 and a.shape[0] not in (1, self.num_heads):
                    raise ValueError(f"set_attention_block_policy: {a.shape[0]} heads in always, 1 or {self.num_heads} expected")
            for i in idx:
                if self.blocks[i].self_attn._block_mask is not None:
                    raise ValueError(f"set_attention_block_policy: block {i} has a static block mask; clear it first "
                                     "(set_attention_block_mask(None))")
        for i in idx:
            self.blocks[i].self_attn._block_policy = policy
            if policy is None:
                self.blocks[i].self_attn.last_block_mask = None

    # ------------------------------------------------------------------ causal chunks
    def set_causal_chunks(self, frames_per_chunk, left_chunks=-1, sink_chunks=0):
        """Run every SELF-attention of ``forward`` under the chunk-causal staircase (the rule: include/omh.h,
        omh_chunk_causal): with C = frames_per_chunk * (h / p_h) * (w / p_w) tokens per chunk, token i sees token j iff
        j // C <= i // C and, for ``left_chunks`` >= 0, j // C >= i // C - left_chunks (< 0: every earlier chunk).
        ``frames_per_chunk`` = None clears it.  Honoured by ``forward`` (inference, training, the ``use_checkpoint``
        re-run, input gradients, LoRA) and ``forward_cfg_pair``; ``forward_chunk`` takes its chunk length and look-back
        from it.  Cross-attention is never masked.  A run-time attribute like the block mask: in neither ``config`` nor
        the ``state_dict``.  ValueError for a model with a bounded ``window_size`` and for a layer that has a block mask
        or a block policy (here and again at ``forward``), and at ``forward`` for a batch whose clips do not share h, w
        (one C serves the call; clips of different frame counts padded to ``seq_len`` are fine).

        ``sink_chunks`` = S > 0 (with ``left_chunks`` = W >= 0; it is 0 otherwise): an attention sink — the first S chunks
        stay visible behind the window, j // C < S or j // C >= i // C - W.  ``forward`` and ``forward_cfg_pair`` then run
        self-attention under ``causal.IntervalMask(causal.sink_window_groups(ceil(seq_len / C), S, W), C)`` (two runs, the
        interval kernels) in place of the staircase kernels, ``forward_teacher_forcing`` under the three-run teacher-forcing
        mask, and ``forward_chunk`` needs a ``causal.RollingKVCache`` of the same (C, W, S)."""
        if frames_per_chunk is None:
            self._causal_chunks = None
            return
        fpc, left, sink = int(frames_per_chunk), int(left_chunks), int(sink_chunks)
        if fpc < 1:
            raise ValueError(f"set_causal_chunks: frames_per_chunk = {frames_per_chunk}, at least 1 expected")
        if sink < 0:
            raise ValueError(f"set_causal_chunks: sink_chunks = {sink_chunks}, at least 0 expected")
        self._causal_check("set_causal_chunks")
        # (fpc, W) as ever without a sink; (fpc, W, S) with one — causal.sample saves and restores the tuple whole
        self._causal_chunks = (fpc, -1 if left < 0 else left) + ((sink,) if left >= 0 and sink > 0 else ())

    def _causal_sink(self):
        """``sink_chunks`` of ``set_causal_chunks`` (0: none, or no causal chunks)."""
        cc = getattr(self, "_causal_chunks", None)
        return cc[2] if cc is not None and len(cc) > 2 else 0

    def _causal_check(self, who):
        if self.window_size[0] >= 0 or self.window_size[1] >= 0:
            raise ValueError(f"{who}: the model has window_size={tuple(self.window_size)}; causal chunks exclude a "
                             "bounded window (it is not an intersection)")
        for i, blk in enumerate(self.blocks):
            if blk.self_attn._block_mask is not None or blk.self_attn._block_policy is not None:
                raise ValueError(f"{who}: block {i} has a block mask / block policy; causal chunks exclude it "
                                 "(clear it first)")

    def _causal_rule(self, grids):
        """(tokens per chunk, left_chunks, 0) for a forward over clips with these (f, h, w) grids, or None."""
        cc = getattr(self, "_causal_chunks", None)
        if cc is None:
            return None
        self._causal_check("forward under set_causal_chunks")
        hw = {(g[1], g[2]) for g in grids}
        if len(hw) != 1:
            raise ValueError(f"forward under set_causal_chunks: the clips of a batch must share h, w (one chunk length "
                             f"serves the call), got {sorted(hw)}")
        h, w = next(iter(hw))
        return (cc[0] * h * w, cc[1], 0)

    def _sink_mask(self, seq_len, chunk_tokens, device):
        """The sink + window mask of a ``forward`` over ``seq_len`` tokens (cached per shape, as ``_tf_masks`` is)."""
        from ... import causal as _causal
        cc = self._causal_chunks
        n = (seq_len + chunk_tokens - 1) // chunk_tokens
        key = ("sink", n, cc[1], cc[2], chunk_tokens, str(device))
        masks = self.__dict__.setdefault("_tf_masks", {})
        if key not in masks:
            if len(masks) > 64:
                masks.clear()
            masks[key] = _causal.IntervalMask(_causal.sink_window_groups(n, cc[2], cc[1]), chunk_tokens, device)
        return masks[key]

    def _stale_mask(self, cache, pos, C, tpf, device):
        """The interval mask of a short chunk (``C`` tokens at ``pos``) in a wrapped ring: every query sees the keys
        [0, pos + C) and [pos + chunk_tokens, cap) — not the stale keys behind it in its slot.  Groups of one frame's
        tokens (>= 8: ValueError otherwise); resolved (an ``ops.AttnMask``) and cached per shape."""
        from ... import causal as _causal
        if tpf < 8:
            raise ValueError(f"forward_chunk: a short last chunk in a full RollingKVCache needs at least 8 tokens per frame, "
                             f"got {tpf}")
        key = ("stale", pos, C, tpf, cache.cap, cache.chunk_tokens, str(device))
        masks = self.__dict__.setdefault("_tf_masks", {})
        if key not in masks:
            if len(masks) > 64:
                masks.clear()
            vis = torch.ones(C // tpf, cache.cap // tpf, dtype=torch.bool)
            vis[:, (pos + C) // tpf:(pos + cache.chunk_tokens) // tpf] = False
            masks[key] = ops.attn_mask(interval_mask=_causal.IntervalMask(vis, tpf, device), H=self.num_heads, Lq=C,
                                       Lk=cache.cap, device=device)
        return masks[key]

    def _rope_shifted(self, device, frame_offset, frames):
        """The cos / sin tables with the FRAME columns moved up by ``frame_offset`` rows: frame f < ``frames`` of a chunk
        then rotates like frame frame_offset + f of the clip; the h / w columns stay.  While the chunk ends inside the
        table its rows are slices of it; past the table (an unbounded rollout) the frame angles of rows [frame_offset,
        frame_offset + frames) are computed in fp64 by ``rope_params``' formula — the same fp32 cos / sin a longer table
        would hold.  The few most recent offsets are kept (a rollout asks for a new one every chunk)."""
        cos, sin = self._rope(device)
        if frame_offset == 0:
            return cos, sin
        inside = frame_offset + frames <= cos.shape[0]
        key = (str(device), int(frame_offset)) + (() if inside else (int(frames),))
        tabs = getattr(self, "_rope_shift_cache", None)
        if tabs is None or tabs[0] is not cos:
            tabs = self._rope_shift_cache = (cos, {})
        hit = tabs[1].pop(key, None)
        if hit is None:
            d = self.dim // self.num_heads
            nf = (d - 4 * (d // 6)) // 2                                     # pair-columns of the frame axis
            c2, s2 = cos.clone(), sin.clone()
            if inside:
                n = cos.shape[0] - frame_offset
                c2[:n, :nf] = cos[frame_offset:, :nf]
                s2[:n, :nf] = sin[frame_offset:, :nf]
            else:
                inv = 1.0 / torch.pow(10000, torch.arange(0, 2 * nf, 2).to(torch.float64).div(2 * nf))
                ang = torch.outer(torch.arange(frame_offset, frame_offset + frames), inv)     # fp64, as rope_params
                c2[:frames, :nf] = torch.cos(ang).to(torch.float32).to(device)
                s2[:frames, :nf] = torch.sin(ang).to(torch.float32).to(device)
            hit = (c2, s2)
        tabs[1][key] = hit                                                   # (re-inserted: the newest entry)
        while len(tabs[1]) > 4:
            tabs[1].pop(next(iter(tabs[1])))
        return hit

    def _rope_repeated(self, device, frames):
        """The cos / sin tables with rows [frames, 2 frames) of the FRAME columns repeating rows [0, frames): frame
        frames + f of a doubled clip rotates like frame f; the h / w columns stay.  Cached per frame count."""
        cos, sin = self._rope(device)
        key = (str(device), int(frames))
        tabs = getattr(self, "_rope_repeat_cache", None)
        if tabs is None or tabs[0] is not cos:
            tabs = self._rope_repeat_cache = (cos, {})
        hit = tabs[1].get(key)
        if hit is None:
            if len(tabs[1]) > 64:
                tabs[1].clear()
            d = self.dim // self.num_heads
            nf = (d - 4 * (d // 6)) // 2                                     # pair-columns of the frame axis
            c2, s2 = cos.clone(), sin.clone()
            c2[frames:2 * frames, :nf] = cos[:frames, :nf]
            s2[frames:2 * frames, :nf] = sin[:frames, :nf]
            hit = tabs[1][key] = (c2, s2)
        return hit

    def forward_teacher_forcing(self, x_clean, x_noisy, t, context, context_t=0.0, clip_fea=None, y=None,
                                extra_conditions=None, pin_sink=False):
        """All chunks of a clip in one pass, as the rollout sees them (teacher forcing).  Needs ``set_causal_chunks(fpc,
        W)``.  ``x_clean`` / ``x_noisy``: lists of [C_in, F, H, W], every clip of one shape, F a multiple of fpc;
        ``t``: [B, F / fpc], one timestep per noisy chunk.  The sequence of a sample is [clean tokens | noisy tokens]
        (2 S tokens): the clean frames are modulated at ``context_t`` and the frames of noisy chunk I at ``t[:, I]``
        (per-frame timesteps), q and k of both halves rotate with the SAME frame positions, and every self-attention
        runs under ``causal.IntervalMask(causal.teacher_forcing_groups(F / fpc, W), fpc h w)``: a clean chunk sees the
        clean chunks up to itself, noisy chunk I the clean chunks before it and itself — what ``forward_chunk`` attends
        to at chunk I (both cut to W chunks back; with ``sink_chunks`` = S > 0 the first S clean chunks stay visible:
        ``teacher_forcing_groups(F / fpc, W, S)`` and the three-run kernels).  Cross-attention and the FFN are unchanged
        (frame-aligned ``extra_conditions``: clean frame f and noisy frame f see the same tokens),
        ``y`` goes to both halves, the head runs on the noisy rows only.  Returns the list of fp32 [C_out, F, H, W] for the
        noisy half.
        ``pin_sink=True`` (needs S >= 1 and W >= 0): the rollout is the one on ``causal.RollingKVCache(pin_sink=True)`` — the
        queries of chunk I > S + W, clean and noisy, score the clean sink chunks with the sink keys rotated by
        Delta_I = (I - W - S) fpc more frames, where the pinned cache holds them when chunk I runs.  Every such chunk gets
        its own rotated image of the sink keys behind the 2 S tokens of the key axis (``causal.sink_copy_deltas``,
        ``ops.rope_shift_fan``: the bits the cache holds), the mask is ``teacher_forcing_groups(.., pin_sink=True)``, and the
        backward folds the images' dK / dV into the sink rows (``ops.rope_shift_fold``); K and V of a layer grow by
        (n - S - W - 1) S chunks.  A clip that does not outlast the ring (n <= S + W + 1) runs the call without it, bit for bit.
        ValueError without causal chunks, for a bounded ``window_size``, a block mask or policy, clips of different
        shapes, F no multiple of fpc, h w no multiple of 8, a ``t`` of another shape and ``pin_sink`` without a sink."""
        cc = getattr(self, "_causal_chunks", None)
        if cc is None:
            raise ValueError("forward_teacher_forcing: set_causal_chunks(frames_per_chunk, left_chunks) first")
        self._causal_check("forward_teacher_forcing")
        if pin_sink and (self._causal_sink() < 1 or cc[1] < 0):
            raise ValueError("forward_teacher_forcing: pin_sink=True needs set_causal_chunks(fpc, W, S) with sink_chunks >= 1 "
                             "and left_chunks >= 0 (there is no sink to pin)")
        x_clean, x_noisy = list(x_clean), list(x_noisy)
        shapes = {tuple(u.shape) for u in x_clean} | {tuple(u.shape) for u in x_noisy}
        if len(x_clean) != len(x_noisy) or len(shapes) != 1:
            raise ValueError("forward_teacher_forcing: clean and noisy latents of ONE shape per clip are expected")
        pt, ph, pw = self.patch_size
        F, h, w = x_noisy[0].shape[1] // pt, x_noisy[0].shape[2] // ph, x_noisy[0].shape[3] // pw
        fpc, B = cc[0], len(x_noisy)
        if F % fpc:
            raise ValueError(f"forward_teacher_forcing: {F} latent frames are no multiple of frames_per_chunk = {fpc}")
        if not isinstance(t, torch.Tensor) or t.shape != (B, F // fpc):
            raise ValueError(f"forward_teacher_forcing: t of shape [{B}, {F // fpc}] expected (one timestep per noisy chunk)")
        if (h * w) % 8:
            raise ValueError(f"forward_teacher_forcing: {h * w} tokens per frame; a multiple of 8 is needed")
        if 2 * F > self.freqs.shape[0]:
            raise ValueError(f"forward_teacher_forcing: 2 x {F} frames leave the rotary table ({self.freqs.shape[0]} rows)")
        device = self.patch_embedding.weight.device
        if device.type != "cuda":
            raise ops.OmhError("WanModel.forward_teacher_forcing runs on the MI355X only (no CPU fallback): move the "
                               "model to a GPU device")
        from ... import causal as _causal
        sink = self._causal_sink()
        # pin_sink: the chunks past the ring, each with the shift its sink keys carry at rollout (none: today's call)
        copies = _causal.sink_copy_deltas(F // fpc, cc[1], sink, fpc) if pin_sink else ()
        key = (F // fpc, cc[1], fpc * h * w, str(device)) + ((sink,) if sink else ())
        masks = self.__dict__.setdefault("_tf_masks", {})
        if key not in masks and not copies:
            if len(masks) > 64:
                masks.clear()
            if sink:                                       # clean sink | clean window | own chunk: three runs
                masks[key] = _causal.IntervalMask(_causal.teacher_forcing_groups(F // fpc, cc[1], sink), fpc * h * w, device,
                                                  runs=3)
            else:
                masks[key] = _causal.IntervalMask(_causal.teacher_forcing_groups(F // fpc, cc[1]), fpc * h * w, device)
        x = [torch.cat([c.to(n.device), n], dim=1) for c, n in zip(x_clean, x_noisy)]
        if y is not None:
            y = [torch.cat([v, v], dim=1) for v in y]
        t = t.to(device)
        if not t.is_floating_point():
            t = t.float()
        t_frames = torch.cat([torch.full((B, F), float(context_t), dtype=t.dtype, device=device),
                              t.repeat_interleave(fpc, dim=1)], dim=1)
        fan = None
        if copies:
            # the extended key axis [clean | noisy | sink @ Delta_{S+W+1} | ...]: its mask and the copies' (cos, sin) tables
            n, Ct = F // fpc, fpc * h * w
            key = ("pin", n, cc[1], sink, fpc, Ct, str(device))
            if key not in masks:
                if len(masks) > 64:
                    masks.clear()
                masks[key] = (_causal.IntervalMask(_causal.teacher_forcing_groups(n, cc[1], sink, pin_sink=True), Ct, device,
                                                   runs=3),
                              ops.rope_shift_table([delta for _, delta in copies], self.dim // self.num_heads, device=device))
            mask, table = masks[key]
            fan = (table, len(copies), sink * Ct)
        else:
            mask = masks[key]
        self._tf_state = (mask, self._rope_repeated(device, F), fan)
        try:
            out = self.forward(x, t_frames, context, 2 * F * h * w, clip_fea, y, extra_conditions)
        finally:
            self._tf_state = None
        # (the inference blocks ran the head on the noisy rows only; the training forward runs it on every row, and the
        # clean half's output is cut off here: no gradient enters through it)
        return [o if o.shape[1] == F * pt else o[:, F * pt:] for o in out]

    def forward_chunk(self, x, t, context, cache, frame_offset=None, commit=True, clip_fea=None, y=None, grad=False,
                      extra_conditions=None):
        """One chunk of a clip against the keys and values kept from the chunks before it (the rollout of the
        frame-causal model).  ``x``: the latents [C_in, f, H, W] of ONE chunk per sample, all of one shape (the last chunk
        of a clip may have fewer frames); ``cache``: a ``causal.KVCache`` of this model and batch.  Each block projects
        q, k, v for the chunk's rows only, rotates q and k with the frame axis starting at ``frame_offset`` (default:
        ``cache.length`` / tokens per frame), writes k and V^T at rows / columns [length, length + C) of its cache and
        attends over the keys [lo, length + C): lo = 0, or the first token of the look-back when ``set_causal_chunks``
        set ``left_chunks`` >= 0 (then ``cache.length`` must sit on a chunk boundary and the chunk may not exceed
        ``frames_per_chunk``).  With a ``causal.RollingKVCache`` (its geometry must equal the model's (fpc h w, W, S):
        ValueError otherwise) k and V^T go to the chunk's slot and attention runs over every filled slot — the sink, the
        window and the chunk itself, one contiguous key range; a plain ``KVCache`` under ``sink_chunks`` > 0 is a
        ValueError.  A ``RollingKVCache(pin_sink=True)`` first brings its sink keys to the rotary distance this chunk needs
        (``RollingKVCache.pin``: at most one ``ops.rope_shift_frames`` launch per layer when the shift changes; denoising and
        commit passes alike).  ``frame_offset`` may be any value >= 0: past the model's rotary table (1 024 frames) the
        frame angles are computed in fp64 by the table's formula.  ``commit=True`` advances ``cache.length`` by C once, after the last block;
        ``commit=False`` leaves the cache as it was (the rows behind ``length`` are scratch) — a denoising step of the
        current chunk.  Cross-attention, FFN and head as in ``forward``.  Tokens per chunk must be a multiple of 8 (the
        16-byte stores into the cache and the look-back offset): ValueError otherwise, and when the chunk does not fit.
        Inference only by default: RuntimeError with grad enabled and parameters or inputs that require it.

        ``grad=True`` (self forcing: ``causal.self_forcing_rollout``): with grad enabled and a trainable parameter or an
        input that requires grad the call is an autograd node chain like ``forward``'s (model_train.forward_chunk_train) —
        the same launches, the bits of the inference call on the same cache state.  The gradient reaches every parameter
        ``forward`` trains and x, t, context, y, clip_fea; the chunk's keys and values get theirs through its own rows
        only — the cached rows [lo, length) are constants.  The chunk's own k and V are kept with the activations (the
        next call overwrites them in the cache); the cached rows are read in place by the backward, which raises
        RuntimeError when the cache was ``reset()`` or ``truncate()``d below them in between.  Activations are always
        kept (a re-run would need the cache as it was): ``use_checkpoint`` is ignored and ``checkpoint_policy="always"``
        is a ValueError, as are a ``RollingKVCache`` (its slots are evicted before the backward runs: use ``KVCache``
        with ``left_chunks``; with ``pin_sink`` its sink rows are re-rotated as well), hence ``sink_chunks`` > 0, and a
        2-D ``t``.  Without anything that requires grad it is the
        inference call.

        ``extra_conditions``: as in ``forward``.  With ``"frames"`` the frames are clip-absolute, the chunk's queries are
        the frames from ``frame_offset`` on and nothing behind the chunk's last frame is seen; the tokens no query of the
        chunk sees are dropped before the embedding, so passing a stream's later tokens or leaving them out is the same
        computation.  With ``grad=True`` the gradient reaches the tokens.
        Returns the list of fp32 [C_out, f, H, W]."""
        if isinstance(extra_conditions, dict) and extra_conditions.get("frames") is not None:
            x = list(x)
            f = x[0].shape[1] // self.patch_size[0]
            fo = self._chunk_geometry(x, t, cache, frame_offset)[2]       # (its ValueErrors; nothing touches a device)
            extra_conditions = self._normal_conditions(extra_conditions, chunk=(fo, f))
        if grad:
            # (the refusals come before anything touches a device)
            if getattr(cache, "pin_sink", False):
                raise ValueError("forward_chunk(grad=True): a cache with pin_sink=True re-rotates its sink rows for later "
                                 "chunks, and the backward reads cached rows in place; self forcing under a pinned sink is "
                                 "what is still missing (teacher forcing trains under it: "
                                 "forward_teacher_forcing(pin_sink=True))")
            if getattr(cache, "rolling", False):
                raise ValueError("forward_chunk(grad=True): a RollingKVCache evicts slots the backward still reads; use a "
                                 "causal.KVCache with set_causal_chunks(frames_per_chunk, left_chunks)")
            if self._causal_sink():
                raise ValueError("forward_chunk(grad=True): sink_chunks > 0 needs a RollingKVCache, which has no gradient "
                                 "path; use set_causal_chunks(frames_per_chunk, left_chunks) and a causal.KVCache")
            if isinstance(t, torch.Tensor) and t.dim() != 1:
                raise ValueError(f"forward_chunk: t of shape {tuple(t.shape)}; one timestep per sample, [B], is expected")
            from .model_train import check_chunk_grad_policy
            check_chunk_grad_policy(self)                  # checkpoint_policy="always": ValueError
        device = self.patch_embedding.weight.device
        if device.type != "cuda":
            raise ops.OmhError("WanModel.forward_chunk runs on the MI355X only (no CPU fallback): move the model "
                               "to a GPU device")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                        or self._input_requires_grad(x, t, context, clip_fea, y, extra_conditions)):
            if not grad:
                raise RuntimeError("forward_chunk is an inference path (no gradient flows through the cache): call it "
                                   "under torch.no_grad() with inputs that do not require grad")
            if isinstance(context, ContextState):
                raise ValueError("a ContextState is an inference-time cache: pass the raw context when training")
            from .model_train import forward_chunk_train
            return forward_chunk_train(self, list(x), t, context, cache, frame_offset, commit, clip_fea, y, extra_conditions)
        with torch.no_grad():
            return self._forward_chunk(list(x), t, context, cache, frame_offset, commit, clip_fea, y, extra_conditions)

    def _chunk_geometry(self, x, t, cache, frame_offset):
        """The argument rules of ``forward_chunk`` -> (C tokens of the chunk, first visible key lo, frame_offset)."""
        if t.dim() != 1:
            raise ValueError(f"forward_chunk: t of shape {tuple(t.shape)}; one timestep per sample, [B], is expected")
        if len({tuple(u.shape) for u in x}) != 1:
            raise ValueError("forward_chunk: the chunks of a batch must have one shape")
        if cache.model_id != id(self) or cache.batch != len(x):
            raise ValueError("forward_chunk: the KVCache belongs to another model or batch size")
        pt, ph, pw = self.patch_size
        f, h, w = x[0].shape[1] // pt, x[0].shape[2] // ph, x[0].shape[3] // pw
        tpf, L0 = h * w, cache.length
        C = f * tpf
        if C == 0 or C % 8:
            raise ValueError(f"forward_chunk: {C} tokens per chunk; a positive multiple of 8 is needed (16-byte stores "
                             "into the cache)")
        if L0 % 8:
            raise ValueError(f"forward_chunk: cache.length = {L0} is no multiple of 8")
        cache.check_room(C)                                # ValueError past max_tokens
        lo = 0
        cc = getattr(self, "_causal_chunks", None)
        rolling = getattr(cache, "rolling", False)
        if rolling:
            if cc is None or cc[1] < 0 or (cache.chunk_tokens, cache.left_chunks, cache.sink_chunks) != \
                    (cc[0] * tpf, cc[1], self._causal_sink()):
                raise ValueError(f"forward_chunk: a RollingKVCache of (chunk_tokens, left_chunks, sink_chunks) = "
                                 f"({cache.chunk_tokens}, {cache.left_chunks}, {cache.sink_chunks}) on a model set to "
                                 f"{None if cc is None else (cc[0] * tpf, cc[1], self._causal_sink())}")
        elif self._causal_sink():
            raise ValueError("forward_chunk: set_causal_chunks has sink_chunks > 0 — a plain KVCache never evicts and cannot "
                             "keep a sink; use causal.RollingKVCache")
        if cc is not None:
            Ct = cc[0] * tpf
            if f > cc[0] or L0 % Ct:
                raise ValueError(f"forward_chunk: a chunk of {f} frames at {L0} cached tokens does not fit chunks of "
                                 f"{cc[0]} frames ({Ct} tokens)")
            if cc[1] >= 0 and not rolling:
                lo = max(0, L0 // Ct - cc[1]) * Ct
        if frame_offset is None:
            if L0 % tpf:
                raise ValueError(f"forward_chunk: cache.length = {L0} is no multiple of {tpf} tokens per frame; pass frame_offset")
            frame_offset = L0 // tpf
        frame_offset = int(frame_offset)
        if frame_offset < 0 or f > self.freqs.shape[0]:
            raise ValueError(f"forward_chunk: frame_offset = {frame_offset} >= 0 and at most {self.freqs.shape[0]} frames per "
                             f"chunk expected (frames past the rotary table get their angles computed: _rope_shifted)")
        return C, lo, frame_offset

    def _chunk_ctx(self, fc, cache, lo, frame_offset, frames):
        """An embedded context as that of one chunk of ``frames`` frames against ``cache`` from key ``lo`` on, at
        ``frame_offset``."""
        fc.chunk = fc.interval = None                      # the cache IS the causal structure: plain attention over it
        fc.rope_cos, fc.rope_sin = self._rope_shifted(fc.e0.device, frame_offset, frames)
        fc.cache, fc.cache_lo = cache, lo
        fc.cache_pos = fc.cache_hi = fc.cache_mask = None

    def _forward_chunk(self, x, t, context, cache, frame_offset, commit, clip_fea, y, extra_conditions=None):
        C, lo, frame_offset = self._chunk_geometry(x, t, cache, frame_offset)
        L0 = cache.length
        rolling = getattr(cache, "rolling", False)
        if rolling:
            tpf = (x[0].shape[2] // self.patch_size[1]) * (x[0].shape[3] // self.patch_size[2])
            Ct = self._causal_chunks[0] * tpf
        xs, e, fc, grids, lens, ctx_lens = self._embed(x, t, context, C, clip_fea, y, extra_conditions,
                                                       chunk=(frame_offset, C // self._tokens_per_frame(x)))
        self._chunk_ctx(fc, cache, lo, frame_offset, C // self._tokens_per_frame(x))
        if rolling:
            cache.pin(self._causal_chunks[0], self.dim // self.num_heads)   # (a pinned sink: its rows where this chunk needs them)
            # the chunk's slot; the keys are every filled slot.  Before the ring wraps they are [0, L0 + C), KVCache's range;
            # afterwards all slots — one contiguous range, whatever chunk sits where
            fc.cache_pos = cache.slot(L0 // Ct) * Ct
            wrapped = L0 // Ct >= cache.slots
            fc.cache_hi = cache.cap if wrapped else fc.cache_pos + C
            if wrapped and C < Ct and fc.cache_pos + Ct < cache.cap:
                fc.cache_mask = self._stale_mask(cache, fc.cache_pos, C, tpf, xs.device)
            elif wrapped and C < Ct:                       # the last slot: the stale keys are the end of the range
                fc.cache_hi = fc.cache_pos + C
        seq_lens = _dev_ints(lens, torch.long, xs.device)
        grid_sizes = _dev_ints(grids, torch.long, xs.device)
        context_lens = _dev_ints(ctx_lens, torch.long, xs.device)
        freqs = (fc.rope_cos, fc.rope_sin)
        for i, block in enumerate(self.blocks):
            fc.cache_layer = i
            xs = block(xs, fc.e0, seq_lens, grid_sizes, freqs, fc.ctx, context_lens, block_idx=i, _fc=fc)
        out = self.head(xs, e)
        if commit:
            cache.advance(C)
        return self.unpatchify(out, grid_sizes, _grids=grids)

    # ------------------------------------------------------------------ forward
    def _rope(self, device):
        if self._rope_dev is None or self._rope_dev[0] != str(device):
            self._rope_dev = (str(device),) + _rope_tables(self.freqs, device)
        return self._rope_dev[1], self._rope_dev[2]

    def forward(self, x, t, context, seq_len, clip_fea=None, y=None, extra_conditions=None):
        r"""Same contract as the reference (model.py:502-563):
        x: list (or batched tensor) of [C_in, F, H, W]; t: [B]; context: list of [L, text_dim];
        returns list of fp32 [C_out, F, H, W].

        ``extra_conditions`` is the keyword Omnihuman/omnihuman_wan_t2v.py:408-414 passes (the reference model does
        not accept it): a ``[B, Ne, dim]`` tensor of condition tokens in model width, or a dict holding it under
        ``"tokens"``.  They are prepended to the embedded text context (t2v, inference), so every block's
        cross-attention attends to them — see omnihuman_wan_t2v.OmniHumanWanT2V.condition_tokens.

        Frame-aligned condition tokens: the dict may hold ``"frames"``, an int tensor [Ne] shared by the batch — the latent
        frame of token j on the model's frame grid, or -1 for a token every query sees — and then must hold ``"window"`` =
        (back, ahead) in latent frames, a side < 0 unbounded.  The queries of latent frame f see the text, the -1 tokens
        and the tokens of frames f - back .. min(f + ahead, E), E the last frame of f's chunk under
        ``set_causal_chunks`` (no E otherwise): ``causal.condition_window_visible`` states the rule, every block's
        cross-attention runs under it as a ``causal.IntervalMask(k_group=1)`` over (latent frames, context rows), built once
        per call.  The model orders the tokens itself (stable: frame tokens ascending, then the -1 tokens, then the text),
        and their gradient comes back in the caller's order.  Every clip of the batch must have the same h, w, with
        h w >= 8.  ValueError (before any device call) for ``"frames"`` of another length or dtype, a missing
        ``"window"`` and an i2v model.  Without ``"frames"`` nothing changes."""
        extra_conditions = self._normal_conditions(extra_conditions)
        device = self.patch_embedding.weight.device
        if device.type != "cuda":
            raise ops.OmhError("WanModel.forward runs on the MI355X only (no CPU fallback): move the model "
                               "to a GPU device")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                        or self._input_requires_grad(x, t, context, clip_fea, y, extra_conditions)):
            # a frozen model whose INPUT requires grad (a critic backbone, guidance by a gradient, a rollout) takes the
            # training forward too: the reference's autograd differentiates through x, y, context, clip_fea and t
            if isinstance(context, ContextState):
                raise ValueError("a ContextState is an inference-time cache: pass the raw context when training")
            from .model_train import forward_train
            return forward_train(self, x, t, context, seq_len, clip_fea, y, extra_conditions)
        with torch.no_grad():
            return self._forward_infer(x, t, context, seq_len, clip_fea, y, extra_conditions)

    @staticmethod
    def _input_requires_grad(x, t, context, clip_fea, y, extra_conditions):
        """Does any tensor input ask for a gradient: the elements of x, y and context, clip_fea, a floating t, the
        condition tokens."""
        def any_of(v):
            if v is None or isinstance(v, ContextState):
                return False
            if isinstance(v, torch.Tensor):
                return v.requires_grad
            if isinstance(v, dict):
                return any_of(v.get("tokens"))
            return any(isinstance(u, torch.Tensor) and u.requires_grad for u in v)
        return any(any_of(v) for v in (x, y, context, clip_fea, t, extra_conditions))

    def _tokens_per_frame(self, x):
        return (x[0].shape[2] // self.patch_size[1]) * (x[0].shape[3] // self.patch_size[2])

    def _normal_conditions(self, extra_conditions, chunk=None):
        """``extra_conditions`` with ``"frames"`` in its normal form: the tokens in the model's order — frame tokens
        ascending, then the -1 tokens (a stable sort; ``index_select``, so autograd hands the gradient back in the
        caller's order) —, ``"frames"`` as a tuple of host ints in that order and ``"window"`` = (back, ahead).  ``chunk`` =
        (frame_offset, frames) of a ``forward_chunk`` call: the tokens no query of the chunk sees are dropped (None when
        none is left).  Anything without ``"frames"`` is returned as it is.  Checks only: no device is touched but by the
        ``index_select``."""
        ec = extra_conditions
        if not isinstance(ec, dict) or ec.get("frames") is None or ec.get("_normal"):
            return ec
        if self.model_type != "t2v":
            raise ValueError("frame-aligned condition tokens ('frames') are defined for the t2v backbone")
        tok, frames, window = ec.get("tokens"), ec["frames"], ec.get("window")
        if not isinstance(tok, torch.Tensor) or tok.dim() != 3:
            raise ValueError("extra_conditions: 'tokens' [B, Ne, dim] expected beside 'frames'")
        if not isinstance(frames, torch.Tensor) or frames.is_floating_point() or frames.is_complex() or \
                frames.dtype == torch.bool or tuple(frames.shape) != (tok.shape[1],):
            raise ValueError(f"extra_conditions: 'frames' must be an int tensor [Ne = {tok.shape[1]}], got "
                             f"{getattr(frames, 'dtype', type(frames))} {tuple(getattr(frames, 'shape', ()))}")
        if window is None or len(window) != 2:
            raise ValueError("extra_conditions: 'window' = (back, ahead) is required beside 'frames'")
        back, ahead = int(window[0]), int(window[1])
        fr = [int(v) for v in frames.tolist()]
        if any(v < -1 for v in fr):
            raise ValueError("extra_conditions: 'frames' holds latent frames >= 0, or -1 for a token every query sees")
        order = sorted(range(len(fr)), key=lambda j: (fr[j] < 0, fr[j]))
        if chunk is not None:
            from ... import causal as _causal
            fo, f = chunk
            # (one chunk from frame 0 to the chunk's last frame: E = fo + f - 1 for every query)
            seen = _causal.condition_window_visible(f, torch.tensor([fr[j] for j in order], dtype=torch.int64), 0, back, ahead,
                                                    frames_per_chunk=fo + f, frame_offset=fo).any(0).tolist()
            order = [j for j, on in zip(order, seen) if on]
            if not order:
                return None
        if order != list(range(len(fr))):
            tok = tok.index_select(1, _dev_ints(order, torch.long, tok.device))
        return {"tokens": tok, "frames": tuple(fr[j] for j in order), "window": (back, ahead), "chunk": chunk, "_normal": True}

    def _condition_mask(self, fc, cond):
        """The resolved mask of every cross-attention of a forward whose context starts with frame-aligned condition tokens
        (``cond``: the normal form of ``_normal_conditions``, tokens aside), or None when every query sees every token.
        Rows: the latent frames of the sequence (both halves under teacher forcing; the chunk's frames in
        ``forward_chunk``), columns: the rows of the context, one by one."""
        from ... import causal as _causal
        frames, (back, ahead), chunk = cond["frames"], cond["window"], cond.get("chunk")
        hw = {(g[1], g[2]) for g in fc.grids}
        if len(hw) != 1:
            raise ValueError(f"frame-aligned condition tokens: the clips of a batch must share h, w, got {sorted(hw)}")
        tpf = hw.pop()
        tpf = tpf[0] * tpf[1]
        if tpf < 8:
            raise ValueError(f"frame-aligned condition tokens: {tpf} tokens per frame; at least 8 are needed")
        n_text = fc.Lc - len(frames)
        cc = getattr(self, "_causal_chunks", None)
        if chunk is not None:                              # one chunk from frame 0 to the chunk's last frame (see above)
            q_frames, offset, fpc, segments = chunk[1], chunk[0], chunk[0] + chunk[1], 1
        elif getattr(self, "_tf_state", None) is not None:
            q_frames, offset, fpc, segments = fc.S // (2 * tpf), 0, cc[0], 2
        else:
            q_frames, offset, fpc, segments = (fc.S + tpf - 1) // tpf, 0, None if cc is None else cc[0], 1
        device = fc.ctx.device
        key = (frames, back, ahead, n_text, q_frames, offset, fpc, segments, tpf, fc.S, str(device))
        masks = self.__dict__.setdefault("_cond_masks", {})
        if key not in masks:
            if len(masks) > 64:
                masks.clear()
            vis = _causal.condition_window_visible(q_frames, torch.tensor(frames, dtype=torch.int64), n_text, back, ahead,
                                                   fpc, segments, offset)
            masks[key] = None if bool(vis.all()) else ops.attn_mask(
                interval_mask=_causal.IntervalMask(vis, tpf, device, k_group=1), H=self.num_heads, Lq=fc.S, Lk=fc.Lc,
                device=device)
        return masks[key]

    def _embed(self, x, t, context, seq_len, clip_fea, y, extra_conditions=None, chunk=None):
        device = self.patch_embedding.weight.device
        d = self.dim
        if y is not None:
            x = [torch.cat([u, v], dim=0) for u, v in zip(x, y)]
        x = [u.to(device=device, dtype=torch.float32).contiguous() for u in x]
        B = len(x)
        pt, ph, pw = self.patch_size
        grids = [(u.shape[1] // pt, u.shape[2] // ph, u.shape[3] // pw) for u in x]
        lens = [g[0] * g[1] * g[2] for g in grids]
        assert max(lens) <= seq_len, f"Max seq len {max(lens)} exceeds limit {seq_len}"
        # ---- patch embedding (Conv3d k=s=patch as a GEMM); padded rows stay zero  model.py:515-522
        kin = self.in_dim * pt * ph * pw
        Kp = _round_up(kin, 8)
        wpe, bpe = self._packed.get("patch", (self.patch_embedding.weight, self.patch_embedding.bias), lambda: (
            _bf16(torch.nn.functional.pad(self.patch_embedding.weight.detach().flatten(1).float(), (0, Kp - kin))),
            self.patch_embedding.bias.detach().float().contiguous()))
        xs = torch.empty(B, seq_len, d, dtype=torch.float32, device=device)
        for b, u in enumerate(x):
            assert u.shape[0] == self.in_dim, f"expected {self.in_dim} input channels, got {u.shape[0]}"
            tok = ops.patchify(u, self.patch_size, Kp)
            ops.gemm_raw(ptr(tok), ptr(wpe), ptr(xs, b * seq_len * d), lens[b], d, Kp, Kp, Kp, d, EPI_F32,
                         bias=ptr(bpe), bias_mode=BIAS_N)
            if lens[b] < seq_len:
                xs[b, lens[b]:].zero_()                 # only the padding rows need the fill; the GEMM wrote the rest
        # ---- time embedding (fp32)                                              model.py:526-528
        t = t.to(device=device)
        rpb = seq_len
        if t.dim() == 2:                                                    # per-frame timesteps: one row of e0 per frame
            t, rpb = self._per_frame_t(t, grids, seq_len)
        te0, te2, tp1 = self.time_embedding[0], self.time_embedding[2], self.time_projection[1]
        sin = ops.sinusoidal_embedding(t, self.freq_dim)
        e = ops.dense_f32(ops.dense_f32(sin, te0.weight.detach().float(), te0.bias.detach().float(), 0, 1),
                          te2.weight.detach().float(), te2.bias.detach().float(), 0, 0)
        e0 = ops.dense_f32(e, tp1.weight.detach().float(), tp1.bias.detach().float(), 1, 0).view(-1, 6, d)
        fc = _FwdCtx()
        fc.B, fc.S, fc.dim = B, seq_len, d
        fc.rpb = rpb
        fc.split_k = not getattr(self, "batch_invariant", False)
        fc.e0 = e0.contiguous()
        fc.seq_lens32 = _dev_ints(lens, torch.int32, device)
        fc.grid32 = _dev_ints(grids, torch.int32, device)
        fc.rope_cos, fc.rope_sin = self._rope(device)
        fc.seq_lens_host = list(lens)                                       # host copies: no device sync later
        fc.grids = list(grids)
        fc.chunk = self._causal_rule(grids)
        if fc.chunk is not None and self._causal_sink():                    # a sink: the interval kernels, not the staircase
            fc.chunk, fc.interval = None, self._sink_mask(seq_len, fc.chunk[0], device)
        tf = getattr(self, "_tf_state", None)                               # forward_teacher_forcing: its mask and rotary table
        if tf is not None:
            fc.chunk, fc.interval = None, tf[0]
            fc.rope_cos, fc.rope_sin = tf[1]
            fc.sink_fan = tf[2]                                             # (pin_sink=True past the ring; else None)
        ctx_lens = self._attach_context(fc, context, clip_fea, extra_conditions, chunk)
        return xs, e, fc, grids, lens, ctx_lens

    def _per_frame_t(self, t, grids, seq_len):
        """``t`` [B, F] (F: the latent frames of the longest clip) -> (the timesteps of the B * G frames of the padded
        sequences, flat; h * w), G = seq_len / (h w); frames past F take the last frame's t.  Plain torch: a gradient
        w.r.t. ``t`` flows back to [B, F].  ValueError when the clips do not share h, w, when seq_len is no multiple of
        h w, when h w is no multiple of 8, and when F is not the frame count of the longest clip."""
        hw = {(g[1], g[2]) for g in grids}
        if len(hw) != 1:
            raise ValueError(f"per-frame t: the clips of a batch must share h, w, got {sorted(hw)}")
        h, w = next(iter(hw))
        tpf = h * w
        if tpf % 8:
            raise ValueError(f"per-frame t: {tpf} tokens per frame; a multiple of 8 is needed")
        if seq_len % tpf:
            raise ValueError(f"per-frame t: seq_len = {seq_len} is no multiple of the {tpf} tokens of a frame")
        G, F = seq_len // tpf, max(g[0] for g in grids)
        if t.shape != (len(grids), F):
            raise ValueError(f"per-frame t: shape {tuple(t.shape)}, [{len(grids)}, {F}] expected (one timestep per latent "
                             "frame of the longest clip)")
        if G > F:
            t = torch.cat([t, t[:, -1:].expand(-1, G - F)], dim=1)
        return t.reshape(-1), tpf

    def _attach_context(self, fc, context, clip_fea=None, extra_conditions=None, chunk=None):
        """The context-dependent fields of a forward's shared state: text (+ image) embedding, model.py:531-537.
        ``chunk``: (frame_offset, frames) of a ``forward_chunk`` call, for the mask of frame-aligned condition tokens."""
        device = self.patch_embedding.weight.device
        state = context if isinstance(context, ContextState) else None
        if state is not None:
            if state.model_id != id(self) or state.version != self._context_signature() or state.B != fc.B:
                raise ValueError("ContextState does not belong to this model / batch or the weights changed since "
                                 "encode_context(): call encode_context() again")
            ctx, ctx_lens = state.ctx, list(state.ctx_lens)
            if extra_conditions is not None:
                raise ValueError("pass extra condition tokens to encode_context(), not next to a ContextState")
            cond = state.cond
        else:
            extra_conditions = self._normal_conditions(extra_conditions)
            ctx, ctx_lens = self._embed_context(context, clip_fea, extra_conditions)
            cond = extra_conditions if isinstance(extra_conditions, dict) and extra_conditions.get("_normal") else None
        fc.ctx_lens32 = _dev_ints(ctx_lens, torch.int32, device)
        fc.ctx, fc.Lc = ctx, ctx.shape[1]
        fc.kv = state.kv if state is not None else None
        fc.ctx_lens_host = list(ctx_lens)
        fc.ctx_mask = None
        if cond is not None:
            fc.ctx_mask = self._condition_mask(fc, cond if chunk is None else dict(cond, chunk=chunk))
        return ctx_lens

    def _embed_context(self, context, clip_fea=None, extra_tokens=None):
        """text_embedding (and img_emb) of zero-padded contexts: bf16 [B, (257+ | Ne+)text_len, dim] and true lengths."""
        device = self.patch_embedding.weight.device
        d, B = self.dim, len(context)
        ctx_lens = [int(u.shape[0]) for u in context]
        ctx_in = torch.zeros(B, self.text_len, self.text_dim, dtype=torch.float32, device=device)
        for b, u in enumerate(context):
            ctx_in[b, :u.shape[0]] = u.to(device=device, dtype=torch.float32)
        w0, b0 = self._packed.get("text0", (self.text_embedding[0].weight, self.text_embedding[0].bias), lambda: (
            _bf16(self.text_embedding[0].weight), self.text_embedding[0].bias.detach().float().contiguous()))
        w2, b2 = self._packed.get("text2", (self.text_embedding[2].weight, self.text_embedding[2].bias), lambda: (
            _bf16(self.text_embedding[2].weight), self.text_embedding[2].bias.detach().float().contiguous()))
        cin = ops.cast_bf16(ctx_in).view(B * self.text_len, self.text_dim)
        ctx = ops.gemm(ops.gemm(cin, w0, bias=b0, epilogue=EPI_GELU_BF16), w2, bias=b2, epilogue=EPI_BF16)
        ctx = ctx.view(B, self.text_len, d)
        if clip_fea is not None:
            ctx_img = self.img_emb(clip_fea.to(device))                    # bf16 [B, 257, dim]
            ctx = torch.cat([ctx_img, ctx], dim=1).contiguous()
            ctx_lens = [c + ctx_img.shape[1] for c in ctx_lens]
        if extra_tokens is not None:
            tok = extra_tokens.get("tokens") if isinstance(extra_tokens, dict) else extra_tokens
            if tok is not None:
                if self.model_type != "t2v":
                    raise NotImplementedError("extra condition tokens are defined for the t2v backbone")
                if tok.dim() != 3 or tok.shape[0] != B or tok.shape[2] != d:
                    raise ValueError(f"extra condition tokens must be [B={B}, Ne, dim={d}], got {tuple(tok.shape)}")
                tokb = ops.cast_bf16(tok.to(device=device, dtype=torch.float32).contiguous())
                ctx = torch.cat([tokb, ctx], dim=1).contiguous()
                ctx_lens = [c + tok.shape[1] for c in ctx_lens]
        return ctx, ctx_lens

    def _context_signature(self):
        """Identity + version of every parameter a ContextState depends on."""
        mods = [self.text_embedding]
        if hasattr(self, "img_emb"):
            mods.append(self.img_emb)
        ps = [p for m in mods for p in m.parameters()]
        scales = ()
        for blk in self.blocks:
            ca = blk.cross_attn
            for name in ("k", "v", "norm_k", "k_img", "v_img", "norm_k_img"):
                m = getattr(ca, name, None)
                if isinstance(m, nn.Module):
                    ps.extend(m.parameters())            # (an adapter's lora_A / lora_B are parameters of the Linear)
                    if isinstance(m, nn.Linear) and lora_of(m) is not None:
                        scales += (lora_of(m)[2],)      # ... and its strength may be overridden without touching them
        return tuple((p.data_ptr(), p._version) for p in ps) + scales

    @torch.no_grad()
    def encode_context(self, context, clip_fea=None, extra_conditions=None) -> "ContextState":
        """Pre-compute what depends only on (context, clip_fea, extra_conditions).  Pass the result as ``context`` to
        forward() (inference only); every block adds its cross-attention K / V^T on first use and reuses them
        afterwards.  Frame-aligned ``extra_conditions`` (``"frames"``, ``"window"``: see ``forward``) stay with the state:
        every forward it is passed to masks its cross-attention accordingly, ``forward_cfg_pair`` included."""
        st = ContextState()
        extra_conditions = self._normal_conditions(extra_conditions)
        st.ctx, st.ctx_lens = self._embed_context(context, clip_fea, extra_conditions)
        st.cond = None
        if isinstance(extra_conditions, dict) and extra_conditions.get("_normal"):     # frames and window: the mask follows
            st.cond = {k: v for k, v in extra_conditions.items() if k != "tokens"}     # the geometry of each forward
        st.kv, st.B, st.model_id, st.version = {}, len(context), id(self), self._context_signature()
        return st

    def _forward_infer(self, x, t, context, seq_len, clip_fea=None, y=None, extra_conditions=None):
        xs, e, fc, grids, lens, ctx_lens = self._embed(x, t, context, seq_len, clip_fea, y, extra_conditions)
        seq_lens = _dev_ints(lens, torch.long, xs.device)
        grid_sizes = _dev_ints(grids, torch.long, xs.device)
        context_lens = _dev_ints(ctx_lens, torch.long, xs.device)
        freqs = (fc.rope_cos, fc.rope_sin)
        for i, block in enumerate(self.blocks):
            # module __call__ so forward hooks on blocks fire (seaweed_apt/model.py:150-155)
            xs = block(xs, fc.e0, seq_lens, grid_sizes, freqs, fc.ctx, context_lens, block_idx=i, _fc=fc)
        if getattr(self, "_tf_state", None) is not None:         # teacher forcing: the head runs on the noisy half only
            half = seq_len // 2
            xs = xs[:, half:].contiguous()
            e = e.view(len(grids), -1, e.shape[-1])[:, half // fc.rpb:].reshape(-1, e.shape[-1])
            grids = [(g[0] // 2, g[1], g[2]) for g in grids]
        out = self.head(xs, e, fc.rpb)                           # fp32 [B, seq_len, prod(patch)*out_dim]
        return self.unpatchify(out, grid_sizes, _grids=grids)

    def forward_cfg_pair(self, x, t, context, context_null, seq_len, clip_fea=None, y=None):
        """The two forwards of a classifier-free-guided step — ``forward(x, t, context, ...)`` and ``forward(x, t,
        context_null, ...)`` on the SAME latents and timestep (text2video.py:238-241, generate.py:205-229) — with what
        they share computed once: the patch / time embedding and block 0's self-attention sub-layer (LayerNorm + modulate,
        q | k | v, RoPE, self-attention, o-projection: its inputs are x and t alone; the context enters at block 0's
        cross-attention).  Everything after that point runs per branch, with the launches of a batch-of-one forward, so
        both results equal the two separate calls BIT FOR BIT (the kernels are deterministic); at S = 32 760 it is one
        self-attention launch of 60 less per step.  Inference only (a model whose parameters require grad must be called
        under torch.no_grad(): the training step has no such pair); contexts may be ContextStates.
        Returns (list of cond outputs, list of uncond outputs)."""
        device = self.patch_embedding.weight.device
        if device.type != "cuda":
            raise ops.OmhError("WanModel.forward_cfg_pair runs on the MI355X only (no CPU fallback): move the model "
                               "to a GPU device")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("forward_cfg_pair is an inference path: call it under torch.no_grad() or on a model "
                               "with requires_grad_(False) (training goes through forward())")
        with torch.no_grad():
            return self._forward_cfg_pair(x, t, context, context_null, seq_len, clip_fea, y)

    def _forward_cfg_pair(self, x, t, context, context_null, seq_len, clip_fea, y):
        if t.dim() != 1:
            raise ValueError(f"forward_cfg_pair: t of shape {tuple(t.shape)}; one timestep per sample, [B], is expected")
        xs, e, fc, grids, lens, ctx_lens = self._embed(x, t, context, seq_len, clip_fea, y)
        seq_lens = _dev_ints(lens, torch.long, xs.device)
        grid_sizes = _dev_ints(grids, torch.long, xs.device)
        freqs = (fc.rope_cos, fc.rope_sin)
        blk0 = self.blocks[0]
        # (no module __call__ here: a forward hook on block 0 fires once per branch, below, with the block's full output)
        xs = blk0.forward(xs, fc.e0, seq_lens, grid_sizes, freqs, fc.ctx, None, block_idx=0, _fc=fc, _part="self")
        fc_u = _FwdCtx()
        for name in _FwdCtx.__slots__:
            if hasattr(fc, name):
                setattr(fc_u, name, getattr(fc, name))
        self._attach_context(fc_u, context_null, clip_fea)
        outs = []
        for f, xb in ((fc, xs.clone()), (fc_u, xs)):
            context_lens = _dev_ints(f.ctx_lens_host, torch.long, xs.device)
            for i, block in enumerate(self.blocks):
                xb = block(xb, f.e0, seq_lens, grid_sizes, freqs, f.ctx, context_lens, block_idx=i, _fc=f,
                           _part="rest" if i == 0 else "all")
            outs.append(self.unpatchify(self.head(xb, e), grid_sizes, _grids=grids))
        return outs[0], outs[1]

    def unpatchify(self, x, grid_sizes, _grids=None):
        """model.py:565-588 — 'fhwpqrc->cfphqwr' per sample."""
        grids = _grids if _grids is not None else [tuple(int(a) for a in g) for g in grid_sizes.tolist()]
        return [ops.unpatchify(u.contiguous(), self.out_dim, g, self.patch_size) for u, g in zip(x, grids)]

    def init_weights(self):
        """model.py:590-612."""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        nn.init.xavier_uniform_(self.patch_embedding.weight.flatten(1))
        for m in self.text_embedding.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=.02)
        for m in self.time_embedding.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=.02)
        nn.init.zeros_(self.head.head.weight)
