"""Block masks for the block-sparse attention entries (include/omh.h, ``omh_block_mask``).

A mask is a bool array over 128 x 128 blocks of the (padded) score matrix, ``[nQb, nKb]`` shared by all heads or
``[H, nQb, nKb]`` one per head, always shared by the samples of a batch: query i sees key j iff the block
``(i // 128, j // 128)`` is kept, ``j < k_lens[b]`` and ``i < q_lens[b]``.  ``BlockMask`` turns it into the four int32
tables the kernels walk (per query block the ascending list of its key blocks, and the transposed lists for dK / dV);
``block_mask_from_3d_window`` builds the mask of a 3-D local window on a frame-major token lattice.  Building those masks
and tables is plain tensor arithmetic on the mask's device (CPU included); only the kernels need the GPU.

``block_mask_from_qk`` chooses the mask from the data instead: top-p selection over block-pooled q . k scores under a
``DynamicBlockPolicy``, built by three launches on the device (include/omh.h: omh_block_pool_d128, omh_block_select,
omh_block_mask_tables) with no host round trip.  The rule is stated in include/omh.h.
"""
import ctypes as C
import math

import torch

BLOCK = 128

__all__ = ["BLOCK", "BlockMask", "DynamicBlockPolicy", "block_mask_from_3d_window", "block_mask_from_qk"]


def _lists(mask: torch.Tensor):
    """mask [h, n, m] bool -> (cnt int32 [h, n], idx int32 [h, n, m]): the kept column indices of every row, ascending,
    in the first ``cnt`` entries (a stable sort of "dropped" puts them first, in their own order)."""
    cnt = mask.sum(-1).to(torch.int32).contiguous()
    idx = torch.argsort((~mask).to(torch.uint8), dim=-1, stable=True).to(torch.int32).contiguous()
    return cnt, idx


class BlockMask:
    """The tables of one block mask for a call with ``Lq`` queries and ``Lk`` keys.

    ``mask``: bool ``[nQb, nKb]`` or ``[heads, nQb, nKb]`` with nQb = ceil(Lq / 128), nKb = ceil(Lk / 128).  Attributes:
    ``heads`` (1 for a shared mask), ``q_blocks``, ``k_blocks``, ``row_cnt [heads, nQb]``, ``row_idx [heads, nQb, nKb]``,
    ``col_cnt [heads, nKb]``, ``col_idx [heads, nKb, nQb]`` (int32, on the mask's device; only the first ``cnt`` entries
    of a list mean anything) and ``density``, the share of kept blocks — computed on first read (for a mask on the
    device that read is a host synchronisation; nothing else here is).  ``BlockMask.from_tables`` wraps a mask and
    tables that already exist (the device-built masks of ``block_mask_from_qk``)."""

    def __init__(self, mask, Lq: int, Lk: int):
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
            raise ValueError("BlockMask: the mask must be a bool tensor")
        if mask.dim() not in (2, 3):
            raise ValueError(f"BlockMask: the mask must be [nQb, nKb] or [heads, nQb, nKb], got {tuple(mask.shape)}")
        Lq, Lk = int(Lq), int(Lk)
        nqb, nkb = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
        if Lq <= 0 or Lk <= 0 or tuple(mask.shape[-2:]) != (nqb, nkb):
            raise ValueError(f"BlockMask: Lq = {Lq}, Lk = {Lk} need a mask of [{nqb}, {nkb}] blocks, got "
                             f"{tuple(mask.shape[-2:])}")
        m3 = (mask if mask.dim() == 3 else mask[None]).contiguous()
        if m3.shape[0] < 1:
            raise ValueError("BlockMask: no heads")
        self.mask = m3
        self.Lq, self.Lk = Lq, Lk
        self.heads, self.q_blocks, self.k_blocks = int(m3.shape[0]), nqb, nkb
        self.row_cnt, self.row_idx = _lists(m3)
        self.col_cnt, self.col_idx = _lists(m3.transpose(1, 2))
        self._density = None
        self._moved = {}

    @classmethod
    def from_tables(cls, mask, row_cnt, row_idx, col_cnt, col_idx, Lq: int, Lk: int) -> "BlockMask":
        """A BlockMask over an existing bool ``mask [heads, nQb, nKb]`` and its four int32 tables, all on one device and
        contiguous — taken as they are: nothing is computed, copied or read back, so the caller vouches that the tables
        are those of the mask (ascending kept indices in the first ``cnt`` entries of every list)."""
        Lq, Lk = int(Lq), int(Lk)
        nqb, nkb = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 3 or \
                tuple(mask.shape[1:]) != (nqb, nkb) or mask.shape[0] < 1:
            raise ValueError(f"BlockMask.from_tables: Lq = {Lq}, Lk = {Lk} need a bool mask [heads, {nqb}, {nkb}]")
        h = int(mask.shape[0])
        for name, t, shape in (("row_cnt", row_cnt, (h, nqb)), ("row_idx", row_idx, (h, nqb, nkb)),
                               ("col_cnt", col_cnt, (h, nkb)), ("col_idx", col_idx, (h, nkb, nqb))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != shape or \
                    t.device != mask.device or not t.is_contiguous():
                raise ValueError(f"BlockMask.from_tables: {name} must be a contiguous int32 {list(shape)} on the mask's device")
        if not mask.is_contiguous():
            raise ValueError("BlockMask.from_tables: the mask must be contiguous")
        bm = object.__new__(cls)
        bm.mask, bm.Lq, bm.Lk = mask, Lq, Lk
        bm.heads, bm.q_blocks, bm.k_blocks = h, nqb, nkb
        bm.row_cnt, bm.row_idx, bm.col_cnt, bm.col_idx = row_cnt, row_idx, col_cnt, col_idx
        bm._density = None
        bm._moved = {}
        return bm

    @property
    def density(self) -> float:
        """The share of kept blocks (read back from the mask's device on first use, then remembered)."""
        if self._density is None:
            self._density = float(self.mask.float().mean())
        return self._density

    @property
    def device(self):
        return self.mask.device

    def to(self, device) -> "BlockMask":
        """The same mask with its tables on ``device`` (kept: one copy per device)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.mask.device:
            return self
        got = self._moved.get(device)
        if got is None:
            got = object.__new__(BlockMask)
            got.__dict__.update(self.__dict__)
            for name in ("mask", "row_cnt", "row_idx", "col_cnt", "col_idx"):
                setattr(got, name, getattr(self, name).to(device))
            got._moved = {}
            self._moved[device] = got
        return got

    def c_struct(self):
        """The ``omh_block_mask`` of these tables (the tensors must stay alive for the call)."""
        from ._lib import BlockMaskArgs
        return BlockMaskArgs(self.heads, self.q_blocks, self.k_blocks, self.row_cnt.data_ptr(), self.row_idx.data_ptr(),
                             self.col_cnt.data_ptr(), self.col_idx.data_ptr())


def _dilate(t: torch.Tensor, dim: int, w: int) -> torch.Tensor:
    """out[x] = any(t[x - w .. x + w]) along ``dim`` (a prefix-sum difference)."""
    n = t.shape[dim]
    w = min(int(w), n - 1)
    if w <= 0:
        return t
    c = torch.cumsum(t.to(torch.int32), dim)
    c = torch.cat([torch.zeros_like(c.narrow(dim, 0, 1)), c], dim)               # c[x] = sum of t[:x]
    x = torch.arange(n, device=t.device)
    hi = c.index_select(dim, (x + w + 1).clamp(max=n))
    lo = c.index_select(dim, (x - w).clamp(min=0))
    return (hi - lo) > 0


def block_mask_from_3d_window(grid, window, seq_len=None, block: int = BLOCK) -> torch.Tensor:
    """The block mask of a 3-D local window on a ``grid = (F, H, W)`` token lattice in frame-major order
    ``((f * H + h) * W + w)`` — the order of the model's patch embedding.  Returns bool ``[nb, nb]`` (CPU), nb =
    ceil(seq_len / block), seq_len defaulting to F * H * W.

    Block pair (I, J) is kept iff some token a of block I and some token b of block J, both below F * H * W, satisfy
    ``|fa - fb| <= wt``, ``|ha - hb| <= wh`` and ``|wa - wb| <= ww`` for ``window = (wt, wh, ww)``: a conservative cover —
    every pair the element-wise window allows is visible.  Blocks wholly in the padding up to ``seq_len`` keep only
    themselves."""
    F, H, W = (int(g) for g in grid)
    wt, wh, ww = (int(w) for w in window)
    if min(F, H, W) <= 0 or min(wt, wh, ww) < 0 or block <= 0:
        raise ValueError(f"block_mask_from_3d_window: bad grid {grid} / window {window} / block {block}")
    n = F * H * W
    seq_len = n if seq_len is None else int(seq_len)
    if seq_len < n:
        raise ValueError(f"block_mask_from_3d_window: seq_len {seq_len} is shorter than the grid's {n} tokens")
    nb = (seq_len + block - 1) // block
    live = (n + block - 1) // block                                  # blocks that hold a token
    out = torch.zeros(nb, nb, dtype=torch.bool)
    blk = torch.arange(n) // block                                   # block of every token
    for i0 in range(0, live, 64):                                    # 64 query blocks at a time (bounded memory)
        i1 = min(i0 + 64, live)
        ind = (blk[None, :] == torch.arange(i0, i1)[:, None]).view(i1 - i0, F, H, W)
        reach = _dilate(_dilate(_dilate(ind, 1, wt), 2, wh), 3, ww).view(i1 - i0, n)
        hit = torch.zeros(i1 - i0, live, dtype=torch.int32)
        hit.index_add_(1, blk, reach.to(torch.int32))                # tokens of block J that block I reaches
        out[i0:i1, :live] = hit > 0
    pad = torch.arange(live, nb)
    out[pad, pad] = True
    return out



class DynamicBlockPolicy:
    """How a self-attention call chooses its own block mask from its q and k (``block_mask_from_qk``; the rule is stated
    in include/omh.h): per query block the smallest set of key blocks, largest block probability first and ties together,
    whose probability under the softmax of the block-pooled scores reaches ``mass``.

    ``mass`` in (0, 1] (1 keeps every live block).  ``always``: None or a bool tensor ``[nQb, nKb]`` / ``[heads, nQb,
    nKb]`` of blocks kept whatever the scores say.  ``min_coherence`` in [0, 1] (0: off): a block whose rows disagree
    (|mean|^2 / mean |row|^2 below it) is not judged by its mean — such a query block keeps every live key block, such a
    key block is kept by every live query block.  ``keep_diagonal``: on a square call, block (I, I) is always kept.
    A value object: no parameters, no state beyond device copies of ``always``.  The mask of a batched call is shared by
    its samples (the union of the per-sample selections); no gradient flows through the selection."""

    def __init__(self, mass, always=None, min_coherence: float = 0.0, keep_diagonal: bool = True):
        if isinstance(mass, bool) or not isinstance(mass, (int, float)) or not (0.0 < float(mass) <= 1.0):
            raise ValueError(f"DynamicBlockPolicy: mass must be a number in (0, 1], got {mass!r}")
        if isinstance(min_coherence, bool) or not isinstance(min_coherence, (int, float)) or \
                not (0.0 <= float(min_coherence) <= 1.0):
            raise ValueError(f"DynamicBlockPolicy: min_coherence must be a number in [0, 1], got {min_coherence!r}")
        if always is not None:
            if not isinstance(always, torch.Tensor) or always.dtype != torch.bool or always.dim() not in (2, 3) or \
                    always.numel() == 0:
                raise ValueError("DynamicBlockPolicy: always must be a bool tensor [nQb, nKb] or [heads, nQb, nKb]")
        self.mass, self.min_coherence = float(mass), float(min_coherence)
        self.always = always
        self.keep_diagonal = bool(keep_diagonal)
        self._always_dev = {}

    def __repr__(self):
        a = None if self.always is None else tuple(self.always.shape)
        return (f"DynamicBlockPolicy(mass={self.mass}, always={a}, min_coherence={self.min_coherence}, "
                f"keep_diagonal={self.keep_diagonal})")

    def check_blocks(self, nqb: int, nkb: int, heads: int):
        """ValueError unless ``always`` fits a call of nqb x nkb blocks and ``heads`` heads."""
        a = self.always
        if a is None:
            return
        if tuple(a.shape[-2:]) != (nqb, nkb):
            raise ValueError(f"DynamicBlockPolicy: always has {tuple(a.shape[-2:])} blocks, the call needs ({nqb}, {nkb})")
        if a.dim() == 3 and a.shape[0] not in (1, heads):
            raise ValueError(f"DynamicBlockPolicy: always has {a.shape[0]} heads, 1 or {heads} expected")

    def always_on(self, device, nqb: int, nkb: int, heads: int):
        """``always`` (with the diagonal of a square call) as uint8 ``[1 or heads, nqb, nkb]`` on ``device``, or None;
        one copy per device and shape."""
        self.check_blocks(nqb, nkb, heads)
        diag = self.keep_diagonal and nqb == nkb
        if self.always is None and not diag:
            return None
        key = (str(device), nqb, nkb)
        got = self._always_dev.get(key)
        if got is None:
            if self.always is not None:
                a = self.always if self.always.dim() == 3 else self.always[None]
                a = a.to(device)
                if diag:
                    a = a | torch.eye(nqb, dtype=torch.bool, device=device)[None]
            else:
                a = torch.eye(nqb, dtype=torch.bool, device=device)[None]
            got = a.to(torch.uint8).contiguous()
            self._always_dev[key] = got
        return got


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pool_blocks(x, B: int, L: int, H: int, ld: int, lens=None, x2=None, L2: int = 0, ld2: int = 0, lens2=None):
    """omh_block_pool_d128 on one or two bf16 operands with rows ``[B * L, ld]`` (head h in columns [128 h, 128 h + 128)):
    returns ``(mean fp32 [B, H, nb, 128], coherence fp32 [B, H, nb])`` per operand — a pair, or two pairs with ``x2``;
    both operands go through one launch."""
    from . import _lib
    from .ops import _stream
    ops_ = (_lib.BlockPoolOperand * 2)()
    out = []
    for i, (t, L_, ld_, ln) in enumerate(((x, L, ld, lens), (x2, L2, ld2, lens2))[:1 if x2 is None else 2]):
        if not t.is_cuda or t.dtype != torch.bfloat16:
            raise _lib.OmhError("pool_blocks: bf16 tensors on the GPU are expected (there is no CPU fallback)")
        nb = (L_ + BLOCK - 1) // BLOCK
        mean = torch.empty(B, H, nb, BLOCK, dtype=torch.float32, device=t.device)
        coh = torch.empty(B, H, nb, dtype=torch.float32, device=t.device)
        ops_[i] = _lib.BlockPoolOperand(t.data_ptr(), ld_, L_, 0, None if ln is None else ln.data_ptr(), mean.data_ptr(),
                                        coh.data_ptr())
        out.append((mean, coh))
    _lib.check(_lib.lib.omh_block_pool_d128(ops_, len(out), B, H, _stream()), "omh_block_pool_d128")
    return out[0] if x2 is None else tuple(out)


def select_blocks(q_pool, k_pool, Lq: int, Lk: int, score_scale: float, mass: float, min_coherence: float = 0.0,
                  always=None, q_lens=None, k_lens=None):
    """omh_block_select: pooled ``(mean, coherence)`` pairs of q and k -> bool mask ``[H, nQb, nKb]`` (the union over the
    samples).  ``always``: uint8 ``[1 or H, nQb, nKb]`` on the device, or None."""
    from . import _lib
    from .ops import _stream
    (qm, qc), (km, kc) = q_pool, k_pool
    B, H = int(qm.shape[0]), int(qm.shape[1])
    nqb, nkb = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
    mask = torch.empty(H, nqb, nkb, dtype=torch.uint8, device=qm.device)
    a = _lib.BlockSelectArgs(qm.data_ptr(), qc.data_ptr(), km.data_ptr(), kc.data_ptr(),
                             None if q_lens is None else q_lens.data_ptr(), None if k_lens is None else k_lens.data_ptr(),
                             None if always is None else always.data_ptr(), mask.data_ptr(), B, H, Lq, Lk,
                             1 if always is None else int(always.shape[0]), float(score_scale), float(mass),
                             float(min_coherence))
    _lib.check(_lib.lib.omh_block_select(C.byref(a), _stream()), "omh_block_select")
    return mask.view(torch.bool)


def tables_from_mask(mask: torch.Tensor, Lq: int, Lk: int) -> BlockMask:
    """omh_block_mask_tables: a bool (or uint8 0 / 1) device mask ``[heads, nQb, nKb]`` -> its BlockMask, tables built on
    the device."""
    from . import _lib
    from .ops import _stream
    if not mask.is_cuda or mask.dim() != 3 or mask.dtype not in (torch.bool, torch.uint8):
        raise _lib.OmhError("tables_from_mask: a bool mask [heads, nQb, nKb] on the GPU is expected")
    mask = mask.contiguous()
    mb = mask if mask.dtype == torch.bool else mask.view(torch.bool)
    h, nqb, nkb = (int(v) for v in mask.shape)
    i32 = dict(dtype=torch.int32, device=mask.device)
    row_cnt, row_idx = torch.empty(h, nqb, **i32), torch.empty(h, nqb, nkb, **i32)
    col_cnt, col_idx = torch.empty(h, nkb, **i32), torch.empty(h, nkb, nqb, **i32)
    _lib.check(_lib.lib.omh_block_mask_tables(_p(mask), h, nqb, nkb, _p(row_cnt), _p(row_idx), _p(col_cnt), _p(col_idx),
                                              _stream()), "omh_block_mask_tables")
    return BlockMask.from_tables(mb, row_cnt, row_idx, col_cnt, col_idx, Lq, Lk)


def block_mask_from_rows(q, k, B: int, H: int, Lq: int, Lk: int, ldq: int, ldk: int, policy: DynamicBlockPolicy,
                         score_scale: float, q_lens=None, k_lens=None) -> BlockMask:
    """``block_mask_from_qk`` on operands laid out as rows: q bf16 ``[B * Lq, ldq]``, k bf16 ``[B * Lk, ldk]``, head h in
    columns [128 h, 128 h + 128); lens int32 ``[B]`` on the device or None.  Three launches, nothing read back."""
    if not isinstance(policy, DynamicBlockPolicy):
        raise ValueError("block_mask_from_rows: a DynamicBlockPolicy is expected")
    nqb, nkb = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
    if nkb > 1024:
        raise ValueError(f"a dynamic block mask supports at most 1024 key blocks (Lk <= 131072), got Lk = {Lk}")
    always = policy.always_on(q.device, nqb, nkb, H)
    with torch.no_grad():
        qp, kp = pool_blocks(q, B, Lq, H, ldq, q_lens, k, Lk, ldk, k_lens)
        mask = select_blocks(qp, kp, Lq, Lk, score_scale, policy.mass, policy.min_coherence, always, q_lens, k_lens)
        return tables_from_mask(mask, Lq, Lk)


def block_mask_from_qk(q, k, policy: DynamicBlockPolicy, q_lens=None, k_lens=None, score_scale=None) -> BlockMask:
    """The block mask ``policy`` chooses for the attention of ``q [B, Lq, H, 128]`` over ``k [B, Lk, H, 128]`` (bf16, on
    the GPU), built on the device with no host synchronisation: block means of q and k, the softmax over key blocks of
    ``score_scale * mean_q . mean_k + log2(live keys of the block)`` in base 2, top-p selection at ``policy.mass``, then
    the tables.  ``score_scale`` defaults to ``128 ** -0.5 * log2(e)``, the attention's own scale for an unscaled q; pass
    1.0 for a q that already carries it.  ``q_lens`` / ``k_lens``: int32 ``[B]`` or None, as the attention call gets them.
    The mask is shared by the samples of the batch — the union (OR) of the per-sample selections; at B = 1 it is that
    sample's own.  Deterministic; no gradient flows through the selection (the inputs are read detached)."""
    if not (isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor) and q.dim() == 4 and k.dim() == 4):
        raise ValueError("block_mask_from_qk: q [B, Lq, H, 128] and k [B, Lk, H, 128] are expected")
    if not q.is_cuda or not k.is_cuda:
        from ._lib import OmhError
        raise OmhError("block_mask_from_qk runs on the MI355X only (there is no CPU fallback)")
    B, Lq, H, D = q.shape
    if D != BLOCK or k.shape[0] != B or k.shape[2] != H or k.shape[3] != D:
        raise ValueError(f"block_mask_from_qk: head dim 128 and matching batch / heads are required, got {tuple(q.shape)} "
                         f"and {tuple(k.shape)}")
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16:
        raise ValueError("block_mask_from_qk: bf16 operands are expected (the attention kernel's own)")
    Lk = int(k.shape[1])
    q, k = q.detach().contiguous(), k.detach().contiguous()
    lens = []
    for t in (q_lens, k_lens):
        lens.append(None if t is None else t.to(device=q.device, dtype=torch.int32).contiguous())
    if score_scale is None:
        score_scale = D ** -0.5 * math.log2(math.e)
    return block_mask_from_rows(q, k, B, H, int(Lq), Lk, H * D, H * D, policy, float(score_scale), lens[0], lens[1])
