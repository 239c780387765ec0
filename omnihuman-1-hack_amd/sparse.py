"""Block masks for the block-sparse attention entries (include/omh.h, ``omh_block_mask``).

A mask is a bool array over 128 x 128 blocks of the (padded) score matrix, ``[nQb, nKb]`` shared by all heads or
``[H, nQb, nKb]`` one per head, always shared by the samples of a batch: query i sees key j iff the block
``(i // 128, j // 128)`` is kept, ``j < k_lens[b]`` and ``i < q_lens[b]``.  ``BlockMask`` turns it into the four int32
tables the kernels walk (per query block the ascending list of its key blocks, and the transposed lists for dK / dV);
``block_mask_from_3d_window`` builds the mask of a 3-D local window on a frame-major token lattice.  Building masks and
tables is plain tensor arithmetic on the mask's device (CPU included); only the kernels need the GPU.
"""
import torch

BLOCK = 128

__all__ = ["BLOCK", "BlockMask", "block_mask_from_3d_window"]


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
    of a list mean anything) and ``density``, the share of kept blocks."""

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
        self.density = float(m3.float().mean())
        self._moved = {}

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

