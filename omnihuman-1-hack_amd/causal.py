"""Chunk-causal attention on the host side: the rule as a dense mask, the per-layer K / V cache of a rollout, and the
rollout loop itself.

The rule (include/omh.h, ``omh_chunk_causal``): with ``chunk`` = C >= 1 tokens, ``left_chunks`` = W (< 0: unbounded) and
``q_offset`` = P >= 0 (the position of query row 0 on the key axis), query i sees key j iff

    i < qlen  and  j < klen  and  j // C <= (P + i) // C  and  (W < 0 or j // C >= (P + i) // C - W).

Positions are absolute (no bottom-right shift).  ``WanModel.set_causal_chunks`` runs every self-attention of a forward
under it with C = a group of latent frames; ``WanModel.forward_chunk`` produces the same clip frame group by frame group
against a ``KVCache``, and ``sample`` denoises a clip that way; ``stream`` is the same rollout as a generator that hands every
chunk out as soon as it is denoised, with its pixel frames from a ``WanVAE.decode_stream`` when a VAE is given.

Interval masks (include/omh.h, ``omh_interval_mask``) are the table-driven generalisation: both axes are cut into groups
of ``group`` tokens and a bool matrix ``vis[q_groups, k_groups]`` with at most two runs of True per row and per column
says which key groups a query group sees.  ``IntervalMask`` holds such a matrix with its device tables;
``teacher_forcing_groups`` and ``sink_window_groups`` build two useful ones, ``interval_visible`` is the dense mask.
``IntervalMask(..., runs=3)`` is the three-run form (``omh_interval3_mask``): teacher forcing with an attention sink.

An attention sink plus a window (``WanModel.set_causal_chunks(fpc, W, S)``) rolls out on a ``RollingKVCache``: S sink slots
and a ring of W + 1, so the cache's size does not depend on the clip's length.  ``RollingKVCache(pin_sink=True)`` also
keeps the sink at a fixed rotary distance behind the window (include/omh.h, ``omh_rope_shift_frames``), and ``sample`` /
``stream`` take their noise chunk by chunk: a rollout without an end.  ``forcing_loss(pin_sink=True)`` /
``WanModel.forward_teacher_forcing(pin_sink=True)`` train under that geometry: ``teacher_forcing_groups(pin_sink=True)``
is the mask over the key axis extended by the rotated sink copies of ``sink_copy_deltas``.

Self forcing trains the student on its own rollouts: ``self_forcing_rollout`` returns clips attached to a graph,
``dmd_loss`` puts the distribution-matching objective on them (a frozen teacher and a trainable critic score the noised
clips; include/omh.h, ``omh_dmd_grad``), ``critic_loss`` is the critic's own flow-matching loss on the same generated
clips and ``dmd_sigmas`` draws the noise levels of both.
"""
import ctypes
import itertools

import torch

__all__ = ["chunk_causal_visible", "KVCache", "RollingKVCache", "sample", "stream", "StreamChunk", "IntervalMask", "interval_visible",
           "teacher_forcing_groups", "sink_copy_deltas", "condition_window_visible",
           "sink_window_groups", "forcing_loss", "self_forcing_rollout", "dmd_sigmas", "dmd_loss", "critic_loss"]


def chunk_causal_visible(Lq, Lk, chunk, left_chunks=-1, q_offset=0, qlen=None, klen=None):
    """The rule as a dense bool mask [Lq, Lk] (plain torch, on the CPU): True where query i sees key j."""
    chunk, left_chunks, q_offset = int(chunk), int(left_chunks), int(q_offset)
    if chunk < 1 or q_offset < 0:
        raise ValueError(f"chunk_causal_visible: chunk = {chunk} >= 1 and q_offset = {q_offset} >= 0 expected")
    qlen = Lq if qlen is None else min(max(int(qlen), 0), Lq)
    klen = Lk if klen is None else min(max(int(klen), 0), Lk)
    i = torch.arange(Lq, dtype=torch.int64).view(Lq, 1)
    j = torch.arange(Lk, dtype=torch.int64).view(1, Lk)
    ci = torch.div(q_offset + i, chunk, rounding_mode="floor")
    cj = torch.div(j, chunk, rounding_mode="floor")
    vis = (i < qlen) & (j < klen) & (cj <= ci)
    if left_chunks >= 0:
        vis = vis & (cj >= ci - left_chunks)
    return vis


class IntervalMask:
    """An interval mask for ``ops.flash_attn(interval_mask=)`` and its family: ``vis`` is a bool matrix
    [q_groups, k_groups] (anything ``torch.as_tensor`` takes) over groups of ``group`` >= 8 tokens; query i sees key j iff
    ``vis[i // group, j // group]`` (and both are below their sample's lengths).  Every row and every column may hold at
    most two runs of True (ValueError otherwise): the kernels carry two key intervals per query group and two query
    intervals per key group.  Both int32 tables [groups, 4] = lo0, hi0, lo1, hi1 are built once, on the host
    (omh_interval_mask_tables), and held on ``device``.

    ``runs=3``: the three-run form (omh_interval3_mask) — at most THREE runs per row and per column (ValueError for a
    fourth), tables [groups, 6] = lo0, hi0, lo1, hi1, lo2, hi2 from omh_interval_mask_tables3, and the three-run kernels
    wherever the mask is passed.  Teacher forcing with an attention sink needs it.

    ``k_group`` (an int >= 1): the rectangular form (omh_interval_rect_mask) — ``group`` >= 8 then cuts the query axis only
    and ``k_group`` the key axis: query i sees key j iff ``vis[i // group, j // k_group]``.  Two runs (``runs=3`` beside it is
    a ValueError), the same tables, the ..._interval_rect_d128 kernels wherever the mask is passed.  Cross-attention onto
    frame-aligned condition tokens needs it: a query group is a latent frame, a key group a few tokens."""

    def __init__(self, vis, group, device="cpu", runs=2, k_group=None):
        from . import _lib
        runs = int(runs)
        if runs not in (2, 3):
            raise ValueError(f"IntervalMask: runs = {runs}, 2 or 3 expected")
        if k_group is not None:
            k_group = int(k_group)
            if runs != 2:
                raise ValueError("IntervalMask: the rectangular form (k_group=) has two runs")
            if k_group < 1:
                raise ValueError(f"IntervalMask: k_group = {k_group}, at least 1 token expected")
        self.runs, self.k_group = runs, k_group
        vis = torch.as_tensor(vis).detach().to("cpu")
        group = int(group)
        if vis.dim() != 2 or vis.shape[0] < 1 or vis.shape[1] < 1:
            raise ValueError(f"IntervalMask: a matrix [q_groups, k_groups] expected, got {tuple(vis.shape)}")
        if group < 8:
            raise ValueError(f"IntervalMask: group = {group}, at least 8 tokens expected")
        self.vis = (vis != 0).contiguous()
        self.group, self.q_groups, self.k_groups = group, int(vis.shape[0]), int(vis.shape[1])
        bytes_ = self.vis.to(torch.uint8).contiguous()
        q_iv = torch.zeros(self.q_groups, 2 * runs, dtype=torch.int32)
        k_iv = torch.zeros(self.k_groups, 2 * runs, dtype=torch.int32)
        tables = _lib.lib.omh_interval_mask_tables3 if runs == 3 else _lib.lib.omh_interval_mask_tables
        rc = tables(ctypes.c_void_p(bytes_.data_ptr()), self.q_groups, self.k_groups,
                    ctypes.c_void_p(q_iv.data_ptr()), ctypes.c_void_p(k_iv.data_ptr()))
        if rc != 0:
            raise ValueError(f"IntervalMask: a row or a column of vis holds more than {'three' if runs == 3 else 'two'} "
                             f"runs of True")
        self._host = (q_iv, k_iv)
        self.q_iv = self.k_iv = None
        self._move(torch.device(device))

    def _move(self, device):
        self.device = device
        self.q_iv, self.k_iv = (t.to(device) for t in self._host)

    def to(self, device):
        """This mask with its tables on ``device`` (itself when they are there already)."""
        device = torch.device(device)
        if device == self.device:
            return self
        other = object.__new__(IntervalMask)
        other.__dict__.update(self.__dict__)
        other._move(device)
        return other

    def intervals(self):
        """The two tables as nested lists (host copies): ([q_groups][4], [k_groups][4]) of lo0, hi0, lo1, hi1
        (``runs=3``: rows of 6, with lo2, hi2)."""
        return self._host[0].tolist(), self._host[1].tolist()

    def c_struct(self):
        from . import _lib
        if self.k_group is not None:
            return _lib.IntervalRectMaskArgs(self.group, self.k_group, self.q_groups, self.k_groups, self.q_iv.data_ptr(),
                                             self.k_iv.data_ptr())
        if self.runs == 3:
            return _lib.Interval3MaskArgs(self.group, self.q_groups, self.k_groups, 0, self.q_iv.data_ptr(), self.k_iv.data_ptr())
        return _lib.IntervalMaskArgs(self.group, self.q_groups, self.k_groups, 0, self.q_iv.data_ptr(), self.k_iv.data_ptr())

    def tiles(self, Lq, Lk, block=128, tile=64):
        """Key tiles of ``tile`` tokens the forward's workgroups (``block`` query rows each) run on full-length samples,
        per head: what the kernel derives from the q_iv table, computed here from the same numbers."""
        q_iv, total = self.intervals()[0], 0
        gk = self.group if self.k_group is None else self.k_group
        for q0 in range(0, Lq, block):
            rows = q_iv[q0 // self.group:(min(q0 + block, Lq) - 1) // self.group + 1]
            hull = []
            for lo, hi in ((0, 1), (2, 3), (4, 5))[:self.runs]:
                iv = [(r[lo] * gk, min(r[hi] * gk, Lk)) for r in rows if r[hi] > r[lo]]
                iv = [(a, b) for a, b in iv if b > a]
                if not iv:
                    continue
                a, b = min(a for a, _ in iv) // tile, (max(b for _, b in iv) - 1) // tile + 1
                if hull and a <= hull[-1][1]:                     # touches or overlaps the range before it: one range
                    hull[-1] = (hull[-1][0], max(hull[-1][1], b))
                else:
                    hull.append((a, b))
            total += sum(b - a for a, b in hull)
        return total


def interval_visible(mask, Lq, Lk, qlen=None, klen=None):
    """The rule of an ``IntervalMask`` as a dense bool mask [Lq, Lk] (plain torch, on the CPU): True where query i sees
    key j.  ValueError when the mask's group counts are not ceil(Lq / group) x ceil(Lk / group) (ceil(Lk / k_group) for the
    rectangular form)."""
    g, gk = mask.group, mask.group if mask.k_group is None else mask.k_group
    if (mask.q_groups, mask.k_groups) != ((Lq + g - 1) // g, (Lk + gk - 1) // gk):
        raise ValueError(f"interval_visible: a mask of {mask.q_groups} x {mask.k_groups} groups of {g} x {gk} does not cover "
                         f"Lq = {Lq}, Lk = {Lk}")
    qlen = Lq if qlen is None else min(max(int(qlen), 0), Lq)
    klen = Lk if klen is None else min(max(int(klen), 0), Lk)
    i = torch.arange(Lq, dtype=torch.int64).view(Lq, 1)
    j = torch.arange(Lk, dtype=torch.int64).view(1, Lk)
    dense = mask.vis.repeat_interleave(g, 0)[:Lq].repeat_interleave(gk, 1)[:, :Lk]
    return dense & (i < qlen) & (j < klen)


def sink_copy_deltas(n_chunks, left_chunks, sink_chunks, frames_per_chunk):
    """The rotated copies of the sink keys that teacher forcing under a pinned sink appends to the key axis, in copy order:
    the list of (chunk I, Delta_I in frames) for the chunks whose shift Delta_I = (max(S, I - W) - S) fpc is positive —
    I = S + W + 1 ... n - 1, what ``RollingKVCache(pin_sink=True)`` holds its sink keys at when chunk I runs.  Empty when
    the clip does not outlast the ring.  ValueError for S < 1 or W < 0 (there is no sink to pin)."""
    n, W, S, fpc = int(n_chunks), int(left_chunks), int(sink_chunks), int(frames_per_chunk)
    if n < 1 or S < 1 or W < 0 or fpc < 1:
        raise ValueError(f"sink_copy_deltas: n_chunks = {n} >= 1, sink_chunks = {S} >= 1, left_chunks = {W} >= 0 and "
                         f"frames_per_chunk = {fpc} >= 1 expected (a pinned sink needs a sink and a window)")
    return [(I, (max(S, I - W) - S) * fpc) for I in range(S + W + 1, n)]


def teacher_forcing_groups(n_chunks, left_chunks=-1, sink_chunks=0, pin_sink=False):
    """The teacher-forcing matrix over the sequence [n clean chunks | n noisy chunks], bool [2n, 2n]: clean row g sees
    clean j <= g (and j >= g - W when W = ``left_chunks`` >= 0); noisy row n + I sees clean j < I (and j >= I - W) and noisy
    n + I only — what ``WanModel.forward_chunk`` attends to at chunk I with ``left_chunks`` = W.  With W >= 0 and
    S = ``sink_chunks`` > 0 the first S clean chunks stay visible behind the window (j >= . - W or j < S): up to three
    runs per row, an ``IntervalMask(runs=3)``.

    ``pin_sink=True`` (needs S >= 1 and W >= 0: ValueError otherwise): the rectangular matrix [2n, 2n + C S] over the
    EXTENDED key axis [clean | noisy | sink copy 0 | sink copy 1 | ...] — one copy of the S sink chunks per chunk of
    ``sink_copy_deltas`` (C = max(0, n - S - W - 1) of them, the sink keys rotated to where the pinned rollout holds them
    for that chunk).  The rows of such a chunk I, clean and noisy, see their own copy instead of the columns [0, S);
    everything else is the matrix above.  At most three runs per row and two per column."""
    n, W, S = int(n_chunks), int(left_chunks), int(sink_chunks)
    if pin_sink:
        if S < 1 or W < 0:
            raise ValueError(f"teacher_forcing_groups: pin_sink=True needs sink_chunks = {S} >= 1 and left_chunks = {W} >= 0 "
                             "(there is no sink to pin)")
        base = teacher_forcing_groups(n, W, S)
        copies = sink_copy_deltas(n, W, S, 1)
        vis = torch.zeros(2 * n, 2 * n + len(copies) * S, dtype=torch.bool)
        vis[:, :2 * n] = base
        for c, (I, _) in enumerate(copies):
            for r in (I, n + I):
                vis[r, 2 * n + c * S:2 * n + (c + 1) * S] = base[r, :S]
                vis[r, :S] = False
        return vis
    if n < 1 or S < 0:
        raise ValueError(f"teacher_forcing_groups: n_chunks = {n} >= 1 and sink_chunks = {S} >= 0 expected")
    g = torch.arange(n).view(n, 1)
    j = torch.arange(n).view(1, n)
    back = (j >= g - W) if W >= 0 else torch.ones(n, n, dtype=torch.bool)
    if W >= 0 and S > 0:
        back = back | (j < S)
    vis = torch.zeros(2 * n, 2 * n, dtype=torch.bool)
    vis[:n, :n] = (j <= g) & back
    vis[n:, :n] = (j < g) & back
    vis[n:, n:] = torch.eye(n, dtype=torch.bool)
    return vis


def sink_window_groups(n_chunks, sink_chunks, left_chunks):
    """An attention sink plus a causal window, bool [n, n]: row g sees j <= g with j < ``sink_chunks`` or
    j >= g - ``left_chunks``.  Only the mask: nothing here evicts a cache."""
    n, S, W = int(n_chunks), int(sink_chunks), int(left_chunks)
    if n < 1 or S < 0 or W < 0:
        raise ValueError(f"sink_window_groups: n_chunks = {n} >= 1, sink_chunks = {S} >= 0 and left_chunks = {W} >= 0 expected")
    g = torch.arange(n).view(n, 1)
    j = torch.arange(n).view(1, n)
    return (j <= g) & ((j < S) | (j >= g - W))


def condition_window_visible(q_frames, token_frames, n_text, back, ahead, frames_per_chunk=None, segments=1, frame_offset=0):
    """Which context tokens the queries of a latent frame see in cross-attention, bool [segments * q_frames,
    len(token_frames) + n_text] (plain torch, on the CPU) — the one statement of the rule of frame-aligned condition tokens.

    Row r stands for the query tokens of latent frame f = ``frame_offset`` + r mod ``q_frames`` (``segments`` = 2: teacher
    forcing, clean frame f and noisy frame f share the rule).  Column j < len(token_frames) is condition token j, of latent
    frame g = ``token_frames[j]`` (-1: seen by every query); the last ``n_text`` columns are the text, seen by every query.
    Frame f sees the token iff

        g == -1  or  f - back <= g <= min(f + ahead, E)

    where a side of (``back``, ``ahead``) below 0 is unbounded and E is the last frame of f's chunk,
    (f // frames_per_chunk + 1) frames_per_chunk - 1, when ``frames_per_chunk`` is given (a causal student: nothing of a
    later chunk is seen, whatever ``ahead`` says); without it there is no E.  The columns keep the order of ``token_frames``."""
    q_frames, n_text, segments, frame_offset = int(q_frames), int(n_text), int(segments), int(frame_offset)
    back, ahead = int(back), int(ahead)
    g = torch.as_tensor(token_frames).detach().to("cpu")
    if g.dim() != 1 or g.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"condition_window_visible: token_frames must be a 1-D integer tensor, got {tuple(g.shape)} {g.dtype}")
    g = g.to(torch.int64)
    if q_frames < 1 or n_text < 0 or segments < 1 or frame_offset < 0 or bool((g < -1).any()):
        raise ValueError("condition_window_visible: q_frames >= 1, n_text >= 0, segments >= 1, frame_offset >= 0 and "
                         "token_frames >= -1 expected")
    if frames_per_chunk is not None and int(frames_per_chunk) < 1:
        raise ValueError(f"condition_window_visible: frames_per_chunk = {frames_per_chunk}, None or >= 1 expected")
    f = (frame_offset + torch.arange(q_frames, dtype=torch.int64)).view(q_frames, 1)
    g = g.view(1, -1)
    near = torch.ones(q_frames, g.shape[1], dtype=torch.bool)
    if back >= 0:
        near = near & (g >= f - back)
    if ahead >= 0:
        near = near & (g <= f + ahead)
    if frames_per_chunk is not None:
        fpc = int(frames_per_chunk)
        near = near & (g <= (torch.div(f, fpc, rounding_mode="floor") + 1) * fpc - 1)
    vis = torch.cat([near | (g == -1), torch.ones(q_frames, n_text, dtype=torch.bool)], 1)
    return vis.repeat(segments, 1)


class KVCache:
    """The self-attention keys and values of the tokens a rollout has produced so far, per block of ``model``:

    ``k[l]``   bf16 [batch, cap, dim]: the keys after norm and RoPE, token-major (what the attention kernel reads);
    ``vt[l]``  bf16 [batch, dim, pitch], pitch = roundup(cap, 64): V transposed, zero-initialised (the kernel multiplies
               the pad columns by P = 0 and needs them finite);
    ``length`` tokens committed so far (a host integer; ``WanModel.forward_chunk(commit=True)`` advances it).

    ``cap`` = ``max_tokens``; nothing is evicted.  Rows / columns at or past ``length`` are scratch.

    ``WanModel.forward_chunk(grad=True)`` reads the committed rows again in its backward, in place.  They stay what they
    were as long as ``length`` never fell below them in between: ``mark()`` is a token of the cache's state and
    ``intact(mark, n_tokens)`` says whether rows [0, n_tokens) are still the ones that were committed at that mark — False
    once ``reset()`` or ``truncate()`` cut below ``n_tokens`` afterwards (whatever was committed since)."""

    def __init__(self, model, batch, max_tokens, device):
        batch, cap = int(batch), int(max_tokens)
        if batch < 1 or cap < 1:
            raise ValueError(f"KVCache: batch = {batch} and max_tokens = {cap} must be positive")
        self.model_id = id(model)
        self.batch, self.cap, self.dim = batch, cap, int(model.dim)
        self.pitch = (cap + 63) // 64 * 64
        self.length = 0
        self._gen = 0                                      # counts the cuts (reset / truncate below the length)
        self._cuts = []                                    # [(gen, length after the cut)], lengths strictly increasing
        n = len(model.blocks)
        self.k = [torch.zeros(batch, cap, self.dim, dtype=torch.bfloat16, device=device) for _ in range(n)]
        # 64 elements of slack behind the last row: a key tile that starts at a look-back offset may read that far past it
        self._vt_store = [torch.zeros(batch * self.dim * self.pitch + 64, dtype=torch.bfloat16, device=device)
                          for _ in range(n)]
        self.vt = [s[:batch * self.dim * self.pitch].view(batch, self.dim, self.pitch) for s in self._vt_store]

    def check_room(self, n_tokens):
        """ValueError when ``n_tokens`` more do not fit behind ``length``."""
        if n_tokens < 0 or self.length + n_tokens > self.cap:
            raise ValueError(f"KVCache: {self.length} cached tokens + {n_tokens} exceed max_tokens = {self.cap}")

    def advance(self, n_tokens):
        """Commit ``n_tokens`` more (their k / V^T are in place)."""
        self.check_room(n_tokens)
        self.length += int(n_tokens)

    def truncate(self, n_tokens):
        """Forget every token from ``n_tokens`` on (their rows become scratch)."""
        n_tokens = int(n_tokens)
        if not 0 <= n_tokens <= self.length:
            raise ValueError(f"KVCache.truncate({n_tokens}): the cache holds {self.length} tokens")
        self._cut(n_tokens)

    def reset(self):
        self._cut(0)

    def _cut(self, n_tokens):
        if n_tokens < self.length:
            self._gen += 1
            while self._cuts and self._cuts[-1][1] >= n_tokens:      # a deeper cut makes the shallower ones before it moot
                self._cuts.pop()
            self._cuts.append((self._gen, n_tokens))
        self.length = n_tokens

    def mark(self):
        """A token of the cache's state for ``intact``."""
        return self._gen

    def intact(self, mark, n_tokens):
        """Are rows [0, n_tokens) still what was committed when ``mark()`` returned ``mark``."""
        return not any(g > mark and n < n_tokens for g, n in self._cuts)


class RollingKVCache:
    """A ``KVCache`` of constant size for a model under ``set_causal_chunks(fpc, W, S)``, W = ``left_chunks`` >= 0,
    S = ``sink_chunks`` >= 0: ``slots`` = S + W + 1 slots of ``chunk_tokens`` = fpc h w tokens per layer, laid out as in
    ``KVCache`` (``k[l]`` bf16 [batch, cap, dim] token-major, ``vt[l]`` bf16 [batch, dim, pitch] with 64 elements of slack
    behind it), cap = slots * chunk_tokens.  The sink slots come first, the rest is a ring: chunk I < S lives in slot I,
    chunk I >= S in slot S + (I - S) mod (W + 1) — the slot of chunk I - W - 1, which chunk I does not see.  After any
    number of commits the resident chunks are the sink and the last W + 1.

    ``length`` counts the tokens committed since ``reset()`` and does not stop at the capacity.  ``truncate`` reaches
    back to the start of the last committed chunk only: what lay before it may be evicted already.

    ``pin_sink=True`` (needs S > 0: ValueError otherwise): the sink keeps a fixed rotary distance to the window however
    long the rollout runs.  Cached keys carry the rotary position of their frame; for the window that is harmless (RoPE is
    relative), but the sink of chunk I would sit I chunks behind the queries.  Pinned, the key rows of a sink chunk are
    copied as they are committed into ``sink_k[l]`` (bf16 [batch, S chunk_tokens, dim], the pristine copy), and the live
    rows ``k[l][:, :S chunk_tokens]`` are ``ops.rope_shift_frames(sink_k[l], None, sink_delta)`` — always derived from the
    pristine bits, never from rows that were rotated before: a key is rounded once more and no more.  Chunk I needs
    ``sink_shift_chunks(I)`` = max(S, I - W) - S chunks, times the frames of a chunk: 0 until the ring has wrapped,
    afterwards the sink ends where the window's first chunk begins.  ``WanModel.forward_chunk`` calls ``pin()`` before
    its blocks run; ``sink_delta`` is the shift in frames the live rows hold, ``sink_rows`` the pristine rows that are valid
    (a cut into a sink chunk invalidates the rows behind it until they are committed again).  V has no rotary position
    and stays as it is."""
    rolling = True

    def __init__(self, model, batch, chunk_tokens, sink_chunks, left_chunks, device, pin_sink=False):
        batch, Ct, S, W = int(batch), int(chunk_tokens), int(sink_chunks), int(left_chunks)
        if batch < 1 or Ct < 1:
            raise ValueError(f"RollingKVCache: batch = {batch} and chunk_tokens = {Ct} must be positive")
        if S < 0 or W < 0:
            raise ValueError(f"RollingKVCache: sink_chunks = {S} >= 0 and left_chunks = {W} >= 0 expected (an unbounded "
                             f"look-back never evicts: use KVCache)")
        self.pin_sink = bool(pin_sink)
        if self.pin_sink and S < 1:
            raise ValueError("RollingKVCache: pin_sink=True needs sink_chunks > 0 (there is no sink to pin)")
        self.model_id = id(model)
        self.batch, self.dim = batch, int(model.dim)
        self.chunk_tokens, self.sink_chunks, self.left_chunks = Ct, S, W
        self.slots = S + W + 1
        self.cap = self.slots * Ct
        self.pitch = (self.cap + 63) // 64 * 64
        self.length = 0
        self._floor = 0                                    # truncate() may not go below it
        n = len(model.blocks)
        self.k = [torch.zeros(batch, self.cap, self.dim, dtype=torch.bfloat16, device=device) for _ in range(n)]
        self._vt_store = [torch.zeros(batch * self.dim * self.pitch + 64, dtype=torch.bfloat16, device=device)
                          for _ in range(n)]
        self.vt = [s[:batch * self.dim * self.pitch].view(batch, self.dim, self.pitch) for s in self._vt_store]
        self.sink_delta = 0                                # frames the live sink rows are rotated past their own position
        self.sink_rows = 0                                 # pristine rows [0, sink_rows) are the committed ones
        self.sink_k = [torch.zeros(batch, S * Ct, self.dim, dtype=torch.bfloat16, device=device) for _ in range(n)] \
            if self.pin_sink else None

    def sink_shift_chunks(self, chunk):
        """How many chunks the sink is moved up for chunk ``chunk`` of the clip: max(S, chunk - W) - S."""
        return max(self.sink_chunks, int(chunk) - self.left_chunks) - self.sink_chunks

    def pin(self, frames_per_chunk, head_dim, theta=10000.0):
        """Bring the live sink rows of every layer to the shift the chunk ``length`` stands in needs — one
        ``ops.rope_shift_frames`` launch per layer from the pristine copy, and nothing when they hold it already.
        ValueError when the shift is due before every sink row is committed.  Without ``pin_sink`` it does nothing."""
        if not self.pin_sink:
            return
        due = self.sink_shift_chunks(self.length // self.chunk_tokens) * int(frames_per_chunk)
        if due == self.sink_delta:
            return
        n = self.sink_chunks * self.chunk_tokens
        if self.sink_rows < n:
            raise ValueError(f"RollingKVCache.pin: only {self.sink_rows} of {n} sink rows are committed; a short sink chunk "
                             f"cannot be moved")
        shift = self._shift
        if shift is None:
            from . import ops
            shift = ops.rope_shift_frames
        for pristine, live in zip(self.sink_k, self.k):
            shift(pristine, live[:, :n], due, head_dim, theta)
        self.sink_delta = due

    _shift = None                                          # (tests put a CPU statement of ops.rope_shift_frames here)

    def slot(self, chunk):
        """The slot chunk ``chunk`` of the clip lives in."""
        S = self.sink_chunks
        return chunk if chunk < S else S + (chunk - S) % (self.left_chunks + 1)

    def resident(self):
        """{slot: chunk} of the committed chunks that are still in the cache (a partly committed chunk counts)."""
        n = (self.length + self.chunk_tokens - 1) // self.chunk_tokens
        return {self.slot(c): c for c in range(n) if c < self.sink_chunks or c >= n - 1 - self.left_chunks}

    def check_room(self, n_tokens):
        """ValueError when ``n_tokens`` more do not fit into the chunk ``length`` stands in."""
        if n_tokens < 0 or self.length % self.chunk_tokens + n_tokens > self.chunk_tokens:
            raise ValueError(f"RollingKVCache: {n_tokens} tokens at {self.length} committed ones cross the end of a chunk of "
                             f"{self.chunk_tokens} tokens")

    def advance(self, n_tokens):
        """Commit ``n_tokens`` more (their k / V^T are in their slot)."""
        self.check_room(n_tokens)
        if n_tokens > 0:
            self._floor = self.length - self.length % self.chunk_tokens
            if self.pin_sink and self.length < self.sink_chunks * self.chunk_tokens:
                # a sink chunk (its slot is its place, and the shift is 0 until the ring wraps): keep the rows as committed
                rows = slice(self.length, self.length + int(n_tokens))
                for pristine, live in zip(self.sink_k, self.k):
                    pristine[:, rows].copy_(live[:, rows])
                self.sink_rows = rows.stop
        self.length += int(n_tokens)

    def truncate(self, n_tokens):
        """Forget every token from ``n_tokens`` on — within the last committed chunk (ValueError otherwise: the chunk
        before the window of an earlier one has been overwritten)."""
        n_tokens = int(n_tokens)
        if not self._floor <= n_tokens <= self.length:
            raise ValueError(f"RollingKVCache.truncate({n_tokens}): only [{self._floor}, {self.length}], the last committed "
                             f"chunk, can be cut")
        self.length = n_tokens
        self.sink_rows = min(self.sink_rows, n_tokens)

    def reset(self):
        # (the live sink rows are scratch again: the sink chunks rewrite them at their own positions, shift 0)
        self.length = self._floor = self.sink_rows = self.sink_delta = 0


@torch.no_grad()
def sample(model, noise, context, context_null, *, frames_per_chunk, left_chunks=-1, make_scheduler, guide_scale,
           context_t=0.0, sink_chunks=0, rolling=False, caches=None, extra_conditions=None, pin_sink=False):
    """Denoise one clip chunk by chunk.  ``noise``: the initial latents [C, F, H, W] of the clip; ``context`` /
    ``context_null``: what ``WanModel.forward`` takes for a batch of one (a list with one [L, text_dim] tensor, or a
    ``ContextState``).  For every group of ``frames_per_chunk`` latent frames (the last one may be shorter):

    1. a fresh scheduler from ``make_scheduler()`` (timesteps already set);
    2. its sampling steps — ``forward_chunk(..., commit=False)`` on two caches, conditional and unconditional, then
       ``scheduler.step_cfg`` with ``guide_scale``;
    3. one ``commit=True`` pass of the finished chunk at t = ``context_t`` on both caches, so that the later chunks
       attend to its keys and values (skipped behind the last chunk: nothing reads them).

    A chunk sees itself and the ``left_chunks`` chunks before it (< 0: all of them), and with ``sink_chunks`` > 0 the
    first ``sink_chunks`` chunks of the clip as well.  ``rolling=True`` (needs ``left_chunks`` >= 0; implied by a sink):
    two ``RollingKVCache``s in place of the two ``KVCache``s — cache memory then does not depend on the clip's length.
    ``caches``: a pair (conditional, unconditional) of caches of batch 1 to use in place of fresh ones (they are reset).
    ``pin_sink=True`` (needs ``sink_chunks`` > 0, implies the rolling caches; caches passed in must have been built with
    the same value): ``RollingKVCache(pin_sink=True)`` — once the ring has wrapped the sink keys are re-rotated to sit
    directly behind the window, so that a chunk's result does not depend on how far into the clip it lies; the chunks up
    to ``sink_chunks + left_chunks`` keep the bits of the unpinned rollout.
    ``noise`` may also be an iterable that yields the noise one chunk [C, f <= fpc, H, W] at a time — a rollout whose length
    nobody knows up front (a shorter item must be the last; the iterable is read one chunk ahead).  That form needs
    rolling caches (ValueError otherwise, before anything runs) and gives the bits of the concatenated tensor.
    ``extra_conditions``: condition tokens as ``WanModel.forward`` takes them, for the conditional branch only (``context``
    is then the raw text, no ``ContextState``).  With ``"frames"`` and ``"window"`` every ``forward_chunk`` call — denoising
    and commit passes alike — keeps only the tokens of the frames from the chunk's first frame - back to its last frame
    (and the -1 tokens): a live stream needs nothing it does not have yet.
    The model's own
    ``set_causal_chunks`` setting is restored on the way out.  Returns the latents of the whole clip, fp32 [C, F, H, W]
    — the chunks of ``stream`` with the same arguments, concatenated."""
    caches = None if caches is None else tuple(caches)
    geom = _rollout_geometry("sample", noise, frames_per_chunk, left_chunks, sink_chunks, rolling, pin_sink, caches)
    chunks = _rollout(model, noise, context, context_null, geom, make_scheduler, guide_scale, context_t, rolling, caches,
                      extra_conditions, who="sample")
    return torch.cat([c.latents for c in chunks], dim=1)


class StreamChunk:
    """One chunk of ``stream``: ``index`` (0, 1, ...), ``frames`` = (f0, f1), the chunk's latent frame range in the clip,
    ``latents`` fp32 [C, f1 - f0, h, w], ``video`` — the pixel frames ``DecodeStream.push`` returned for them, or None
    without a VAE — and ``ready``, a ``torch.cuda.Event`` behind the last launch that writes either.  ``wait()`` makes the
    current stream wait for it (and tells the caching allocator that the tensors are used there)."""
    __slots__ = ("index", "frames", "latents", "video", "ready")

    def __init__(self, index, frames, latents, video=None, ready=None):
        self.index, self.frames, self.latents, self.video, self.ready = index, frames, latents, video, ready

    def wait(self):
        if self.ready is not None:
            cur = torch.cuda.current_stream(self.latents.device)
            cur.wait_event(self.ready)
            for u in (self.latents, self.video):
                if u is not None:
                    u.record_stream(cur)
        return self


def _rollout_geometry(who, noise, frames_per_chunk, left_chunks, sink_chunks, rolling, pin_sink=False, caches=None):
    """The argument rules ``sample`` and ``stream`` share (nothing touches a device).  Returns (fpc, left_chunks,
    sink_chunks, pin_sink) as the model and the caches are set up with them."""
    fpc = int(frames_per_chunk)
    if isinstance(noise, torch.Tensor) and noise.dim() != 4:
        raise ValueError(f"{who}: noise [C, F, H, W] of one clip expected, got {tuple(noise.shape)}")
    left_chunks, sink_chunks = int(left_chunks), int(sink_chunks)
    if rolling and left_chunks < 0:
        raise ValueError(f"{who}: rolling=True needs left_chunks >= 0 (an unbounded look-back never evicts)")
    if sink_chunks < 0:
        raise ValueError(f"{who}: sink_chunks = {sink_chunks} >= 0 expected")
    if left_chunks < 0:
        sink_chunks = 0
    if pin_sink and sink_chunks < 1:
        raise ValueError(f"{who}: pin_sink=True needs sink_chunks > 0 and left_chunks >= 0 (there is no sink to pin)")
    if caches is not None:
        caches = tuple(caches)
        if len(caches) != 2:
            raise ValueError(f"{who}: caches = (conditional, unconditional) expected")
        if any(bool(getattr(c, "pin_sink", False)) != bool(pin_sink) for c in caches):
            raise ValueError(f"{who}: pin_sink = {bool(pin_sink)}, but the caches were built with "
                             f"pin_sink = {[bool(getattr(c, 'pin_sink', False)) for c in caches]}")
    if not isinstance(noise, torch.Tensor):
        if not hasattr(noise, "__iter__"):
            raise ValueError(f"{who}: noise is a tensor [C, F, H, W] or an iterable of chunks [C, f, H, W]")
        ring = all(getattr(c, "rolling", False) for c in caches) if caches is not None else (rolling or sink_chunks > 0)
        if not ring:
            raise ValueError(f"{who}: noise given chunk by chunk has no length to size a KVCache with; it needs rolling "
                             f"caches (rolling=True with left_chunks >= 0, or a sink)")
    return fpc, left_chunks, sink_chunks, bool(pin_sink)


def _noise_chunks(who, noise, fpc):
    """(first frame, noise of the chunk, is it the last) per chunk, from a clip [C, F, H, W] or from an iterable of
    chunks [C, f <= fpc, H, W] of one C, H, W and device — read one chunk ahead, so that the last one is known as such;
    an item shorter than ``fpc`` must be the last (ValueError)."""
    if isinstance(noise, torch.Tensor):
        F = noise.shape[1]
        for f0 in range(0, F, fpc):
            yield f0, noise[:, f0:f0 + fpc], f0 + fpc >= F
        return
    f0, cur, shape = 0, None, None
    for item in noise:
        if not isinstance(item, torch.Tensor) or item.dim() != 4 or not 1 <= item.shape[1] <= fpc:
            raise ValueError(f"{who}: every item of noise is a chunk [C, f, H, W] with 1 <= f <= {fpc} frames")
        key = (item.shape[0], item.shape[2], item.shape[3], item.device)
        if shape is not None and key != shape:
            raise ValueError(f"{who}: the chunks of noise must share C, H, W and the device")
        shape = key
        if cur is not None:
            if cur.shape[1] < fpc:
                raise ValueError(f"{who}: a chunk of {cur.shape[1]} < {fpc} frames must be the last item of noise")
            yield f0, cur, False
            f0 += cur.shape[1]
        cur = item
    if cur is not None:
        yield f0, cur, True


@torch.no_grad()
def _rollout(model, noise, context, context_null, geom, make_scheduler, guide_scale, context_t, rolling, caches,
             extra_conditions, who, decoder=None, overlap=False, events=False):
    """The one statement of the chunk-by-chunk rollout: a generator of ``StreamChunk``s (``sample`` concatenates their
    latents, ``stream`` hands them out).  ``decoder``: a ``DecodeStream`` every finished chunk is pushed into; ``overlap``:
    on a side stream of this generator's, see ``stream``; ``events``: record ``ready``."""
    fpc, left_chunks, sink_chunks, pin_sink = geom
    source = _noise_chunks(who, noise, fpc)
    head = next(source, None)                              # (an iterable: its first chunk gives the geometry and the device)
    if head is None:
        return
    first = noise if isinstance(noise, torch.Tensor) else head[1]
    dev = first.device
    pt, ph, pw = model.patch_size
    prev = getattr(model, "_causal_chunks", None)
    model.set_causal_chunks(fpc, left_chunks, sink_chunks)
    try:
        if caches is not None:
            caches = tuple(caches)
            if len(caches) != 2:
                raise ValueError(f"{who}: caches = (conditional, unconditional) expected")
            for c in caches:
                c.reset()
        elif rolling or sink_chunks > 0:
            Ct = fpc * (first.shape[2] // ph) * (first.shape[3] // pw)
            caches = tuple(RollingKVCache(model, 1, Ct, sink_chunks, left_chunks, dev, pin_sink=pin_sink) for _ in range(2))
        else:
            tokens = (first.shape[1] // pt) * (first.shape[2] // ph) * (first.shape[3] // pw)
            caches = (KVCache(model, 1, tokens, dev), KVCache(model, 1, tokens, dev))
        t_ctx = torch.full((1,), float(context_t), device=dev)
        side = torch.cuda.Stream(dev) if (overlap and decoder is not None) else None
        held = None
        for index, (f0, chunk_noise, last) in enumerate(itertools.chain((head,), source)):
            lat = chunk_noise.float().contiguous()
            scheduler = make_scheduler()
            for t in scheduler.timesteps:
                tt = torch.stack([t])
                cond = model.forward_chunk([lat], tt, context, caches[0], commit=False, extra_conditions=extra_conditions)[0]
                uncond = model.forward_chunk([lat], tt, context_null, caches[1], commit=False)[0]
                lat = scheduler.step_cfg(cond, uncond, guide_scale, lat)
            if held is not None:                  # overlap: the chunk before goes out now that this one's launches are enqueued
                yield held
                held = None
            chunk = StreamChunk(index, (f0, f0 + lat.shape[1]), lat)
            if side is not None:
                main = torch.cuda.current_stream(dev)
                fence = torch.cuda.Event()
                fence.record(main)                # behind the chunk's last sampler update
                lat.record_stream(side)
                with torch.cuda.stream(side):
                    side.wait_event(fence)
                    chunk.video = decoder.push(lat)
                    chunk.ready = torch.cuda.Event()
                    chunk.ready.record(side)
            else:
                if decoder is not None:
                    chunk.video = decoder.push(lat)
                if events:
                    chunk.ready = torch.cuda.Event()
                    chunk.ready.record(torch.cuda.current_stream(dev))
            if side is None or last:
                yield chunk
            else:
                held = chunk
            if not last:
                model.forward_chunk([lat], t_ctx, context, caches[0], commit=True, extra_conditions=extra_conditions)
                model.forward_chunk([lat], t_ctx, context_null, caches[1], commit=True)
    finally:
        model._causal_chunks = prev


def stream(model, noise, context, context_null, *, frames_per_chunk, left_chunks=-1, make_scheduler, guide_scale,
           context_t=0.0, sink_chunks=0, rolling=False, caches=None, extra_conditions=None, vae=None, output="float",
           overlap=False, pin_sink=False):
    """``sample`` as a generator: one ``StreamChunk`` per chunk, as soon as the chunk is denoised — ``sample(...)`` equals
    ``torch.cat([c.latents for c in stream(...)], 1)`` bit for bit.  ``vae``: a ``WanVAE``; every chunk is pushed into one
    ``vae.decode_stream(output)`` and ``chunk.video`` holds the pixel frames it completes (``output`` = "float": fp32
    [3, frames, 8h, 8w]; "uint8": packed RGB [frames, 8h, 8w, 3]), together the frames of ``vae.decode`` on the whole clip,
    bit for bit: 4 (n - 1) + 1 frames for the first chunk of n latent frames, 4 n for every later one.

    ``overlap=False`` (the default): everything runs on the current stream; chunk I is yielded behind its decode, and its
    commit pass is enqueued when the consumer asks for the next chunk.  ``overlap=True`` (with a ``vae``): the decode of
    chunk I runs on a side stream this generator owns, fenced by an event behind the chunk's last sampler update, and the
    chunk is yielded only after the commit pass and the denoising launches of chunk I + 1 are enqueued on the main stream
    (the last chunk at once) — a consumer that blocks on ``chunk.ready`` does not serialise the two.  The bits are the
    same.  Either way call ``chunk.wait()`` (or wait for ``chunk.ready``) before reading the tensors from another stream.

    While the generator is suspended the model stays under this rollout's ``set_causal_chunks`` setting; it is restored
    when the generator finishes or is closed.  The arguments are checked here, before the first chunk is asked for
    (ValueError, as ``sample``).  ``pin_sink`` and ``noise`` as an iterable of chunks: as in ``sample`` — together an
    open-ended stream, whose frame positions may pass the model's rotary table."""
    caches = None if caches is None else tuple(caches)
    geom = _rollout_geometry("stream", noise, frames_per_chunk, left_chunks, sink_chunks, rolling, pin_sink, caches)
    if output not in ("float", "uint8"):
        raise ValueError(f"stream: output = {output!r}, 'float' or 'uint8' expected")
    decoder = vae.decode_stream(output) if vae is not None else None
    return _rollout(model, noise, context, context_null, geom, make_scheduler, guide_scale, context_t, rolling, caches,
                    extra_conditions, who="stream", decoder=decoder, overlap=bool(overlap), events=True)


def forcing_loss(model, latents, noise, sigmas, timesteps, context, mode="teacher", pin_sink=False):
    """The flow-matching loss of a frame-causal student with one noise level per chunk.  ``latents`` / ``noise``: lists of
    [C, F, H, W] (x_0 and epsilon, every clip of one shape); ``sigmas`` / ``timesteps``: [B, F / fpc], per chunk
    (fpc = the model's ``set_causal_chunks`` frames per chunk).  x_t = (1 - sigma) x_0 + sigma epsilon per chunk, the
    target is epsilon - x_0.  ``mode="teacher"``: ``model.forward_teacher_forcing(latents, x_t, timesteps, context)`` —
    the noisy chunks attend to the CLEAN chunks before them; ``mode="diffusion"``: ``model.forward`` on x_t alone with
    the per-frame timesteps under the staircase (diffusion forcing: they attend to the noisy ones).
    ``pin_sink=True`` (``mode="teacher"`` under ``set_causal_chunks(fpc, W, S)`` with S >= 1 and W >= 0: ValueError otherwise):
    ``forward_teacher_forcing(..., pin_sink=True)`` — every chunk sees the sink where ``RollingKVCache(pin_sink=True)`` holds it
    at rollout.  Returns the mean squared error over all clips (plain torch on the model's outputs)."""
    cc = getattr(model, "_causal_chunks", None)
    if cc is None:
        raise ValueError("forcing_loss: model.set_causal_chunks(frames_per_chunk, left_chunks) first")
    if mode not in ("teacher", "diffusion"):
        raise ValueError(f"forcing_loss: mode = {mode!r}, 'teacher' or 'diffusion' expected")
    if pin_sink and mode != "teacher":
        raise ValueError("forcing_loss: pin_sink=True is teacher forcing under the pinned rollout's geometry (mode='teacher')")
    fpc = cc[0]
    latents, noise = list(latents), list(noise)
    F = latents[0].shape[1] // model.patch_size[0]
    if F % fpc or tuple(sigmas.shape) != (len(latents), F // fpc) or tuple(timesteps.shape) != tuple(sigmas.shape):
        raise ValueError(f"forcing_loss: sigmas and timesteps of shape [{len(latents)}, F / {fpc}] expected for F = {F}")
    per_frame = lambda v: v.repeat_interleave(fpc * model.patch_size[0], dim=1)
    x_t, target = [], []
    for b, (x0, eps) in enumerate(zip(latents, noise)):
        s = per_frame(sigmas[b:b + 1]).to(device=x0.device, dtype=x0.dtype).view(1, -1, 1, 1)
        x_t.append((1 - s) * x0 + s * eps)
        target.append(eps - x0)
    if mode == "teacher":
        out = model.forward_teacher_forcing(latents, x_t, timesteps, context, **({"pin_sink": True} if pin_sink else {}))
    else:
        pt, ph, pw = model.patch_size
        tokens = F * (latents[0].shape[2] // ph) * (latents[0].shape[3] // pw)
        out = model(x_t, timesteps.repeat_interleave(fpc, dim=1), context, tokens)
    return torch.stack([(o.float() - v.to(o.device).float()).square().mean() for o, v in zip(out, target)]).mean()


def self_forcing_rollout(model, noise, context, *, frames_per_chunk, left_chunks=-1, sigmas, timesteps, exit_step,
                         context_t=0.0, generator=None, cache=None, extra_conditions=None):
    """Roll a batch of clips out chunk by chunk with the few-step student sampler against a ``KVCache``, as at inference,
    and keep the graph of the LAST denoising step of every chunk (self forcing).  ``noise``: a list of B clips
    [C, F, H, W] of one shape, F a multiple of ``frames_per_chunk`` (ValueError otherwise); ``sigmas`` / ``timesteps``: the
    n descending levels of the schedule (sequences or 1-D tensors of one length); ``exit_step``: an int in [0, n), or one
    per chunk — the step whose output is kept.  The student is guidance-free: one cache of batch B, fresh or the caller's
    (``cache``; it is reset).  For chunk I in order:

    1. steps j < exit under ``no_grad``: ``forward_chunk(commit=False)``, ``ops.flow_x0_step`` to x0 and on to level
       j + 1 with fresh ``torch.randn(generator=)`` noise;
    2. step exit: ``forward_chunk(grad=True, commit=False)`` and x0_I = x - sigma v through ``ops.flow_x0_step``, attached;
    3. except behind the last chunk: ``forward_chunk(x0_I.detach(), context_t, commit=True)`` under ``no_grad`` — the later
       chunks attend to its keys and values as constants.

    ``extra_conditions``: condition tokens as ``WanModel.forward`` takes them, handed to every ``forward_chunk`` call (with
    ``"frames"`` and ``"window"`` each chunk keeps the tokens of its first frame - back to its last frame and the -1
    tokens); tokens that require grad get it through the exit steps.

    Returns the list of B clips, fp32 [C, F, H, W], attached to the graph (the loss is the caller's).  The cache must
    stay as it is until ``backward()`` has run (a ``reset()`` in between makes the backward raise RuntimeError).  The
    model's ``set_causal_chunks`` setting is restored on the way out."""
    from . import ops
    fpc, left_chunks = int(frames_per_chunk), int(left_chunks)
    noise = list(noise)
    if not noise or any(u.dim() != 4 for u in noise) or len({tuple(u.shape) for u in noise}) != 1:
        raise ValueError("self_forcing_rollout: noise is a list of clips [C, F, H, W] of one shape")
    B, F = len(noise), noise[0].shape[1]
    if fpc < 1 or F % fpc:
        raise ValueError(f"self_forcing_rollout: F = {F} latent frames are no multiple of frames_per_chunk = {frames_per_chunk}")
    sig = [float(s) for s in (sigmas.tolist() if isinstance(sigmas, torch.Tensor) else sigmas)]
    tms = [float(t) for t in (timesteps.tolist() if isinstance(timesteps, torch.Tensor) else timesteps)]
    n, chunks = len(sig), F // fpc
    if n < 1 or len(tms) != n:
        raise ValueError(f"self_forcing_rollout: {n} sigmas and {len(tms)} timesteps; one non-empty schedule expected")
    exits = [int(exit_step)] * chunks if isinstance(exit_step, int) else [int(e) for e in exit_step]
    if len(exits) != chunks or any(not 0 <= e < n for e in exits):
        raise ValueError(f"self_forcing_rollout: exit_step = {exit_step}; an int in [0, {n}) or one per chunk ({chunks}) expected")
    if cache is not None and getattr(cache, "rolling", False):
        raise ValueError("self_forcing_rollout: a RollingKVCache evicts what the backward reads; pass a KVCache "
                         "(left_chunks bounds the look-back)")
    pt, ph, pw = model.patch_size
    dev = noise[0].device
    tokens = (F // pt) * (noise[0].shape[2] // ph) * (noise[0].shape[3] // pw)
    prev = getattr(model, "_causal_chunks", None)
    model.set_causal_chunks(fpc, left_chunks)
    try:
        if cache is None:
            cache = KVCache(model, B, tokens, dev)
        else:
            cache.reset()
        lvl = lambda vals: [torch.full((B,), v, dtype=torch.float32, device=dev) for v in vals]
        sig_d, t_d = lvl(sig), lvl(tms)
        t_ctx = torch.full((B,), float(context_t), dtype=torch.float32, device=dev)
        done = []
        for I in range(chunks):
            x = torch.stack([u[:, I * fpc:(I + 1) * fpc] for u in noise]).float().contiguous().detach()
            for j in range(exits[I]):
                with torch.no_grad():
                    v = torch.stack(model.forward_chunk(list(x.unbind(0)), t_d[j], context, cache, commit=False,
                                                        extra_conditions=extra_conditions))
                    eps = torch.randn(x.shape, dtype=torch.float32, device=dev, generator=generator)
                    _, x = ops.flow_x0_step(v, x, sig_d[j], eps, sig_d[j + 1])
            j = exits[I]
            v = torch.stack(model.forward_chunk(list(x.unbind(0)), t_d[j], context, cache, commit=False, grad=True,
                                                extra_conditions=extra_conditions))
            x0 = ops.flow_x0_step(v, x, sig_d[j])
            done.append(x0)
            if I + 1 < chunks:
                with torch.no_grad():
                    model.forward_chunk(list(x0.detach().unbind(0)), t_ctx, context, cache, commit=True,
                                        extra_conditions=extra_conditions)
        clip = torch.cat(done, dim=2)                                       # [B, C, F, H, W]
        return list(clip.unbind(0))
    finally:
        model._causal_chunks = prev


def dmd_sigmas(B, generator=None, lo=0.02, hi=0.98, shift=5.0, device=None):
    """One noise level per clip for ``dmd_loss`` / ``critic_loss``: u uniform in [``lo``, ``hi``] (``torch.rand`` with
    ``generator``), sigma = shift u / (1 + (shift - 1) u) — the timestep shift of the flow schedules — and timesteps =
    1000 sigma.  Returns (sigma [B], timesteps [B]), fp32 on ``device`` (default: the generator's device, else "cuda");
    nothing is read back to the host."""
    B, lo, hi, shift = int(B), float(lo), float(hi), float(shift)
    if B < 1:
        raise ValueError(f"dmd_sigmas: B = {B} >= 1 expected")
    if not 0.0 < lo <= hi < 1.0:
        raise ValueError(f"dmd_sigmas: 0 < lo <= hi < 1 expected, got lo = {lo}, hi = {hi}")
    if shift <= 0.0:
        raise ValueError(f"dmd_sigmas: shift = {shift} > 0 expected")
    if device is None:
        device = generator.device if generator is not None else "cuda"
    u = lo + (hi - lo) * torch.rand(B, dtype=torch.float32, device=device, generator=generator)
    sigma = shift * u / (1.0 + (shift - 1.0) * u)
    return sigma, 1000.0 * sigma


def _score_inputs(who, clips, sigma, timesteps, eps):
    """The shared argument rules of ``dmd_loss`` and ``critic_loss`` (shapes only: nothing touches a device).  Returns the
    clips as a list and B."""
    clips = list(clips)
    if not clips or any(not isinstance(c, torch.Tensor) or c.dim() != 4 for c in clips) or \
            len({tuple(c.shape) for c in clips}) != 1:
        raise ValueError(f"{who}: clips is a list of tensors [C, F, H, W] of one shape")
    B = len(clips)
    for name, v in (("sigma", sigma), ("timesteps", timesteps)):
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != (B,):
            raise ValueError(f"{who}: {name} of shape [{B}] expected (one level per clip), got "
                             f"{tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    if eps is not None and tuple(eps.shape) != (B,) + tuple(clips[0].shape):
        raise ValueError(f"{who}: eps of shape {[B] + list(clips[0].shape)} expected, got {list(eps.shape)}")
    return clips, B


def _awaits_backward(model):
    return any(not o.__dict__.get("bwd_done", False) for o in model.__dict__.get("_omh_live_states", ()))


def _noised(clips, sigma, eps, generator):
    """(x [B, C, F, H, W] fp32 stacked, attached as the clips are; eps; x_t = ops.flow_noise(x, eps, sigma), graph-free;
    sigma fp32 on x's device)."""
    from . import ops
    x = torch.stack(clips).float().contiguous()
    sigma = sigma.detach().to(device=x.device, dtype=torch.float32).contiguous()
    with torch.no_grad():
        if eps is None:
            eps = torch.randn(x.shape, dtype=torch.float32, device=x.device, generator=generator)
        eps = eps.detach().to(device=x.device, dtype=torch.float32).contiguous()
        x_t = ops.flow_noise(x, eps, sigma)
    return x, eps, x_t, sigma


def _seq_len(model, clip):
    pt, ph, pw = model.patch_size
    return (clip.shape[1] // pt) * (clip.shape[2] // ph) * (clip.shape[3] // pw)


def dmd_loss(clips, teacher, critic, context, context_null=None, *, sigma, timesteps, guide_scale=3.0, eps=None,
             generator=None):
    """The distribution-matching (DMD) loss of a self-forcing generator step, DMD2 / Self-Forcing form in the flow
    parameterisation.  ``clips``: the list ``self_forcing_rollout`` returns — B clips fp32 [C, F, H, W] of one shape,
    attached to the student's graph; ``teacher``: a frozen bidirectional ``WanModel``; ``critic``: the trainable one that
    tracks the student's distribution; ``context`` / ``context_null``: what ``WanModel.forward`` takes for B clips;
    ``sigma`` / ``timesteps``: [B] (``dmd_sigmas``); ``eps``: the noise [B, C, F, H, W] (default: ``torch.randn`` with
    ``generator``).  With x the stacked clips:

        x_t    = (1 - sigma_b) x + sigma_b eps                    ``ops.flow_noise``, under ``no_grad``
        v_real = v_u + guide_scale (v_c - v_u)                    ``teacher.forward_cfg_pair(x_t, t, context, context_null,
                                                                  seq_len)``; without ``context_null`` v_real =
                                                                  ``teacher.forward(x_t, t, context, seq_len)``
        v_fake = ``critic.forward(x_t, t, context, seq_len)``
        n_b    = mean over the clip of |(x - x_t) + sigma_b v_real|
        grad   = nan_to_num(sigma_b (v_real - v_fake) / n_b)
        loss   = 0.5 * mean(grad^2),   d loss / d x = grad / x.numel()        ``ops.dmd_loss``

    Both score models run under ``no_grad``: nothing flows into them, the critic's training flag and the teacher's
    ``set_causal_chunks`` setting are left alone (the teacher is the caller's object, and bidirectional as the caller
    made it).  Returns the fp64 scalar loss, attached to ``clips``.

    ValueError: clips of different shapes, a ``sigma`` or ``timesteps`` that is not [B], an ``eps`` of another shape.
    RuntimeError: a ``teacher`` or ``critic`` with forwards that still await their ``backward()`` — the student itself:
    its causal setting and its set of live forwards would be disturbed; pass separate models.

    One training iteration, the optimisers and their alternation being the caller's:

        # generator step
        clips = causal.self_forcing_rollout(student, noise, context, frames_per_chunk=3, sigmas=..., timesteps=...,
                                            exit_step=...)
        sigma, t = causal.dmd_sigmas(len(clips))
        causal.dmd_loss(clips, teacher, critic, context, context_null, sigma=sigma, timesteps=t).backward()
        # critic step
        with torch.no_grad():
            clips = causal.self_forcing_rollout(student, noise, context, ...)
        sigma, t = causal.dmd_sigmas(len(clips))
        causal.critic_loss(critic, clips, context, sigma=sigma, timesteps=t).backward()"""
    from . import ops
    clips, B = _score_inputs("dmd_loss", clips, sigma, timesteps, eps)
    for name, m in (("teacher", teacher), ("critic", critic)):
        if _awaits_backward(m):
            raise RuntimeError(f"dmd_loss: {name} has forwards that await their backward() — the student itself?  Its causal "
                               f"setting and its live forwards would be disturbed: pass a separate model")
    x, eps, x_t, sigma = _noised(clips, sigma, eps, generator)
    seq_len = _seq_len(teacher, clips[0])
    with torch.no_grad():
        t = timesteps.detach().to(device=x.device, dtype=torch.float32)
        xs = list(x_t.unbind(0))
        if context_null is not None:
            v_c, v_u = teacher.forward_cfg_pair(xs, t, context, context_null, seq_len)
            v_c, v_u = torch.stack(v_c).float().contiguous(), torch.stack(v_u).float().contiguous()
        else:
            v_c, v_u = torch.stack(teacher.forward(xs, t, context, seq_len)).float().contiguous(), None
        v_f = torch.stack(critic.forward(xs, t, context, seq_len)).float().contiguous()
    return ops.dmd_loss(x, x_t, v_c, v_u, v_f, sigma, guide_scale)


def critic_loss(critic, clips, context, *, sigma, timesteps, eps=None, generator=None):
    """The critic's flow-matching loss on generated clips (the critic step of DMD): the clips are DETACHED (their graph,
    if they have one, is neither read nor written), x_t = ``ops.flow_noise(x, eps, sigma)`` with ``eps`` given or drawn
    by ``torch.randn(generator=)``, ``critic.forward(x_t, timesteps, context, seq_len)`` on the training path, and the mean
    squared error against eps - x in plain torch on the model's outputs, as ``forcing_loss`` has it.  ``sigma`` /
    ``timesteps``: [B] (ValueError otherwise, as for clips of different shapes).  Gradients reach the critic alone."""
    clips, B = _score_inputs("critic_loss", clips, sigma, timesteps, eps)
    x, eps, x_t, sigma = _noised([c.detach() for c in clips], sigma, eps, generator)
    t = timesteps.detach().to(device=x.device, dtype=torch.float32)
    out = critic.forward(list(x_t.unbind(0)), t, context, _seq_len(critic, clips[0]))
    target = eps - x
    return torch.stack([(o.float() - v.to(o.device).float()).square().mean() for o, v in zip(out, target)]).mean()
