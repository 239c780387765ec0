"""Chunk-causal attention on the host side: the rule as a dense mask, the per-layer K / V cache of a rollout, and the
rollout loop itself.

The rule (include/omh.h, ``omh_chunk_causal``): with ``chunk`` = C >= 1 tokens, ``left_chunks`` = W (< 0: unbounded) and
``q_offset`` = P >= 0 (the position of query row 0 on the key axis), query i sees key j iff

    i < qlen  and  j < klen  and  j // C <= (P + i) // C  and  (W < 0 or j // C >= (P + i) // C - W).

Positions are absolute (no bottom-right shift).  ``WanModel.set_causal_chunks`` runs every self-attention of a forward
under it with C = a group of latent frames; ``WanModel.forward_chunk`` produces the same clip frame group by frame group
against a ``KVCache``, and ``sample`` denoises a clip that way.
"""
import torch

__all__ = ["chunk_causal_visible", "KVCache", "sample"]


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


class KVCache:
    """The self-attention keys and values of the tokens a rollout has produced so far, per block of ``model``:

    ``k[l]``   bf16 [batch, cap, dim]: the keys after norm and RoPE, token-major (what the attention kernel reads);
    ``vt[l]``  bf16 [batch, dim, pitch], pitch = roundup(cap, 64): V transposed, zero-initialised (the kernel multiplies
               the pad columns by P = 0 and needs them finite);
    ``length`` tokens committed so far (a host integer; ``WanModel.forward_chunk(commit=True)`` advances it).

    ``cap`` = ``max_tokens``; nothing is evicted.  Rows / columns at or past ``length`` are scratch."""

    def __init__(self, model, batch, max_tokens, device):
        batch, cap = int(batch), int(max_tokens)
        if batch < 1 or cap < 1:
            raise ValueError(f"KVCache: batch = {batch} and max_tokens = {cap} must be positive")
        self.model_id = id(model)
        self.batch, self.cap, self.dim = batch, cap, int(model.dim)
        self.pitch = (cap + 63) // 64 * 64
        self.length = 0
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
        self.length = n_tokens

    def reset(self):
        self.length = 0


@torch.no_grad()
def sample(model, noise, context, context_null, *, frames_per_chunk, left_chunks=-1, make_scheduler, guide_scale,
           context_t=0.0):
    """Denoise one clip chunk by chunk.  ``noise``: the initial latents [C, F, H, W] of the clip; ``context`` /
    ``context_null``: what ``WanModel.forward`` takes for a batch of one (a list with one [L, text_dim] tensor, or a
    ``ContextState``).  For every group of ``frames_per_chunk`` latent frames (the last one may be shorter):

    1. a fresh scheduler from ``make_scheduler()`` (timesteps already set);
    2. its sampling steps — ``forward_chunk(..., commit=False)`` on two caches, conditional and unconditional, then
       ``scheduler.step_cfg`` with ``guide_scale``;
    3. one ``commit=True`` pass of the finished chunk at t = ``context_t`` on both caches, so that the later chunks
       attend to its keys and values (skipped behind the last chunk: nothing reads them).

    A chunk sees itself and the ``left_chunks`` chunks before it (< 0: all of them).  The model's own
    ``set_causal_chunks`` setting is restored on the way out.  Returns the latents of the whole clip, fp32 [C, F, H, W]."""
    fpc = int(frames_per_chunk)
    if noise.dim() != 4:
        raise ValueError(f"sample: noise [C, F, H, W] of one clip expected, got {tuple(noise.shape)}")
    F = noise.shape[1]
    pt, ph, pw = model.patch_size
    tokens = (F // pt) * (noise.shape[2] // ph) * (noise.shape[3] // pw)
    prev = getattr(model, "_causal_chunks", None)
    model.set_causal_chunks(fpc, left_chunks)
    try:
        caches = (KVCache(model, 1, tokens, noise.device), KVCache(model, 1, tokens, noise.device))
        t_ctx = torch.full((1,), float(context_t), device=noise.device)
        done = []
        for f0 in range(0, F, fpc):
            lat = noise[:, f0:f0 + fpc].float().contiguous()
            scheduler = make_scheduler()
            for t in scheduler.timesteps:
                tt = torch.stack([t])
                cond = model.forward_chunk([lat], tt, context, caches[0], commit=False)[0]
                uncond = model.forward_chunk([lat], tt, context_null, caches[1], commit=False)[0]
                lat = scheduler.step_cfg(cond, uncond, guide_scale, lat)
            done.append(lat)
            if f0 + fpc < F:
                model.forward_chunk([lat], t_ctx, context, caches[0], commit=True)
                model.forward_chunk([lat], t_ctx, context_null, caches[1], commit=True)
        return torch.cat(done, dim=1)
    finally:
        model._causal_chunks = prev
