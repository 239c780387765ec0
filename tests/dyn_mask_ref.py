"""The selection rule of the dynamic block masks (include/omh.h, "Block masks chosen from q and k") restated in torch, in
a dtype of the caller's choice so that fp32 and fp64 runs share one text — the reference of tests/test_block_policy_host.py
and tests/test_gpu_block_select.py — and the deterministic structured operands those tests use."""
import math

import torch

BLOCK = 128
DELTA = 1e-4                 # the margin of a "decided" row
SCALE = BLOCK ** -0.5 * math.log2(math.e)


def live_counts(L, lens, B):
    """c[b, I] = clamp(len_b - 128 I, 0, 128), int64 [B, nb]."""
    nb = (L + BLOCK - 1) // BLOCK
    lens = torch.full((B,), L, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64).clamp(0, L)
    return (lens[:, None] - BLOCK * torch.arange(nb)[None, :]).clamp(0, BLOCK)


def pool(x, lens=None, dtype=torch.float64):
    """x bf16 [B, L, H, 128] -> (mean [B, H, nb, 128], coherence [B, H, nb], live counts [B, nb]) in ``dtype``."""
    B, L, H, D = x.shape
    nb = (L + BLOCK - 1) // BLOCK
    c = live_counts(L, lens, B)
    xp = torch.zeros(B, nb * BLOCK, H, D, dtype=dtype)
    xp[:, :L] = x.to(dtype)
    row = torch.arange(nb * BLOCK).view(nb, BLOCK)
    live = (row[None] - BLOCK * torch.arange(nb)[None, :, None]) < c[:, :, None]                # [B, nb, 128]
    xb = xp.view(B, nb, BLOCK, H, D) * live[..., None, None].to(dtype)
    cf = c.to(dtype).clamp(min=1)[:, :, None, None]
    mean = (xb.sum(2) / cf).permute(0, 2, 1, 3).contiguous()                                    # [B, H, nb, 128]
    mean = mean * (c > 0).to(dtype)[:, None, :, None]
    den = ((xb * xb).sum((2, 4)) / cf[..., 0]).permute(0, 2, 1)                                # [B, H, nb]
    num = (mean * mean).sum(-1)
    coh = torch.where(den > 0, num / den.clamp(min=torch.finfo(dtype).tiny), torch.ones_like(den))
    return mean, coh.clamp(max=1.0), c


def select(q, k, mass, q_lens=None, k_lens=None, score_scale=SCALE, min_coherence=0.0, dtype=torch.float64):
    """The per-sample selections of the rule, without ``always``:
    keep bool [B, H, nQb, nKb], p [B, H, nQb, nKb] (0 in dead rows / columns), decided bool [B, H, nQb] (dead rows count as
    decided), and the pooled (q_mean, q_coh, cq), (k_mean, k_coh, ck)."""
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    qm, qcoh, cq = pool(q, q_lens, dtype)
    km, kcoh, ck = pool(k, k_lens, dtype)
    live_q, live_k = cq > 0, ck > 0                                                             # [B, nQb], [B, nKb]
    s = score_scale * torch.einsum("bhid,bhjd->bhij", qm, km) + torch.log2(ck.to(dtype).clamp(min=1))[:, None, None, :]
    s = s.masked_fill(~live_k[:, None, None, :], float("-inf"))
    s = s - s.amax(-1, keepdim=True).nan_to_num(neginf=0.0)
    e = torch.exp2(s)
    p = e / e.sum(-1, keepdim=True).clamp(min=torch.finfo(dtype).tiny)
    p = p * live_q[:, None, :, None].to(dtype)
    # mass_ge[.., J] = sum of the p that are >= p[J] (ties together: a function of the values, not of an order)
    ps, order = torch.sort(p, dim=-1, descending=True)
    cs = torch.cumsum(ps, -1)
    last = torch.searchsorted((-ps).contiguous(), (-ps).contiguous(), right=True) - 1            # end of each run of ties
    mass_ge = torch.empty_like(p).scatter_(-1, order, cs.gather(-1, last))
    ok = (mass_ge >= mass) & live_k[:, None, None, :]
    theta = torch.where(ok, p, torch.zeros_like(p)).amax(-1, keepdim=True)                      # 0: nothing reaches the mass
    if mass >= 1.0:
        theta = torch.zeros_like(theta)                                                         # every live block
    live2 = live_q[:, None, :, None] & live_k[:, None, None, :]
    keep = (p >= theta) & live2
    # decided rows (in this dtype; the tests read it from the fp64 run)
    at = torch.where(p >= theta, p, torch.zeros_like(p)).sum(-1)
    before = torch.where(p > theta, p, torch.zeros_like(p)).sum(-1)
    nxt = torch.where((p < theta) & live2, p, torch.zeros_like(p)).amax(-1)
    th = theta[..., 0]
    decided = (at > mass + DELTA) & (before < mass - DELTA) & (nxt < th * (1 - DELTA))
    if mass >= 1.0:
        decided = torch.ones_like(decided)
    decided = decided | ~live_q[:, None, :]
    if min_coherence > 0:
        keep = keep | ((qcoh < min_coherence)[..., None] & live2) | ((kcoh < min_coherence)[:, :, None, :] & live2)
    return keep, p, decided, (qm, qcoh, cq), (km, kcoh, ck)


def union(keep, always=None):
    """The mask of a call: OR over the samples, OR ``always`` ([nQb, nKb] or [H, nQb, nKb]) -> bool [H, nQb, nKb]."""
    m = keep.any(0)
    if always is not None:
        m = m | (always if always.dim() == 3 else always[None])
    return m


def check_against(dev_mask, q, k, mass, q_lens=None, k_lens=None, always=None, min_coherence=0.0, score_scale=SCALE):
    """Hold a device-built mask bool [H, nQb, nKb] (CPU copy) to the fp64 rule.  On rows (h, I) whose every sample is
    decided the mask must equal the reference exactly; on the others each live sample's kept set must hold fp64 mass
    >= mass - DELTA.  Returns (undecided live rows, live rows); asserts the rest."""
    keep, p, decided, (_, _, cq), _ = select(q, k, mass, q_lens, k_lens, score_scale, min_coherence, torch.float64)
    ref = union(keep, always)
    row_decided = decided.all(0)                                                                # [H, nQb]
    bad = (dev_mask != ref).any(-1) & row_decided
    assert not bad.any(), f"{int(bad.sum())} decided rows differ from the fp64 rule, first {bad.nonzero()[0].tolist()}"
    held = (p * dev_mask[None].to(p.dtype)).sum(-1)                                             # [B, H, nQb]
    live_q = (cq > 0)[:, None, :].expand_as(held)
    short = live_q & (held < mass - DELTA)
    assert not short.any(), f"{int(short.sum())} rows keep less than mass - delta, min {float(held[live_q].min()):.6f}"
    return int((~decided & live_q).sum()), int(live_q.sum())


def structured_qk(B, F, H, seed, L=None):
    """Deterministic lattice-structured operands: tokens on an (F, 30, 52) lattice in frame-major order, 20 spatial
    groups (group = (h // 6) * 4 + w // 13); per head centre[group] ~ N(0, 1), frame[f] ~ 0.5 N(0, 1), base = centre +
    frame, q = 1.5 base + 0.7 N(0, 1) and k likewise with its own noise, rounded to bf16.  Returns q, k [B, L, H, 128]
    (L defaults to F * 1560; a shorter L truncates the lattice, a longer one leaves zeros)."""
    g = torch.Generator().manual_seed(seed)
    n = F * 30 * 52
    L = n if L is None else L
    tok = torch.arange(n)
    f, hh, ww = tok // 1560, (tok // 52) % 30, tok % 52
    group = (hh // 6) * 4 + ww // 13
    q = torch.zeros(B, L, H, BLOCK, dtype=torch.bfloat16)
    k = torch.zeros(B, L, H, BLOCK, dtype=torch.bfloat16)
    m = min(n, L)
    for b in range(B):
        centre = torch.randn(H, 20, BLOCK, generator=g)
        frame = 0.5 * torch.randn(H, F, BLOCK, generator=g)
        base = (centre[:, group] + frame[:, f]).permute(1, 0, 2)[:m]                            # [m, H, 128]
        q[b, :m] = (1.5 * base + 0.7 * torch.randn(m, H, BLOCK, generator=g)).to(torch.bfloat16)
        k[b, :m] = (1.5 * base + 0.7 * torch.randn(m, H, BLOCK, generator=g)).to(torch.bfloat16)
    return q, k


# (B, frames, H, seed, L, lens, masses): the select cases of tests/test_gpu_block_select.py, checked on the CPU by
# tests/test_block_policy_host.py
CASES = {
    "one_clip_74_blocks": (1, 6, 12, 11, None, None, (0.5, 0.9)),
    "batch_union_lens": (2, 1, 12, 12, None, [1560, 1000], (0.5, 0.9)),
    "300_blocks": (1, 25, 2, 13, 38400, [38333], (0.5,)),
}
UNDECIDED_CAP = 0.02


def case_operands(name):
    B, F, H, seed, L, lens, masses = CASES[name]
    q, k = structured_qk(B, F, H, seed, L)
    if lens is not None and L is not None:
        q[:, lens[0]:] = 0                                     # the tail past the live rows is left as zeros
        k[:, lens[0]:] = 0
    return q, k, lens, masses
