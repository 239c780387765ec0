"""Coded inputs, boolean visibility, float64 references, per-element bounds and fp32 restatements for the attention
entries of include/omh.h (csrc/attention.hip, attention_w64.hip, attention_bwd.hip, attention_bwd2.hip).  Test
infrastructure, not a test module; plain torch, importable without a GPU.  The canvases and the bf16 helpers are those of
tests/gemm_exact_ref.py.

The construction.  Randn operands give near-uniform softmax rows: an output element is a mean over all keys, and one wrong
key moves it by 1 / Lk of itself.  Here the softmax has almost no freedom.  Keys are rows of the 128 x 128 Sylvester
Hadamard matrix Hd (+-1, orthogonal, exact in bf16): k[b, j, h] = Hd[kc[b, h, j]] with a code kc per key; a query is
c Hd[code], so its score is 128 c against the keys of its code and exactly 0 against every other key.  c is chosen so
that the gap is 32 log2 units (q_prescaled: c = 1/4, exactly 32; else c = 2 with scale = 128^-1/2, 32.6): the keys of
another code weigh 2^-32.  A FLAT row's output is the plain mean of v over its visible keys of its code.  v holds
integers in [-32, 32], drawn per (b, j, h, d), so every key, head and sample has its own row; keys at or past k_lens and
the pad columns of vt hold 2^14 (finite, as the contract asks; never NaN).
Aiming: row i takes the code of one of its own mask-edge keys, rotating with i % 4 through the key just below a run of
visible keys, the run's first key, its last key and the key just above it (the runs of a row in turn, (i // 4) % runs).
An aimed key that is masked and leaks in enters at full weight; an aimed key that is visible and gets dropped takes the
row's target away.  The codes of aimed masked keys are fixed so that the row still has a visible key of that code (the
leak then changes a mean, it does not create one); rows where that fails see all their keys at score 0 and are UNIFORM
rows: they check the count of visible keys.  One row in eight is GRADED: q = c Hd[a] + c2 Hd[a'], the second code about
2 log2 units lower (P = {4/5, 1/5} / n): exp2, the running-max rescale and lse with non-trivial weights.

The reference is float64 softmax attention on the bf16 operands under a dense boolean visibility [B, H, Lq, Lk], built
per mask kind from the rules as include/omh.h words them (``visibility``; ``visibility_slow`` states each rule once more,
per (i, j), for the host test).  The backward reference follows omh.h's formulas with the lse and o32 THE KERNEL IS FED
(the float64 forward rounded to fp32, or the forward kernel's own in the chained cases): P = exp(s - lse),
delta = rowsum(dO o32), dP = dO V^T, dS = P (dP - delta), dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q.

Bounds, per element, delta = kappa S with S the condition sum of the output (the same formula over magnitudes):
  forward          S    = sum_j P_ij |v_jd|
  dv               S_dv = sum_i P_ij |dO_id|
  dq               S_dq = scale sum_j P_ij (sum_d |dO_id| |v_jd| + sum_d |dO_id| |O_id|) |k_jd|
  dk               S_dk = the same summed over i with |q_id|
  delta            S_dl = sum_d |dO_id| |O_id|      (the kernels without o32: delta = sum_j P_ij dP_ij, S = sum_j P_ij sum_d |dO_id| |v_jd|)
  lse              S_l  = max(1, |lse|)
  bf16 outputs     |got - ref| <= 0.5 ulp_bf16(|ref| + delta) + delta
  fp32 outputs     |got - ref| <= delta
Forward rows come in two classes.  FLAT rows (not graded, at least one visible key of their code): P is 1 for every target
before the rounding to bf16, so only the fp32 accumulation, the reciprocal and one product remain: KAPPA["o_flat"].
GRADED and UNIFORM rows: P is rounded to bf16 before the MFMA: KAPPA["o"].  In the backward P = 1 / n is rounded to bf16
on every row (and so is dS), so each backward output has one kappa.
Every kappa is four times the worst ratio |restatement - ref| / S of the fp32 restatements below (``restate_forward``,
``restate_backward``) over the GPU test's own cases, rounded up to a power of two; tests/test_attn_exact_host.py
measures the ratios again and asserts that KAPPA still covers them four times.  Never set from a GPU kernel's output."""
import collections
import math
from types import SimpleNamespace as NS

import torch

from gemm_exact_ref import Canvas, rne_bf16, ulp_bf16  # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
D = 128
POISON = 2.0 ** 14
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
SCALE = float(torch.tensor(128 ** -0.5, dtype=F32))
UNIT = float(torch.tensor(SCALE, dtype=F32) * torch.tensor(LOG2E, dtype=F32))      # the kernels' fp32 scale * log2(e)
GAP_MIN = 32.0

# measured by tests/test_attn_exact_host.py, worst |restatement - ref| / S over the cases of this module (its ``[kappa]`` line):
#   o_flat 1.600e-07 (over the own code's share, the tails at kappa_o / 4)   o 1.753e-03   lse 9.172e-08
#   o_flat_split 8.947e-07 (the split tail: slabs weighted by exp(lse_s - max lse), not by a power of two)
#   dq 3.167e-04   dk 1.004e-03   dv 3.676e-03   delta 6.492e-08   delta_p 1.948e-07 (sum_j P dP of the kernels without o32)
# times four, rounded up to a power of two.  o32 takes the kappas of o; bf16 gradients those of the fp32 ones (plus the
# half ulp of their one rounding).
KAPPA = {"o_flat": 2.0 ** -20, "o_flat_split": 2.0 ** -18, "o": 2.0 ** -7, "lse": 2.0 ** -21, "dq": 2.0 ** -9, "dk": 2.0 ** -7, "dv": 2.0 ** -6,
         "delta": 2.0 ** -21, "delta_p": 2.0 ** -20}
MEASURED = {"o_flat": 1.600e-07, "o_flat_split": 8.947e-07, "o": 1.753e-03, "lse": 9.172e-08, "dq": 3.167e-04, "dk": 1.004e-03,
            "dv": 3.676e-03, "delta": 6.492e-08, "delta_p": 1.948e-07}

WORST = collections.defaultdict(float)
COUNTS = collections.Counter()


def hadamard(n=D):
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


HD = hadamard()


def _up(x, m):
    return (x + m - 1) // m * m


def _gen(*seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(hash(tuple(int(s) for s in seed)) & 0x7FFFFFFF)
    return g


def bf(x):
    return x.to(BF16).to(x.dtype)


# ----------------------------------------------------------------------------------------------------------------------
# visibility, per mask kind, from the wording of include/omh.h
# ----------------------------------------------------------------------------------------------------------------------
def _lens(lens, B, L):
    """clamp(lens[b], 0, L), L where lens is None"""
    return [L] * B if lens is None else [min(max(int(x), 0), L) for x in lens]


def mask_full():
    return NS(kind="full")


def mask_band(left, right):
    return NS(kind="band", left=int(left), right=int(right))


def mask_chunk(chunk, left_chunks, q_offset):
    return NS(kind="chunk", chunk=int(chunk), left_chunks=int(left_chunks), q_offset=int(q_offset))


def mask_interval(vis, group, k_group=None, runs=2):
    """vis [q_groups, k_groups] bool; k_group: the rectangular form; runs 3: the three-run entries"""
    return NS(kind="interval", vis=torch.as_tensor(vis, dtype=torch.bool), group=int(group), k_group=k_group, runs=runs)


def mask_block(m):
    """m [heads, nQb, nKb] bool over 128 x 128 blocks, heads 1 or H"""
    m = torch.as_tensor(m, dtype=torch.bool)
    return NS(kind="block", m=m if m.dim() == 3 else m[None])


def visibility(mask, B, H, Lq, Lk, q_lens=None, k_lens=None):
    """bool [B, H, Lq, Lk]: query i of sample b, head h sees key j"""
    ql, kl = _lens(q_lens, B, Lq), _lens(k_lens, B, Lk)
    i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
    out = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
    for b in range(B):
        qlen, klen = ql[b], kl[b]
        ok = (i < qlen) & (j < klen)
        if mask.kind == "band":             # bottom-right aligned: i + klen - qlen - left <= j <= i + klen - qlen + right
            c = i + (klen - (Lq if getattr(mask, "shift_from_Lq", False) else qlen))      # (shift_from_Lq: a planted defect)
            if mask.left >= 0:
                ok = ok & (j >= c - mask.left)
            if mask.right >= 0:
                ok = ok & (j <= c + mask.right)
        elif mask.kind == "chunk":          # j div C <= (P + i) div C and (W < 0 or j div C >= (P + i) div C - W)
            ci, cj = (mask.q_offset + i) // mask.chunk, j // mask.chunk
            ok = ok & (cj <= ci)
            if mask.left_chunks >= 0:
                ok = ok & (cj >= ci - mask.left_chunks)
        elif mask.kind == "interval":       # vis[i div group][j div k_group]
            kg = mask.group if mask.k_group is None else mask.k_group
            ok = ok & mask.vis[(i // mask.group).expand(Lq, Lk), (j // kg).expand(Lq, Lk)]
        if mask.kind == "block":            # M[h][i / 128][j / 128]
            for h in range(H):
                m = mask.m[0 if mask.m.shape[0] == 1 else h]
                out[b, h] = ok & m[(i // 128).expand(Lq, Lk), (j // 128).expand(Lq, Lk)]
        else:
            out[b] = ok[None]
    return out


def visibility_slow(mask, B, H, Lq, Lk, q_lens=None, k_lens=None):
    """the same, one (i, j) at a time: an independent statement for the host test"""
    out = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
    for b in range(B):
        qlen = Lq if q_lens is None else min(max(int(q_lens[b]), 0), Lq)
        klen = Lk if k_lens is None else min(max(int(k_lens[b]), 0), Lk)
        for h in range(H):
            for i in range(qlen):
                for j in range(klen):
                    if mask.kind == "full":
                        see = True
                    elif mask.kind == "band":
                        lo = i + klen - qlen - mask.left if mask.left >= 0 else 0
                        hi = i + klen - qlen + mask.right if mask.right >= 0 else klen
                        see = lo <= j <= hi
                    elif mask.kind == "chunk":
                        I = (mask.q_offset + i) // mask.chunk
                        lo = 0 if mask.left_chunks < 0 else max(0, (I - mask.left_chunks) * mask.chunk)
                        see = lo <= j < (I + 1) * mask.chunk
                    elif mask.kind == "interval":
                        kg = mask.group if mask.k_group is None else mask.k_group
                        see = bool(mask.vis[i // mask.group][j // kg])
                    else:
                        see = bool(mask.m[0 if mask.m.shape[0] == 1 else h][i // 128][j // 128])
                    out[b, h, i, j] = see
    return out


# ----------------------------------------------------------------------------------------------------------------------
# coded inputs
# ----------------------------------------------------------------------------------------------------------------------
def _run_edges(vis):
    """vis [Lq, Lk] -> (starts, ends) bool [Lq, Lk]: first and last key of every run of visible keys"""
    pad = torch.zeros(vis.shape[0], 1, dtype=torch.bool)
    prev, nxt = torch.cat([pad, vis[:, :-1]], 1), torch.cat([vis[:, 1:], pad], 1)
    return vis & ~prev, vis & ~nxt


def aimed_keys(vis):
    """vis [Lq, Lk] -> the key each row aims at [Lq] (i % Lk for a row that sees nothing), and for the graded rows' second
    code the key two steps further in the rotation"""
    Lq, Lk = vis.shape
    starts, ends = _run_edges(vis)
    nruns = starts.sum(-1)
    i = torch.arange(Lq)
    r = (i // 4) % nruns.clamp_min(1)
    first = ((starts.cumsum(-1) == (r + 1)[:, None]) & starts).int().argmax(-1)
    last = ((ends.cumsum(-1) == (r + 1)[:, None]) & ends).int().argmax(-1)

    def pick(rot):
        e = torch.where(rot == 0, first - 1, torch.where(rot == 1, first, torch.where(rot == 2, last, last + 1)))
        return torch.where(nruns > 0, e.clamp(0, Lk - 1), i % Lk)
    return pick(i % 4), pick((i + 2) % 4)


def graded_rows(Lq):
    """one row in eight, its place in the group of eight rotating so that every i % 4 occurs"""
    i = torch.arange(Lq)
    return (i % 8) == ((i // 8) * 3) % 8


def build(cs):
    """The operands of one case.  ``cs``: dict(B, H, Lq, Lk[, q_lens][, k_lens][, mask][, prescaled][, seed][, codes]).
    Returns a namespace with q [B, Lq, H, 128], k, v [B, Lk, H, 128], vt [B, H * 128, ldv], dout [B, Lq, H, 128] (bf16),
    the visibility, the codes, and the row classes (flat / graded / uniform / dead, bool [B, H, Lq])."""
    B, H, Lq, Lk = cs["B"], cs["H"], cs["Lq"], cs["Lk"]
    mask = cs.get("mask") or mask_full()
    pre = bool(cs.get("prescaled", True))
    g = _gen(cs.get("seed", 0), B, H, Lq, Lk)
    c = NS(B=B, H=H, Lq=Lq, Lk=Lk, mask=mask, prescaled=pre, q_lens=cs.get("q_lens"), k_lens=cs.get("k_lens"), cs=cs,
           scale=SCALE, ldv=_up(Lk, 64) + 64)
    c.ql, c.kl = _lens(c.q_lens, B, Lq), _lens(c.k_lens, B, Lk)
    c.vis = visibility(mask, B, H, Lq, Lk, c.q_lens, c.k_lens)
    nc = int(cs.get("codes") or min(128, max(1, Lk // 4)))
    kc = torch.randint(0, nc, (B, H, Lk), generator=g)
    aim, aim2 = torch.zeros(B, H, Lq, dtype=torch.long), torch.zeros(B, H, Lq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            v_bh = c.vis[b, h]
            aim[b, h], aim2[b, h] = aimed_keys(v_bh)
            for i in range(Lq):             # an aimed masked key takes the code of one of the row's visible keys
                e = int(aim[b, h, i])
                if v_bh[i, e] or not bool(v_bh[i].any()):
                    continue
                if not bool((v_bh[i] & (kc[b, h] == kc[b, h, e])).any()):
                    seen = v_bh[i].nonzero().flatten()
                    kc[b, h, e] = kc[b, h, seen[(i // 4) % len(seen)]]
    c.kc, c.aim = kc, aim
    c.qc = torch.gather(kc, 2, aim)
    qc2 = torch.gather(kc, 2, aim2)
    c.qc2 = torch.where(qc2 == c.qc, (c.qc + 1) % 128, qc2)
    c.c1, c.c2 = (0.25, 0.25 - 2.0 / 128) if pre else (2.0, 1.875)
    graded = graded_rows(Lq)[None, None].expand(B, H, Lq)
    q = c.c1 * HD[c.qc] + torch.where(graded[..., None], c.c2 * HD[c.qc2], torch.zeros((), dtype=F64))    # [B, H, Lq, D]
    k = HD[kc]                                                                                             # [B, H, Lk, D]
    v = torch.randint(-32, 33, (B, Lk, H, D), generator=g).double()
    for b in range(B):
        v[b, c.kl[b]:] = POISON
    c.q, c.k, c.v = q.permute(0, 2, 1, 3).contiguous().to(BF16), k.permute(0, 2, 1, 3).contiguous().to(BF16), v.to(BF16)
    assert torch.equal(c.q.double(), q.permute(0, 2, 1, 3)) and torch.equal(c.v.double(), v), "operands are not exact in bf16"
    vt = torch.full((B, H * D, c.ldv), POISON, dtype=F64)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    c.vt = vt.to(BF16)
    c.dout = torch.randint(-4, 5, (B, Lq, H, D), generator=g).to(BF16)
    # row classes
    same = (c.kc[:, :, None, :] == c.qc[:, :, :, None]) & c.vis
    live = c.vis.any(-1)
    c.dead = ~live
    c.graded = graded & live
    c.flat = live & ~graded & same.any(-1)
    c.uniform = live & ~graded & ~same.any(-1)
    c.n_targets = same.sum(-1)
    return c


def check_inputs(c, bounded=False):
    """The input conditions of a case (conditions on the inputs, not measurements)."""
    live = int((~c.dead).sum())
    assert int(c.uniform.sum()) * 4 <= max(live, 4), f"{c.cs}: {int(c.uniform.sum())} uniform rows of {live} live ones"
    unit = 1.0 if c.prescaled else UNIT
    s = torch.einsum("bihd,bjhd->bhij", c.q.double(), c.k.double()) * unit
    same = (c.kc[:, :, None, :] == c.qc[:, :, :, None])
    tgt = torch.where(same & c.vis, s, torch.full_like(s, float("nan")))
    oth = torch.where(~same & c.vis, s, torch.full_like(s, -float("inf")))
    f = c.flat
    if bool(f.any()):
        t_hi = torch.nan_to_num(tgt, nan=-float("inf")).amax(-1)[f]
        t_lo = torch.nan_to_num(tgt, nan=float("inf")).amin(-1)[f]
        assert torch.equal(t_hi, t_lo), f"{c.cs}: the targets of a flat row differ in score"
        assert float((t_lo - oth.amax(-1)[f]).min()) >= GAP_MIN, f"{c.cs}: gap below {GAP_MIN} log2 units"
    if bounded:
        assert bound_m(c) <= 48, f"{c.cs}: m = {bound_m(c)} > 48"


def qk_norm2_max(c, q=None):
    """float [B, H, 2]: max over rows of |q_row|^2 and |k_row|^2 of the STORED q and k"""
    q = c.q if q is None else q
    return torch.stack([(q.double() ** 2).sum(-1).amax(1), (c.k.double() ** 2).sum(-1).amax(1)], -1).float()


def bound_m(c, nm=None):
    """ceil(|q|max |k|max (1 + 2^-6)) in the bounded stream's fp32 arithmetic, the largest over (b, h)"""
    nm = qk_norm2_max(c) if nm is None else nm
    qs = torch.tensor(1.0 if c.prescaled else UNIT, dtype=F32)
    return float(torch.ceil(torch.sqrt(nm[..., 0] * nm[..., 1]) * qs * torch.tensor(1.015625, dtype=F32)).max())


# ----------------------------------------------------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------------------------------------------------
def effective_q(c, requant=False):
    """q in log2 units as float64 [B, Lq, H, D]: prescaled as stored; else q * fp32(scale log2 e), re-rounded to bf16 where
    the long-sequence kernel does that (``requant``)"""
    if c.prescaled:
        return c.q.double()
    qs = c.q.float() * torch.tensor(UNIT, dtype=F32)
    return (qs.to(BF16) if requant else qs).double()


def _scores(c, b, h, requant=False):
    return effective_q(c, requant)[b, :, h] @ c.k[b, :, h].double().t()          # log2 units [Lq, Lk]


def reference_forward(c, requant=False):
    """o, S [B, Lq, H, D], lse [B, H, Lq] (natural log, -inf for a row that sees nothing), P [B, H, Lq, Lk]"""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    r = NS(o=torch.zeros(B, Lq, H, D, dtype=F64), S=torch.zeros(B, Lq, H, D, dtype=F64), S_t=torch.zeros(B, Lq, H, D, dtype=F64),
           lse=torch.full((B, H, Lq), -float("inf"), dtype=F64), P=torch.zeros(B, H, Lq, Lk, dtype=F64))
    for b in range(B):
        for h in range(H):
            s = _scores(c, b, h, requant).masked_fill(~c.vis[b, h], -float("inf"))
            mx = s.amax(-1, keepdim=True)
            mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
            e = torch.exp2(s - mx)
            l = e.sum(-1, keepdim=True)
            p = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
            v = c.v[b, :, h].double()
            r.P[b, h], r.o[b, :, h], r.S[b, :, h] = p, p @ v, p @ v.abs()
            r.S_t[b, :, h] = (p * (c.kc[b, h][None, :] == c.qc[b, h][:, None])) @ v.abs()      # the share of the row's own code
            r.lse[b, h] = torch.where(l[:, 0] > 0, (mx[:, 0] + torch.log2(l[:, 0].clamp_min(1e-300))) * math.log(2.0),
                                      torch.full_like(mx[:, 0], -float("inf")))
    return r


def reference_backward(c, lse, o32, requant=False):
    """dq, dk, dv, delta and their condition sums from the lse [B, H, Lq] and o32 [B, Lq, H, D] the kernel is fed (any
    float dtype; rows that see nothing: ignored)"""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    r = NS(dq=torch.zeros(B, Lq, H, D, dtype=F64), dk=torch.zeros(B, Lk, H, D, dtype=F64), dv=torch.zeros(B, Lk, H, D, dtype=F64),
           delta=torch.zeros(B, H, Lq, dtype=F64))
    r.S_dq, r.S_dk, r.S_dv, r.S_delta = (torch.zeros_like(t) for t in (r.dq, r.dk, r.dv, r.delta))
    r.delta_p, r.S_delta_p = torch.zeros_like(r.delta), torch.zeros_like(r.delta)
    kq = c.scale                                                      # dq = scale dS K
    kk = 1.0 / LOG2E if c.prescaled else c.scale                      # dk = dS^T q' / log2(e)  |  scale dS^T q
    for b in range(B):
        for h in range(H):
            vis = c.vis[b, h]
            live = vis.any(-1)
            s = _scores(c, b, h, requant)
            l2 = torch.where(live, lse[b, h].double(), torch.zeros(Lq, dtype=F64)) * LOG2E
            p = torch.where(vis, torch.exp2(s - l2[:, None]), torch.zeros_like(s))
            do = torch.where(live[:, None], c.dout[b, :, h].double(), torch.zeros((), dtype=F64))
            o = torch.where(live[:, None], o32[b, :, h].double(), torch.zeros((), dtype=F64))
            q, k, v = torch.where(live[:, None], c.q[b, :, h].double(), torch.zeros((), dtype=F64)), c.k[b, :, h].double(), \
                torch.where(vis.any(0)[:, None], c.v[b, :, h].double(), torch.zeros((), dtype=F64))
            delta, bsum = (do * o).sum(-1), (do.abs() * o.abs()).sum(-1)
            dp, a = do @ v.t(), do.abs() @ v.abs().t()
            ds, sds = p * (dp - delta[:, None]), p * (a + bsum[:, None])
            r.delta[b, h], r.S_delta[b, h] = delta, bsum
            r.delta_p[b, h], r.S_delta_p[b, h] = (p * dp).sum(-1), (p * a).sum(-1)      # the kernels without o32: sum_j P_ij dP_ij
            r.dv[b, :, h], r.S_dv[b, :, h] = p.t() @ do, p.t() @ do.abs()
            r.dq[b, :, h], r.S_dq[b, :, h] = kq * (ds @ k), kq * (sds @ k.abs())
            r.dk[b, :, h], r.S_dk[b, :, h] = kk * (ds.t() @ q), kk * (sds.t() @ q.abs())
    return r


def analytic_case(B, H, Lq, Lk, k_lens=None):
    """Full attention at sizes where a dense score matrix is too large: codes by formula (every code has Lk / 128 keys), all
    rows flat or graded, q_prescaled.  The fields ``reference_forward`` reads are there too, except the visibility."""
    c = NS(B=B, H=H, Lq=Lq, Lk=Lk, mask=mask_full(), prescaled=True, q_lens=None, k_lens=k_lens, scale=SCALE, ldv=_up(Lk, 64) + 64,
           cs=dict(B=B, H=H, Lq=Lq, Lk=Lk, k_lens=k_lens, analytic=True))
    c.ql, c.kl = _lens(None, B, Lq), _lens(k_lens, B, Lk)
    b, h = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None]
    c.kc = (torch.arange(Lk)[None, None] * 37 + 11 * h + 5 * b) % 128
    c.qc = (torch.arange(Lq)[None, None] * 29 + 3 * h + b) % 128
    c.qc2 = (c.qc + 1 + (torch.arange(Lq)[None, None] % 7)) % 128
    c.c1, c.c2 = 0.25, 0.25 - 2.0 / 128
    c.graded = graded_rows(Lq)[None, None].expand(B, H, Lq) & torch.tensor([k > 0 for k in c.kl])[:, None, None]
    c.dead = torch.tensor([k == 0 for k in c.kl])[:, None, None].expand(B, H, Lq)
    c.flat, c.uniform = ~c.graded & ~c.dead, torch.zeros(B, H, Lq, dtype=torch.bool)
    g = _gen(B, H, Lq, Lk, 9)
    q = c.c1 * HD[c.qc] + torch.where(c.graded[..., None], c.c2 * HD[c.qc2], torch.zeros((), dtype=F64))
    v = torch.randint(-32, 33, (B, Lk, H, D), generator=g).double()
    for bb in range(B):
        v[bb, c.kl[bb]:] = POISON
    c.q, c.k, c.v = q.permute(0, 2, 1, 3).contiguous().to(BF16), HD[c.kc].permute(0, 2, 1, 3).contiguous().to(BF16), v.to(BF16)
    vt = torch.full((B, H * D, c.ldv), POISON, dtype=F64)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    c.vt = vt.to(BF16)
    c.aim = torch.zeros(B, H, Lq, dtype=torch.long)
    return c


def analytic_forward(c):
    """o, S, S_t, lse of an ``analytic_case`` in float64 without a score matrix: per code the sum of v over its live keys; a
    row weighs its own code 1, a graded row's second code 1 / 4, every other key 2^-32 (scores 32, 30 and 0)."""
    B, H, Lq = c.B, c.H, c.Lq
    r = NS(o=torch.zeros(B, Lq, H, D, dtype=F64), S=torch.zeros(B, Lq, H, D, dtype=F64), S_t=torch.zeros(B, Lq, H, D, dtype=F64),
           lse=torch.full((B, H, Lq), -float("inf"), dtype=F64))
    tiny = 2.0 ** -32
    for b in range(B):
        kl = c.kl[b]
        if kl == 0:
            continue
        for h in range(H):
            code, v = c.kc[b, h, :kl], c.v[b, :kl, h].double()
            vc, ac = torch.zeros(128, D, dtype=F64).index_add_(0, code, v), torch.zeros(128, D, dtype=F64).index_add_(0, code, v.abs())
            nc = torch.zeros(128, dtype=F64).index_add_(0, code, torch.ones(kl, dtype=F64))
            a, a2 = c.qc[b, h], c.qc2[b, h]
            w2 = torch.where(c.graded[b, h], 0.25, tiny)[:, None]          # a flat row's second code is one of the others
            den = nc[a][:, None] + w2 * nc[a2][:, None] + tiny * (kl - nc[a] - nc[a2])[:, None]
            r.o[b, :, h] = (vc[a] + w2 * vc[a2] + tiny * (vc.sum(0)[None] - vc[a] - vc[a2])) / den
            r.S[b, :, h] = (ac[a] + w2 * ac[a2] + tiny * (ac.sum(0)[None] - ac[a] - ac[a2])) / den
            r.S_t[b, :, h] = ac[a] / den
            r.lse[b, h] = (32.0 + torch.log2(den[:, 0])) * math.log(2.0)
    return r


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the kernels' arithmetic (host test: they fix the kappas) with planted defects
# ----------------------------------------------------------------------------------------------------------------------
FWD_DEFECTS = ("leak_at_klen", "drop_visible", "left_plus_1", "right_minus_1", "wrong_shift", "whole_unmasked", "block_late",
               "neighbour_head_v")
BWD_DEFECTS = ("dk_shifted_row", "own_lo_ignored", "leak_at_klen", "drop_visible")


def defect_visibility(c, defect):
    """(the visibility a kernel with this forward defect would use, the rows [B, H, Lq] it may touch) or None where the
    defect does not apply to the case"""
    m, B, H, Lq, Lk = c.mask, c.B, c.H, c.Lq, c.Lk
    vis = c.vis.clone()
    rows = torch.zeros(B, H, Lq, dtype=torch.bool)
    live = ~c.dead
    if defect == "leak_at_klen":            # the key at k_lens[b] enters one row that aims at its code
        for b in range(B):
            e = c.kl[b]
            if 0 < e < Lk:
                cand = (live[b] & (c.qc[b] == c.kc[b, :, e][:, None]) & ~vis[b, :, :, e]).nonzero()
                if len(cand):
                    h, i = (int(x) for x in cand[0])
                    vis[b, h, i, e] = True
                    rows[b, h, i] = True
    elif defect == "drop_visible":          # one row loses the visible key it aims at
        cand = (live & torch.gather(vis, 3, c.aim[..., None])[..., 0] & ~c.graded).nonzero()
        if len(cand):
            b, h, i = (int(x) for x in cand[len(cand) // 2])
            vis[b, h, i, c.aim[b, h, i]] = False
            rows[b, h, i] = True
    elif defect in ("left_plus_1", "right_minus_1", "wrong_shift") and m.kind == "band":
        if defect == "left_plus_1" and m.left >= 0:
            vis = visibility(mask_band(m.left + 1, m.right), B, H, Lq, Lk, c.q_lens, c.k_lens)
        elif defect == "right_minus_1" and m.right >= 1:
            vis = visibility(mask_band(m.left, m.right - 1), B, H, Lq, Lk, c.q_lens, c.k_lens)
        elif defect == "wrong_shift":       # the shift klen - Lq instead of klen - qlen
            if c.q_lens is None or all(x == Lq for x in c.ql):
                return None
            wrong = mask_band(m.left, m.right)
            wrong.shift_from_Lq = True
            vis = visibility(wrong, B, H, Lq, Lk, c.q_lens, c.k_lens)
        else:
            return None
        rows = (vis != c.vis).any(-1)
    elif defect == "whole_unmasked" and m.kind in ("chunk", "interval"):
        # a 64-key tile that the first row of a 128-row workgroup sees whole is run unmasked for all its rows
        for b in range(B):
            for h in range(H):
                for q0 in range(0, Lq, 128):
                    if c.dead[b, h, q0]:
                        continue
                    for t0 in range(0, c.kl[b], 64):
                        t1 = min(t0 + 64, c.kl[b])
                        blk = vis[b, h, q0:min(q0 + 128, c.ql[b]), t0:t1]
                        if bool(c.vis[b, h, q0, t0:t1].all()) and not bool(blk.all()):
                            blk[:] = True
        rows = (vis != c.vis).any(-1)
    elif defect == "block_late" and m.kind == "block":
        # the list cut one block late: the block that holds klen's successor is run although it has no live key ... its
        # keys at or past klen (poison) enter the rows whose list holds that block
        for b in range(B):
            e = c.kl[b]
            if 0 < e < Lk:
                blk = e // 128
                hi = min(Lk, (blk + 1) * 128)
                for h in range(H):
                    mm = m.m[0 if m.m.shape[0] == 1 else h]
                    for i in range(c.ql[b]):
                        if mm[i // 128, blk]:
                            vis[b, h, i, e:hi] = True
        rows = (vis != c.vis).any(-1)
    else:
        return None
    if not bool(rows.any()):
        return None
    return vis, rows


def restate_forward(c, form="short", vis=None, neighbour_head_v=False, requant=False, splits=1):
    """The forward in fp32 as the kernels compute it: 64-key tiles in ascending order, P rounded to bf16 for P V, the row sum
    from the fp32 P, one reciprocal, one product.  form "short": running max with rescale (csrc/attention.hip);
    "lazy": the long-sequence stream (csrc/gen_attn_w64.py), whose running max starts at the first tile's row maximum and
    moves only when a tile's row maximum exceeds it by more than 4 log2 units (p <= 16); "fixed": p = 2^(s - m) against
    the bound m of the bounded stream, no maximum.  splits > 1: the key tiles cut into that many ranges, each normalised on
    its own, combined by out = sum_s w_s o_s / sum_s w_s with w_s = exp(lse_s - max lse) (the flash-decoding reduction of the
    split tails).
    Returns o32 [B, Lq, H, D] fp32 (before the rounding to bf16) and lse [B, H, Lq] fp32."""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    vis = c.vis if vis is None else vis
    o = torch.zeros(B, Lq, H, D, dtype=F32)
    lse = torch.full((B, H, Lq), -float("inf"), dtype=F32)
    unit = torch.tensor(1.0 if (c.prescaled or requant) else UNIT, dtype=F32)
    qe = effective_q(c, True).float() if requant and not c.prescaled else c.q.float()
    m_fixed = torch.tensor(bound_m(c), dtype=F32) if form == "fixed" else None
    ninf = torch.tensor(-float("inf"), dtype=F32)
    for b in range(B):
        for h in range(H):
            hv = (h + 1) % H if neighbour_head_v else h
            q, k, v = qe[b, :, h], c.k[b, :, h].float(), c.v[b, :, hv].float()

            def part(t_lo, t_hi):
                m = torch.full((Lq,), -float("inf"), dtype=F32)
                l, acc = torch.zeros(Lq, dtype=F32), torch.zeros(Lq, D, dtype=F32)
                for t0 in range(64 * t_lo, min(64 * t_hi, c.kl[b]), 64):
                    vt = vis[b, h, :, t0:t0 + 64]
                    if not bool(vt.any()):
                        continue
                    s = torch.where(vt, (q @ k[t0:t0 + 64].t()) * unit, ninf)
                    if form == "fixed":
                        mu = m_fixed.expand(Lq)
                        alpha = torch.ones(Lq, dtype=F32)
                        m = mu
                    else:
                        mn = torch.maximum(m, s.amax(-1))
                        if form == "lazy":
                            mn = torch.where(torch.isinf(m) | (s.amax(-1) > m + 4.0), mn, m)
                        mu = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
                        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mu))
                        m = mn
                    p = torch.exp2(s - mu[:, None])
                    l = l * alpha + p.sum(-1)
                    acc = acc * alpha[:, None] + bf(p) @ v[t0:t0 + 64]
                inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
                mm = torch.where(torch.isinf(m), torch.zeros_like(m), m)
                return acc * inv[:, None], torch.where(l > 0, (mm + torch.log2(l.clamp_min(1e-37))) * torch.tensor(LN2, dtype=F32), ninf)

            tiles = _up(c.kl[b], 64) // 64
            if splits == 1:
                o[b, :, h], lse[b, h] = part(0, tiles)
                continue
            per = (tiles + splits - 1) // splits
            parts = [part(min(sp * per, tiles), min(sp * per + per, tiles)) for sp in range(splits)]
            ls = torch.stack([pl for _, pl in parts])                                   # [splits, Lq]
            mx = ls.amax(0)
            w = torch.where(torch.isinf(ls), torch.zeros_like(ls), torch.exp2((ls - mx[None]) * torch.tensor(LOG2E, dtype=F32)))
            acc, wsum = torch.zeros(Lq, D, dtype=F32), torch.zeros(Lq, dtype=F32)
            for sp in range(splits):
                acc, wsum = acc + w[sp][:, None] * parts[sp][0], wsum + w[sp]
            inv = torch.where(wsum > 0, 1.0 / wsum, torch.zeros_like(wsum))
            o[b, :, h] = acc * inv[:, None]
            lse[b, h] = torch.where(wsum > 0, mx + torch.log(wsum.clamp_min(1e-37)), ninf)
    return o, lse


def restate_backward(c, lse, o32, vis=None, dk_shift=0):
    """The backward in fp32 as the kernels compute it: P = exp2(s - lse log2 e) in fp32, rounded to bf16 for dV = P^T dO;
    dP = dO V^T in fp32; dS = P (dP - delta) in fp32, rounded to bf16 for dQ and dK; fp32 accumulation over 64-position tiles;
    the scales applied to the fp32 sums.  dk_shift: the planted defect (row r of dk holds key r + shift)."""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    vis = c.vis if vis is None else vis
    dq, dk, dv = torch.zeros(B, Lq, H, D, dtype=F32), torch.zeros(B, Lk, H, D, dtype=F32), torch.zeros(B, Lk, H, D, dtype=F32)
    delta, delta_p = torch.zeros(B, H, Lq, dtype=F32), torch.zeros(B, H, Lq, dtype=F32)
    unit = torch.tensor(1.0 if c.prescaled else UNIT, dtype=F32)
    kq = torch.tensor(c.scale, dtype=F32)
    kk = torch.tensor(1.0 / LOG2E if c.prescaled else c.scale, dtype=F32)
    zero = torch.zeros((), dtype=F32)
    for b in range(B):
        for h in range(H):
            vb = vis[b, h]
            live = vb.any(-1)
            q, k, v = torch.where(live[:, None], c.q[b, :, h].float(), zero), c.k[b, :, h].float(), c.v[b, :, h].float()
            do = torch.where(live[:, None], c.dout[b, :, h].float(), zero)
            o = torch.where(live[:, None], o32[b, :, h].float(), zero)
            l2 = torch.where(live, lse[b, h].float(), zero) * torch.tensor(LOG2E, dtype=F32)
            dl = (do * o).sum(-1)
            delta[b, h] = dl
            aq = torch.zeros(Lq, D, dtype=F32)
            for t0 in range(0, c.kl[b], 64):
                kt, vt_, vv = k[t0:t0 + 64], v[t0:t0 + 64], vb[:, t0:t0 + 64]
                if not bool(vv.any()):
                    continue
                vt_ = torch.where(vv.any(0)[:, None], vt_, zero)
                p = torch.where(vv, torch.exp2((q @ kt.t()) * unit - l2[:, None]), zero)
                dp = do @ vt_.t()
                delta_p[b, h] += (p * dp).sum(-1)                    # csrc/attention_bwd.hip: delta from the fp32 P and dP, tile by tile
                ds = bf(p * (dp - dl[:, None]))
                aq = aq + ds @ kt
                dv[b, t0:t0 + 64, h] = bf(p).t() @ do
                dk[b, t0:t0 + 64, h] = (ds.t() @ q) * kk
            dq[b, :, h] = aq * kq
    if dk_shift:
        dk = torch.roll(dk, -dk_shift, 1)
    return NS(dq=dq, dk=dk, dv=dv, delta=delta, delta_p=delta_p)


# ----------------------------------------------------------------------------------------------------------------------
# bounds and the comparison
# ----------------------------------------------------------------------------------------------------------------------
def flat_ok(c, form):
    """Do the flat rows of this stream keep P = 2^-k?  Not where the fixed m (an integer) is subtracted from a score that is
    no integer: q_prescaled = 0 gives 32.75 units once the stream has re-rounded q (1 / 4 Hd gives exactly 32)."""
    return not (form == "fixed" and not c.prescaled)


def fwd_delta(c, ref, flat_ok=True, quarter=False, flat_key="o_flat"):
    """delta of the forward per element [B, Lq, H, D]: kappa_o S on graded and uniform rows; on flat rows kappa_flat on the
    share of the row's own code (P = 1 there) and kappa_o on the 2^-32 tails of the other codes, whose P is rounded to
    bf16 like any other.  flat_ok False: a stream whose flat rows take the graded kappa.  quarter: the host test's bar."""
    f = (0.25 if quarter else 1.0)
    ko, kf = KAPPA["o"] * f, KAPPA[flat_key] * f
    flat = c.flat.permute(0, 2, 1)[..., None] if flat_ok else torch.zeros(c.B, c.Lq, c.H, 1, dtype=torch.bool)
    return torch.where(flat, kf * ref.S_t + ko * (ref.S - ref.S_t), ko * ref.S)


def bound(ref, S, kappa, is_bf16):
    """S: a condition sum with its kappa, or (kappa None) a delta"""
    d = S if kappa is None else kappa * S
    return 0.5 * ulp_bf16(ref.abs() + d) + d if is_bf16 else d


def ratio_to_bound(got, ref, bnd):
    """|got - ref| / bound per element: 0 where they agree exactly (two -inf agree), inf where got is not finite"""
    got = got.double()
    err = (got - ref).abs()
    ratio = torch.where((err == 0) | (got == ref), torch.zeros_like(err), err / bnd.clamp_min(2.0 ** -300))
    return torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))


def describe_row(c, b, h, i):
    """what a failure message says of query row i: aimed key, visible targets, class"""
    vis = c.vis[b, h, i]
    tg = (vis & (c.kc[b, h] == c.qc[b, h, i])).nonzero().flatten().tolist()
    cls = "flat" if c.flat[b, h, i] else "graded" if c.graded[b, h, i] else "uniform" if c.uniform[b, h, i] else "dead"
    seen = vis.nonzero().flatten()
    span = f"{int(seen[0])}..{int(seen[-1])} ({len(seen)})" if len(seen) else "none"
    return (f"sample {b} head {h} row {i} [{cls}] aims at key {int(c.aim[b, h, i])} (code {int(c.qc[b, h, i])}, "
            f"{'visible' if vis[c.aim[b, h, i]] else 'masked'}); visible keys {span}; visible targets {tg[:8]}"
            f"{'...' if len(tg) > 8 else ''}; qlen {c.ql[b]} klen {c.kl[b]}")


def compare(entry, what, got, ref, bnd, c=None, layout=None, context="", record=True):
    """None when |got - ref| <= bnd on every element, else a line that names the count of wrong elements and the worst one.
    layout "bihd" / "bhi" (query rows) adds the row's description; "bjhd": key rows."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, f"[{entry}] {context} {what}: got {tuple(got.shape)}, want {tuple(ref.shape)}"
    ratio = ratio_to_bound(got, ref, bnd)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if record:
        COUNTS[entry + "/" + what] += got.numel()
        WORST[entry + "/" + what] = max(WORST[entry + "/" + what], worst)
    if worst <= 1.0:
        return None
    idx = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), got.shape))
    where = ""
    if c is not None and layout == "bihd":
        where = describe_row(c, idx[0], idx[2], idx[1]) + f"; expected mean {float(ref[idx]):.6g}"
    elif c is not None and layout == "bhi":
        where = describe_row(c, idx[0], idx[1], idx[2])
    elif c is not None and layout == "bjhd":
        where = f"sample {idx[0]} head {idx[2]} key {idx[1]} (code {int(c.kc[idx[0], idx[2], min(idx[1], c.Lk - 1)])}); klen {c.kl[idx[0]]}"
    rows = int((ratio > 1.0).reshape(ratio.shape[0], -1).any(-1).sum()) if ratio.dim() else 0
    return (f"[{entry}] {context} {what}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements miss their bound ({rows} samples "
            f"touched); worst at {idx}: got {float(got[idx])!r}, want {float(ref[idx])!r}, bound {float(bnd[idx]):.3e}, "
            f"ratio {worst:.3f}; {where}")


def bad_rows(got, ref, bnd):
    """bool over the leading dimensions: rows with at least one element over its bound ([..., D] -> [...])"""
    return (ratio_to_bound(got, ref, bnd) > 1.0).any(-1)


def summary_line():
    return "[measured] worst ratio to the bound: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())) + \
        "  | kappa (host restatement's worst ratio to S): " + "  ".join(f"{k}=2^{int(math.log2(v))} ({MEASURED[k]:.3e})" for k, v in KAPPA.items())


# ----------------------------------------------------------------------------------------------------------------------
# dispatch, restated from the .hip files
# ----------------------------------------------------------------------------------------------------------------------
def tail_split_plan(nwg, slots, loop_tiles, min_tiles, single_round_only=False, max_cost=0.67):
    """omh_tail_split_plan of csrc/omh_common.h -> (n_regular, n_tail, splits)"""
    if nwg <= 0 or slots <= 0 or (single_round_only and nwg >= slots) or nwg % slots == 0:
        return nwg, 0, 1
    r = nwg % slots
    best_s, best = 1, 1.0
    for sp in range(2, min(loop_tiles // min_tiles, 8) + 1):
        cost = ((r * sp + slots - 1) // slots) / sp
        if cost < best - 1e-9:
            best, best_s = cost, sp
    if best_s < 2 or best > max_cost:
        return nwg, 0, 1
    return nwg - r, r, best_s


def short_split_plan(cs, cus, option="tail"):
    """base_split_plan of csrc/attention.hip for a call with OMH_ATTN_ALLOW_SPLIT and option ATTN_SPLIT = ``option``"""
    nwg = _up(cs["Lq"], 128) // 128 * cs["H"] * cs["B"]
    mask = cs.get("mask")
    if cs.get("q_lens") is not None or (mask is not None and mask.kind != "full") or option == "0":
        return nwg, 0, 1
    tail = option == "tail"
    return tail_split_plan(nwg, 2 * cus, _up(cs["Lk"], 64) // 64, 4 if tail else 16, not tail, 0.8 if tail else 0.67)


def bwd_split_plan(cs, cus, dq, option="tail"):
    """bwd2_plan of csrc/attention_bwd2.hip (ATTN_BWD_W64 = cs["w64"])"""
    nwg = _up(cs["Lq"] if dq else cs["Lk"], 128) // 128 * cs["H"] * cs["B"]
    if option == "0":
        return nwg, 0, 1
    tail = option == "tail"
    slots = (2 if dq and cs.get("w64") in ("0", "k") else 1) * cus
    return tail_split_plan(nwg, slots, _up(cs["Lk"] if dq else cs["Lq"], 64) // 64, 4, not tail, 0.8 if tail else 0.67)


def takes_w64(B, H, Lq, Lk, q_rs, k_rs, o_rs, ldv, option=None, o32=False, q_lens=False, flags=0, band=False):
    """attn_choice of csrc/attention.hip: does omh_flash_attn_fwd_d128 take the long-sequence stream?  option: ATTN_KERNEL"""
    big = _up(Lq, 256) // 256 * H * B >= 512 and Lk >= 1024
    fits32 = Lq * q_rs * 2 < 0x7fffffff and Lk * k_rs * 2 < 0x7fffffff and Lq * o_rs * 2 < 0x7fffffff and D * ldv * 2 < 0x7fffffff
    if o32 or q_lens or (flags & 1) or band:               # fp32 output / q_lens / OMH_ATTN_SHORT_KERNEL / a bounded side: short kernel only
        return False
    return (option[0] == "w" and fits32) if option else (big and fits32)


def masked_entry_accepts(c):
    """the argument rules of the masked entries (attn_fwd_masked / bwd_masked_entry and the omh_*_mask_check of
    csrc/omh_common.h) for the case's mask, handed over with the band (0, 0): they run the short-sequence kernels' instantiation of
    the mask kind whatever the shape, unsplit"""
    m, Lq, Lk = c.mask, c.Lq, c.Lk
    if m.kind == "chunk":
        return m.chunk > 0 and m.q_offset >= 0 and m.q_offset + Lq + Lk < 1 << 28
    if m.kind == "interval":
        kg = m.group if m.k_group is None else m.k_group
        return m.group >= 8 and kg >= 1 and Lq + Lk < 1 << 28 and tuple(m.vis.shape) == (_up(Lq, m.group) // m.group, _up(Lk, kg) // kg)
    if m.kind == "block":
        return m.m.shape[0] in (1, c.H) and tuple(m.m.shape[1:]) == (_up(Lq, 128) // 128, _up(Lk, 128) // 128)
    return False


def w64_plan(B, H, Lq, Lk, cus):
    """w64_plan of csrc/attention_w64.hip -> (n_regular, n_tail, splits)"""
    nwg = _up(Lq, 256) // 256 * H * B
    cus -= cus % 8
    r = nwg % cus
    if nwg > cus and 0 < r <= 64 and _up(Lk, 64) // 64 >= 64:
        splits = min(cus // r, 16)
        if splits >= 4:
            return nwg - r, r, splits
    return nwg, 0, 1


# ----------------------------------------------------------------------------------------------------------------------
# the cases, shared by tests/test_attn_exact_host.py and tests/test_gpu_attn_exact.py
# ----------------------------------------------------------------------------------------------------------------------
def _stairs(n, sink=False):
    """[n, n] chunk staircase over groups; sink: first group | a window of two | (three runs with the clean / noisy halves)"""
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    if sink:
        return (j == 0) | ((j <= i) & (j >= i - 1))
    return j <= i


def _teacher(n):
    """teacher forcing over [n clean | n noisy] groups: clean rows see clean <= own; noisy rows see clean < own and their own"""
    i, j = torch.arange(2 * n)[:, None], torch.arange(2 * n)[None, :]
    clean_rows = (i < n) & (j <= i)
    noisy_rows = (i >= n) & (((j < n) & (j < i - n)) | (j == i))
    return clean_rows | noisy_rows


def _teacher_sink(n):
    """three runs: clean sink group 0 | clean window of one group before the own | own noisy group"""
    i, j = torch.arange(2 * n)[:, None], torch.arange(2 * n)[None, :]
    clean_rows = (i < n) & ((j == 0) | ((j <= i) & (j >= i - 1)))
    own = i - n
    noisy_rows = (i >= n) & (((j == 0) & (own > 0)) | ((j < n) & (j == own - 2) & (own > 2)) | (j == i))
    return clean_rows | noisy_rows


def fwd_short_cases():
    """the short-sequence kernel, full attention: dict(B, H, Lq, Lk, q_lens, k_lens, prescaled, lse, o32, seed)"""
    out = []
    lqs, lks = (1, 31, 33, 127, 128, 129, 257), (1, 63, 64, 65, 129, 200, 320)
    kl_pool, ql_pool = (0, 1, 63, 64, 65, None), (0, 1, 129, None)
    for n, (lq, lk) in enumerate(zip(lqs, lks)):
        for m, lk2 in enumerate((lk, lks[(n + 3) % 7])):
            x = 2 * n + m
            kls = [kl_pool[(x + t) % 6] for t in range(2)]
            qls = [ql_pool[(x + t) % 4] for t in range(2)]
            # q_lens (odd x), q_prescaled, lse and o32 vary independently: q_lens meets q_prescaled = 0 (x = 1, 5, 9, 13) and a call
            # without lse (x = 3, 9)
            out.append(dict(B=2, H=2 + x % 2, Lq=lq, Lk=lk2, k_lens=[lk2 if v is None else min(v, lk2) for v in kls] if x % 3 else None,
                            q_lens=[lq if v is None else min(v, lq) for v in qls] if x % 2 else None,
                            prescaled=bool((x // 2) % 2), lse=bool(x % 3), o32=bool((x // 3) % 2), seed=x))
    return out


def fwd_split_cases():
    """ATTN_SPLIT = "tail", OMH_ATTN_ALLOW_SPLIT: Lk >= 1024 (workers of >= 4 tiles); workspace given / withheld"""
    return [dict(B=2, H=3, Lq=129, Lk=1024, k_lens=[1000, 1024], prescaled=True, lse=True, o32=True, seed=40, workspace=True),
            dict(B=2, H=3, Lq=129, Lk=1030, k_lens=[517, 1030], prescaled=False, lse=True, o32=False, seed=41, workspace=False)]


def band_cases():
    """dict(..., mask band): causal square; more keys than queries; fewer keys than queries (first rows see nothing);
    (40, 25) across tiles; (0, -1); a band that skips whole key tiles on both sides; q_lens / k_lens move the shift"""
    mk = lambda lq, lk, l, r, ql, kl, s, pre=True: dict(B=2, H=2, Lq=lq, Lk=lk, mask=mask_band(l, r), q_lens=ql, k_lens=kl,
                                                         prescaled=pre, lse=True, o32=bool(s % 2), seed=50 + s)
    return [mk(257, 257, -1, 0, None, None, 0), mk(130, 333, -1, 0, [77, 130], [150, 333], 1, False),
            mk(300, 100, -1, 0, [300, 200], [90, 100], 2), mk(257, 257, 40, 25, [257, 200], [257, 230], 3),
            mk(200, 260, 0, -1, None, [260, 129], 4, False), mk(300, 320, 20, 10, [300, 255], [320, 300], 5)]


def masked_cases():
    """the masked entries: run ends at -1, 0, +1 around 64-key tile ends and 128-row workgroup ends"""
    out = []
    # chunk-causal: chunk 43 (no multiple of anything), 64, 65; left_chunks 0, 1, -1; q_offset > 0; q_lens inside a workgroup
    for s, (lq, lk, ch, left, off, ql, kl) in enumerate(((257, 320, 43, -1, 0, [257, 200], [320, 300]),
                                                         (200, 321, 64, 1, 65, None, [321, 129]),
                                                         (130, 260, 65, 0, 130, [130, 127], None))):
        out.append(dict(B=2, H=2, Lq=lq, Lk=lk, mask=mask_chunk(ch, left, off), q_lens=ql, k_lens=kl, prescaled=bool(s % 2), lse=True,
                        o32=True, seed=60 + s))
    # interval, group 63 / 64 / 65: a workgroup's rows span two table rows; teacher forcing has touching and non-touching runs
    for s, g in enumerate((63, 64, 65)):
        n = 3
        L = 2 * n * g - (5 if s == 1 else 0)
        out.append(dict(B=2, H=2, Lq=L, Lk=L, mask=mask_interval(_teacher(n), g), q_lens=[L, L - g - 1] if s else None,
                        k_lens=[L - 1, L] if s == 2 else None, prescaled=bool(s % 2), lse=True, o32=True, seed=70 + s))
    # a workgroup whose ``whole`` intersection is empty: group 24, every group sees only itself and the first
    vis = torch.eye(11, dtype=torch.bool)
    vis[:, 0] = True
    out.append(dict(B=2, H=2, Lq=260, Lk=260, mask=mask_interval(vis, 24), q_lens=[260, 131], k_lens=None, prescaled=True, lse=True,
                    o32=True, seed=75))
    # three runs
    out.append(dict(B=2, H=2, Lq=384, Lk=384, mask=mask_interval(_teacher_sink(4), 48, runs=3), q_lens=[384, 300], k_lens=None,
                    prescaled=False, lse=True, o32=True, seed=76))
    # rectangular: query groups of 65 rows onto key groups of 5 tokens, a window of two key groups per frame + the first
    qg, kg = 4, 13
    i, j = torch.arange(qg)[:, None], torch.arange(kg)[None, :]
    rect = ((j >= 3 * i + 1) & (j <= 3 * i + 3)) | (j == 0)
    out.append(dict(B=2, H=3, Lq=4 * 65 - 3, Lk=13 * 5 - 1, mask=mask_interval(rect, 65, k_group=5), q_lens=[257, 140], k_lens=[64, 63],
                    prescaled=True, lse=True, o32=True, seed=77, codes=8))
    # block masks: heads 1 and heads H; k_lens inside the first and inside the second tile of the last kept block
    g = _gen(78)
    for s, heads in enumerate((1, 3)):
        m = torch.rand(heads, 3, 4, generator=g) < 0.6
        m[:, :, 2] = True
        m[:, 1, 0] = True
        out.append(dict(B=2, H=3, Lq=300, Lk=500, mask=mask_block(m), q_lens=[300, 129] if s else None, k_lens=[256 + 30, 256 + 64 + 30],
                        prescaled=bool(s), lse=True, o32=True, seed=78 + s))
    return out


def _last_tile_klen(lk, n):
    """a key count inside the last 64-key tile of lk keys: lk - (1..63), not below the tile's first key + 1"""
    return max(lk - 1 - (n * 9 + 4) % 63, (lk - 1) // 64 * 64 + 1)


def w64_cases():
    """ATTN_KERNEL = "w64": dict(..., sched, bounded); q_prescaled = n % 2 and W64_SCHED = (n // 2) % 2 vary independently
    (the bounded stream meets all four pairs); k_lens inside the last key tile"""
    out = []
    lqs, lks = (1, 63, 65, 255, 256, 257, 300), (1, 64, 65, 449, 1000, 449, 1000)
    for n, (lq, lk) in enumerate(zip(lqs, lks)):
        kl = [lk, _last_tile_klen(lk, n)] if n % 3 != 1 else None
        out.append(dict(B=2, H=2, Lq=lq, Lk=lk, k_lens=kl, prescaled=bool(n % 2), lse=bool(n % 3), sched=str((n // 2) % 2), seed=90 + n,
                        bounded=n >= 3))
    out.append(dict(B=2, H=2, Lq=300, Lk=449, k_lens=[449, _last_tile_klen(449, 8)], prescaled=False, lse=True, sched="1", seed=98, bounded=True))
    out.append(dict(B=2, H=2, Lq=257, Lk=1000, k_lens=[_last_tile_klen(1000, 9), 1000], prescaled=True, lse=True, sched="0", seed=99, bounded=False))
    out.append(dict(B=2, H=2, Lq=63, Lk=65, k_lens=None, prescaled=True, lse=True, sched="1", seed=100, bounded=False))
    return out


def bwd_cases():
    """the o32 kernels, full attention: dict(..., w64 option, phases, out_bf16, split, workspace).  Every Lq of {1, 63, 65, 127,
    129, 300} with three Lk of the same set and with all three ATTN_BWD_W64 settings; Lk = 1, 65 and 129 (a single key, a
    one-key last tile, a one-key last block) each meet all three settings too."""
    out = []
    ls = (1, 63, 65, 127, 129, 300)
    settings = ("0", "k", None)
    for n, lq in enumerate(ls):
        for m in range(3):
            x = 3 * n + m
            lk = ls[(n + 2 * m + 1) % 6]
            out.append(dict(B=2, H=2, Lq=lq, Lk=lk, k_lens=[lk, max(1, lk - 7)] if x % 4 in (1, 2) else None, prescaled=bool(x % 2),
                            w64=settings[(n + m) % 3], phases=bool((x // 2) % 2), out_bf16=bool((x // 3) % 2), seed=110 + x))
    for n in range(6):
        assert {cs["w64"] for cs in out if cs["Lq"] == ls[n]} == set(settings)
        assert n % 2 or {cs["w64"] for cs in out if cs["Lk"] == ls[n]} == set(settings)
    # ATTN_SPLIT = "tail": workers of >= 4 tiles need 8 tiles per loop; phases 1 + 2 + 3 with the workspace given and withheld
    for n, (opt, phases, ws) in enumerate((("0", False, True), ("k", True, True), (None, False, True), (None, True, False))):
        out.append(dict(B=2, H=3, Lq=520, Lk=513, k_lens=[513, 449], prescaled=bool(n % 2), w64=opt, phases=phases, out_bf16=n == 2,
                        split=True, workspace=ws, seed=140 + n))
    return out


def bwd_old_cases():
    """the kernels without o32 (csrc/attention_bwd.hip, through ops.flash_attn_bwd's transposed operands)"""
    ls = (1, 31, 33, 65, 129, 200)
    return [dict(B=2, H=2, Lq=lq, Lk=ls[(n + 3) % 6], k_lens=[ls[(n + 3) % 6], max(1, ls[(n + 3) % 6] - 5)] if n % 2 else None,
                 prescaled=bool(n % 2), seed=130 + n) for n, lq in enumerate(ls)]


def cached_cases():
    """own_lo in {8, 64, 72, Lk - 8}; k_bs wider than Lk rows"""
    return [dict(B=2, H=2, Lq=130, Lk=200, own_lo=lo, prescaled=bool(n % 2), out_bf16=n == 2, seed=150 + n)
            for n, lo in enumerate((8, 64, 72, 192))]


def ident(cs):
    m = cs.get("mask")
    tag = "" if m is None else {"band": lambda: f"band{m.left}_{m.right}", "chunk": lambda: f"chunk{m.chunk}_{m.left_chunks}_{m.q_offset}",
                                "interval": lambda: f"ivl{m.runs}g{m.group}" + (f"x{m.k_group}" if m.k_group else ""),
                                "block": lambda: f"blk{m.m.shape[0]}"}[m.kind]() + "-"
    rest = "-".join(f"{k}{v}" for k, v in cs.items() if k not in ("seed", "mask", "B", "H", "codes") and v is not None and v is not False)
    return (tag + rest).replace(" ", "").replace("[", "").replace("]", "").replace(",", "_").replace("True", "1")
