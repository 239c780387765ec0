"""Three-run interval-mask attention, forward and backward: omh_flash_attn_fwd_interval3_d128 /
omh_flash_attn_bwd_interval3_d128 through ``ops.flash_attn(interval_mask=IntervalMask(..., runs=3))``,
``flash_attention`` and ``ops.flash_attn_func`` against autograd through a dense-masked fp32 softmax attention on the same
bf16 operands (the reference of test_gpu_attn_interval.py, taken head by head so that the long cases stay small).

Bounds: the project's own for this arithmetic (test_gpu_attn_interval.py): forward rel-RMS < 8e-3 and max abs error
< 3e-2, attention gradients rel-RMS < 1.2e-2."""
import importlib

import pytest
import torch

from conftest import PKG, rel_rms, set_option

pytestmark = pytest.mark.gpu
FWD_RMS, FWD_MAX, GRAD_RMS = 8e-3, 3e-2, 1.2e-2


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def attn_mod():
    return importlib.import_module(PKG + ".wan.modules.attention")


def _runs(v):
    v = v.bool()
    return int(v[0]) + int((v[1:] & ~v[:-1]).sum())


def random_three_runs(seed, nq=9, nk=24):
    """A seeded random bool matrix [nq, nk]: three jittered runs per row, row 4 blind, key groups 5 and 6 dead; drawn
    again until no row and no column has a fourth run and both a row and a column have three."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(1000):
        m = torch.zeros(nq, nk, dtype=torch.bool)
        base = torch.sort(torch.randperm(nk - 1, generator=g)[:6] + 1).values.tolist()
        for r in range(nq):
            j = sorted(min(max(b + int(torch.randint(-1, 2, (1,), generator=g)), 0), nk) for b in base)
            for a, b in zip(j[0::2], j[1::2]):
                m[r, a:b] = True
        m[4] = False
        m[:, 5:7] = False
        rows, cols = [_runs(m[r]) for r in range(nq)], [_runs(m[:, c]) for c in range(nk)]
        if max(rows) == 3 and max(cols) == 3:
            return m
    raise AssertionError("no three-run matrix drawn")


# Tables written by hand (not built from a matrix), (number of groups, row) pairs: rows with EMPTY earlier slots and a live
# later one, bounds below 0 and above the other axis's group count (the kernels clamp them), and — group 8, Lq = 200,
# Lk = 328 — the first 128-row workgroup runs key tiles 0, 2 and 4..5 (both jumps, a whole tile skipped at each), the second
# tiles 0..2 (two ranges that touch) and 5; the first 128-key workgroup runs query tiles 0 and 2..3 around an empty middle
# hull.  HAND_K says of the key groups what HAND_Q says of the query groups.
HAND_Q = [(4, [-3, 6, 17, 22, 36, 99]), (4, [4, 6, 22, 22, 36, 41]), (4, [3, 3, 18, 20, 33, 46]), (4, [2, 2, 20, 20, 34, 38]),
          (4, [7, 7, 8, 17, 17, 17]), (5, [0, 4, 8, 17, 40, 41])]
HAND_K = [(4, [0, 4, 4, 4, 20, 99]), (2, [-2, 8, 8, 8, 8, 8]), (2, [0, 0, 0, 0, 0, 0]), (9, [9, 9, 9, 9, 16, 25]),
          (1, [0, 4, 4, 4, 4, 4]), (2, [0, 0, 0, 4, 8, 12]), (2, [0, 4, 4, 4, 4, 4]), (11, [0, 0, 0, 0, 0, 0]),
          (1, [8, 12, 12, 12, 12, 12]), (2, [8, 16, 16, 16, 16, 16]), (2, [0, 16, 16, 16, 16, 16]), (2, [-7, 12, 12, 12, 12, 12]),
          (1, [0, 12, 12, 12, 20, 30])]


def hand_rows(pairs):
    return torch.tensor([row for n, row in pairs for _ in range(n)], dtype=torch.int32)


def table_matrix(rows, other):
    """The bool matrix [len(rows), other] a table says, read as the kernels read it: bounds clamped to [0, other]."""
    m = torch.zeros(rows.shape[0], other, dtype=torch.bool)
    for g, row in enumerate(rows.tolist()):
        for lo, hi in zip(row[0::2], row[1::2]):
            m[g, min(max(lo, 0), other):min(max(hi, 0), other)] = True
    return m


def hand_mask(causal, device="cpu"):
    """The IntervalMask of the matrix HAND_Q says, with the hand-written tables in place of the ones built from it."""
    q_rows, k_rows = hand_rows(HAND_Q), hand_rows(HAND_K)
    mask = causal.IntervalMask(table_matrix(q_rows, k_rows.shape[0]), 8, runs=3)
    mask._host = (q_rows, k_rows)
    mask._move(torch.device(device))
    return mask


def _tf(n, W, S):
    return lambda c: c.teacher_forcing_groups(n, W, S)


CASES = [
    # B, H, Lq, Lk, k_lens, q_lens, group, matrix
    (1, 2, 480, 480, None, None, 40, _tf(6, 1, 1)),                              # gaps shorter than a tile: the ranges merge
    (1, 2, 2400, 2400, None, None, 200, _tf(6, 1, 1)),                           # both jumps taken, runs end inside tiles
    (2, 2, 200, 560, [560, 430], [200, 150], 24, lambda c: random_three_runs(3)),   # several groups per workgroup, ragged, blind, dead
    (1, 2, 256, 256, None, None, 8, _tf(16, 1, 1)),                              # group 8: 16 table rows per workgroup
    (1, 12, 12480, 12480, None, None, 1560, _tf(4, 1, 1)),                       # the workload's group, 12 heads through xcd_remap
    (2, 2, 560, 560, [560, 400], None, 56, lambda c: c.teacher_forcing_groups(5)),   # two runs: the bits of runs=2
    (1, 2, 240, 240, None, None, 40, lambda c: c.sink_window_groups(6, 1, 1)),   # two runs that merge: the bits of runs=2
    (1, 2, 300, 300, None, None, 300, lambda c: torch.tensor([[1]])),            # full attention: the plain kernel's bits
    (1, 2, 200, 328, None, None, 8, None),                                       # hand_mask: tables no matrix builds
]
MERGE, JUMPS, RANDOM, GROUP8, WORKLOAD, TWO_A, TWO_B, FULL, HAND = range(9)
_CACHE = {}


def _case(idx, causal):
    """Inputs, the mask, the fp32 reference (output, liveness, gradients) — computed once per case and left unchanged."""
    if idx in _CACHE:
        return _CACHE[idx]
    B, H, Lq, Lk, klens, qlens, group, make = CASES[idx]
    mask = hand_mask(causal, "cuda") if idx == HAND else causal.IntervalMask(make(causal), group, "cuda", runs=3)
    g = torch.Generator(device="cuda").manual_seed(700 + idx)
    q, k, v = (torch.randn(B, L, H, 128, device="cuda", generator=g).bfloat16() for L in (Lq, Lk, Lk))
    do = torch.randn(B, Lq, H, 128, device="cuda", generator=g).bfloat16()
    vis = torch.stack([causal.interval_visible(mask, Lq, Lk, None if qlens is None else qlens[b],
                                               None if klens is None else klens[b]) for b in range(B)])
    vis = vis.cuda()[:, None]                                                      # [B, 1, Lq, Lk]
    if qlens is not None:
        for b in range(B):
            do[b, qlens[b]:] = float("nan")                                        # nothing may depend on those rows
    out, grads = [], []
    for h in range(H):                                                             # head by head: [B, 1, Lq, Lk] scores at a time
        qr, kr, vr = (t[:, :, h:h + 1].float().transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
        s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
        s = s.masked_fill(~vis, float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)                     # rows that see no key
        o = torch.einsum("bhij,bhjd->bhid", p, vr)
        o.backward(torch.nan_to_num(do[:, :, h:h + 1].float(), nan=0.0).transpose(1, 2))
        out.append(o.detach().transpose(1, 2))
        grads.append([t.grad.transpose(1, 2) for t in (qr, kr, vr)])
        del s, p, o
    ref = dict(out=torch.cat(out, 2).contiguous(),
               grads=tuple(torch.cat([g_[i] for g_ in grads], 2).contiguous() for i in range(3)),
               row_live=vis.any(3).expand(B, H, Lq).contiguous(),                  # [B, H, Lq]: the row sees a key
               key_live=vis.any(2).expand(B, H, Lk).contiguous())                  # [B, H, Lk]: a live query sees the key
    del vis
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
    ql = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device="cuda")
    _CACHE[idx] = (q, k, v, do, kl, ql, mask, ref)
    return _CACHE[idx]


def _vt(v):
    B, Lk, H, D = v.shape
    Lp = (Lk + 63) // 64 * 64
    vt = torch.zeros(B, H * D, Lp, device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.reshape(B, Lk, H * D).transpose(1, 2)
    return vt


def test_cases_hold_what_they_are_for(causal):
    """On the CPU, before relying on them: three-run rows whose gaps are shorter than a tile (MERGE) and rows whose two
    gaps both force a jump (JUMPS, WORKLOAD); a blind live row group, dead key groups, three-run rows and columns and
    several groups per workgroup (RANDOM); 16 table rows per workgroup (GROUP8); at most two runs (TWO_A, TWO_B)."""
    def table(idx):
        B, H, Lq, Lk, klens, qlens, group, make = CASES[idx]
        return causal.IntervalMask(make(causal), group, runs=3), group
    three = lambda t: (t[:, 1] > t[:, 0]) & (t[:, 3] > t[:, 2]) & (t[:, 5] > t[:, 4])
    m, g = table(MERGE)
    t = m.q_iv
    assert bool((three(t) & ((t[:, 2] - t[:, 1]) * g < 64)).any())
    for idx in (JUMPS, WORKLOAD):
        m, g = table(idx)
        t = m.q_iv
        # a gap of at least two tiles is never closed by rounding the hulls to tiles: both jumps are taken
        assert bool((three(t) & ((t[:, 2] - t[:, 1]) * g >= 128) & ((t[:, 4] - t[:, 3]) * g >= 128)).any())
    assert CASES[JUMPS][6] % 64 != 0                                              # runs end inside tiles
    m, g = table(RANDOM)
    B, H, Lq, Lk, klens, qlens = CASES[RANDOM][:6]
    assert bool(three(m.q_iv).any()) and bool(three(m.k_iv).any()) and 128 // g >= 5 and Lq != Lk
    for b in range(B):
        vis = causal.interval_visible(m, Lq, Lk, qlens[b], klens[b])
        assert bool((~vis.any(1))[:qlens[b]].any())                               # a live row that sees nothing
        assert int((~vis.any(0))[:klens[b]].sum()) >= 2 * g                       # whole key groups nobody sees
    m, g = table(GROUP8)
    assert 128 // g == 16 and bool(three(m.q_iv).any())
    for idx in (TWO_A, TWO_B, FULL):
        B, H, Lq, Lk, klens, qlens, group, make = CASES[idx]
        causal.IntervalMask(make(causal), group)                                  # two runs hold it
        assert not bool(three(table(idx)[0].q_iv).any())
    with pytest.raises(ValueError):                                               # and they do not hold the others
        causal.IntervalMask(CASES[MERGE][7](causal), 40)
    # the hand-written tables: both say one matrix, no matrix builds them, and they hold what their comment promises
    B, H, Lq, Lk, klens, qlens, group, make = CASES[HAND]
    m = hand_mask(causal)
    built = causal.IntervalMask(m.vis, group, runs=3)
    assert (m.q_groups, m.k_groups) == ((Lq + group - 1) // group, (Lk + group - 1) // group) == (25, 41)
    assert torch.equal(table_matrix(m.k_iv, m.q_groups), m.vis.t())
    assert not torch.equal(m.q_iv, built.q_iv) and not torch.equal(m.k_iv, built.k_iv)
    for t, other in ((m.q_iv, m.k_groups), (m.k_iv, m.q_groups)):
        assert bool(((t[:, 1] <= t[:, 0]) & (t[:, 3] <= t[:, 2]) & (t[:, 5] > t[:, 4])).any())   # two empty slots, a live third
        assert bool(((t[:, 1] > t[:, 0]) & (t[:, 3] <= t[:, 2]) & (t[:, 5] > t[:, 4])).any())    # an empty middle slot
        assert bool((t < 0).any()) and bool((t > other).any())                     # bounds the kernels clamp
        assert bool(((t[:, 0] <= t[:, 2]) & (t[:, 2] <= t[:, 4])).all())           # rows ascend
    assert bool(three(m.q_iv).any())
    vis = causal.interval_visible(m, Lq, Lk)
    assert bool(vis.any(1).all())                                                  # no live row is blind
    seen = [bool(vis[:128, 64 * t:64 * t + 64].any()) for t in range(6)]           # key tiles of the first query workgroup
    assert seen == [True, False, True, False, True, True]
    seen = [bool(vis[128:, 64 * t:64 * t + 64].any()) for t in range(6)]           # ... of the second
    assert seen == [True, True, True, False, False, True]
    seen = [bool(vis[64 * t:64 * t + 64, :128].any()) for t in range(4)]           # query tiles of the first key workgroup
    assert seen == [True, False, True, True]
    assert Lq % 128 != 0 and (Lk + 63) // 64 == 6 and Lk % 64 != 0


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_interval3_forward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, causal)
    assert mask.runs == 3 and mask.q_iv.shape[1] == 6
    lse = torch.full((B, H, Lq), float("nan"), device="cuda")
    o = ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=mask, lse=lse)
    err_rms, err_max = rel_rms(o, ref["out"]), float((o.float() - ref["out"]).abs().max())
    print(f"case {idx}: forward rel-RMS {err_rms:.2e} max abs {err_max:.2e}")
    assert torch.isfinite(o.float()).all()
    assert err_rms < FWD_RMS and err_max < FWD_MAX
    # rows that see no key: exact zeros and lse = -inf; every other row a finite lse
    live = ref["row_live"]                                                   # [B, H, Lq]
    assert float(o.float().transpose(1, 2)[~live].abs().sum()) == 0.0
    assert bool((lse[~live] == float("-inf")).all()) and bool(torch.isfinite(lse[live]).all())
    # the wrapper with the reference's signature, and a second run: the same bits
    with torch.no_grad():
        ow = attn_mod.flash_attention(q, k, v, q_lens=ql, k_lens=kl, interval_mask=mask)
    assert torch.equal(ow, o)
    assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=mask), o)
    if idx in (TWO_A, TWO_B, FULL):                                          # at most two runs: the two-run kernels' bits
        two = causal.IntervalMask(CASES[idx][7](causal), CASES[idx][6], "cuda")
        lse2 = torch.full((B, H, Lq), float("nan"), device="cuda")
        assert torch.equal(ops.flash_attn(q, k, _vt(v), kl, q_lens=ql, interval_mask=two, lse=lse2), o)
        assert torch.equal(lse2, lse)
    if idx == FULL:                                                          # vis = [[1]]: the plain kernel's bits
        set_option("OMH_ATTN_KERNEL", "base")
        assert torch.equal(o, ops.flash_attn(q, k, _vt(v), kl))


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_interval3_backward(ops, causal, attn_mod, idx):
    B, H, Lq, Lk = CASES[idx][:4]
    q, k, v, do, kl, ql, mask, ref = _case(idx, causal)

    def run(through_wrapper=False, m=mask):
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        if through_wrapper:
            attn_mod.flash_attention(qg, kg, vg, q_lens=ql, k_lens=kl, interval_mask=m).backward(do)
        else:
            ops.flash_attn_func(qg, kg, vg, kl, ql, interval_mask=m).backward(do)
        return qg.grad, kg.grad, vg.grad

    got = run()
    for name, gt, rf in zip(("dq", "dk", "dv"), got, ref["grads"]):
        err = rel_rms(gt, rf)
        print(f"case {idx}: {name} rel-RMS {err:.2e}")
        assert torch.isfinite(gt.float()).all()
        assert err < GRAD_RMS, name
    # rows that see no key (dead queries included) and keys no live query sees: exact zeros, written
    assert float(got[0].float().transpose(1, 2)[~ref["row_live"]].abs().sum()) == 0.0
    dead_k = ~ref["key_live"]
    assert float(got[1].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    assert float(got[2].float().transpose(1, 2)[dead_k].abs().sum()) == 0.0
    for a, b in zip(run(), got):                                             # no atomics: repeatable bit for bit
        assert torch.equal(a, b)
    if idx != WORKLOAD:
        for a, b in zip(run(through_wrapper=True), got):                     # flash_attention(interval_mask=) is differentiable
            assert torch.equal(a, b)
    if idx in (TWO_A, TWO_B, FULL):                                          # at most two runs: the two-run kernels' bits
        two = causal.IntervalMask(CASES[idx][7](causal), CASES[idx][6], "cuda")
        for a, b in zip(run(m=two), got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("idx", [JUMPS, RANDOM])
def test_interval3_backward_modes(ops, causal, idx):
    """bf16 outputs and q_prescaled agree with the plain call; phases 1 + 2 + 3 give phase 0's bits; the forward without
    lse writes the same output."""
    B, H, Lq, Lk = CASES[idx][:4]
    q4, k4, v4, do4, kl, ql, mask, _ = _case(idx, causal)
    d = H * 128
    q, k, v, do = q4.view(B * Lq, d), k4.view(B * Lk, d), v4.view(B * Lk, d), do4.view(B * Lq, d)
    vt = _vt(v4)
    LOG2E = 1.4426950408889634

    def forward(qq, pre, with_lse=True):
        o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(qq), ops.ptr(k), ops.ptr(vt), ops.ptr(o), None if kl is None else ops.ptr(kl), B, H, Lq, Lk,
                           Lq * d, d, Lk * d, d,
                           d * vt.shape[2], Lq * d, d, vt.shape[2], 128 ** -0.5, lse=ops.ptr(lse) if with_lse else None,
                           q_prescaled=pre, o32=ops.ptr(o32), q_lens=None if ql is None else ops.ptr(ql), interval_mask=mask)
        return o, o32, lse

    o, o32, lse = forward(q, 0)
    assert torch.equal(forward(q, 0, with_lse=False)[0], o)
    kw = dict(o32=o32, interval_mask=mask, q_lens=ql)
    dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, **kw)
    out = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, out=out, **kw)
    for got, ref in zip(out, (dq, dk, dv)):
        assert rel_rms(got.float(), ref) < 8e-3
    qp = (q.float() * (128 ** -0.5 * LOG2E)).bfloat16()
    op, o32p, lsep = forward(qp, 1)
    gp = ops.flash_attn_bwd(qp, k, v, op, do, lsep, kl, B, H, Lq, Lk, q_prescaled=True, o32=o32p, interval_mask=mask, q_lens=ql)
    for got, ref in zip(gp, (dq, dk, dv)):
        assert rel_rms(got, ref) < GRAD_RMS
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=1, out=None, delta=delta, **kw)
    ph = [torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=3, out=tuple(ph), delta=delta, **kw)
    ops.flash_attn_bwd(q, k, v, o, do, lse, kl, B, H, Lq, Lk, phase=2, out=tuple(ph), delta=delta, **kw)
    for a, b in zip(ph, out):
        assert torch.equal(a, b)


def test_interval3_refusals(ops, causal):
    q = torch.randn(1, 480, 2, 128, device="cuda").bfloat16()
    m = causal.IntervalMask(causal.teacher_forcing_groups(6, 1, 1), 40, "cuda", runs=3)
    with pytest.raises(ValueError):
        ops.flash_attn_func(q, q, q, window=(16, -1), interval_mask=m)
    with pytest.raises(ValueError):
        ops.flash_attn(q, q, _vt(q), chunk_causal=(40, -1, 0), interval_mask=m)
    with pytest.raises(ValueError):                                              # 12 x 12 groups of 40 do not cover 480 x 520
        ops.flash_attn(q, torch.cat([q, q[:, :40]], 1), _vt(torch.cat([q, q[:, :40]], 1)), interval_mask=m)
    host = causal.IntervalMask(causal.teacher_forcing_groups(6, 1, 1), 40, runs=3)    # tables on the CPU: moved beside q
    assert torch.equal(ops.flash_attn(q, q, _vt(q), interval_mask=host), ops.flash_attn(q, q, _vt(q), interval_mask=m))
