"""Interval masks, the part that needs no GPU: the group matrices (causal.teacher_forcing_groups, sink_window_groups), the
tables of causal.IntervalMask against runs counted in Python, causal.interval_visible against loops, the argument checks
of omh_flash_attn_fwd_interval_d128 / omh_flash_attn_bwd_interval_d128 / omh_interval_mask_tables, and the ValueErrors of
the Python layers."""
import ctypes
import importlib
import inspect

import pytest
import torch

from conftest import PKG


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


def _runs(values):
    """The runs of True in a sequence as half-open (lo, hi) pairs."""
    out, start = [], None
    for i, v in enumerate(list(values) + [False]):
        if v and start is None:
            start = i
        if not v and start is not None:
            out.append((start, i))
            start = None
    return out


def _staircase(n):
    return torch.ones(n, n).tril().bool()


MATRICES = [
    ("tf2", lambda c: c.teacher_forcing_groups(2)),
    ("tf5", lambda c: c.teacher_forcing_groups(5)),
    ("tf4w1", lambda c: c.teacher_forcing_groups(4, 1)),
    ("tf7w0", lambda c: c.teacher_forcing_groups(7, 0)),
    ("tf1", lambda c: c.teacher_forcing_groups(1)),
    ("sink", lambda c: c.sink_window_groups(6, 1, 1)),
    ("sink2", lambda c: c.sink_window_groups(9, 2, 3)),
    ("stairs", lambda c: _staircase(6)),
]


@pytest.mark.parametrize("name,make", MATRICES)
def test_builders_fit_two_intervals(causal, name, make):
    """Rows <= 2 runs, columns <= 2 runs, no blind row; the tables hold exactly those runs."""
    vis = make(causal)
    assert vis.dtype == torch.bool and vis.dim() == 2
    for row in vis.tolist():
        assert 1 <= len(_runs(row)) <= 2
    for col in vis.t().tolist():
        assert len(_runs(col)) <= 2
    m = causal.IntervalMask(vis, 56)
    assert (m.q_groups, m.k_groups, m.group) == (vis.shape[0], vis.shape[1], 56)
    assert m.q_iv.dtype == torch.int32 and m.q_iv.shape == (vis.shape[0], 4) and m.k_iv.shape == (vis.shape[1], 4)
    for table, lines in ((m.q_iv, vis.tolist()), (m.k_iv, vis.t().tolist())):
        for got, line in zip(table.tolist(), lines):
            runs = _runs(line)
            lo0, hi0, lo1, hi1 = got
            assert lo0 <= hi0 <= lo1 <= hi1
            assert [(a, b) for a, b in ((lo0, hi0), (lo1, hi1)) if b > a] == runs


def test_teacher_forcing_rule(causal):
    """The matrix written out: clean row g sees clean j <= g (j >= g - W), noisy row n + I clean j < I (j >= I - W) and
    noisy n + I only."""
    for n, W in ((1, -1), (3, -1), (5, 1), (5, 0), (4, 7)):
        vis = causal.teacher_forcing_groups(n, W)
        assert vis.shape == (2 * n, 2 * n)
        for g in range(n):
            for j in range(n):
                back = W < 0 or j >= g - W
                assert bool(vis[g, j]) == (j <= g and back)
                assert not bool(vis[g, n + j])
                assert bool(vis[n + g, j]) == (j < g and back)
                assert bool(vis[n + g, n + j]) == (j == g)
    with pytest.raises(ValueError):
        causal.teacher_forcing_groups(0)


def test_teacher_forcing_row_is_the_rollout_key_set(causal):
    """Noisy chunk I under teacher forcing attends to what WanModel.forward_chunk attends to at chunk I: the cached chunks
    the staircase rule (chunk C, left_chunks W, q_offset I C) lets it see — the clean chunks here — and itself."""
    C = 8
    for n, W in ((4, -1), (5, 1), (5, 0), (3, 2)):
        mask = causal.IntervalMask(causal.teacher_forcing_groups(n, W), C)
        dense = causal.interval_visible(mask, 2 * n * C, 2 * n * C)
        for I in range(n):
            rollout = causal.chunk_causal_visible(C, (I + 1) * C, C, W, I * C)       # rows: chunk I; keys: the cache + itself
            rows = dense[(n + I) * C:(n + I + 1) * C]
            assert torch.equal(rows[:, :I * C], rollout[:, :I * C])                  # cached chunk j <-> clean chunk j
            assert torch.equal(rows[:, (n + I) * C:(n + I + 1) * C], rollout[:, I * C:])   # itself <-> noisy chunk I
            assert not bool(rows[:, I * C:n * C].any()) and not bool(rows[:, n * C:(n + I) * C].any())
            assert not bool(rows[:, (n + I + 1) * C:].any())


def test_sink_window_rule(causal):
    vis = causal.sink_window_groups(6, 1, 1)
    for g in range(6):
        for j in range(6):
            assert bool(vis[g, j]) == (j <= g and (j < 1 or j >= g - 1))
    assert torch.equal(causal.sink_window_groups(5, 0, 4), _staircase(5))
    for bad in ((0, 1, 1), (4, -1, 1), (4, 1, -1)):
        with pytest.raises(ValueError):
            causal.sink_window_groups(*bad)


def test_three_runs_are_refused(causal):
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 0, 1, 0, 1]], 8)
    with pytest.raises(ValueError):
        causal.IntervalMask([[1], [0], [1], [0], [1]], 8)
    causal.IntervalMask([[1, 0, 1, 1, 0]], 8)                                    # two runs pass
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 1]], 7)                                         # group < 8
    with pytest.raises(ValueError):
        causal.IntervalMask([1, 1], 8)                                           # not a matrix
    with pytest.raises(ValueError):
        causal.IntervalMask(torch.zeros(0, 3), 8)


@pytest.mark.parametrize("Lq,Lk,group,qlen,klen,vis", [
    (32, 32, 8, None, None, [[1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0], [1, 0, 0, 1]]),
    (30, 27, 9, 25, 20, [[1, 0, 1], [0, 1, 1], [1, 1, 1], [0, 0, 0]]),     # ragged ends, a blind group
    (10, 50, 10, None, 44, [[1, 0, 0, 1, 1]]),
])
def test_visible_against_loops(causal, Lq, Lk, group, qlen, klen, vis):
    m = causal.IntervalMask(vis, group)
    got = causal.interval_visible(m, Lq, Lk, qlen, klen)
    assert got.dtype == torch.bool and got.shape == (Lq, Lk) and got.device.type == "cpu"
    ql, kl = Lq if qlen is None else qlen, Lk if klen is None else klen
    for i in range(Lq):
        for j in range(Lk):
            assert bool(got[i, j]) == (i < ql and j < kl and bool(vis[i // group][j // group]))
    with pytest.raises(ValueError):
        causal.interval_visible(m, Lq + group, Lk)


def test_tile_count_of_a_table(causal):
    """IntervalMask.tiles: full attention runs every tile, teacher forcing skips the gap between its two ranges."""
    assert causal.IntervalMask([[1]], 300).tiles(300, 300) == 3 * 5
    m = causal.IntervalMask(causal.teacher_forcing_groups(2), 128)              # groups = query blocks = 2 key tiles
    # clean 0: 2 tiles; clean 1: 4; noisy 0: its own 2; noisy 1: clean 0 (2) + its own (2), the 4 between skipped
    assert m.tiles(512, 512) == 2 + 4 + 2 + 4


def test_interval_entries_validate_without_gpu(omh):
    """The entries reject bad arguments before touching the device (fake, aligned pointers throughout)."""
    binding = importlib.import_module(PKG + "._lib")
    lib, by = binding.lib, ctypes.byref
    P = 4096

    def fwd_args(**kw):
        a = binding.AttnArgs(P, P, P, P, None, 1, 2, 256, 384, 0, 256, 0, 256, 0, 0, 256, 384, 0.1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def bwd_args(**kw):
        a = binding.AttnBwdArgs()
        for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv", "o32"):
            setattr(a, name, P)
        a.B, a.H, a.Lq, a.Lk = 1, 2, 256, 384
        for name in ("q_rs", "k_rs", "o_rs", "dq_rs", "dk_rs"):
            setattr(a, name, 256)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def mask(group=64, qg=4, kg=6, reserved=0, q_iv=P, k_iv=P):
        return binding.IntervalMaskArgs(group, qg, kg, reserved, q_iv, k_iv)

    bad, align, shape = -1, -2, -3
    fwd = lambda a, m: lib.omh_flash_attn_fwd_interval_d128(by(a), None if m is None else by(m), None)
    bwd = lambda a, m: lib.omh_flash_attn_bwd_interval_d128(by(a), None, None if m is None else by(m), None)
    assert lib.omh_flash_attn_fwd_interval_d128(None, None, None) == bad
    assert lib.omh_flash_attn_bwd_interval_d128(None, None, None, None) == bad
    assert lib.omh_flash_attn_fwd_interval_d128(None, by(mask()), None) == bad
    assert lib.omh_flash_attn_bwd_interval_d128(None, None, by(mask()), None) == bad
    for entry, args in ((fwd, fwd_args), (bwd, bwd_args)):
        assert entry(args(), None) == bad                                        # a null struct
        assert entry(args(), mask(group=7, qg=37, kg=55)) == bad                 # group < 8
        assert entry(args(), mask(reserved=1)) == bad
        assert entry(args(), mask(qg=5)) == bad                                  # not ceil(Lq / group)
        assert entry(args(), mask(kg=5)) == bad                                  # not ceil(Lk / group)
        assert entry(args(), mask(q_iv=None)) == bad
        assert entry(args(), mask(k_iv=None)) == bad
        assert entry(args(), mask(q_iv=P + 2)) == align
        assert entry(args(), mask(k_iv=P + 1)) == align
    # Lq + Lk >= 2^28 (few keys: the checks on K / V^T in front of it pass)
    g = 2 ** 20
    assert fwd(fwd_args(Lq=2 ** 28, Lk=64, ldv=64), mask(group=g, qg=256, kg=1)) == shape
    assert fwd(fwd_args(Lq=2 ** 28 - 128, Lk=64, ldv=64, q_lens=P + 2), mask(group=g, qg=256, kg=1)) == align   # just below: passes it
    # a band beside the mask; (0, 0) and (-1, -1) pass THAT check and are stopped by q_lens' alignment
    for wl, wr in ((16, 16), (-1, 0), (0, 5), (3, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr), mask()) == bad
    for wl, wr in ((0, 0), (-1, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr, q_lens=P + 2), mask()) == align
    assert bwd(bwd_args(o32=None), mask()) == bad                                # the backward needs the fp32 output
    assert lib.omh_flash_attn_bwd_interval_d128(by(bwd_args()), P + 2, by(mask()), None) == align
    assert bwd(bwd_args(phase=4, o_rs=256), mask()) == bad
    # the host table builder
    vis = (ctypes.c_uint8 * 5)(1, 0, 1, 0, 1)
    out = (ctypes.c_int32 * 20)()
    tables = lib.omh_interval_mask_tables
    addr = lambda x: ctypes.cast(x, ctypes.c_void_p)
    assert tables(addr(vis), 1, 5, addr(out), addr(out)) == bad                  # three runs in the row
    assert tables(addr(vis), 5, 1, addr(out), addr(out)) == bad                  # ... in the column
    assert tables(None, 1, 5, addr(out), addr(out)) == bad
    assert tables(addr(vis), 0, 5, addr(out), addr(out)) == bad
    assert tables(addr(vis), 1, 5, None, addr(out)) == bad
    two = (ctypes.c_uint8 * 5)(0, 1, 0, 1, 1)
    q_iv, k_iv = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 20)()
    assert tables(addr(two), 1, 5, addr(q_iv), addr(k_iv)) == 0
    assert list(q_iv) == [1, 2, 3, 5]
    assert [list(k_iv[4 * j:4 * j + 2]) for j in range(5)] == [[0, 0], [0, 1], [0, 0], [0, 1], [0, 1]]
    assert lib.omh_abi_version() == 12
    for name in ("omh_flash_attn_fwd_interval_d128", "omh_flash_attn_bwd_interval_d128", "omh_interval_mask_tables"):
        assert name in binding.EXPORTED and hasattr(lib, name)
    assert ctypes.sizeof(binding.IntervalMaskArgs) == 32


def test_python_refusals_without_gpu(omh, causal):
    ops = importlib.import_module(PKG + ".ops")
    attn = importlib.import_module(PKG + ".wan.modules.attention")
    m = causal.IntervalMask(causal.teacher_forcing_groups(2), 64)
    blocks = torch.ones(2, 2, dtype=torch.bool)
    at = dict(H=2, Lq=256, Lk=256, device=torch.device("cpu"))
    assert ops.attn_mask((16, 16), interval_mask=None, **at).kind == "band"
    with pytest.raises(ValueError):
        ops.attn_mask((16, -1), interval_mask=m, **at)
    with pytest.raises(ValueError):
        ops.attn_mask((-1, 0), interval_mask=m, **at)
    with pytest.raises(ValueError):
        ops.attn_mask(interval_mask=m, block_mask=blocks, **at)
    with pytest.raises(ValueError):
        ops.attn_mask(interval_mask=m, chunk_causal=(64, -1, 0), **at)
    with pytest.raises(ValueError):
        ops.attn_mask(interval_mask=m, **dict(at, Lq=320))                       # 5 x 4 groups expected
    with pytest.raises(ValueError):
        ops.attn_mask(interval_mask=m.vis, **at)                                 # the bare matrix carries no group size
    assert ops.attn_mask(interval_mask=m, **at).rule is m                        # already there: the same object
    q_iv, k_iv = m.intervals()                                                   # the tables, as lists
    assert q_iv == [[0, 1, 1, 1], [0, 2, 2, 2], [2, 3, 3, 3], [0, 1, 3, 4]]
    assert k_iv == [[0, 2, 3, 4], [1, 2, 2, 2], [2, 3, 3, 3], [3, 4, 4, 4]]
    # (the wrapper's own refusals run on real tensors in test_gpu_attn_interval.py)
    for fn in (attn.flash_attention, attn.attention, ops.flash_attn, ops.flash_attn_raw, ops.flash_attn_bwd, ops.flash_attn_func):
        assert "interval_mask" in inspect.signature(fn).parameters



def test_teacher_forcing_ref_is_pinned_to_the_oracle():
    """tests/teacher_forcing_ref.py with a uniform t, no clean half and an all-True mask is O.dit_forward (< 1e-6)."""
    import teacher_forcing_ref as R
    import make_golden_chunk_causal as MC
    from oracle import wan_dit_oracle as O
    cfg, xs, ctx, t, _ = MC.case()
    xs = [xs[0][:, :4], xs[1]]                                                  # 4 and 3 frames, padded to 4 x 56 tokens
    sd = O.synth_state_dict(cfg, MC.TAG)
    S = 4 * MC.TOKENS_PER_FRAME
    ref = O.dit_forward(sd, cfg, xs, t, ctx, S)
    with torch.no_grad():
        got = R.forward(sd, cfg, xs, t[:, None].expand(2, 4), ctx, S)
        masked = R.forward(sd, cfg, xs, t[:, None].expand(2, 4), ctx, S, mask=torch.ones(2, S, S, dtype=torch.bool))
    for a, b, c in zip(got, masked, ref):
        assert a.shape == c.shape
        assert float((a.double() - c.double()).norm() / c.double().norm()) < 1e-6
        assert float((b.double() - c.double()).norm() / c.double().norm()) < 1e-6
