"""Three-run interval masks and the rolling cache, the part that needs no GPU: omh_interval_mask_tables3 against a
brute-force run finder, causal.IntervalMask(runs=2 / 3), its tile count against the dense mask,
causal.teacher_forcing_groups with a sink, the slot arithmetic of causal.RollingKVCache and the argument checks of
omh_flash_attn_fwd_interval3_d128 / omh_flash_attn_bwd_interval3_d128."""
import ctypes
import importlib

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


def _random_matrix(g, nq, nk, max_runs=3):
    """A random bool matrix with at most ``max_runs`` runs per row and per column (rows drawn, then redrawn until the
    columns fit)."""
    while True:
        m = torch.zeros(nq, nk, dtype=torch.bool)
        for r in range(nq):
            cuts = sorted(torch.randint(0, nk + 1, (2 * int(torch.randint(0, max_runs + 1, (1,), generator=g)),),
                                        generator=g).tolist())
            for a, b in zip(cuts[0::2], cuts[1::2]):
                m[r, a:b] = True
        if all(len(_runs(row)) <= max_runs for row in m.tolist()) and all(len(_runs(c)) <= max_runs for c in m.t().tolist()):
            return m


def _check_tables(mask, vis, slots):
    for table, lines in ((mask.q_iv, vis.tolist()), (mask.k_iv, vis.t().tolist())):
        assert table.dtype == torch.int32 and table.shape == (len(lines), 2 * slots)
        for got, line in zip(table.tolist(), lines):
            assert all(a <= b for a, b in zip(got, got[1:]))                     # lo0 <= hi0 <= lo1 <= ...
            pairs = list(zip(got[0::2], got[1::2]))
            runs = _runs(line)
            assert [p for p in pairs if p[1] > p[0]] == runs
            assert all(p[1] > p[0] for p in pairs[:len(runs)])                   # filled in ascending order from slot 0


def test_tables3_against_brute_force(causal):
    g = torch.Generator().manual_seed(11)
    seen = 0
    for _ in range(40):
        nq, nk = (int(torch.randint(1, 12, (1,), generator=g)) for _ in range(2))
        vis = _random_matrix(g, nq, nk)
        m = causal.IntervalMask(vis, 8, runs=3)
        assert m.runs == 3 and (m.q_groups, m.k_groups) == (nq, nk)
        _check_tables(m, vis, 3)
        seen = max(seen, max(len(_runs(r)) for r in vis.tolist()))
    assert seen == 3
    # slot order and empties, written out
    m = causal.IntervalMask([[0, 1, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1, 1]], 8, runs=3)
    assert m.intervals()[0] == [[1, 2, 3, 5, 6, 7], [0, 0, 0, 0, 0, 0], [0, 2, 2, 2, 2, 2], [2, 3, 5, 7, 7, 7]]
    assert m.intervals()[1][0] == [2, 3, 3, 3, 3, 3] and m.intervals()[1][6] == [0, 1, 3, 4, 4, 4]
    # a fourth run, in a row and in a column
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 0, 1, 0, 1, 0, 1]], 8, runs=3)
    with pytest.raises(ValueError):
        causal.IntervalMask([[1], [0], [1], [0], [1], [0], [1]], 8, runs=3)
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 1]], 7, runs=3)                                 # group < 8
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 1]], 8, runs=4)


def test_runs_2_is_unchanged(causal):
    g = torch.Generator().manual_seed(12)
    for _ in range(20):
        nq, nk = (int(torch.randint(1, 10, (1,), generator=g)) for _ in range(2))
        vis = _random_matrix(g, nq, nk, max_runs=2)
        m, m2 = causal.IntervalMask(vis, 16), causal.IntervalMask(vis, 16, runs=2)
        assert m.runs == 2 and torch.equal(m.q_iv, m2.q_iv) and torch.equal(m.k_iv, m2.k_iv)
        _check_tables(m, vis, 2)
        m3 = causal.IntervalMask(vis, 16, runs=3)                                # the same runs, one more empty slot
        assert torch.equal(m3.q_iv[:, :4], m.q_iv) and torch.equal(m3.k_iv[:, :4], m.k_iv)
        assert m3.tiles(nq * 16, nk * 16) == m.tiles(nq * 16, nk * 16)
    m = causal.IntervalMask(causal.teacher_forcing_groups(2), 64)
    assert m.intervals()[0] == [[0, 1, 1, 1], [0, 2, 2, 2], [2, 3, 3, 3], [0, 1, 3, 4]]
    binding = importlib.import_module(PKG + "._lib")
    assert isinstance(m.c_struct(), binding.IntervalMaskArgs)
    assert isinstance(causal.IntervalMask([[1]], 8, runs=3).c_struct(), binding.Interval3MaskArgs)
    assert m.to("cpu") is m and causal.IntervalMask([[1]], 8, runs=3).to("cpu").runs == 3
    with pytest.raises(ValueError):                                              # a third run is still refused
        causal.IntervalMask([[1, 0, 1, 0, 1]], 8)
    with pytest.raises(ValueError):
        causal.IntervalMask(causal.teacher_forcing_groups(6, 1, 1), 8)


def _dense_tiles(causal, mask, Lq, Lk, block=128, tile=64):
    """The tile count from the dense mask: per workgroup, per slot i the hull of the i-th runs of its rows' groups, then
    the union of the hulls in tiles, neighbours that touch merged (a merge adds no tile: the ranges are counted as sets,
    plus the tiles between two ranges that touch or overlap — none, by definition)."""
    dense = causal.interval_visible(mask, Lq, Lk)
    total = 0
    for q0 in range(0, Lq, block):
        hulls = {}
        for g0 in range(q0 // mask.group * mask.group, min(q0 + block, Lq), mask.group):   # one row per group
            for i, (a, b) in enumerate(_runs(dense[max(g0, q0)].tolist())):
                lo, hi = hulls.get(i, (a, b))
                hulls[i] = (min(lo, a), max(hi, b))
        tiles = set()
        for a, b in hulls.values():
            tiles |= set(range(a // tile, (b - 1) // tile + 1))
        total += len(tiles)
    return total


@pytest.mark.parametrize("n,W,S,group", [(6, 1, 1, 40), (6, 1, 1, 200), (4, 1, 1, 1560), (5, 2, 2, 24), (16, 1, 1, 8)])
def test_tiles_of_three_runs_against_the_dense_mask(causal, n, W, S, group):
    m = causal.IntervalMask(causal.teacher_forcing_groups(n, W, S), group, runs=3)
    L = 2 * n * group
    assert m.tiles(L, L) == _dense_tiles(causal, m, L, L)
    assert m.tiles(L, L) < ((L + 127) // 128) * ((L + 63) // 64)                 # and it skips something


def test_teacher_forcing_groups_with_a_sink(causal):
    for n in range(1, 12):
        for W in range(-1, 6):
            assert torch.equal(causal.teacher_forcing_groups(n, W, 0), causal.teacher_forcing_groups(n, W))
            for S in range(1, 5):
                vis = causal.teacher_forcing_groups(n, W, S)
                if W < 0:
                    assert torch.equal(vis, causal.teacher_forcing_groups(n, W))
                    continue
                for I in range(n):
                    clean = [j < I and (j >= I - W or j < S) for j in range(n)]
                    assert vis[n + I].tolist() == clean + [j == I for j in range(n)]   # clean sink U clean window U own
                    assert vis[I].tolist() == [j <= I and (j >= I - W or j < S) for j in range(n)] + [False] * n
                assert max(len(_runs(r)) for r in vis.tolist()) <= 3
                assert max(len(_runs(c)) for c in vis.t().tolist()) <= 2
    assert max(len(_runs(r)) for r in causal.teacher_forcing_groups(6, 1, 1).tolist()) == 3
    with pytest.raises(ValueError):
        causal.teacher_forcing_groups(4, 1, -1)


class _FakeModel:
    dim = 16
    patch_size = (1, 2, 2)
    blocks = [None, None]


def test_rolling_cache_slots(causal):
    for S in range(0, 4):
        for W in range(0, 4):
            C = 16
            c = causal.RollingKVCache(_FakeModel(), 2, C, S, W, "cpu")
            assert c.slots == S + W + 1 and c.cap == (S + W + 1) * C and c.rolling
            assert len(c.k) == 2 and c.k[0].shape == (2, c.cap, 16) and c.vt[0].shape == (2, 16, (c.cap + 63) // 64 * 64)
            assert c._vt_store[0].numel() == c.vt[0].numel() + 64
            assert c.resident() == {}
            for I in range(3 * (S + W + 1) + 2):
                # chunk I goes to the slot of a chunk it does not see (or a free one)
                before = c.resident()
                slot = c.slot(I)
                assert 0 <= slot < c.slots
                if slot in before:
                    assert before[slot] == I - W - 1 and before[slot] >= S
                c.advance(C)
                assert c.length == (I + 1) * C                                   # it does not stop at the capacity
                want = {j for j in range(I + 1) if j < S or j >= I - W}
                res = c.resident()
                assert set(res.values()) == want and all(c.slot(j) == s for s, j in res.items())
                assert len(set(res)) == len(want)                                # no two resident chunks share a slot
            c.reset()
            assert c.length == 0 and c.resident() == {}


def test_rolling_cache_refusals(causal):
    M = _FakeModel()
    for bad in ((0, 16, 1, 1), (1, 0, 1, 1), (1, 16, -1, 1), (1, 16, 1, -1)):
        with pytest.raises(ValueError):
            causal.RollingKVCache(M, *bad, "cpu")
    c = causal.RollingKVCache(M, 1, 16, 1, 1, "cpu")
    c.advance(16)
    c.advance(8)
    with pytest.raises(ValueError):
        c.advance(16)                                                            # crosses the end of the chunk
    c.truncate(16)
    c.advance(16)
    c.advance(16)
    assert c.length == 48
    c.truncate(40)
    c.truncate(32)                                                               # the start of the last committed chunk
    with pytest.raises(ValueError):
        c.truncate(16)                                                           # an earlier chunk: its window may be gone
    with pytest.raises(ValueError):
        c.truncate(48)
    sample = causal.sample
    with pytest.raises(ValueError):                                              # rolling needs a bounded look-back
        sample(M, torch.zeros(16, 4, 14, 16), None, None, frames_per_chunk=1, left_chunks=-1, make_scheduler=None,
               guide_scale=1.0, rolling=True)


def test_interval3_entries_validate_without_gpu(omh):
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
        return binding.Interval3MaskArgs(group, qg, kg, reserved, q_iv, k_iv)

    bad, align, shape = -1, -2, -3
    fwd = lambda a, m: lib.omh_flash_attn_fwd_interval3_d128(by(a), None if m is None else by(m), None)
    bwd = lambda a, m: lib.omh_flash_attn_bwd_interval3_d128(by(a), None, None if m is None else by(m), None)
    assert lib.omh_flash_attn_fwd_interval3_d128(None, by(mask()), None) == bad
    assert lib.omh_flash_attn_bwd_interval3_d128(None, None, by(mask()), None) == bad
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
    g = 2 ** 20
    assert fwd(fwd_args(Lq=2 ** 28, Lk=64, ldv=64), mask(group=g, qg=256, kg=1)) == shape
    for wl, wr in ((16, 16), (-1, 0), (0, 5), (3, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr), mask()) == bad
    for wl, wr in ((0, 0), (-1, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr, q_lens=P + 2), mask()) == align
    assert bwd(bwd_args(o32=None), mask()) == bad                                # the backward needs the fp32 output
    assert lib.omh_flash_attn_bwd_interval3_d128(by(bwd_args()), P + 2, by(mask()), None) == align
    assert bwd(bwd_args(phase=4, o_rs=256), mask()) == bad
    # the host table builder
    addr = lambda x: ctypes.cast(x, ctypes.c_void_p)
    tables = lib.omh_interval_mask_tables3
    four = (ctypes.c_uint8 * 7)(1, 0, 1, 0, 1, 0, 1)
    out = (ctypes.c_int32 * 42)()
    assert tables(addr(four), 1, 7, addr(out), addr(out)) == bad                 # four runs in the row
    assert tables(addr(four), 7, 1, addr(out), addr(out)) == bad                 # ... in the column
    assert tables(None, 1, 7, addr(out), addr(out)) == bad
    assert tables(addr(four), 0, 7, addr(out), addr(out)) == bad
    assert tables(addr(four), 1, 7, None, addr(out)) == bad
    three = (ctypes.c_uint8 * 5)(1, 0, 1, 0, 1)
    q_iv, k_iv = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 30)()
    assert tables(addr(three), 1, 5, addr(q_iv), addr(k_iv)) == 0
    assert list(q_iv) == [0, 1, 2, 3, 4, 5]
    assert [list(k_iv[6 * j:6 * j + 2]) for j in range(5)] == [[0, 1], [0, 0], [0, 1], [0, 0], [0, 1]]
    assert lib.omh_interval_mask_tables(addr(three), 1, 5, addr(out), addr(out)) == bad   # the two-run builder still refuses it
    assert lib.omh_abi_version() == 12
    for name in ("omh_flash_attn_fwd_interval3_d128", "omh_flash_attn_bwd_interval3_d128", "omh_interval_mask_tables3"):
        assert name in binding.EXPORTED and hasattr(lib, name)
    assert ctypes.sizeof(binding.Interval3MaskArgs) == 32


def test_set_causal_chunks_sink_is_normalised(omh):
    model_mod = importlib.import_module(PKG + ".wan.modules.model")
    import make_golden_chunk_causal as MC
    m = model_mod.WanModel(num_layers=1, **MC.make_golden.TINY)
    m.set_causal_chunks(2, 1)
    assert m._causal_chunks == (2, 1) and m._causal_sink() == 0                  # no sink: the tuple as it always was
    m.set_causal_chunks(2, 1, 0)
    assert m._causal_chunks == (2, 1)
    m.set_causal_chunks(2, 1, 3)
    assert m._causal_chunks == (2, 1, 3) and m._causal_sink() == 3
    assert m._causal_rule([(4, 7, 8)]) == (2 * 56, 1, 0)
    m.set_causal_chunks(2, -1, 3)                                                # an unbounded look-back sees the sink anyway
    assert m._causal_chunks == (2, -1) and m._causal_sink() == 0
    with pytest.raises(ValueError):
        m.set_causal_chunks(2, 1, -1)
    m.set_causal_chunks(None)
    assert m._causal_chunks is None and m._causal_sink() == 0
