"""Host checks for unbounded rollouts (no GPU): the restatement of a pinned attention sink (tests/pinned_sink_ref.py) and
its translation invariance, rotary positions past the table, the bookkeeping of causal.RollingKVCache(pin_sink=True), the
new refusals and the header entry."""
import importlib
import os
import re

import pytest
import torch

import make_golden_chunk_causal as MC
import pinned_sink_ref as PR
import teacher_forcing_ref as R
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPF = MC.TOKENS_PER_FRAME
DELTAS = (0, 1, 3, 1000, 10 ** 6)


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def periodic(causal):
    """The periodic clip at (fpc, W, S, F) = (1, 1, 1, 12) through the restatement, pinned and not — once."""
    return PR.periodic_restatement(causal, True), PR.periodic_restatement(causal, False)


def test_sink_deltas():
    assert PR.sink_deltas(7, 1, 1, 1) == [0, 0, 0, 1, 2, 3, 4]
    assert PR.sink_deltas(7, 1, 2, 2) == [0, 0, 0, 0, 2, 4, 6]
    assert PR.sink_deltas(6, 2, 1, 3) == [0, 0, 0, 0, 3, 6]


def test_restatement_without_a_shift_is_teacher_forcing(causal):
    """Every Delta_I = 0 (a clip that ends before the ring wraps, and ``pinned=False`` on a longer one): the operations of
    teacher_forcing_ref.forward, hence its result exactly."""
    cfg, _, ctx, _, _ = MC.case()
    sd = O.synth_state_dict(cfg, MC.TAG)
    g = torch.Generator().manual_seed(3)
    for F, pinned in ((3, True), (5, False)):
        clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
        noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
        t = torch.stack([torch.linspace(900., 100., F), torch.linspace(50., 950., F)])
        assert pinned is False or not any(PR.sink_deltas(F, 1, 1, 1))
        got = PR.forward(sd, cfg, clean, noisy, t, ctx, causal, 1, 1, 1, pinned=pinned)
        m = causal.IntervalMask(causal.teacher_forcing_groups(F, 1, 1), TPF, runs=3)
        mask = causal.interval_visible(m, 2 * F * TPF, 2 * F * TPF)[None].expand(2, -1, -1)
        with torch.no_grad():
            ref = R.forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(clean, noisy)],
                            torch.cat([torch.zeros(2, F), t], 1), ctx, 2 * F * TPF, mask=mask, segments=2, out_from=F)
        for a, b in zip(got, ref):
            err = float((a - b).abs().max())
            print(f"F = {F} pinned = {pinned}: restatement against teacher forcing, max |diff| {err}")
            assert err == 0.0


def test_pinned_rollout_is_translation_invariant(periodic):
    """The periodic clip: pinned, every chunk past the wrap computes what the last one does (fp32 noise); with absolute
    positions the output drifts with the clip index, for no reason but the sink's growing distance."""
    pinned, plain = periodic
    for b in range(2):
        last_p, last_u = pinned[b][:, 11], plain[b][:, 11]
        for I in range(4, 11):
            err = rel_rms(pinned[b][:, I], last_p)
            print(f"clip {b} chunk {I}: pinned against chunk 11 rel-RMS {err:.2e}")
            assert err < 1e-5
        for I in range(4, 9):
            err = rel_rms(plain[b][:, I], last_u)
            print(f"clip {b} chunk {I}: unpinned against chunk 11 rel-RMS {err:.2e}")
            assert err > 2e-3
        for I in range(3):                                                       # before the wrap nothing is shifted
            assert torch.equal(pinned[b][:, I], plain[b][:, I])


def test_emulated_shift_meets_the_kernel_bound():
    """The bound of tests/test_gpu_rope_shift.py, |err| <= 2^-8 |y| + 2^-20 hypot(x0, x1), holds for the stated arithmetic
    at every delta — and is broken by an fp32 angle at delta = 10^6, which is what it is there to catch."""
    g = torch.Generator().manual_seed(11)
    src = torch.randn(2, 56, 256, generator=g).to(torch.bfloat16)
    for delta in DELTAS:
        y, rotated, hyp = PR.shift_exact(src, delta)
        bound = 2.0 ** -8 * y.abs() + 2.0 ** -20 * hyp
        got = PR.shift_emulated(src, None, delta)
        err = (got.double() - y).abs()
        assert bool((err <= bound)[rotated].all()), delta
        assert torch.equal(got[~rotated], src[~rotated])
        if delta == 0:
            assert torch.equal(got, src)
    bad = PR.shift_emulated(src, None, 10 ** 6, fp32_angle=True)
    frac = float(((bad.double() - y).abs() > bound)[rotated].double().mean())
    print(f"fp32 angle at delta = 1e6: {100 * frac:.1f} % of the rotated elements leave the bound")
    assert frac > 0.05


def test_rope_positions_past_the_table(model_mod):
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    assert m.freqs.shape == (1024, 64)
    cos, sin = m._rope("cpu")
    D = 128
    nf = (D - 4 * (D // 6)) // 2
    assert m._rope_shifted("cpu", 0, 3)[0] is cos
    for fo, f in ((5, 3), (1021, 3), (1000, 24)):                                # inside the table: its rows, sliced
        c2, s2 = m._rope_shifted("cpu", fo, f)
        assert torch.equal(c2[:f, :nf], cos[fo:fo + f, :nf]) and torch.equal(s2[:f, :nf], sin[fo:fo + f, :nf])
        assert torch.equal(c2[:, nf:], cos[:, nf:]) and torch.equal(s2[:, nf:], sin[:, nf:])
    for fo, f in ((5000, 3), (1022, 3), (20000, 2)):                         # past it: what a longer table would hold
        c2, s2 = m._rope_shifted("cpu", fo, f)
        ang = O.rope_table(D, max_len=fo + f)[fo:, :nf]
        assert torch.equal(c2[:f, :nf], torch.cos(ang).float()) and torch.equal(s2[:f, :nf], torch.sin(ang).float())
        assert torch.equal(c2[:, nf:], cos[:, nf:]) and torch.equal(s2[:, nf:], sin[:, nf:])
        assert c2.shape == cos.shape
    for fo in range(2000, 2040):                                                 # a stream: a new offset every chunk
        m._rope_shifted("cpu", fo, 1)
    assert len(m._rope_shift_cache[1]) <= 4
    assert m._rope_shifted("cpu", 2039, 1)[0] is m._rope_shifted("cpu", 2039, 1)[0]


class _FakeModel:
    dim = 16
    patch_size = (1, 2, 2)
    blocks = [None, None]


def _fill(cache, chunk, g):
    """What a forward_chunk pass leaves in the chunk's slot: fresh key rows."""
    C, s = cache.chunk_tokens, cache.slot(chunk)
    for k in cache.k:
        k[:, s * C:(s + 1) * C] = torch.randn(cache.batch, C, cache.dim, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("S,W,fpc", ((1, 1, 1), (2, 1, 2), (1, 2, 3)))
def test_pinned_cache_bookkeeping(causal, S, W, fpc):
    C, HD = 8, 16
    g = torch.Generator().manual_seed(5)
    c = causal.RollingKVCache(_FakeModel(), 2, C, S, W, "cpu", pin_sink=True)
    c._shift = PR.shift_emulated                                                 # (ops.rope_shift_frames runs on the GPU only)
    assert c.pin_sink and c.sink_delta == 0 and c.sink_rows == 0
    assert len(c.sink_k) == 2 and c.sink_k[0].shape == (2, S * C, 16) and c.sink_k[0].dtype == torch.bfloat16
    n = S * C

    def live_is_shifted():
        for pristine, k in zip(c.sink_k, c.k):
            assert torch.equal(k[:, :n], PR.shift_emulated(pristine, None, c.sink_delta, HD))

    first = None
    for I in range(S + W + 5):
        assert c.sink_shift_chunks(I) == max(S, I - W) - S
        c.pin(fpc, HD)
        assert c.sink_delta == PR.sink_deltas(I + 1, W, S, fpc)[I]
        _fill(c, I, g)
        if I < S:
            assert c.sink_delta == 0
        c.advance(C)
        assert c.sink_rows == min(I + 1, S) * C
        if I == S - 1:
            first = [p.clone() for p in c.sink_k]
            for p, k in zip(c.sink_k, c.k):
                assert torch.equal(p, k[:, :n])                                  # the pristine copy: the rows as committed
        if I >= S:
            live_is_shifted()
            for p, q in zip(c.sink_k, first):
                assert torch.equal(p, q)                                         # and it never changes afterwards
    last = S + W + 4
    assert c.sink_delta == (last - W - S) * fpc > 0
    # cut the last committed chunk and run it again: the shift it needs is still the one the rows hold; one chunk on, the next
    c.truncate(last * C)
    c.pin(fpc, HD)
    assert c.sink_delta == (last - W - S) * fpc
    c.advance(C)
    c.pin(fpc, HD)
    assert c.sink_delta == (last + 1 - W - S) * fpc
    live_is_shifted()
    c.truncate(last * C)                                                         # ... and back: derived from the pristine rows again
    c.pin(fpc, HD)
    assert c.sink_delta == (last - W - S) * fpc
    live_is_shifted()
    c.reset()
    assert (c.length, c.sink_delta, c.sink_rows) == (0, 0, 0)
    # a cut into a sink chunk invalidates its pristine rows until they are committed again
    _fill(c, 0, g)
    c.advance(C)
    assert c.sink_rows == C
    c.truncate(C // 2)
    assert c.sink_rows == C // 2
    _fill(c, 0, g)
    c.advance(C // 2)
    assert c.sink_rows == C
    for p, k in zip(c.sink_k, c.k):
        assert torch.equal(p[:, C // 2:C], k[:, C // 2:C])
    # without pin_sink nothing of this exists, and pin() is a no-op
    plain = causal.RollingKVCache(_FakeModel(), 2, C, S, W, "cpu")
    assert plain.pin_sink is False and plain.sink_k is None
    for I in range(S + W + 3):
        plain.pin(fpc, HD)
        plain.advance(C)
    assert plain.sink_delta == 0


def test_refusals(causal, model_mod):
    M = _FakeModel()
    with pytest.raises(ValueError, match="pin_sink"):
        causal.RollingKVCache(M, 1, 8, 0, 1, "cpu", pin_sink=True)
    noise = torch.zeros(16, 4, 14, 16)
    kw = dict(frames_per_chunk=1, make_scheduler=None, guide_scale=1.0)
    for fn in (causal.sample, causal.stream):
        with pytest.raises(ValueError, match="pin_sink"):                        # no sink to pin
            fn(None, noise, None, None, left_chunks=1, pin_sink=True, **kw)
        with pytest.raises(ValueError, match="pin_sink"):                        # (a sink needs a window)
            fn(None, noise, None, None, left_chunks=-1, sink_chunks=1, pin_sink=True, **kw)
        plain = tuple(causal.RollingKVCache(M, 1, 56, 1, 1, "cpu") for _ in range(2))
        pinned = tuple(causal.RollingKVCache(M, 1, 56, 1, 1, "cpu", pin_sink=True) for _ in range(2))
        with pytest.raises(ValueError, match="pin_sink"):                        # the caller's caches must match
            fn(None, noise, None, None, left_chunks=1, sink_chunks=1, pin_sink=True, caches=plain, **kw)
        with pytest.raises(ValueError, match="pin_sink"):
            fn(None, noise, None, None, left_chunks=1, sink_chunks=1, caches=pinned, **kw)
        chunks = lambda: iter([noise[:, :1], noise[:, 1:2]])
        with pytest.raises(ValueError, match="rolling"):                         # chunk by chunk: no length for a KVCache
            fn(None, chunks(), None, None, left_chunks=1, **kw)
        with pytest.raises(ValueError, match="rolling"):
            fn(None, chunks(), None, None, left_chunks=-1, **kw)
        flat = (causal.KVCache(M, 1, 224, "cpu"), causal.KVCache(M, 1, 224, "cpu"))
        with pytest.raises(ValueError, match="rolling"):
            fn(None, chunks(), None, None, left_chunks=1, caches=flat, **kw)
    src = lambda items: list(causal._noise_chunks("t", iter(items), 2))
    got = src([noise[:, :2], noise[:, 2:4], noise[:, :1]])
    assert [(f0, u.shape[1], last) for f0, u, last in got] == [(0, 2, False), (2, 2, False), (4, 1, True)]
    assert [(f0, u.shape[1], last) for f0, u, last in causal._noise_chunks("t", noise[:, :3], 2)] == [(0, 2, False), (2, 1, True)]
    with pytest.raises(ValueError, match="last"):                                # a short chunk in the middle
        src([noise[:, :1], noise[:, 2:4]])
    with pytest.raises(ValueError):                                              # three frames in chunks of two
        src([noise[:, :3]])
    with pytest.raises(ValueError):                                              # another H
        src([noise[:, :2], noise[:, :2, :7]])
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.set_causal_chunks(1, 1, 1)
    cache = causal.RollingKVCache(m, 1, TPF, 1, 1, "cpu", pin_sink=True)
    with pytest.raises(ValueError, match="pin_sink"):                            # no gradient path under a pinned sink
        m.forward_chunk([noise[:, :1]], torch.zeros(1), [torch.zeros(4, 64)], cache, grad=True)


def test_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "omh.h")).read()
    assert re.search(r"#define\s+OMH_ABI_VERSION\s+12\b", text)
    assert re.search(r"\bint\s+omh_rope_shift_frames\s*\(", text)
    lib = importlib.import_module(PKG + "._lib")
    assert "omh_rope_shift_frames" in lib.EXPORTED and lib.ABI_VERSION == 12 and lib.lib.omh_abi_version() == 12
    ops = importlib.import_module(PKG + ".ops")
    assert "rope_shift_frames" in ops.__all__
    with pytest.raises(ops.OmhError):                                            # no CPU path
        ops.rope_shift_frames(torch.zeros(1, 8, 128, dtype=torch.bfloat16), None, 1)
