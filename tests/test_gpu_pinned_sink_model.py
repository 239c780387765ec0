"""Unbounded rollouts on the GPU: ``causal.RollingKVCache(pin_sink=True)`` under ``WanModel.forward_chunk`` (state, bits,
translation invariance in time, parity with the fp32 restatement tests/pinned_sink_ref.py), rotary positions past the
table, and ``causal.sample`` / ``causal.stream`` with ``pin_sink`` and with the noise given chunk by chunk.  The tiny t2v
model of tests/make_golden_chunk_causal.py (2 layers, 56 tokens per frame), B = 2 clips.  Bounds as in
test_gpu_sink_model.py: forward against the restatement 8e-3, the same arithmetic on differently rounded keys 2e-3."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import pinned_sink_ref as PR
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_ROLLOUT = 8e-3, 2e-3
TPF = MC.TOKENS_PER_FRAME
PERIODIC = (1, 1, 1, 12)                                                         # fpc, W, S, F
_MEMO = {}


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _model(model_mod):
    cfg = MC.case()[0]
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    return m.cuda().eval().requires_grad_(False)


def _cuda(v):
    return [u.cuda() for u in v]


def _random_clip(F):
    g = torch.Generator().manual_seed(17)
    clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    return clean, noisy, torch.stack([torch.linspace(900., 100., F), torch.linspace(50., 950., F)])


def _rollout(m, cache, clean, noisy, ctx, t, fpc, F, after=None):
    """forward_chunk of every noisy chunk (commit=False) at t[:, I], the cache committed from the clean chunks at 0 (the
    pattern of test_gpu_sink_model._rollout); ``after(I)`` runs behind each of the two calls."""
    zero = torch.zeros(2, device="cuda")
    ctx, t = _cuda(ctx), t.cuda()
    out = []
    for I in range(F // fpc):
        sl = slice(I * fpc, (I + 1) * fpc)
        out.append(m.forward_chunk([u[:, sl].cuda() for u in noisy], t[:, I].contiguous(), ctx, cache, commit=False))
        if after is not None:
            after(I)
        m.forward_chunk([u[:, sl].cuda() for u in clean], zero, ctx, cache, commit=True)
        if after is not None:
            after(I)
    return out


def _periodic(model_mod, causal, pinned):
    """The periodic clip rolled out on the GPU, pinned or not — once."""
    key = ("gpu", pinned)
    if key not in _MEMO:
        fpc, W, S, F = PERIODIC
        clean, noisy, t = PR.periodic_clip(F)
        m = _model(model_mod)
        m.set_causal_chunks(fpc, W, S)
        cache = causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda", pin_sink=pinned)
        _MEMO[key] = _rollout(m, cache, clean, noisy, MC.case()[2], t, fpc, F)
    return _MEMO[key]


@pytest.mark.parametrize("fpc,W,S,F", ((1, 1, 1, 6), (2, 1, 1, 10)))
def test_pinned_cache_state_and_bits(model_mod, causal, ops, fpc, W, S, F):
    clean, noisy, t_frames = _random_clip(F)
    t, ctx = t_frames[:, ::fpc], MC.case()[2]
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W, S)
    Ct, n = fpc * TPF, S * fpc * TPF
    pinned = causal.RollingKVCache(m, 2, Ct, S, W, "cuda", pin_sink=True)
    plain = causal.RollingKVCache(m, 2, Ct, S, W, "cuda")
    deltas = PR.sink_deltas(F // fpc, W, S, fpc)
    seen = []

    def state(I):
        assert pinned.sink_delta == deltas[I]
        seen.append(pinned.sink_delta)
        if pinned.sink_rows == n:                                                # the live rows: the pristine ones, shifted once
            for live, pristine in zip(pinned.k, pinned.sink_k):
                assert torch.equal(live[:, :n], ops.rope_shift_frames(pristine, None, deltas[I]))

    a = _rollout(m, pinned, clean, noisy, ctx, t, fpc, F, after=state)
    b = _rollout(m, plain, clean, noisy, ctx, t, fpc, F)
    assert max(seen) == deltas[-1] > 0 and pinned.sink_rows == n
    for pristine, k in zip(pinned.sink_k, plain.k):                              # what an unpinned run keeps in its sink slots
        assert torch.equal(pristine, k[:, :n])
    for I in range(F // fpc):
        same = all(torch.equal(a[I][s], b[I][s]) for s in range(2))
        assert same == (I <= S + W), I                                           # nothing moves until the ring has wrapped
    pinned.reset()
    again = _rollout(m, pinned, clean, noisy, ctx, t, fpc, F)
    for I in range(F // fpc):
        assert torch.equal(again[I][0], a[I][0]) and torch.equal(again[I][1], a[I][1])
    # cut the last committed chunk and commit it again: the same bits, the same state
    last = F // fpc - 1
    sl = slice(last * fpc, F)
    args = ([u[:, sl].cuda() for u in clean], torch.zeros(2, device="cuda"), _cuda(ctx), pinned)
    pinned.truncate(last * Ct)
    one = m.forward_chunk(*args, commit=True)
    keys = [k.clone() for k in pinned.k]
    pinned.truncate(last * Ct)
    two = m.forward_chunk(*args, commit=True)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and pinned.sink_delta == deltas[-1]
    for k, k2 in zip(keys, pinned.k):
        assert torch.equal(k, k2)


def test_pinned_rollout_is_translation_invariant(model_mod, causal):
    """The periodic clip (identical non-sink chunks, identical noisy chunks, one t): with the sink pinned, every chunk past
    the wrap attends to the same keys at the same relative positions — the outputs agree up to the rounding of the
    re-rotated sink keys.  With absolute positions they drift with the clip index (the restatement: >= 4.4e-3)."""
    pinned, plain = _periodic(model_mod, causal, True), _periodic(model_mod, causal, False)
    for b in range(2):
        for I in range(4, 9):
            print(f"clip {b} chunk {I} against chunk 11: pinned rel-RMS {rel_rms(pinned[I][b], pinned[11][b]):.2e}, "
                  f"unpinned {rel_rms(plain[I][b], plain[11][b]):.2e}")
    for b in range(2):
        for I in range(4, 9):
            assert rel_rms(pinned[I][b], pinned[11][b]) < TOL_ROLLOUT, (b, I)


@pytest.mark.parametrize("setting", (PERIODIC, (2, 1, 1, 10)))
def test_pinned_rollout_against_the_restatement(model_mod, causal, setting):
    fpc, W, S, F = setting
    cfg, _, ctx, _, _ = MC.case()
    if setting == PERIODIC:
        clean, noisy, t = PR.periodic_clip(F)
        got = _periodic(model_mod, causal, True)
    else:
        clean, noisy, t_frames = _random_clip(F)
        t = t_frames[:, ::fpc]
        m = _model(model_mod)
        m.set_causal_chunks(fpc, W, S)
        got = _rollout(m, causal.RollingKVCache(m, 2, fpc * TPF, S, W, "cuda", pin_sink=True), clean, noisy, ctx, t, fpc, F)
    ref = PR.forward(O.synth_state_dict(cfg, MC.TAG), cfg, clean, noisy, t, ctx, causal, fpc, W, S)
    for I, chunk in enumerate(got):
        for b in range(2):
            err = rel_rms(chunk[b], ref[b][:, I * fpc:(I + 1) * fpc])
            print(f"{setting} chunk {I} clip {b}: pinned rollout against the restatement rel-RMS {err:.2e}")
            assert err < TOL_FWD


def test_frames_past_the_rotary_table(model_mod, causal):
    """Positions are relative: a chunk alone in its cache computes the same at frame 5 000 as at frame 0, up to the
    rounding of other cos / sin values.  (The table has 1 024 rows.)"""
    clean, _, _ = _random_clip(2)
    m = _model(model_mod)
    x, ctx, t = [u.cuda() for u in clean], _cuda(MC.case()[2]), torch.tensor([700., 300.], device="cuda")
    cache = causal.KVCache(m, 2, 2 * TPF, "cuda")
    base = m.forward_chunk(x, t, ctx, cache, frame_offset=0, commit=False)
    far = m.forward_chunk(x, t, ctx, cache, frame_offset=5000, commit=False)
    edge = m.forward_chunk(x, t, ctx, cache, frame_offset=1023, commit=False)    # one frame in the table, one past it
    for b in range(2):
        print(f"clip {b}: frame_offset 5000 against 0 rel-RMS {rel_rms(far[b], base[b]):.2e}, 1023 against 0 "
              f"{rel_rms(edge[b], base[b]):.2e}")
        assert torch.isfinite(far[b]).all()
        assert rel_rms(far[b], base[b]) < TOL_ROLLOUT and rel_rms(edge[b], base[b]) < TOL_ROLLOUT
    assert len(m._rope_shift_cache[1]) <= 4


def test_sample_and_stream_open_ended(model_mod, causal):
    unipc = importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc")
    ctx = _cuda(MC.case()[2])
    m = _model(model_mod)
    noise = torch.randn(16, 6, 14, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    cond, null = ctx[:1], [ctx[0][:5]]

    def make_scheduler():
        s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(2, device="cuda", shift=3.0)
        return s

    kw = dict(frames_per_chunk=1, left_chunks=1, sink_chunks=1, make_scheduler=make_scheduler, guide_scale=5.0)
    plain = causal.sample(m, noise, cond, null, **kw)
    pinned = causal.sample(m, noise, cond, null, pin_sink=True, **kw)
    assert pinned.shape == (16, 6, 14, 16) and torch.isfinite(pinned).all() and m._causal_chunks is None
    assert torch.equal(pinned[:, :3], plain[:, :3]) and not torch.equal(pinned[:, 3:], plain[:, 3:])
    caches = tuple(causal.RollingKVCache(m, 1, TPF, 1, 1, "cuda", pin_sink=True) for _ in range(2))
    assert torch.equal(causal.sample(m, noise, cond, null, pin_sink=True, caches=caches, **kw), pinned)
    assert caches[0].sink_delta == caches[1].sink_delta == PR.sink_deltas(6, 1, 1, 1)[-1] == 3
    # the noise chunk by chunk, from a generator that does not know its length: the bits of the whole tensor
    for pin in (False, True):
        whole = list(causal.stream(m, noise, cond, null, pin_sink=pin, **kw))
        parts = list(causal.stream(m, (noise[:, f:f + 1] for f in range(6)), cond, null, pin_sink=pin, **kw))
        assert len(parts) == len(whole) == 6 and m._causal_chunks is None
        for a, b in zip(parts, whole):
            assert a.index == b.index and a.frames == b.frames and torch.equal(a.wait().latents, b.wait().latents)
        assert torch.equal(torch.cat([c.latents for c in whole], 1), pinned if pin else plain)
    kw2 = dict(kw, frames_per_chunk=2)                                           # a short last item
    whole = causal.sample(m, noise[:, :5], cond, null, pin_sink=True, **kw2)
    parts = causal.sample(m, iter([noise[:, 0:2], noise[:, 2:4], noise[:, 4:5]]), cond, null, pin_sink=True, **kw2)
    assert torch.equal(whole, parts)
