"""``WanModel.forward_chunk(grad=True)`` and ``causal.self_forcing_rollout`` (self forcing) against the fp32 restatement
tests/self_forcing_ref.py: the tiny 2-layer t2v model of tests/make_golden_chunk_causal.py (56 tokens per frame), B = 2
clips [16, F, 14, 16], settings (frames per chunk, left_chunks, F) = (1, -1, 6) and (2, 1, 8).

Bounds: the project's own (test_gpu_teacher_forcing_model.py, test_gpu_sink_model.py): forward 8e-3, gradients and loss
2e-2.  Bitwise comparisons of gradients run under ``ops.set_deterministic(True)``, the mode in which the library promises
a backward that repeats bit for bit (a few launches add partial sums with float atomics otherwise)."""
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import self_forcing_ref as SF
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD, TOL_LOSS = 8e-3, 2e-2, 2e-2
TPF = SF.TPF
mse = torch.nn.functional.mse_loss


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


@pytest.fixture()
def deterministic():
    ops = importlib.import_module(PKG + ".ops")
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


def _model(model_mod, train=True):
    cfg = MC.case()[0]
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(cfg, MC.TAG))
    m = m.cuda()
    return m.train() if train else m.eval().requires_grad_(False)


def _cuda(v):
    return [u.cuda() for u in v]


def _chunk(v, I, fpc):
    return [u[:, I * fpc:(I + 1) * fpc].contiguous() for u in v]


def _teacher_rollout(m, causal, fpc, W, F, mode="one", clean=None, only=None, x_grad=True, t_grad=True):
    """For I = 0 .. n - 1: out_I = forward_chunk(noisy_I, t[:, I], grad=True, commit=False), then, under no_grad, the commit
    of clean_I at t = 0 (which overwrites the chunk's own rows).  loss_I = sum over the clips of MSE(out_I, target_I) / n.
    ``mode`` "one": one backward() of the summed loss at the end; "each": backward() of loss_I right behind its forward,
    accumulated into .grad; "separate": likewise, but each chunk's parameter gradients are taken out and returned as a
    list.  ``only``: the loss of that chunk alone."""
    cfg, clean0, noisy, target, ctx, t = SF.inputs(F, fpc)
    clean = clean0 if clean is None else clean
    n, ctx_d = F // fpc, _cuda(ctx)
    m.set_causal_chunks(fpc, W)
    cache = causal.KVCache(m, 2, F * TPF, "cuda")
    tg = t.cuda().requires_grad_(t_grad)
    xc = [u.cuda().requires_grad_(True) for u in clean]
    xn, outs, losses, per_chunk = [], [], [], []
    zero = torch.zeros(2, device="cuda")
    params = dict(m.named_parameters())
    for I in range(n):
        x = [u.cuda().requires_grad_(x_grad) for u in _chunk(noisy, I, fpc)]
        out = m.forward_chunk(x, tg[:, I].contiguous(), ctx_d, cache, commit=False, grad=True)
        loss = sum(mse(o, v.cuda()) for o, v in zip(out, _chunk(target, I, fpc))) / n
        xn.append(x), outs.append([o.detach() for o in out]), losses.append(loss)
        if mode != "one" and (only is None or only == I):
            loss.backward()
            if mode == "separate":
                per_chunk.append({k: p.grad for k, p in params.items() if p.grad is not None})
                m.zero_grad(set_to_none=True)
        with torch.no_grad():
            m.forward_chunk(_chunk([u.detach() for u in xc], I, fpc), zero, ctx_d, cache, commit=True)
    assert cache.length == F * TPF
    total = sum(losses) if only is None else losses[only]
    if mode == "one":
        total.backward()
    assert all(u.grad is None for u in xc)                                   # the clean latents get no gradient
    return dict(loss=total.detach(), grads={k: p.grad for k, p in params.items()}, per_chunk=per_chunk, outs=outs,
                d_noisy=[torch.cat([torch.zeros_like(xn[I][b]) if xn[I][b].grad is None else xn[I][b].grad
                                    for I in range(n)], 1) if x_grad else None for b in range(2)],
                d_t=tg.grad, cache=cache)


@pytest.mark.parametrize("fpc,W,F", SF.SETTINGS)
def test_forward_bits_are_the_inference_call(model_mod, causal, fpc, W, F):
    """grad=True on a trainable model: the bits of the no_grad call on the same cache state, at an empty cache and behind
    committed chunks; commit= keeps its meaning; without anything that requires grad it is the inference call."""
    cfg, clean, noisy, _, ctx, t = SF.inputs(F, fpc)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    cache = causal.KVCache(m, 2, F * TPF, "cuda")
    ctx_d, zero, C = _cuda(ctx), torch.zeros(2, device="cuda"), fpc * TPF
    for I in range(3):
        x, tt = _cuda(_chunk(noisy, I, fpc)), t[:, I].cuda().contiguous()
        with torch.no_grad():
            want = m.forward_chunk(x, tt, ctx_d, cache, commit=False)
            same = m.forward_chunk(x, tt, ctx_d, cache, commit=False, grad=True)      # nothing to differentiate: inference
        got = m.forward_chunk(x, tt, ctx_d, cache, commit=False, grad=True)
        assert cache.length == I * C
        for a, b, c in zip(got, want, same):
            assert a.requires_grad and a.grad_fn is not None and not c.requires_grad
            assert a.shape == (16, fpc, 14, 16) and a.dtype == torch.float32
            assert torch.equal(a.detach(), b) and torch.equal(c, b)
        with pytest.raises(RuntimeError):                                    # today's refusal stays the default
            m.forward_chunk(x, tt, ctx_d, cache, commit=False)
        if I < 2:
            with torch.no_grad():
                m.forward_chunk(_cuda(_chunk(clean, I, fpc)), zero, ctx_d, cache, commit=True)
    got = m.forward_chunk(x, tt, ctx_d, cache, commit=True, grad=True)     # commit=True under grad advances the cache
    assert cache.length == 3 * C and torch.equal(got[0].detach(), want[0])


@pytest.mark.parametrize("fpc,W,F", SF.SETTINGS)
def test_gradient_parity_with_the_restatement(model_mod, causal, fpc, W, F):
    ref = SF.reference(causal, fpc, W, F)
    got = _teacher_rollout(_model(model_mod), causal, fpc, W, F)
    worst = max(rel_rms(got["outs"][I][b], ref["out"][b][:, I * fpc:(I + 1) * fpc]) for I in range(F // fpc) for b in range(2))
    print(f"({fpc}, {W}, {F}): forward, worst chunk rel-RMS {worst:.2e}")
    assert worst < TOL_FWD
    print(f"({fpc}, {W}, {F}): loss {float(got['loss']):.6f} reference {ref['loss']:.6f}")
    assert abs(float(got["loss"]) - ref["loss"]) < TOL_LOSS * ref["loss"]
    for name in SF.COMPARED:
        err = rel_rms(got["grads"][name], ref["grads"][name])
        print(f"({fpc}, {W}, {F}) {name}: rel-RMS {err:.2e}")
        assert err < TOL_GRAD, name
    assert got["d_t"].shape == ref["d_t"].shape
    print(f"({fpc}, {W}, {F}) d t {rel_rms(got['d_t'], ref['d_t']):.2e} d noisy {rel_rms(got['d_noisy'][0], ref['d_noisy'][0]):.2e}")
    assert rel_rms(got["d_t"], ref["d_t"]) < TOL_GRAD
    for b in range(2):
        assert rel_rms(got["d_noisy"][b], ref["d_noisy"][b]) < TOL_GRAD


@pytest.mark.parametrize("fpc,W,F", SF.SETTINGS)
def test_overwrite_safety(model_mod, causal, deterministic, fpc, W, F):
    """One backward() at the end — every chunk's own cache rows overwritten by then, n graphs pending — gives the bits of
    backward() on each chunk's loss right behind its forward.  Parameter gradients are sums over the chunks and fp32
    addition is not associative: the per-chunk gradients are added here in the order the engine adds them (the last
    chunk's graph runs first).  Accumulated into .grad chunk by chunk (the direct accumulation route, first chunk first)
    they agree to fp32 rounding.  A second run of the one-pass form gives the same bits."""
    one = _teacher_rollout(_model(model_mod), causal, fpc, W, F)
    sep = _teacher_rollout(_model(model_mod), causal, fpc, W, F, mode="separate")
    assert torch.equal(one["d_t"], sep["d_t"])
    for b in range(2):
        assert torch.equal(one["d_noisy"][b], sep["d_noisy"][b])
    for name, g in one["grads"].items():
        parts = [pc[name] for pc in reversed(sep["per_chunk"]) if name in pc]
        total = parts[0].clone()
        for p in parts[1:]:
            total += p
        assert torch.equal(g, total), name
    each = _teacher_rollout(_model(model_mod), causal, fpc, W, F, mode="each")
    for name, g in one["grads"].items():
        assert rel_rms(each["grads"][name], g) < 1e-5, name
    again = _teacher_rollout(_model(model_mod), causal, fpc, W, F)
    assert torch.equal(again["loss"], one["loss"]) and torch.equal(again["d_t"], one["d_t"])
    for name, g in one["grads"].items():
        assert torch.equal(again["grads"][name], g), name


def test_stale_cache_raises(model_mod, causal):
    """reset() and commits of other data between forward and backward: RuntimeError, never other numbers.  A cache that
    only grew, or was truncated above the rows the chunk read, is fine."""
    fpc, W, F = SF.SETTINGS[0]
    cfg, clean, noisy, target, ctx, t = SF.inputs(F, fpc)
    m = _model(model_mod)
    m.set_causal_chunks(fpc, W)
    cache = causal.KVCache(m, 2, F * TPF, "cuda")
    ctx_d, zero = _cuda(ctx), torch.zeros(2, device="cuda")

    def commit(v, I):
        with torch.no_grad():
            m.forward_chunk(_cuda(_chunk(v, I, fpc)), zero, ctx_d, cache, commit=True)
    commit(clean, 0)
    loss = lambda: m.forward_chunk(_cuda(_chunk(noisy, 1, fpc)), t[:, 1].cuda().contiguous(), ctx_d, cache, commit=False,
                                   grad=True)[0].square().mean()
    ok = loss()
    commit(clean, 1), commit(clean, 2)
    cache.truncate(2 * TPF)                                                  # above the rows [0, 56) the chunk read
    ok.backward()
    want = m.blocks[0].self_attn.v.weight.grad.clone()
    m.zero_grad(set_to_none=True)
    cache.truncate(TPF)
    stale = loss()
    cache.reset()
    commit(target, 0), commit(target, 1)                                     # other data in the same rows
    with pytest.raises(RuntimeError, match="KVCache"):
        stale.backward()
    m.zero_grad(set_to_none=True)
    cache.reset()
    commit(clean, 0)
    fresh = loss()                                                           # the model is usable after the refusal
    fresh.backward()
    assert rel_rms(m.blocks[0].self_attn.v.weight.grad, want) < 1e-3
    with pytest.raises(RuntimeError):                                        # the kept activations are released: once only
        fresh.backward()


def test_window_isolation(model_mod, causal, deterministic):
    """left_chunks = 1: chunk 3 attends to clean chunk 2 and itself.  The keys and values of clean chunk 2 were computed
    by a commit pass that attended to clean chunk 1, so through the model's two layers chunk 3 depends on the clean chunks
    1 and 2 — the window reaches one chunk further per layer — and on nothing before them: another clean chunk 0 changes
    neither out_3 nor any gradient of its loss, bit for bit; another clean chunk 2 changes both."""
    fpc, W, F = SF.SETTINGS[1]
    clean = SF.inputs(F, fpc)[1]
    I = 3

    def run(chunk):
        other = [u.clone() for u in clean]
        if chunk is not None:
            for u in other:
                u[:, chunk * fpc:(chunk + 1) * fpc] += 1.0
        return _teacher_rollout(_model(model_mod), causal, fpc, W, F, clean=other, only=I)
    base, outside, inside = run(None), run(0), run(2)
    same = lambda a, b: all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"] if a["grads"][k] is not None)
    assert any(g is not None for g in base["grads"].values())
    assert torch.equal(outside["outs"][I][0], base["outs"][I][0]) and torch.equal(outside["loss"], base["loss"])
    assert same(outside, base) and torch.equal(outside["d_noisy"][0], base["d_noisy"][0])
    assert torch.equal(outside["d_t"], base["d_t"])
    assert not torch.equal(inside["outs"][I][0], base["outs"][I][0]) and not same(inside, base)


def test_frozen_model_input_gradient(model_mod, causal):
    fpc, W, F = SF.SETTINGS[1]
    ref = SF.reference(causal, fpc, W, F)
    m = _model(model_mod, train=False)
    got = _teacher_rollout(m, causal, fpc, W, F, t_grad=False)
    for b in range(2):
        err = rel_rms(got["d_noisy"][b], ref["d_noisy"][b])
        print(f"frozen model: d noisy clip {b} rel-RMS {err:.2e}")
        assert err < TOL_GRAD
    assert all(p.grad is None for p in m.parameters())
    assert abs(float(got["loss"]) - ref["loss"]) < TOL_LOSS * ref["loss"]


SIGMAS, TIMESTEPS = (1.0, 0.75, 0.4), (1000.0, 750.0, 400.0)


def _by_hand(m, causal, ops, noise, ctx, fpc, W, exits, gen):
    """self_forcing_rollout written out with forward_chunk and ops.flow_x0_step."""
    F, n_chunks = noise[0].shape[1], noise[0].shape[1] // fpc
    m.set_causal_chunks(fpc, W)
    cache = causal.KVCache(m, 2, F * TPF, "cuda")
    lvl = lambda v: torch.full((2,), v, dtype=torch.float32, device="cuda")
    done = []
    for I in range(n_chunks):
        x = torch.stack(_chunk(noise, I, fpc)).float().contiguous()
        for j in range(exits[I]):
            with torch.no_grad():
                v = torch.stack(m.forward_chunk(list(x.unbind(0)), lvl(TIMESTEPS[j]), ctx, cache, commit=False))
                eps = torch.randn(x.shape, dtype=torch.float32, device="cuda", generator=gen)
                x = ops.flow_x0_step(v, x, lvl(SIGMAS[j]), eps, lvl(SIGMAS[j + 1]))[1]
        j = exits[I]
        v = torch.stack(m.forward_chunk(list(x.unbind(0)), lvl(TIMESTEPS[j]), ctx, cache, commit=False, grad=True))
        x0 = ops.flow_x0_step(v, x, lvl(SIGMAS[j]))
        done.append(x0)
        if I + 1 < n_chunks:
            with torch.no_grad():
                m.forward_chunk(list(x0.detach().unbind(0)), lvl(0.0), ctx, cache, commit=True)
    return list(torch.cat(done, dim=2).unbind(0))


@pytest.mark.parametrize("exits", [[0, 2, 1, 2], 0, 2])
def test_rollout_is_the_sequence_written_out(model_mod, causal, deterministic, exits):
    ops = deterministic
    fpc, W, F = SF.SETTINGS[1]
    cfg, _, noise, target, ctx, _ = SF.inputs(F, fpc)
    noise, ctx_d, n_chunks = _cuda(noise), _cuda(ctx), F // fpc
    per_chunk = [exits] * n_chunks if isinstance(exits, int) else exits
    results = []
    for by_hand in (False, True):
        m = _model(model_mod)
        m.set_causal_chunks(1, -1)                                           # the caller's own setting: restored
        gen = torch.Generator(device="cuda").manual_seed(123)
        if by_hand:
            clips = _by_hand(m, causal, ops, noise, ctx_d, fpc, W, per_chunk, gen)
        else:
            cache = causal.KVCache(m, 2, F * TPF, "cuda")
            cache.advance(TPF)                                               # the caller's cache is reset
            clips = causal.self_forcing_rollout(m, noise, ctx_d, frames_per_chunk=fpc, left_chunks=W, sigmas=SIGMAS,
                                                timesteps=torch.tensor(TIMESTEPS), exit_step=exits, generator=gen,
                                                cache=cache)
            assert cache.length == (n_chunks - 1) * fpc * TPF
            assert m._causal_chunks == (1, -1)
        assert len(clips) == 2 and all(c.shape == (16, F, 14, 16) and c.dtype == torch.float32 and c.requires_grad
                                       for c in clips)
        sum(mse(c, v.cuda()) for c, v in zip(clips, target)).backward()
        results.append((clips, {k: p.grad for k, p in m.named_parameters()}))
    (a, ga), (b, gb) = results
    for u, v in zip(a, b):
        assert torch.equal(u.detach(), v.detach())
    assert any(g is not None and float(g.abs().sum()) > 0 for g in ga.values())
    for name in ga:
        assert (ga[name] is None) == (gb[name] is None), name
        if ga[name] is not None:
            assert torch.equal(ga[name], gb[name]), name


def test_rollout_restores_the_setting_after_an_exception(model_mod, causal):
    fpc, W, F = SF.SETTINGS[1]
    cfg, _, noise, _, ctx, _ = SF.inputs(F, fpc)
    m = _model(model_mod)
    m.set_causal_chunks(1, 0)
    wrong = causal.KVCache(m, 1, F * TPF, "cuda")                            # a cache of another batch size
    with pytest.raises(ValueError):
        causal.self_forcing_rollout(m, _cuda(noise), _cuda(ctx), frames_per_chunk=fpc, left_chunks=W, sigmas=SIGMAS,
                                    timesteps=TIMESTEPS, exit_step=1, cache=wrong)
    assert m._causal_chunks == (1, 0)


def test_lora_adapter_gradients(model_mod, causal):
    """Adapters on a frozen base through forward_chunk(grad=True): the shared block backward forms their gradients; they
    equal dB = s dW A^T, dA = s B^T dW with dW from the restatement on the effective weights W + s B A."""
    omh = importlib.import_module(PKG)
    lora = importlib.import_module(PKG + ".lora")
    fpc, W, F = SF.SETTINGS[1]
    cfg = MC.case()[0]
    m = _model(model_mod, train=False)
    adapters = omh.add_lora(m, rank=4)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for _, lin in lora.lora_modules(m):
            lin.lora_A.copy_((torch.randn(lin.lora_A.shape, generator=gen) * 0.05).cuda())
            lin.lora_B.copy_((torch.randn(lin.lora_B.shape, generator=gen) * 0.05).cuda())
    sd = O.synth_state_dict(cfg, MC.TAG)
    factors = {}
    for name, lin in lora.lora_modules(m):
        A, B, s = model_mod.lora_of(lin)
        factors[name] = (A.detach().cpu().float(), B.detach().cpu().float(), float(s))
        sd[name + ".weight"] = sd[name + ".weight"] + float(s) * (factors[name][1] @ factors[name][0])
    ref = SF.reference(causal, fpc, W, F, sd=sd)
    got = _teacher_rollout(m, causal, fpc, W, F, x_grad=False, t_grad=False)
    assert abs(float(got["loss"]) - ref["loss"]) < TOL_LOSS * ref["loss"]
    assert all(p.grad is None for n, p in m.named_parameters() if "lora_" not in n)          # the base is frozen
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0 for p in adapters)
    worst = 0.0
    for name, lin in lora.lora_modules(m):
        A, B, s = factors[name]
        dW = ref["grads"][name + ".weight"]
        for nm, g, want in (("lora_A", lin.lora_A.grad, s * B.t() @ dW), ("lora_B", lin.lora_B.grad, s * dW @ A.t())):
            err = rel_rms(g, want)
            worst = max(worst, err)
            assert err < TOL_GRAD, (name, nm, err)
    print(f"LoRA through forward_chunk(grad=True): worst adapter gradient rel-RMS {worst:.2e}")
