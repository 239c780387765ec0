"""CPU: the self-forcing restatement (tests/self_forcing_ref.py) against tests/teacher_forcing_ref.py, that it tells a
detached clean half from an attached one, the argument rules of ``WanModel.forward_chunk(grad=True)`` and
``causal.self_forcing_rollout``, ``KVCache``'s cut tracking, and the ``own_lo`` rules of
omh_flash_attn_bwd_cached_d128 — nothing here launches a kernel."""
import ctypes as C
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
import self_forcing_ref as SF
import teacher_forcing_ref as R
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

TOL_GRAD = 2e-2                                      # the project's gradient bound (test_gpu_teacher_forcing_model.py)


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


def test_attached_restatement_is_teacher_forcing_bit_for_bit(causal):
    fpc, W, F = SF.SETTINGS[1]
    cfg, clean, noisy, _, ctx, t = SF.inputs(F, fpc)
    sd = O.synth_state_dict(cfg, MC.TAG)
    x = [torch.cat([c, n], 1) for c, n in zip(clean, noisy)]
    t_all = torch.cat([torch.zeros(2, F), t.repeat_interleave(fpc, dim=1)], dim=1)
    mask = SF.tf_mask(causal, F, fpc, W)
    with torch.no_grad():
        a = SF.forward(sd, cfg, x, t_all, ctx, 2 * F * SF.TPF, mask, F, detach=False)
        b = R.forward(sd, cfg, x, t_all, ctx, 2 * F * SF.TPF, mask=mask, segments=2, out_from=F)
        c = SF.forward(sd, cfg, x, t_all, ctx, 2 * F * SF.TPF, mask, F, detach=True)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v)
        assert torch.equal(w, v)                     # detaching changes no forward value


@pytest.mark.parametrize("fpc,W,F", SF.SETTINGS)
def test_the_restatement_discriminates(causal, fpc, W, F):
    """Detached and attached clean halves must differ by more than 3 x the gradient bound in at least three of the
    compared parameter gradients — the value and key weights carry direct clean-row terms — or a GPU comparison within
    the bound could not tell self forcing from teacher forcing."""
    det = SF.reference(causal, fpc, W, F, detach=True)
    att = SF.reference(causal, fpc, W, F, detach=False)
    assert abs(det["loss"] - att["loss"]) == 0.0
    far = []
    for name in SF.COMPARED:
        err = rel_rms(det["grads"][name], att["grads"][name])
        print(f"({fpc}, {W}, {F}) {name}: detached against attached rel-RMS {err:.3e}")
        if err > 3 * TOL_GRAD:
            far.append(name)
    assert len(far) >= 3, far
    assert "blocks.0.self_attn.v.weight" in far and "blocks.1.self_attn.k.weight" in far
    for g in det["d_clean"]:                         # the clean latents reach the loss through constants only
        assert g is None or float(g.abs().max()) == 0.0
    assert all(float(g.abs().max()) > 0.0 for g in att["d_clean"])


def _cpu_model(wan_model_mod):
    return wan_model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)


def test_grad_true_refusals_come_before_the_device(omh, wan_model_mod, causal):
    m = _cpu_model(wan_model_mod)
    x = [torch.zeros(16, 1, 14, 16) for _ in range(2)]
    ctx = [torch.zeros(8, 64) for _ in range(2)]
    t = torch.zeros(2)
    m.set_causal_chunks(1, 1)
    rolling = causal.RollingKVCache(m, 2, SF.TPF, 0, 1, "cpu")
    with pytest.raises(ValueError, match="KVCache"):                      # its slots are evicted before the backward runs
        m.forward_chunk(x, t, ctx, rolling, grad=True)
    m.set_causal_chunks(1, 1, 1)
    with pytest.raises(ValueError, match="sink_chunks"):
        m.forward_chunk(x, t, ctx, causal.KVCache(m, 2, 4 * SF.TPF, "cpu"), grad=True)
    m.set_causal_chunks(1, 1)
    cache = causal.KVCache(m, 2, 4 * SF.TPF, "cpu")
    with pytest.raises(ValueError, match=r"\[B\]"):                       # a 2-D t
        m.forward_chunk(x, torch.zeros(2, 1), ctx, cache, grad=True)
    m.checkpoint_policy = "always"
    with pytest.raises(ValueError, match="checkpoint_policy"):
        m.forward_chunk(x, t, ctx, cache, grad=True)
    m.checkpoint_policy = "auto"
    ops = importlib.import_module(PKG + ".ops")
    with pytest.raises(ops.OmhError):                                     # and then: no CPU fallback, as ever
        m.forward_chunk(x, t, ctx, cache, grad=True)


def test_rollout_argument_errors(omh, wan_model_mod, causal):
    m = _cpu_model(wan_model_mod)
    m.set_causal_chunks(3, 0)
    noise = [torch.zeros(16, 4, 14, 16) for _ in range(2)]
    ctx = [torch.zeros(8, 64) for _ in range(2)]
    kw = dict(sigmas=[1.0, 0.5], timesteps=[1000.0, 500.0])
    with pytest.raises(ValueError, match="multiple"):                     # F % fpc
        causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=3, exit_step=0, **kw)
    for bad in (2, -1, [0, 1, 0], [0, 2]):                                # outside [0, n), or not one per chunk
        with pytest.raises(ValueError, match="exit_step"):
            causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=2, exit_step=bad, **kw)
    with pytest.raises(ValueError, match="timesteps"):
        causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=2, exit_step=0, sigmas=[1.0, 0.5], timesteps=[1000.0])
    with pytest.raises(ValueError, match="one shape"):
        causal.self_forcing_rollout(m, [noise[0], noise[1][:, :2]], ctx, frames_per_chunk=2, exit_step=0, **kw)
    rolling = causal.RollingKVCache(m, 2, 2 * SF.TPF, 0, 1, "cpu")
    with pytest.raises(ValueError, match="RollingKVCache"):
        causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=2, left_chunks=1, exit_step=0, cache=rolling, **kw)
    assert m._causal_chunks == (3, 0)                                     # untouched by the refused calls
    ops = importlib.import_module(PKG + ".ops")
    with pytest.raises(ops.OmhError):                                     # valid arguments reach the device check ...
        causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=2, exit_step=[1, 0], **kw)
    assert m._causal_chunks == (3, 0)                                     # ... and the setting is restored after an exception


def test_kv_cache_cut_tracking(omh, wan_model_mod, causal):
    m = _cpu_model(wan_model_mod)
    c = causal.KVCache(m, 1, 1024, "cpu")
    c.advance(256)
    a = c.mark()
    c.advance(256)
    b = c.mark()
    assert c.intact(a, 256) and c.intact(b, 512)
    c.truncate(512)                                                      # not a cut: nothing forgotten
    c.truncate(384)
    assert c.intact(a, 256) and c.intact(b, 384) and not c.intact(b, 512)
    later = c.mark()
    c.advance(128)
    assert c.intact(later, 512)                                          # rows committed after the cut, marked after it
    c.reset()
    c.advance(512)
    assert not c.intact(a, 256) and not c.intact(later, 8) and c.intact(c.mark(), 512)
    assert c.intact(a, 0)
    for _ in range(50):                                                   # the log stays short
        c.truncate(c.length - 8)
        c.advance(8)
    assert len(c._cuts) <= 2


def test_cached_backward_argument_rules_without_a_gpu(omh):
    """omh_flash_attn_bwd_cached_d128 refuses before it touches the device; the workspace query is host arithmetic."""
    binding = importlib.import_module(PKG + "._lib")
    lib = binding.lib
    assert lib.omh_flash_attn_bwd_cached_d128(None, 0, None) == -1

    def args(Lq=168, Lk=336, o32=True, k_lens=False, phase=0, B=1, H=2):
        a = binding.AttnBwdArgs()
        for f in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv"):
            setattr(a, f, 4096)
        a.o32 = 4096 if o32 else None
        a.k_lens = 4096 if k_lens else None
        a.B, a.H, a.Lq, a.Lk, a.phase = B, H, Lq, Lk, phase
        d = H * 128
        a.q_rs = a.k_rs = a.o_rs = a.dq_rs = a.dk_rs = d
        a.q_bs = a.o_bs = a.dq_bs = Lq * d
        a.k_bs, a.dk_bs = Lk * d, Lk * d
        return a
    call = lambda a, lo: lib.omh_flash_attn_bwd_cached_d128(C.byref(a), lo, None)
    assert call(args(), 4) == -2 and call(args(), 164) == -2               # own_lo % 8
    assert call(args(), -8) == -1 and call(args(), 336) == -1 and call(args(), 344) == -1     # outside [0, Lk)
    assert call(args(o32=False), 168) == -1                                # o32 required
    assert call(args(k_lens=True), 168) == -1                              # no per-sample key lengths beside own_lo > 0
    assert call(args(phase=4), 168) == -1
    a = args()
    a.dq = None
    assert call(a, 168) == -1
    a = args()
    a.k_rs = 260
    assert call(a, 168) == -2
    # the workspace: own_lo = 0 is the plain query; otherwise dQ is planned over Lq x Lk and dK / dV over the own keys
    ws = lambda a, lo: lib.omh_flash_attn_bwd_cached_workspace_bytes(C.byref(a), lo)
    tile = 128 * 128 * 4
    big = args(Lq=1560, Lk=4680, B=1, H=12)
    assert ws(big, 0) == lib.omh_flash_attn_bwd_workspace_bytes(C.byref(big))
    own = args(Lq=1560, Lk=1560, B=1, H=12)
    for phase in (0, 1, 2, 3):
        big.phase = own.phase = phase
        q_part = lib.omh_flash_attn_bwd_workspace_bytes(C.byref(big)) if phase == 2 else None
        kv_part = lib.omh_flash_attn_bwd_workspace_bytes(C.byref(own)) if phase == 3 else None
        if phase == 2:
            assert ws(big, 3120) == q_part
        if phase == 3:
            assert ws(big, 3120) == kv_part == 156 * 3 * 2 * tile          # 13 key blocks x 12 heads, as at Lk = 1560
        if phase == 1:
            assert ws(big, 3120) == 0
    big.phase, own.phase = 2, 3
    total = lib.omh_flash_attn_bwd_workspace_bytes(C.byref(big)) + lib.omh_flash_attn_bwd_workspace_bytes(C.byref(own))
    big.phase = 0
    assert ws(big, 3120) == total
    assert ws(big, 4680) == 0 and ws(big, -8) == 0


def test_flash_attn_bwd_own_lo_python_rules(omh):
    ops = importlib.import_module(PKG + ".ops")
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(ops.OmhError):                                     # CPU tensors: no fallback (checked first)
        ops.flash_attn_bwd(t, t, t, None, t, torch.zeros(1, 1, 8), None, 1, 1, 8, 8, own_lo=0)
