"""``causal.dmd_loss`` and ``causal.critic_loss`` on the tiny 2-layer t2v model of tests/make_golden_chunk_causal.py: the
student as in test_gpu_self_forcing_model.py, the teacher (frozen, eval) and the critic (train) two more instances with
other synthetic state-dict tags; B = 2 clips [16, 6, 14, 16] (336 tokens), guide 3.

Bounds: the kernel's own (test_gpu_dmd_kernel.py) for ``x.grad`` against the rule in fp64 on the velocities the function
saw — 2e-6 relative RMS per sample, 4e-6 of max|ref| in maximum absolute error — and 1e-5 relative for the loss (the mean
of squares of values that carry 2e-6 each).  Everything else is an equality of bits."""
import gc
import importlib

import pytest
import torch

import make_golden_chunk_causal as MC
from conftest import PKG
from dmd_ref import TOL_MAX, TOL_RMS, rule as _rule
from oracle import wan_dit_oracle as O

pytestmark = pytest.mark.gpu
B, SHAPE, SEQ, GUIDE = 2, (16, 6, 14, 16), 6 * MC.TOKENS_PER_FRAME, 3.0
N = B * 16 * 6 * 14 * 16


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


def _model(model_mod, tag, train=True):
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    m.load_state_dict(O.synth_state_dict(MC.case()[0], tag))
    m = m.cuda()
    return m.train() if train else m.eval().requires_grad_(False)


def _student(model_mod):
    return _model(model_mod, MC.TAG)


def _teacher(model_mod):
    return _model(model_mod, "dmd/teacher", train=False)


def _critic(model_mod):
    return _model(model_mod, "dmd/critic")


def _inputs():
    g = torch.Generator().manual_seed(77)
    clips = [torch.randn(*SHAPE, generator=g).cuda() for _ in range(B)]
    eps = torch.randn(B, *SHAPE, generator=g).cuda()
    ctx = [c.cuda() for c in MC.case()[2]]
    ctx_null = [torch.randn(5, 64, generator=g).cuda() for _ in range(B)]
    sigma = torch.tensor([0.3, 0.8], device="cuda")
    return clips, eps, ctx, ctx_null, sigma, 1000.0 * sigma


def _bits(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _velocities(teacher, critic, x_t, t, ctx, ctx_null):
    """The score models called the way dmd_loss calls them."""
    xs = list(x_t.unbind(0))
    with torch.no_grad():
        if ctx_null is None:
            v_c, v_u = torch.stack(teacher.forward(xs, t, ctx, SEQ)), None
        else:
            v_c, v_u = (torch.stack(v) for v in teacher.forward_cfg_pair(xs, t, ctx, ctx_null, SEQ))
        v_f = torch.stack(critic.forward(xs, t, ctx, SEQ))
    return v_c, v_u, v_f


@pytest.mark.parametrize("cfg", [True, False])
def test_dmd_loss_on_leaf_clips(model_mod, causal, ops, monkeypatch, cfg):
    clips, eps, ctx, ctx_null, sigma, t = _inputs()
    if not cfg:
        ctx_null = None
    teacher, critic = _teacher(model_mod), _critic(model_mod)
    teacher.set_causal_chunks(2, 1)                                  # the caller's setting: not touched
    before = _bits(teacher), _bits(critic)
    seen = {}
    inner = ops.dmd_loss

    def spy(*a):
        seen["args"] = a
        return inner(*a)
    monkeypatch.setattr(ops, "dmd_loss", spy)
    x = [c.clone().requires_grad_(True) for c in clips]
    loss = causal.dmd_loss(x, teacher, critic, ctx, ctx_null, sigma=sigma, timesteps=t, guide_scale=GUIDE, eps=eps)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad
    loss.backward()
    # the same calls outside: the forwards repeat bit for bit
    xd = torch.stack(clips)
    x_t = ops.flow_noise(xd, eps, sigma)
    v_c, v_u, v_f = _velocities(teacher, critic, x_t, t, ctx, ctx_null)
    got = seen["args"]
    assert torch.equal(got[0].detach(), xd) and torch.equal(got[1], x_t) and torch.equal(got[2], v_c)
    assert (got[3] is None and v_u is None) or torch.equal(got[3], v_u)
    assert torch.equal(got[4], v_f) and torch.equal(got[5], sigma) and got[6] == GUIDE
    if cfg:
        assert not torch.equal(v_c, v_u)
    flat = lambda v: None if v is None else v.reshape(B, -1).cpu()
    ref_grad, _ = _rule(flat(xd), flat(x_t), flat(v_c), flat(v_u), flat(v_f), sigma.cpu(), GUIDE)
    want = ref_grad / N
    have = torch.stack([u.grad for u in x]).reshape(B, -1).double().cpu()
    e_rms = float(((have - want).norm(dim=1) / want.norm(dim=1)).max())
    e_max = float((have - want).abs().max() / want.abs().max())
    ref_loss = 0.5 * float(ref_grad.square().mean())
    print(f"dmd_loss (cfg {cfg}): x.grad rel-RMS {e_rms:.2e} max {e_max:.2e}; loss {float(loss.detach()):.9e} fp64 rule {ref_loss:.9e}")
    assert e_rms < TOL_RMS and e_max < TOL_MAX
    assert abs(float(loss.detach()) - ref_loss) < 1e-5 * ref_loss
    for m, was in zip((teacher, critic), before):
        assert all(p.grad is None for p in m.parameters())
        assert all(torch.equal(v, was[k]) for k, v in m.state_dict().items())
    assert teacher._causal_chunks[:2] == (2, 1) and not teacher.training and critic.training


def test_end_to_end_equals_the_surrogate(model_mod, causal, deterministic):
    """Rollout -> dmd_loss -> backward against the same rollout with loss = (stack(clips) * (grad_raw * inv_N)).sum():
    every parameter gradient of the student has the same bits, and a second run repeats them."""
    ops = deterministic
    _, eps, ctx, ctx_null, sigma, t = _inputs()
    g = torch.Generator().manual_seed(3)
    noise = [torch.randn(*SHAPE, generator=g).cuda() for _ in range(B)]
    teacher, critic = _teacher(model_mod), _critic(model_mod)

    def run(surrogate):
        m = _student(model_mod)
        m.set_causal_chunks(2, 1)                                    # the student's own setting survives both calls
        gen = torch.Generator(device="cuda").manual_seed(123)
        clips = causal.self_forcing_rollout(m, noise, ctx, frames_per_chunk=1, left_chunks=-1, sigmas=(1.0, 0.5),
                                            timesteps=(1000.0, 500.0), exit_step=[0, 1, 1, 0, 1, 0], generator=gen)
        assert clips[0].requires_grad and clips[0].shape == SHAPE
        if surrogate:
            x = torch.stack(clips)
            xd = x.detach()
            x_t = ops.flow_noise(xd, eps, sigma)
            v_c, v_u, v_f = _velocities(teacher, critic, x_t, t, ctx, ctx_null)
            grad_raw = ops.dmd_grad(xd, x_t, v_c, v_u, v_f, sigma, GUIDE)[0]
            inv = torch.tensor(1.0 / N, dtype=torch.float32, device="cuda")
            loss = (x * (grad_raw * inv)).sum()
        else:
            loss = causal.dmd_loss(clips, teacher, critic, ctx, ctx_null, sigma=sigma, timesteps=t, guide_scale=GUIDE,
                                   eps=eps)
        loss.backward()
        assert m._causal_chunks[:2] == (2, 1) and critic.training
        return loss.detach(), {k: p.grad for k, p in m.named_parameters()}
    (la, a), (_, b), (lc, c) = run(False), run(True), run(False)
    assert any(v is not None and float(v.abs().sum()) > 0 for v in a.values())
    for name in a:
        assert (a[name] is None) == (b[name] is None) == (c[name] is None), name
        if a[name] is not None:
            assert torch.equal(a[name], b[name]), name
            assert torch.equal(a[name], c[name]), name
    assert torch.equal(la, lc)
    assert all(p.grad is None for p in teacher.parameters()) and all(p.grad is None for p in critic.parameters())


def test_critic_loss(model_mod, causal, ops):
    clips, eps, ctx, _, sigma, t = _inputs()
    critic, other = _critic(model_mod), _teacher(model_mod)
    leaves = [c.clone().requires_grad_(True) for c in clips]
    attached = [u * 1.0 for u in leaves]                            # clips with a graph of their own
    loss = causal.critic_loss(critic, attached, ctx, sigma=sigma, timesteps=t, eps=eps)
    loss.backward()
    assert attached[0].grad_fn is not None and all(u.grad is None for u in leaves)      # the clips' graph: untouched
    grads = [p.grad for p in critic.parameters()]
    assert all(g is not None for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0 and all(p.grad is None for p in other.parameters())
    # the torch expression on critic.forward's outputs for the same x_t (a second critic: this one's graph is spent)
    twin = _critic(model_mod)
    x = torch.stack(clips)
    x_t = ops.flow_noise(x, eps, sigma)
    out = twin.forward(list(x_t.unbind(0)), t, ctx, SEQ)
    assert out[0].requires_grad                                      # the training path
    want = torch.stack([(o.float() - v).square().mean() for o, v in zip(out, eps - x)]).mean().detach()
    del out
    gc.collect()
    assert torch.equal(loss.detach(), want)
    gen = lambda: torch.Generator(device="cuda").manual_seed(9)     # eps drawn inside: torch.randn with the generator
    with torch.no_grad():
        a = causal.critic_loss(twin, clips, ctx, sigma=sigma, timesteps=t, generator=gen())
        b = causal.critic_loss(twin, clips, ctx, sigma=sigma, timesteps=t,
                               eps=torch.randn(B, *SHAPE, dtype=torch.float32, device="cuda", generator=gen()))
    assert torch.equal(a, b) and not torch.equal(a, loss.detach())


def test_the_student_is_refused_as_a_score_model(model_mod, causal):
    _, eps, ctx, ctx_null, sigma, t = _inputs()
    g = torch.Generator().manual_seed(3)
    noise = [torch.randn(16, 2, 14, 16, generator=g).cuda() for _ in range(B)]
    student, critic = _student(model_mod), _critic(model_mod)
    clips = causal.self_forcing_rollout(student, noise, ctx, frames_per_chunk=1, sigmas=(1.0,), timesteps=(1000.0,),
                                        exit_step=0)
    kw = dict(sigma=sigma, timesteps=t)
    with pytest.raises(RuntimeError, match="teacher"):
        causal.dmd_loss(clips, student, critic, ctx, ctx_null, **kw)
    with pytest.raises(RuntimeError, match="critic"):
        causal.dmd_loss(clips, _teacher(model_mod), student, ctx, **kw)
    loss = causal.dmd_loss(clips, _teacher(model_mod), critic, ctx, ctx_null, **kw)        # separate models: fine
    loss.backward()
    assert any(p.grad is not None for p in student.parameters())
