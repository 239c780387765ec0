"""Global gradient-norm clipping on the device (Omnihuman/omnihuman_trainer.py:349-356: clip_grad_norm_(
model.parameters(), max_grad_norm), then optimizer.step()): the multi-tensor norm kernel, the drop-in
``optim.clip_grad_norm_`` and ``optim.AdamW(max_grad_norm=)``, which applies the coefficient inside the AdamW kernels.

Shapes: the tensor bag of test_adamw_and_ema_match_torch, extended — 1, 3, 255, 4095, 4096, 4097, 8192 + 3 and 70001
elements, OMH_NORM_CHUNK - 1 and + 1 (one chunk / two chunks), one 1536 x 1536 matrix (144 chunks) and a view that starts
4 bytes off the 16-byte grid (the scalar route)."""
import importlib

import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

# omh.h: an element passes through at most 27 (<= 64, the contract) chained fp32 additions of non-negative terms before
# the fp64 stage; with the square, the fp64 tail, the square root and one rounding the contract's bound is
# (64 + 3) * 2^-24 / 2 + 2^-24 ~ 2.1e-6 relative.  The allowance is twice that.
TOL_NORM = 4e-6
# ... plus the two roundings of the coefficient and of the product
TOL_CLIP = 5e-6


def _optim():
    return importlib.import_module(PKG + ".optim")


def _sizes(ops):
    return [1, 3, 255, 4095, 4096, 4097, 8192 + 3, 70001, ops.NORM_CHUNK - 1, ops.NORM_CHUNK + 1]


@pytest.fixture(scope="module")
def bag(ops):
    """Gradients of the bag (never written: every test clones) and their norm in fp64."""
    gen = torch.Generator().manual_seed(1234)
    grads = [torch.randn(n, generator=gen).cuda() for n in _sizes(ops)]
    grads.append(torch.randn(1536, 1536, generator=gen).cuda())
    grads.append(torch.randn(4099, generator=gen).cuda())            # handed out 4 bytes off the grid by _grad_copies
    norm64 = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item()
    return grads, norm64


def _grad_copies(grads):
    """Clones; the last one lives at base[1:1 + 4099]: 4 bytes off the 16-byte grid."""
    out = [g.clone() for g in grads[:-1]]
    base = torch.zeros(20000, device="cuda")
    off = base[1:1 + grads[-1].numel()]
    off.copy_(grads[-1])
    assert off.data_ptr() % 16 == 4
    return out + [off]


def _params(grads, seed=7, with_grads=True):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(g.shape, generator=gen).cuda()) for g in grads]
    if with_grads:
        for p, g in zip(ps, _grad_copies(grads)):
            p.grad = g
    return ps


def _norm_table(ops, grads):
    rows, chunk0 = [], 0
    for g in grads:
        rows.append([g.data_ptr(), g.numel(), chunk0])
        chunk0 += (g.numel() + ops.NORM_CHUNK - 1) // ops.NORM_CHUNK
    return torch.tensor(rows, dtype=torch.int64).cuda(), chunk0


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_norm_kernel(ops, bag):
    grads, norm64 = bag
    gs = _grad_copies(grads)
    table, chunks = _norm_table(ops, gs)
    assert chunks == 7 + 5 + 1 + 2 + 144 + 1                          # 70001 takes five chunks, CHUNK + 1 two
    ws = torch.full((chunks,), float("nan"), device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((2,), float("nan"), device="cuda")
        ops.grad_norm_multi(table, len(gs), chunks, ws, out, 0.5 * norm64)
        outs.append(out)
    got, coef = outs[0].tolist()
    print(f"[measured] norm {got!r} against {norm64!r}: relative error {_rel(got, norm64):.3e}")
    assert _rel(got, norm64) <= TOL_NORM
    assert torch.equal(outs[0], outs[1])                              # repeats bit for bit
    assert _rel(coef, 0.5 * norm64 / (norm64 + 1e-6)) <= TOL_CLIP
    for g, g0 in zip(gs, grads):                                      # the norm reads only
        assert torch.equal(g.reshape(-1), g0.reshape(-1))
    # nothing to clip: the coefficient is exactly 1
    ops.grad_norm_multi(table, len(gs), chunks, ws, out, 2.0 * norm64)
    assert out.tolist() == [got, 1.0]
    # the loss scale: the norm is that of g / 8
    ops.grad_norm_multi(table, len(gs), chunks, ws, out, 1.0, grad_scale=8.0)
    got8 = out[0].item()
    print(f"[measured] grad_scale 8: relative error {_rel(got8, norm64 / 8):.3e}")
    assert _rel(got8, norm64 / 8) <= TOL_NORM
    assert _rel(out[1].item(), 1.0 / (norm64 / 8 + 1e-6)) <= TOL_CLIP
    # one tensor alone, on each route, at every size: the partial of every chunk shape
    for g in gs:
        t1, c1 = _norm_table(ops, [g])
        ops.grad_norm_multi(t1, 1, c1, ws, out, 1.0)
        assert _rel(out[0].item(), g.double().norm().item()) <= TOL_NORM, g.shape


def test_clip_grad_norm_drop_in(ops, bag):
    optim = _optim()
    grads, norm64 = bag
    ps = _params(grads)
    ret = optim.clip_grad_norm_(ps, 0.5 * norm64)
    assert ret.dim() == 0 and ret.dtype == torch.float32 and ret.is_cuda
    assert _rel(ret.item(), norm64) <= TOL_NORM
    coef64 = 0.5 * norm64 / (norm64 + 1e-6)
    worst = 0.0
    for p, g0 in zip(ps, grads):
        want = g0.double() * coef64
        err = ((p.grad.double().reshape(-1) - want.reshape(-1)).abs() / want.reshape(-1).abs().clamp_min(1e-300)).max().item()
        worst = max(worst, err)
    print(f"[measured] clipped gradients: worst relative error per element {worst:.3e}")
    assert worst <= TOL_CLIP
    # nothing to clip: not a bit changes, and the norm comes back
    ps = _params(grads)
    keep = [p.grad.clone() for p in ps]
    ret2 = optim.clip_grad_norm_(ps, 2.0 * norm64)
    assert all(torch.equal(p.grad, k) for p, k in zip(ps, keep))
    assert ret2.item() == ret.item()
    # unchanged addresses: the cached table, the same bits (and a result of its own, not a view of the last one)
    n_tables = len(optim._CLIP_TABLES)
    ret3 = optim.clip_grad_norm_(ps, 2.0 * norm64)
    assert len(optim._CLIP_TABLES) == n_tables and ret3.data_ptr() != ret2.data_ptr()
    assert torch.equal(ret3, ret2) and all(torch.equal(p.grad, k) for p, k in zip(ps, keep))
    # a single tensor, parameters without a gradient, a generator
    ps[3].grad = None
    one = optim.clip_grad_norm_(ps[2], 1e9)
    assert _rel(one.item(), grads[2].double().norm().item()) <= TOL_NORM
    rest = optim.clip_grad_norm_((p for p in ps), 1e9)
    want = torch.sqrt(sum((g.double() ** 2).sum() for i, g in enumerate(grads) if i != 3)).item()
    assert _rel(rest.item(), want) <= TOL_NORM
    # what it refuses names the tensor
    keep1 = ps[1]
    ps[1] = torch.nn.Parameter(torch.zeros(3, device="cuda", dtype=torch.bfloat16))   # torch keeps a gradient in its parameter's dtype
    ps[1].grad = torch.zeros(3, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"parameter 1 .*bfloat16"):
        optim.clip_grad_norm_(ps, 1.0)
    ps[1] = keep1
    ps[1].grad = None
    ps[4].grad = torch.zeros(2 * 4096, device="cuda")[::2]
    with pytest.raises(ValueError, match=r"parameter 4 .*contiguous"):
        optim.clip_grad_norm_(ps, 1.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradients_as_torch(ops, bag, bad):
    optim = _optim()
    grads, _ = bag
    ours, theirs = _params(grads), _params(grads)
    for ps in (ours, theirs):
        ps[7].grad[12345] = bad
    before = [p.grad.clone() for p in ours]
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(ours, 1.0, error_if_nonfinite=True)
    for p, b in zip(ours, before):                                    # raised before anything was scaled
        torch.testing.assert_close(p.grad, b, rtol=0, atol=0, equal_nan=True)
    got = optim.clip_grad_norm_(ours, 1.0)
    want = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)
    assert got.item() == bad or (bad != bad and got.item() != got.item())
    for a, b in zip(ours, theirs):
        torch.testing.assert_close(a.grad, b.grad, rtol=0, atol=0, equal_nan=True)


def test_fused_step_equals_clip_then_step_on_the_bag(ops, bag):
    optim = _optim()
    grads, norm64 = bag
    c = 0.25 * norm64
    fused, two = _params(grads, with_grads=False), _params(grads, with_grads=False)
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    of, ot = optim.AdamW(fused, max_grad_norm=c, **kw), optim.AdamW(two, **kw)
    gen = torch.Generator().manual_seed(99)
    for it in range(3):
        step_grads = [g * (1.0 + it) + 0.1 * torch.randn(g.shape, generator=gen).cuda() for g in grads]
        for ps in (fused, two):
            for p, g in zip(ps, _grad_copies(step_grads)):
                p.grad = g
        given = [p.grad.clone() for p in fused]
        of.step()
        ret = optim.clip_grad_norm_(two, c)
        ot.step()
        assert ret.item() > c                                         # this step was clipped
        assert torch.equal(of.grad_norm, ret) and of.grad_norm.dim() == 0 and of.grad_norm.is_cuda
        for pf, pt, g in zip(fused, two, given):
            assert torch.equal(pf.grad, g)                            # the fused step leaves p.grad as it was given
            assert not torch.equal(pt.grad, g)
            assert torch.equal(pf.detach(), pt.detach())
            assert torch.equal(of.state[pf]["exp_avg"], ot.state[pt]["exp_avg"])
            assert torch.equal(of.state[pf]["exp_avg_sq"], ot.state[pt]["exp_avg_sq"])
    assert not any(len(k) == 4 for k in of._tables)                   # the adamw_multi kernel, not the pack kernel
    # the loss scale reaches the norm: that of g / 8
    given = [p.grad.clone() for p in fused]
    of.step(grad_scale=8.0)
    want = torch.sqrt(sum((g.double() ** 2).sum() for g in given)).item() / 8
    assert _rel(of.grad_norm.item(), want) <= TOL_NORM
    # a coefficient of 1.0f on the device: the bits of the entry without one
    a, b = _params(grads), _params(grads)
    tabs = []
    for ps in (a, b):
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        rows = [[p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, m, v in zip(ps, ms, vs)]
        tabs.append((torch.tensor(rows, dtype=torch.int64).cuda(), ms, vs))
    one = torch.tensor([1.0], device="cuda")
    for step in (1, 2):
        ops.adamw_multi(tabs[0][0], len(a), 1e-2, 0.9, 0.999, 1e-8, 0.01, step, 4.0)
        ops.adamw_multi_dev(tabs[1][0], len(b), 1e-2, 0.9, 0.999, 1e-8, 0.01, step, one, 4.0)
    for i in range(len(a)):
        assert torch.equal(a[i].detach(), b[i].detach())
        assert torch.equal(tabs[0][1][i], tabs[1][1][i]) and torch.equal(tabs[0][2][i], tabs[1][2][i])


def test_fused_step_against_torch_end_to_end(ops, bag):
    optim = _optim()
    grads, norm64 = bag
    c = 0.25 * norm64
    ours, theirs = _params(grads, with_grads=False), _params(grads, with_grads=False)
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    oo, ot = optim.AdamW(ours, max_grad_norm=c, **kw), torch.optim.AdamW(theirs, **kw)
    so = torch.optim.lr_scheduler.CosineAnnealingLR(oo, T_max=5)
    st = torch.optim.lr_scheduler.CosineAnnealingLR(ot, T_max=5)
    gen = torch.Generator().manual_seed(5)
    for it in range(5):
        step_grads = [torch.randn(g.shape, generator=gen).cuda() * (0.1 if it == 3 else 1.0) for g in grads]
        for ps in (ours, theirs):
            for p, g in zip(ps, _grad_copies(step_grads)):
                p.grad = g
        oo.step()
        so.step()
        norm = torch.nn.utils.clip_grad_norm_(theirs, c)
        ot.step()
        st.step()
        assert _rel(oo.grad_norm.item(), norm.item()) <= 2 * TOL_NORM   # torch's own fp32 norm is within the bound too
        assert (norm.item() > c) == (it != 3)                          # four clipped steps and one that is not
    assert oo.param_groups[0]["lr"] == ot.param_groups[0]["lr"]
    for a, b in zip(ours, theirs):
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-5)


def _tiny_model(wan_model_mod, sd=None):
    from oracle import make_golden, wan_dit_oracle as O
    cfg = O.DiTConfig(model_type="t2v", in_dim=16, num_layers=2, **make_golden.TINY)
    m = wan_model_mod.WanModel(num_layers=2, **make_golden.TINY)
    m.load_state_dict(sd if sd is not None else O.synth_state_dict(cfg, "gradclip"))
    return m.cuda().train()


def _tiny_batch():
    from oracle import detgen
    noise = torch.from_numpy(detgen.normalish("gradclip/x", (2, 16, 2, 6, 8))).cuda()
    ctx = torch.from_numpy(detgen.normalish("gradclip/c", (2, 32, 64))).cuda()
    vt = torch.from_numpy(detgen.normalish("gradclip/vt", (2, 16, 2, 6, 8))).cuda()
    return noise, ctx, vt


def test_fused_step_equals_clip_then_step_on_a_model(wan_model_mod):
    """The pack kernel (omh_adamw_pack_multi_dev): AdamW and the bf16 operand copies in one pass, clipped."""
    optim = _optim()
    trainer = importlib.import_module(PKG + ".trainer")
    batch = _tiny_batch()
    ma, mb = _tiny_model(wan_model_mod), _tiny_model(wan_model_mod)
    oa = ob = None
    for it in range(3):
        trainer.forward_backward(batch, ma, reference_loss_quirk=False)
        trainer.forward_backward(batch, mb, reference_loss_quirk=False)
        for pa, pb in zip(ma.parameters(), mb.parameters()):           # the very same gradients on both sides
            assert (pa.grad is None) == (pb.grad is None)
            if pa.grad is not None:
                pb.grad.copy_(pa.grad)
        given = {n: p.grad.clone() for n, p in ma.named_parameters() if p.grad is not None}
        if oa is None:
            norm = torch.sqrt(sum((g.double() ** 2).sum() for g in given.values())).item()
            c = 0.5 * norm
            kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
            oa, ob = optim.AdamW(ma.parameters(), max_grad_norm=c, **kw), optim.AdamW(mb.parameters(), **kw)
        oa.step()
        ret = optim.clip_grad_norm_(mb.parameters(), c)
        ob.step()
        assert torch.equal(oa.grad_norm, ret)
        if it == 0:
            assert ret.item() > c
        for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            if pa.grad is None:
                continue
            assert torch.equal(pa.grad, given[n]), n
            assert torch.equal(pa.detach(), pb.detach()), n
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]), n
            assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"]), n
        oa.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
    assert any(len(k) == 4 and k[3] == "pack" for k in oa._tables)     # it was the pack kernel


def test_next_forward_sees_the_clipped_update(wan_model_mod):
    optim = _optim()
    trainer = importlib.import_module(PKG + ".trainer")
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    batch = _tiny_batch()
    m = _tiny_model(wan_model_mod)
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    trainer.forward_backward(batch, m, reference_loss_quirk=False)
    norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)).item()
    opt = optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=0.5 * norm)
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert abs(opt.grad_norm.item() - norm) <= TOL_NORM * norm         # clipped to half of it
    assert any(not torch.equal(p.detach(), start[n]) for n, p in m.named_parameters())
    packs = mt.TrainPacks.of(m)
    assert packs.sig == [p._version for p in packs.params]             # the copies were current when the step returned
    before = [{k: (v.clone() if v is not None else None) for k, v in blk.items()} for blk in packs.blocks]
    packs.sig = None                                                    # force the re-pack launch over every entry
    packs.refresh(m)
    for blk_b, blk_a in zip(before, packs.blocks):
        for k in blk_b:
            if blk_b[k] is not None:
                assert torch.equal(blk_b[k], blk_a[k]), k
    args = (batch[0], torch.ones(2, device="cuda") * 1000.0, [batch[1][0], batch[1][1]], 24)
    with torch.no_grad():
        after = torch.stack(m(*args))
    fresh = _tiny_model(wan_model_mod, m.state_dict()).eval()
    with torch.no_grad():
        ref = torch.stack(fresh(*args))
    assert torch.equal(after, ref)


def test_no_host_round_trip(ops, bag, monkeypatch):
    optim = _optim()
    grads, norm64 = bag
    ps = _params(grads)
    opt = optim.AdamW(ps, lr=1e-3, max_grad_norm=0.5 * norm64)
    optim.clip_grad_norm_(ps, 0.9 * norm64)                             # warm-up: tables uploaded, state allocated
    opt.step()

    def refuse(*a, **k):
        raise AssertionError("host round trip")
    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(torch.cuda, "synchronize", refuse)
    ret = optim.clip_grad_norm_(ps, 0.9 * norm64)
    opt.step()
    monkeypatch.undo()
    assert ret.is_cuda and opt.grad_norm.is_cuda
    assert torch.isfinite(ret).item() and torch.isfinite(opt.grad_norm).item()


def test_torch_state_dict_loads_and_steps(ops, bag):
    optim = _optim()
    grads, _ = bag
    theirs, ours = _params(grads[:4]), _params(grads[:4])
    t_opt = torch.optim.AdamW(theirs, lr=1e-3, weight_decay=0.01)
    t_opt.step()
    opt = optim.AdamW(ours, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    opt.load_state_dict(t_opt.state_dict())
    before = [p.detach().clone() for p in ours]
    opt.step()
    assert opt.max_grad_norm == 1.0 and opt.grad_norm.item() > 1.0
    assert all(int(opt.state[p]["step"]) == 2 for p in ours)
    assert all(not torch.equal(p.detach(), b) and torch.isfinite(p).all() for p, b in zip(ours, before))
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd["param_groups"][0]
    assert set(sd["param_groups"][0]) <= set(t_opt.state_dict()["param_groups"][0])
