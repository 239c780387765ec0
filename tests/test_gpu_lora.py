"""Low-rank adapters on the GPU: the fused effective-weight pack, the fp32 merge, the skinny adapter-gradient kernels,
and the adapted WanModel in inference, training and through its life cycle (lora.py, csrc/lora.hip).

Bounds.  Pack: one bf16 ulp of bf16(fp64 reference).  Merge: 4 x the error of torch's own fp32 ``W + s * (B @ A)``
against fp64, measured on the CPU in the test (another but fixed summation order over the rank).  Gradient kernels:
U = x A^T and T = dy B are kept in bf16 and A, B enter the MFMA as bf16 — two factors of every product chain carry a
rounding of at most 2^-9 relative each, the fp32 accumulation is far below that, so 2^-8 as relative RMS against fp64 of
the same inputs.  Model gradients against the fp32 autograd reference: TOL_GRAD = 2e-2, the bound of
tests/test_gpu_train.py::test_all_gradients_match_autograd_oracle for the full-weight gradients of the same miniature
(dA and dB are linear images of those).  Consistency with the full path: 2 x the error of the same quantity computed in
torch with U and T rounded as the kernel rounds them.  Every figure is printed ``[measured] ...`` before it is asserted;
with OMH_LORA_PARITY_OUT=<file> the module writes them there (the record kept as profiles/lora_parity.json)."""
import copy
import importlib
import json
import os

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu
TOL_GRAD = 2e-2
TOL_SKINNY = 2.0 ** -8
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("OMH_LORA_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as fh:
            json.dump(_FIGURES, fh, indent=1, sort_keys=True)


def _record(key, **kw):
    _FIGURES[key] = kw
    print(f"[measured] {key}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()))


@pytest.fixture(scope="module")
def model_mod():
    return importlib.import_module(PKG + ".wan.modules.model")


@pytest.fixture(scope="module")
def mt():
    return importlib.import_module(PKG + ".wan.modules.model_train")


@pytest.fixture(scope="module")
def lora():
    return importlib.import_module(PKG + ".lora")


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def _tiles(r, c):
    return ((r + 63) // 64) * ((c + 63) // 64)


def _ordered(t_bf16):
    """bf16 bit patterns as integers that are monotone in the value (sign-magnitude -> ordered)."""
    i = t_bf16.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def _adapter(out, inn, r, gen, same_sign=True):
    """|s B A| ~ |W|.  ``same_sign``: every element of W has the sign of its update, so no sum cancels and the fp32
    result is accurate to far below a bf16 ulp of ITSELF; with free signs a few of the 10^5 elements cancel to a small
    fraction of their operands and carry the fp32 rounding of the operands' scale (see test_fused_pack_matches_fp64)."""
    W = (torch.randn(out, inn, generator=gen) * 0.05)
    A = torch.randn(r, inn, generator=gen)
    B = torch.randn(out, r, generator=gen)
    s = 0.05 / r ** 0.5
    if same_sign:
        W = W.abs() * torch.sign(B.double() @ A.double()).float()
    return W, A, B, s


def _pack_case(ops, model_mod, out, inn, r, seed, same_sign=True):
    """Fused pack of one adapted weight into the j = 1 slot of a shared [2 out, in] buffer (the q | k | v layout) and
    of a second weight WITHOUT an adapter in the same table.  Returns what the tests compare."""
    gen = torch.Generator().manual_seed(seed)
    W, A, B, s = _adapter(out, inn, r, gen, same_sign)
    W2 = torch.randn(inn, out, generator=gen) * 0.05
    ref = (W.double() + s * (B.double() @ A.double())).float()
    assert torch.isfinite(ref).all()                         # the reference alone first
    Wd, Ad, Bd, W2d = W.cuda(), A.cuda(), B.cuda(), W2.cuda()
    buf = torch.zeros(2 * out, inn, dtype=torch.bfloat16, device="cuda")
    bufT = torch.zeros(inn, 2 * out, dtype=torch.bfloat16, device="cuda")
    d2, d2T = torch.zeros(inn, out, dtype=torch.bfloat16, device="cuda"), torch.zeros(out, inn, dtype=torch.bfloat16, device="cuda")
    rows = [model_mod.lora_pack_row(Wd, buf[out:], bufT[:, out:], inn, 2 * out, (Ad, Bd, s)),
            model_mod.lora_pack_row(W2d, d2, d2T, out, inn, None)]
    rows[1][7] = _tiles(out, inn)
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    ops.pack_weights_lora_multi(table, 2, _tiles(out, inn) + _tiles(inn, out))
    return dict(W=Wd, A=Ad, B=Bd, s=s, ref=ref, got=buf[out:], gotT=bufT[:, out:], buf=buf, bufT=bufT, W2=W2d, d2=d2, d2T=d2T,
                table=table)


PACK_SHAPES = [(256, 256), (320, 256), (256, 320), (64, 192)]
RANKS = [1, 8, 20, 128]


# ------------------------------------------------------------------------------------------------------ 1. pack kernel
@pytest.mark.parametrize("out,inn", PACK_SHAPES)
@pytest.mark.parametrize("r", RANKS)
def test_fused_pack_matches_fp64(ops, model_mod, out, inn, r):
    """Both copies within ONE bf16 ulp of bf16(fp64 reference), every element, on inputs whose sums do not cancel.
    With free signs the fp32 accumulation the kernel is specified with cannot meet a bound that scales with the RESULT:
    an element whose W and s B A cancel to 10^-3 of their size carries the fp32 rounding of the operands (measured on
    this kernel: up to 4 bf16 codes on 4 of 81 920 elements at 256 x 320, rank 8).  That case is held to one bf16 ulp
    at the scale of the larger of the operands and the result, max(|W|, |s B A|, |W + s B A|), which no cancellation
    excuses."""
    c = _pack_case(ops, model_mod, out, inn, r, 100 + r)
    ref_b = c["ref"].to(torch.bfloat16).cuda()
    ratio = float((c["s"] * (c["B"] @ c["A"])).abs().mean() / c["W"].abs().mean())
    assert 0.3 < ratio < 3.0                                 # not vacuous: the update is comparable to the weight
    for name, got, want in (("copy", c["got"], ref_b), ("transposed", c["gotT"], ref_b.t())):
        ulps = (_ordered(got.contiguous()) - _ordered(want.contiguous())).abs()
        _record(f"pack/{out}x{inn}/r{r}/{name}", max_ulp=int(ulps.max()), differing=float((ulps > 0).float().mean()))
        assert int(ulps.max()) <= 1, (name, int(ulps.max()))
    f = _pack_case(ops, model_mod, out, inn, r, 200 + r, same_sign=False)
    W64, upd = f["W"].double().cpu(), f["s"] * (f["B"].double().cpu() @ f["A"].double().cpu())
    scale = torch.maximum(torch.maximum(W64.abs(), upd.abs()), (W64 + upd).abs())       # (the sum may reach the next binade)
    ulp = torch.exp2(torch.floor(torch.log2(scale)) - 7)
    for name, got in (("copy", f["got"]), ("transposed", f["gotT"].t())):
        err = ((got.double().cpu() - (W64 + upd)).abs() / ulp).max().item()
        own = int((_ordered(got.contiguous()) - _ordered(f["ref"].to(torch.bfloat16).cuda())).abs().max())
        _record(f"pack_free_signs/{out}x{inn}/r{r}/{name}", ulp_of_operand_scale=err, codes_from_reference=own)
        assert err <= 1.0, (name, err)
    # the halves of the shared buffers this entry does not own are untouched
    assert not c["buf"][:out].any() and not c["bufT"][:, :out].any()
    # the entry without an adapter: the bits of omh_pack_weights_multi
    p2, p2T = torch.zeros_like(c["d2"]), torch.zeros_like(c["d2T"])
    t9 = torch.tensor([[c["W2"].data_ptr(), p2.data_ptr(), p2T.data_ptr(), inn, out, out, inn, 0, 0]], dtype=torch.int64).cuda()
    ops.pack_weights_multi(t9, 1, _tiles(inn, out))
    assert torch.equal(c["d2"], p2) and torch.equal(c["d2T"], p2T)


# ------------------------------------------------------------------------------------------------------ 2. merge kernel
@pytest.mark.parametrize("out,inn", PACK_SHAPES)
@pytest.mark.parametrize("r", RANKS)
def test_merge_matches_fp64_and_fused_pack(ops, model_mod, out, inn, r):
    c = _pack_case(ops, model_mod, out, inn, r, 100 + r)
    W, A, B, s = c["W"].cpu(), c["A"].cpu(), c["B"].cpu(), c["s"]
    ref64 = W.double() + s * (B.double() @ A.double())
    e_torch = rel_rms(W + s * (B @ A), ref64)                # torch's own fp32 arithmetic against fp64, on the CPU
    Wm = c["W"].clone()
    row = model_mod.lora_pack_row(Wm, None, None, 0, 0, (c["A"], c["B"], s))
    ops.lora_merge(torch.tensor([row], dtype=torch.int64).cuda(), 1, _tiles(out, inn))
    e_kernel = rel_rms(Wm.cpu(), ref64)
    _record(f"merge/{out}x{inn}/r{r}", torch_fp32=e_torch, kernel=e_kernel, bound=4 * e_torch)
    assert e_kernel <= 4 * e_torch
    # a plain pack of the merged weight: the bits of the fused pack
    p, pT = torch.zeros(out, inn, dtype=torch.bfloat16, device="cuda"), torch.zeros(inn, out, dtype=torch.bfloat16, device="cuda")
    t9 = torch.tensor([[Wm.data_ptr(), p.data_ptr(), pT.data_ptr(), out, inn, inn, out, 0, 0]], dtype=torch.int64).cuda()
    ops.pack_weights_multi(t9, 1, _tiles(out, inn))
    assert torch.equal(p, c["got"]) and torch.equal(pT, c["gotT"])


# ------------------------------------------------------------------------------------------------------ 3. gradient kernels
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("r", RANKS)
def test_adapter_gradient_kernels(ops, M, r):
    gen = torch.Generator().manual_seed(7 * M + r)
    for n_in, n_out in ((128, 320), (320, 128)):
        x = torch.randn(M, n_in, generator=gen).to(torch.bfloat16).cuda()
        full = torch.randn(M, n_out + 64, generator=gen).to(torch.bfloat16).cuda()
        dy = full[:, 64:]                                    # a column slice of a wider buffer, as dq | dk | dv
        A, B = torch.randn(r, n_in, generator=gen).cuda(), torch.randn(n_out, r, generator=gen).cuda()
        s = 0.37
        xd, dyd, Ad, Bd = x.double(), dy.double(), A.double(), B.double()
        refA, refB = s * (dyd @ Bd).t() @ xd, s * dyd.t() @ (xd @ Ad.t())
        assert torch.isfinite(refA).all() and torch.isfinite(refB).all()
        dA, dB, _ = ops.lora_grads(x, dy, A, B, s)
        eA, eB = rel_rms(dA, refA), rel_rms(dB, refB)
        _record(f"grads/M{M}/r{r}/{n_in}->{n_out}", dA=eA, dB=eB, bound=TOL_SKINNY)
        assert eA < TOL_SKINNY and eB < TOL_SKINNY
        dA2, dB2, _ = ops.lora_grads(x, dy, A, B, s)         # no atomics: the same bits
        assert torch.equal(dA, dA2) and torch.equal(dB, dB2)
        prevA, prevB = torch.randn_like(dA), torch.randn_like(dB)
        accA, accB = prevA.clone(), prevB.clone()
        ops.lora_grads(x, dy, A, B, s, accA, accB, True, True)
        assert rel_rms(accA - prevA, refA) < TOL_SKINNY and rel_rms(accB - prevB, refB) < TOL_SKINNY
        assert torch.equal(accA, prevA + dA) and torch.equal(accB, prevB + dB)
        mixA, mixB = prevA.clone(), prevB.clone()             # the two flags are independent
        ops.lora_grads(x, dy, A, B, s, mixA, mixB, False, True)
        assert torch.equal(mixA, dA) and torch.equal(mixB, accB)


# ------------------------------------------------------------------------------------------------------ model fixtures
def _case(model_mod, model_type="t2v", ffn_dim=512, seed_tag=""):
    from oracle import make_golden, wan_dit_oracle as O
    cfg, tag, xs, ctx, t, seq_len, ys, clip = make_golden.tiny_case(model_type, 2)
    tiny = dict(make_golden.TINY, ffn_dim=ffn_dim)
    cfg = O.DiTConfig(model_type=model_type, in_dim=cfg.in_dim, num_layers=2, **tiny)
    sd = O.synth_state_dict(cfg, tag + seed_tag)
    m = model_mod.WanModel(model_type=model_type, in_dim=cfg.in_dim, num_layers=2, **tiny)
    m.load_state_dict(sd)
    gen = torch.Generator().manual_seed(5)
    targets = [torch.randn(16, *u.shape[1:], generator=gen) for u in xs]
    return dict(cfg=cfg, sd=sd, m=m.cuda().train(), xs=xs, ctx=ctx, t=t, seq_len=seq_len, ys=ys, clip=clip, targets=targets)


def _fwd(c, m, grad=True):
    kw = dict(clip_fea=None if c["clip"] is None else c["clip"].cuda(), y=None if c["ys"] is None else [u.cuda() for u in c["ys"]])
    with torch.enable_grad() if grad else torch.no_grad():
        return m([u.cuda() for u in c["xs"]], c["t"].cuda(), [u.cuda() for u in c["ctx"]], c["seq_len"], **kw)


def _loss(c, out):
    return sum(torch.nn.functional.mse_loss(o, v.cuda()) for o, v in zip(out, c["targets"]))


def _randomise(lora, m, seed=11, scale=0.05):
    """Non-zero A and B with an update comparable to the weights' own size."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, lin in lora.lora_modules(m):
            lin.lora_A.copy_((torch.randn(lin.lora_A.shape, generator=gen) * scale).cuda())
            lin.lora_B.copy_((torch.randn(lin.lora_B.shape, generator=gen) * scale).cuda())


# ------------------------------------------------------------------------------------------------------ 4. zero init
@pytest.mark.parametrize("ffn_dim", [512, 320])
def test_zero_init_adapter_changes_no_bit(model_mod, lora, ops, ffn_dim):
    """(The base gradients of two passes are compared bit for bit: as in tests/test_gpu_train.py that asks for the
    library's ordered reductions — by default the bias, gain and modulation sums of the backward use fp32 atomics, and
    two passes over the SAME model differ in their last bits.)"""
    was = ops.set_deterministic(None)
    ops.set_deterministic(True)
    try:
        _zero_init(model_mod, lora, ffn_dim)
    finally:
        ops.set_deterministic(was)


def _zero_init(model_mod, lora, ffn_dim):
    c = _case(model_mod, ffn_dim=ffn_dim)
    bare = c["m"]
    ad = copy.deepcopy(bare)
    lora.add_lora(ad, 8, freeze_base=False)
    assert all(not lin.lora_B.any() for _, lin in lora.lora_modules(ad))
    for a, b in zip(_fwd(c, ad, False), _fwd(c, bare, False)):
        assert torch.equal(a, b)
    x, t = [u.cuda() for u in c["xs"][:1]], c["t"][:1].cuda()
    ctx, null = [c["ctx"][0].cuda()], [c["ctx"][1].cuda()]
    for a, b in zip(_pair(ad, x, t, ctx, null, c["seq_len"]), _pair(bare, x, t, ctx, null, c["seq_len"])):
        assert torch.equal(a[0], b[0])
    oa, ob = _fwd(c, ad), _fwd(c, bare)
    for a, b in zip(oa, ob):
        assert torch.equal(a, b)
    la, lb = _loss(c, oa), _loss(c, ob)
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    pa = dict(ad.named_parameters())
    assert sum(p.grad is not None for p in bare.parameters()) > 50
    for n, p in bare.named_parameters():
        same = (p.grad is None and pa[n].grad is None) or torch.equal(p.grad, pa[n].grad)
        assert same, f"gradient of {n} differs between the adapted and the bare model"
    for _, lin in lora.lora_modules(ad):
        assert lin.lora_B.grad is not None and lin.lora_B.grad.abs().max() > 0      # dB = s dW A^T is not zero
        assert not lin.lora_A.grad.any()                                           # dA = s B^T dW is, with B = 0


def _pair(m, x, t, ctx, null, seq_len):
    with torch.no_grad():
        return m.forward_cfg_pair(x, t, ctx, null, seq_len)


# ------------------------------------------------------------------------------------------------------ 5. autograd reference
@pytest.mark.parametrize("model_type,ffn_dim", [("t2v", 512), ("i2v", 512), ("t2v", 320)])
def test_adapter_gradients_match_autograd_reference(model_mod, lora, model_type, ffn_dim):
    from oracle import wan_dit_oracle as O
    c = _case(model_mod, model_type, ffn_dim)
    m = c["m"]
    lora.add_lora(m, 8, alpha=16)
    _randomise(lora, m)
    # the reference: W + s B A as an autograd expression of the leaves A and B, everything in fp32 on the CPU
    leaves, osd = {}, dict(c["sd"])
    for name, lin in lora.lora_modules(m):
        A = lin.lora_A.detach().cpu().clone().requires_grad_(True)
        B = lin.lora_B.detach().cpu().clone().requires_grad_(True)
        leaves[name] = (A, B)
        osd[name + ".weight"] = c["sd"][name + ".weight"] + (16.0 / 8) * (B @ A)
    xs_o = [u.clone().requires_grad_(True) for u in c["xs"]]
    ctx_o = [u.clone().requires_grad_(True) for u in c["ctx"]]
    oo = O.dit_forward_autograd(osd, c["cfg"], xs_o, c["t"], ctx_o, c["seq_len"], clip_fea=c["clip"], y=c["ys"])
    lo = sum(torch.nn.functional.mse_loss(a, b) for a, b in zip(oo, c["targets"]))
    lo.backward()
    assert all(torch.isfinite(A.grad).all() and torch.isfinite(B.grad).all() for A, B in leaves.values())
    bits = {}
    for ckpt in (False, True):
        m.use_checkpoint, m.checkpoint_policy = ckpt, "always"
        m.zero_grad(set_to_none=True)
        xs = [u.cuda().requires_grad_(True) for u in c["xs"]]
        ctx = [u.cuda().requires_grad_(True) for u in c["ctx"]]
        kw = dict(clip_fea=None if c["clip"] is None else c["clip"].cuda(), y=None if c["ys"] is None else [u.cuda() for u in c["ys"]])
        out = m(xs, c["t"].cuda(), ctx, c["seq_len"], **kw)
        lg = _loss(c, out)
        lg.backward()
        assert abs(lg.item() - lo.item()) < 2e-2 * lo.item()
        assert all(p.grad is None for n, p in m.named_parameters() if "lora_" not in n)     # the base is frozen
        bad, worst = [], 0.0
        for name, lin in lora.lora_modules(m):
            for nm, got, ref in (("lora_A", lin.lora_A.grad, leaves[name][0].grad), ("lora_B", lin.lora_B.grad, leaves[name][1].grad)):
                err = rel_rms(got, ref)
                worst = max(worst, err)
                if err >= TOL_GRAD:
                    bad.append((f"{name}.{nm}", err))
        errs_in = [rel_rms(a.grad, b.grad) for a, b in zip(xs + ctx, xs_o + ctx_o)]
        _record(f"model/{model_type}/ffn{ffn_dim}/checkpoint={ckpt}", worst_adapter=worst, worst_input=max(errs_in), bound=TOL_GRAD)
        assert not bad, bad[:8]
        assert max(errs_in) < TOL_GRAD
        bits[ckpt] = [lin.lora_A.grad.clone() for _, lin in lora.lora_modules(m)] + \
            [lin.lora_B.grad.clone() for _, lin in lora.lora_modules(m)]
    assert all(torch.equal(a, b) for a, b in zip(bits[False], bits[True]))       # use_checkpoint: the same bits


# ------------------------------------------------------------------------------------------------------ 6. the full path
def test_adapter_gradients_consistent_with_weight_gradients(model_mod, lora, mt, monkeypatch):
    c = _case(model_mod)
    m = c["m"]
    lora.add_lora(m, 8, alpha=4, freeze_base=False)
    _randomise(lora, m)
    calls = []
    real = mt.ops.lora_grads

    def spy(x, dy, A, B, s, *a, **k):
        calls.append((x.clone(), dy.clone(), A.data_ptr()))
        return real(x, dy, A, B, s, *a, **k)
    monkeypatch.setattr(mt.ops, "lora_grads", spy)
    _loss(c, _fwd(c, m)).backward()
    torch.cuda.synchronize()
    by_ptr = {a: (x, dy) for x, dy, a in calls}
    assert len(calls) == len(lora.lora_modules(m)) == 20
    bf = lambda v: v.to(torch.bfloat16).float()
    for name, lin in lora.lora_modules(m):
        A, B, s = model_mod.lora_of(lin)
        A, B, dW = A.detach(), B.detach(), lin.weight.grad
        refB, refA = s * dW @ A.t(), s * B.t() @ dW          # from the existing path's weight gradient, fp32 torch
        x, dy = (v.float() for v in by_ptr[A.data_ptr()])
        # the same two quantities with U and T (and the MFMA's A, B operands) rounded the way the kernel rounds them
        emuB = s * dy.t() @ bf(x @ bf(A).t())
        emuA = s * bf(dy @ bf(B)).t() @ x
        bB, bA = 2 * rel_rms(emuB, refB), 2 * rel_rms(emuA, refA)
        eB, eA = rel_rms(lin.lora_B.grad, refB), rel_rms(lin.lora_A.grad, refA)
        _record(f"consistency/{name}", dA=eA, dA_bound=bA, dB=eB, dB_bound=bB)
        assert eB < bB and eA < bA, name


# ------------------------------------------------------------------------------------------------------ 7. frozen-base training
def _train(model_mod, lora, optim, mt, steps):
    c = _case(model_mod)
    m = c["m"]
    torch.manual_seed(3)
    params = lora.add_lora(m, 8)
    base = {n: p.detach().clone() for n, p in m.named_parameters() if "lora_" not in n}
    opt = optim.AdamW(params, lr=2e-3)
    c["pending"] = mt.pending_step_bytes(m)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = _loss(c, _fwd(c, m))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return c, m, params, base, opt, losses


def test_frozen_base_training(model_mod, lora, optim, mt):
    c, m, params, base, opt, losses = _train(model_mod, lora, optim, mt, 20)
    _record("train/frozen_base", first=losses[0], last=losses[-1])
    assert losses[-1] < losses[0]
    for n, p in m.named_parameters():
        if "lora_" not in n:
            assert torch.equal(p, base[n]) and p.grad is None, n
    assert set(map(id, opt.state)) == set(map(id, params)) and len(opt.state) == len(params)
    assert c["pending"] == 12 * sum(p.numel() for p in params)      # before the first step: gradients + two moments
    c2, m2, _, _, _, losses2 = _train(model_mod, lora, optim, mt, 20)
    assert losses2 == losses                                  # the same seed: bit-identical
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)


def test_gradient_accumulation_adds_the_micro_steps(model_mod, lora):
    c = _case(model_mod)
    m = c["m"]
    params = lora.add_lora(m, 8)
    _randomise(lora, m)
    c2 = dict(c, targets=[v + 0.5 for v in c["targets"]])
    single = []
    for cc in (c, c2):
        m.zero_grad(set_to_none=True)
        _loss(cc, _fwd(cc, m)).backward()
        single.append([p.grad.clone() for p in params])
    m.zero_grad(set_to_none=True)
    for cc in (c, c2):                                        # the second micro-step adds into the existing .grad
        _loss(cc, _fwd(cc, m)).backward()
    for p, g1, g2 in zip(params, *single):
        assert torch.equal(p.grad, g1 + g2)


# ------------------------------------------------------------------------------------------------------ 8. life cycle
@pytest.mark.parametrize("model_type", ["t2v", "i2v"])
def test_adapter_life_cycle(model_mod, lora, optim, model_type, tmp_path):
    c = _case(model_mod, model_type)
    m = c["m"]
    bare_out = _fwd(c, m, False)
    bare_keys = list(m.state_dict())
    params = lora.add_lora(m, 8, alpha=16)
    _randomise(lora, m)
    opt = optim.AdamW(params, lr=1e-3)
    _loss(c, _fwd(c, m)).backward()
    opt.step()
    out = _fwd(c, m, False)
    assert not torch.equal(out[0], bare_out[0])
    # a ContextState from before a scale change is rejected
    state = m.encode_context([u.cuda() for u in c["ctx"]], None if c["clip"] is None else c["clip"].cuda())
    # merge on a deep copy: a plain model with W + s B A computes the adapted model's bits
    merged = lora.merge_lora(copy.deepcopy(m))
    assert list(merged.state_dict()) == bare_keys
    for a, b in zip(out, _fwd(c, merged, False)):
        assert torch.equal(a, b)
    # save -> load into a fresh model
    path = tmp_path / "adapter.pt"
    torch.save(lora.lora_state_dict(m), path)
    fresh = _case(model_mod, model_type)["m"]
    lora.load_lora_state_dict(fresh, torch.load(path))
    for a, b in zip(out, _fwd(c, fresh, False)):
        assert torch.equal(a, b)
    # strength 0: the bare model's bits; the cached context is from another scale
    lora.set_lora_scale(m, 0.0)
    for a, b in zip(bare_out, _fwd(c, m, False)):
        assert torch.equal(a, b)
    kw = dict(clip_fea=None if c["clip"] is None else c["clip"].cuda(), y=None if c["ys"] is None else [u.cuda() for u in c["ys"]])
    with pytest.raises(ValueError, match="weights changed"), torch.no_grad():
        m([u.cuda() for u in c["xs"]], c["t"].cuda(), state, c["seq_len"], **kw)
    lora.set_lora_scale(m, None)
    for a, b in zip(out, _fwd(c, m, False)):
        assert torch.equal(a, b)
    lora.remove_lora(m)
    assert list(m.state_dict()) == bare_keys
    for a, b in zip(bare_out, _fwd(c, m, False)):
        assert torch.equal(a, b)
