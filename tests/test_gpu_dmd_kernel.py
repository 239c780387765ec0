"""omh_dmd_grad / omh_dmd_grad_scale and their wrappers ``ops.dmd_grad``, ``ops.dmd_loss``, ``ops.flow_noise`` against the
rule of include/omh.h evaluated in fp64 from the same fp32 inputs (``torch.randn`` with fixed seeds, guide 3,
sigma = (0.02, 0.5, 0.98)).

Shapes (B, n), the smallest at which each dispatch edge exists: (1, 5) scalar path only; (3, 1001) a ragged tail and three
sigmas (samples 1 and 2 start off a 16-byte boundary); (2, 3584) whole float4s; (3, CHUNK + 3) a second chunk of three
elements; (2, 21504) the tiny model's clip 16 x 6 x 14 x 16 — and each once more with every tensor one float off.

Bounds: ``norm`` within 2e-6 relative of fp64; ``grad`` within 2e-6 relative RMS per sample and 4e-6 of max|ref| in
maximum absolute error.  The expression is at most 8 fp32 roundings of 2^-24 on operands within about 4x of the result for
these inputs; the rule evaluated in plain fp32 on the CPU sits at 1.4e-8 - 4.4e-8 for the normaliser, 7e-8 - 1.1e-7
relative RMS and 1.2e-7 - 1.8e-7 maximum for ``grad`` at these sizes, so the bounds keep more than 10x above that for
contraction differences.  ``loss`` against 0.5 * mean(double(grad as stored)^2): 1e-12 relative (fp64 sums of at most
64 512 terms in another order)."""
import ctypes as C
import importlib

import pytest
import torch

from conftest import PKG
from dmd_ref import FLT_MAX, TOL_LOSS, TOL_MAX, TOL_NORM, TOL_RMS, rule as _rule

pytestmark = pytest.mark.gpu
GUIDE, SIGMA = 3.0, (0.02, 0.5, 0.98)
GUARD, SENTINEL = 4, -12345.0
_CASES = {}


@pytest.fixture(scope="module")
def lib(omh):
    return importlib.import_module(PKG + "._lib").lib


def _chunk():
    return importlib.import_module(PKG + ".ops").DMD_CHUNK


def _shapes():
    return [(1, 5), (3, 1001), (2, 3584), (3, _chunk() + 3), (2, 21504)]


def _case(B, n):
    """Inputs (CPU fp32) and the fp64 reference of a shape: made once, shared, left unchanged."""
    if (B, n) not in _CASES:
        g = torch.Generator().manual_seed(1000 * B + n)
        x, eps, vc, vu, vf = (torch.randn(B, n, generator=g) for _ in range(5))
        sigma = torch.tensor(SIGMA[:B])
        s = sigma.view(B, 1)
        xt = (1 - s) * x + s * eps
        inp = dict(x=x, xt=xt, vc=vc, vu=vu, vf=vf, sigma=sigma)
        _CASES[(B, n)] = (inp, _rule(x, xt, vc, vu, vf, sigma, GUIDE))
    return _CASES[(B, n)]


def _place(t, off):
    """``t`` on the device at ``off`` floats behind a fresh (512-byte aligned) allocation."""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def _run(lib, ops, inp, off=0, guide=GUIDE, cfg=True):
    """The raw entry on its own buffers: (grad, norm, loss fp64 [1], the guard elements around grad)."""
    d = {k: _place(v, off) for k, v in inp.items()}
    B, n = inp["x"].shape
    gbuf = torch.full((GUARD + off + B * n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    grad = gbuf[GUARD + off:GUARD + off + B * n].view(B, n)
    norm = _place(torch.zeros(B), off)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.dmd_grad_workspace_bytes(B, n) // 8, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.omh_dmd_grad(p(d["x"]), p(d["xt"]), p(d["vc"]), p(d["vu"]) if cfg else None, p(d["vf"]), p(d["sigma"]),
                          guide, B, n, p(grad), p(norm), p(loss), p(ws), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return grad.clone(), norm.clone(), loss.clone(), (gbuf[:GUARD + off].clone(), gbuf[GUARD + off + B * n:].clone())


def _within_bounds(grad, norm, ref_grad, ref_norm, what):
    grad, norm = grad.double().cpu(), norm.double().cpu()
    e_norm = float(((norm - ref_norm).abs() / ref_norm).max())
    e_rms = float(((grad - ref_grad).norm(dim=1) / ref_grad.norm(dim=1)).max())
    e_max = float((grad - ref_grad).abs().max() / ref_grad.abs().max())
    print(f"{what}: norm {e_norm:.2e} grad rel-RMS {e_rms:.2e} max {e_max:.2e}")
    assert e_norm < TOL_NORM and e_rms < TOL_RMS and e_max < TOL_MAX, what


def _loss_of(grad):
    return 0.5 * float(grad.double().square().mean())


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("B,n", _shapes())
def test_against_the_rule_in_fp64(lib, ops, B, n, off):
    inp, (ref_grad, ref_norm) = _case(B, n)
    grad, norm, loss, guards = _run(lib, ops, inp, off)
    _within_bounds(grad, norm, ref_grad, ref_norm, f"({B}, {n}) off {off}")
    want = _loss_of(grad)
    print(f"({B}, {n}) off {off}: loss {float(loss):.12e} from the stored grad {want:.12e}")
    assert abs(float(loss) - want) <= TOL_LOSS * want
    for g in guards:                                                 # nothing around grad is written
        assert bool((g == SENTINEL).all())
    again = _run(lib, ops, inp, off)                                 # a second run: the same bits
    assert torch.equal(again[0], grad) and torch.equal(again[1], norm) and torch.equal(again[2], loss)
    if off == 1:                                                     # one float off: the bits of the aligned call
        base = _run(lib, ops, inp, 0)
        assert torch.equal(base[0], grad) and torch.equal(base[1], norm) and torch.equal(base[2], loss)
    else:                                                            # the wrapper is this entry
        dev = {k: v.cuda() for k, v in inp.items()}
        g2, n2, l2 = ops.dmd_grad(dev["x"], dev["xt"], dev["vc"], dev["vu"], dev["vf"], dev["sigma"], GUIDE)
        assert torch.equal(g2, grad) and torch.equal(n2, norm) and torch.equal(l2, loss)
        assert not g2.requires_grad and l2.dtype == torch.float64 and n2.shape == (B,)


@pytest.mark.parametrize("n", [1001, "chunk+3"])
def test_a_sample_has_the_bits_it_has_alone(lib, ops, n):
    n = _chunk() + 3 if n == "chunk+3" else n
    inp, _ = _case(3, n)
    grad, norm, loss, _ = _run(lib, ops, inp)
    total = 0.0
    for b in range(3):
        one = {k: v[b:b + 1].clone() for k, v in inp.items()}
        g1, n1, l1, _ = _run(lib, ops, one)
        assert torch.equal(g1[0], grad[b]) and torch.equal(n1[0], norm[b]), b
        want = _loss_of(grad[b])                                     # the loss it would give alone
        assert abs(float(l1) - want) <= TOL_LOSS * want
        total += float(l1) / 3
    assert abs(total - float(loss)) <= TOL_LOSS * float(loss)
    flipped = dict(inp, sigma=inp["sigma"].flip(0))                  # the sigma of each sample is its own
    gf, nf, _, _ = _run(lib, ops, flipped)
    assert not torch.equal(gf[0], grad[0]) and not torch.equal(nf, norm) and torch.equal(nf[1], norm[1])


@pytest.mark.parametrize("B,n", [(3, 1001), (2, 3584)])
def test_no_uncond_is_guide_one(lib, ops, B, n):
    inp, _ = _case(B, n)
    ref_grad, ref_norm = _rule(inp["x"], inp["xt"], inp["vc"], None, inp["vf"], inp["sigma"], 1.0)
    plain = _run(lib, ops, inp, cfg=False)
    _within_bounds(plain[0], plain[1], ref_grad, ref_norm, f"({B}, {n}) without v_uncond")
    one = _run(lib, ops, inp, guide=1.0)
    _within_bounds(one[0], one[1], plain[0].double().cpu(), plain[1].double().cpu(), f"({B}, {n}) guide 1 against none")
    assert torch.equal(_run(lib, ops, inp, cfg=False, guide=7.0)[0], plain[0])          # guide is not read without v_uncond
    assert not torch.equal(_run(lib, ops, inp)[0], plain[0])


def test_degenerate_sample(lib, ops):
    """Sample 1 of 3 with x_t = x and a zero teacher: n_b = 0 exactly, grad = 0 / -+FLT_MAX by the sign of v_fake, a finite
    loss, and the neighbours keep their bits."""
    inp, _ = _case(3, 1001)
    base = _run(lib, ops, inp)
    deg = {k: v.clone() for k, v in inp.items()}
    deg["xt"][1] = deg["x"][1]
    deg["vc"][1] = 0.0
    deg["vu"][1] = 0.0
    deg["vf"][1, ::3] = 0.0
    assert float(deg["sigma"][1]) == 0.5
    grad, norm, loss, _ = _run(lib, ops, deg)
    vf = deg["vf"][1].cuda()
    assert float(norm[1]) == 0.0
    assert bool((grad[1][vf == 0] == 0).all()) and int((vf == 0).sum()) >= 334
    assert bool((grad[1][vf > 0] == -FLT_MAX).all()) and bool((grad[1][vf < 0] == FLT_MAX).all())
    assert int((vf > 0).sum()) > 0 and int((vf < 0).sum()) > 0
    assert bool(torch.isfinite(loss).all()) and float(loss) > 0
    for b in (0, 2):
        assert torch.equal(grad[b], base[0][b]) and torch.equal(norm[b], base[1][b])


@pytest.mark.parametrize("B,n", [(3, 1001), (2, 3584)])
def test_backward_is_one_multiply(ops, B, n):
    inp, _ = _case(B, n)
    dev = {k: v.cuda().requires_grad_(True) for k, v in inp.items()}
    raw, _, raw_loss = ops.dmd_grad(*[dev[k].detach() for k in ("x", "xt", "vc", "vu", "vf", "sigma")], GUIDE)
    inv = torch.tensor(1.0 / (B * n), dtype=torch.float32, device="cuda")
    for up in (None, 0.25):
        for v in dev.values():
            v.grad = None
        loss = ops.dmd_loss(dev["x"], dev["xt"], dev["vc"], dev["vu"], dev["vf"], dev["sigma"], GUIDE)
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad
        assert torch.equal(loss.detach(), raw_loss[0])
        (loss if up is None else loss * up).backward()
        c = inv if up is None else torch.tensor(up, dtype=torch.float32, device="cuda") * inv
        assert torch.equal(dev["x"].grad, raw * c)
        assert all(dev[k].grad is None for k in ("xt", "vc", "vu", "vf", "sigma"))
    with torch.no_grad():
        assert not ops.dmd_loss(dev["x"], dev["xt"], dev["vc"], dev["vu"], dev["vf"], dev["sigma"], GUIDE).requires_grad
    plain = ops.dmd_loss(dev["x"].detach(), dev["xt"], dev["vc"], None, dev["vf"], dev["sigma"], GUIDE)
    assert not plain.requires_grad and plain.dim() == 0


@pytest.mark.parametrize("B,n", [(3, 1001), (2, 3584)])
def test_flow_noise(ops, B, n):
    g = torch.Generator(device="cuda").manual_seed(7)
    x, eps = (torch.randn(B, n, device="cuda", generator=g) for _ in range(2))
    s = torch.tensor(SIGMA[:B], device="cuda")
    a, b = (1 - s.view(B, 1)) * x, s.view(B, 1) * eps               # each product and the sum rounded on its own
    out = ops.flow_noise(x.clone().requires_grad_(True), eps, s)
    assert torch.equal(out, a + b)
    assert not out.requires_grad and out.grad_fn is None and out.shape == x.shape
