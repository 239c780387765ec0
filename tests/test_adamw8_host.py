"""CPU: AdamW with FP8 block-scaled moments — the format's CPU restatement (tests/adamw8_ref.py) checked on its own, that
the format trains a toy regression as fp32 moments do, and what the new surface decides without a device: the keywords
of ``optim.AdamW`` and the argument checks of the four C entries."""
import importlib
import re
import os

import pytest
import torch

import adamw8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "omnihuman-1-hack_amd"
ENTRIES = ("omh_adamw8_pack_multi", "omh_adamw8_pack_multi_dev", "omh_moments_quantize", "omh_moments_dequantize")


# ------------------------------------------------------------------------------------------------- the rule itself
def test_every_finite_code_round_trips():
    codes = torch.arange(256, dtype=torch.uint8)
    vals = R.decode(codes)
    finite = torch.isfinite(vals)
    assert (~finite).nonzero().flatten().tolist() == [0x7f, 0xff]          # e4m3fn: two NaN codes, no infinities
    assert float(vals[0x7e]) == 448.0 and float(vals[0x01]) == 2.0 ** -9 and float(vals[0x08]) == 2.0 ** -6
    assert torch.equal(R.encode(vals[finite]), codes[finite])
    # through the block rule: a block whose largest magnitude is 448 has scale 1 and keeps every code
    x = torch.stack([vals[finite], torch.full((254,), 448.0)], 1)          # [254, 2]: one short block per row
    q, s = R.quantize(x)
    assert torch.equal(s, torch.ones_like(s)) and torch.equal(q[:, 0], codes[finite]) and (q[:, 1] == 0x7e).all()
    assert torch.equal(R.dequantize(q, s), x)


def test_ties_go_to_even():
    mags = R.MAGNITUDES.double()
    mid = ((mags[:-1] + mags[1:]) / 2).float()                              # exact in fp32: neighbours share 4 bits
    assert torch.equal(mid.double(), (mags[:-1] + mags[1:]) / 2)
    got = R.encode(mid).to(torch.int32)
    lo = torch.arange(0, 126, dtype=torch.int32)
    even = torch.where(lo % 2 == 0, lo, lo + 1)
    assert torch.equal(got, even)
    assert torch.equal(R.encode(-mid).to(torch.int32), even | 0x80)
    up = torch.nextafter(mid, torch.full_like(mid, 1e9))
    dn = torch.nextafter(mid, torch.zeros_like(mid))
    assert torch.equal(R.encode(up).to(torch.int32), lo + 1) and torch.equal(R.encode(dn).to(torch.int32), lo)


def test_root_floor_and_zero_block():
    v = torch.zeros(2, 128)
    v[0, 0] = 1.0                                                           # r = 1 -> scale 1 / 448, code 0x7e
    v[0, 1] = 1e-14                                                         # r = 1e-7: 4.5e-5 of a code step -> would be 0
    v[0, 2] = 0.0
    q, s = R.quantize(v, root=True)
    assert q[0, 0] == 0x7e and q[0, 1] == 0x01 and q[0, 2] == 0x00
    assert float(s[0, 0]) == pytest.approx(1 / 448, rel=1e-7)
    # block (0, 1) and row 1 are all zero: scale 0, codes 0, decoded 0 — no NaN
    assert float(s[0, 1]) == 0.0 and not s[1].any() and not q[0, 64:].any() and not q[1].any()
    back = R.dequantize(q, s, root=True)
    assert torch.isfinite(back).all() and not back[1].any() and float(back[0, 1]) > 0.0
    # the first moment has no floor: a tiny value beside a large one becomes a true zero
    qm, sm = R.quantize(torch.tensor([[1.0, 1e-7] + [0.0] * 62]))
    assert qm[0, 1] == 0 and torch.isfinite(R.dequantize(qm, sm)).all()
    # NaN codes are never produced for finite input, whatever the spread
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 200, generator=g) * torch.logspace(-20, 20, 200)[None]
    for root in (False, True):
        q, s = R.quantize(x.abs() if root else x, root=root)
        assert not ((q & 0x7f) == 0x7f).any() and torch.isfinite(s).all()


def test_uniform_decay_lands_in_the_scale():
    """Why the scale is fp32 and not a power of two: v -> beta2 v over a whole block keeps every code."""
    g = torch.Generator().manual_seed(1)
    v = torch.rand(4, 64, generator=g) + 0.01
    q0, s0 = R.quantize(v, root=True)
    v1 = R.dequantize(q0, s0, root=True) * 0.999
    q1, s1 = R.quantize(v1, root=True)
    assert (q1.int() - q0.int()).abs().max() <= 1 and (q1 != q0).float().mean() < 0.02
    assert torch.allclose(s1, s0 * (0.999 ** 0.5), rtol=1e-6, atol=0)


# --------------------------------------------------------------------------------------------- does the format train?
def _toy(eight_bit, steps=400, lr=1e-3):
    g = torch.Generator().manual_seed(1234)
    teacher = torch.randn(64, 8, generator=g) / 8
    lin1, lin2 = torch.nn.Linear(64, 128), torch.nn.Linear(128, 8)
    with torch.no_grad():
        for p in (*lin1.parameters(), *lin2.parameters()):               # torch's default init, from this generator
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / (p.shape[-1] if p.dim() == 2 else p.numel()) ** 0.5)
    W1, b1, W2, b2 = lin1.weight, lin1.bias, lin2.weight, lin2.bias
    params = [W1, b1, W2, b2]
    state = [R.zero_state(*p.shape) if (eight_bit and p.dim() == 2) else (torch.zeros_like(p), torch.zeros_like(p))
             for p in params]
    losses, dead = [], 0
    for t in range(1, steps + 1):
        X = torch.randn(256, 64, generator=g)                              # fresh samples: the floor is the noise, 0.65^2
        Y = X @ teacher + 0.65 * torch.randn(256, 8, generator=g)
        loss = ((torch.relu(X @ W1.t() + b1) @ W2.t() + b2 - Y) ** 2).mean()
        grads = torch.autograd.grad(loss, params)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for i, (p, gr) in enumerate(zip(params, grads)):
                if eight_bit and p.dim() == 2:
                    new, state[i] = R.step8(p, gr, state[i], lr, 0.9, 0.999, 1e-8, 0.01, t)
                    v = R.dequantize(state[i][2], state[i][3], root=True)
                    dead += int(((state[i][2] == 0) & (gr != 0)).sum())   # a gradient was seen: v > 0, so r code >= 1
                    assert (v[gr != 0] > 0).all()
                else:
                    new, m, v = R.adamw_update(p, gr, state[i][0], state[i][1], lr, 0.9, 0.999, 1e-8, 0.01, t)
                    state[i] = (m, v)
                p.copy_(new)
    return losses, [p.detach() for p in params], dead


def test_the_format_trains_a_toy_regression():
    """Two layers 64 -> 128 -> 8 on a noisy linear teacher (fresh samples every step, so the loss ends on the noise
    floor 0.65^2 = 0.42 and nothing is memorised), 400 steps, lr 1e-3, both weight matrices with 8-bit state.  The
    reference alone: it documents that the format trains and says nothing about the kernel.  Mean loss of the last 20
    steps: 0.43676 (8-bit) against 0.43755 (fp32), 0.18 % apart; parameters 1 - 10 % rel-RMS apart; the bound is 1 %.
    (While the loss still falls the two curves are up to 1 % apart at equal step — the 8-bit run is not behind.)"""
    l8, p8, dead = _toy(True)
    l32, p32, _ = _toy(False)
    a8, a32 = sum(l8[-20:]) / 20, sum(l32[-20:]) / 20
    gap = abs(a8 - a32) / a32
    print(f"last-20 mean loss: 8-bit {a8:.5f}, fp32 {a32:.5f}, gap {100 * gap:.3f} %")
    assert a32 < 0.8 * (sum(l32[:20]) / 20), "the toy must train at all"
    assert gap <= 0.01
    assert dead == 0


# ------------------------------------------------------------------------------------------------------- arguments
def test_header_declares_the_entries_and_the_format():
    src = open(os.path.join(ROOT, "include", "omh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"^#define\s+OMH_ABI_VERSION\s+12\s*$", code, flags=re.M)
    at = src.index("int omh_adamw8_pack_multi")
    doc = src[src.rfind("/* Additive", 0, at):at]
    for word in ("e4m3fn", "448", "sqrt(v)", "0x01", "0x7f", "ceil(cols / 64)"):
        assert word in doc, word


def test_bindings_and_argument_checks(omh, ops):
    binding = importlib.import_module(PKG + "._lib")
    lib = binding.lib
    for name in ENTRIES:
        assert name in binding.EXPORTED and hasattr(lib, name)
    assert lib.omh_abi_version() == 12
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.omh_adamw8_pack_multi(None, 1, 1, *hp, 1, 1.0, None) == -1         # null table
    assert lib.omh_adamw8_pack_multi(16, 0, 1, *hp, 1, 1.0, None) == -1
    assert lib.omh_adamw8_pack_multi(16, 1, 0, *hp, 1, 1.0, None) == -1
    assert lib.omh_adamw8_pack_multi(16, 1, 1 << 31, *hp, 1, 1.0, None) == -1
    assert lib.omh_adamw8_pack_multi(16, 1, 1, *hp, 0, 1.0, None) == -1           # step 0
    assert lib.omh_adamw8_pack_multi(16, 1, 1, *hp, 1, 0.0, None) == -1           # a zero loss scale
    assert lib.omh_adamw8_pack_multi_dev(None, 1, 1, *hp, 1, 1.0, 16, None) == -1
    assert lib.omh_adamw8_pack_multi_dev(16, 1, 1, *hp, 1, 1.0, None, None) == -1  # null coefficient
    assert lib.omh_adamw8_pack_multi_dev(16, 1, 1, *hp, 0, 1.0, 16, None) == -1
    for fn in (lib.omh_moments_quantize, lib.omh_moments_dequantize):
        for second in (0, 1):
            assert fn(None, 1, 1, second, None) == -1
            assert fn(16, 0, 1, second, None) == -1
            assert fn(16, 1, 0, second, None) == -1
            assert fn(16, 1, 1 << 31, second, None) == -1
    for name in ("adamw8_pack_multi", "adamw8_pack_multi_dev", "moments_quantize", "moments_dequantize"):
        assert callable(getattr(ops, name))
    with pytest.raises(ops.OmhError):                                             # no CPU fallback
        ops.moments_quantize(torch.zeros(1, 6, dtype=torch.int64), 1, 1, False)


def test_adamw_keywords(omh):
    optim = importlib.import_module(PKG + ".optim")
    mt = importlib.import_module(PKG + ".wan.modules.model_train")
    w = torch.nn.Parameter(torch.zeros(64, 64))
    b = torch.nn.Parameter(torch.zeros(64))
    small = torch.nn.Parameter(torch.zeros(8, 8))
    for bad in ("int4", "bf16", None, 8):
        with pytest.raises(ValueError):
            optim.AdamW([w], moments=bad)
    for bad in (-1, 1.5, "4096"):
        with pytest.raises(ValueError):
            optim.AdamW([w], moments="fp8", min_8bit_size=bad)
    plain = optim.AdamW([w, b, small])
    assert plain.moments == "fp32" and plain.min_8bit_size == 4096
    assert not any(hasattr(p, "_omh_moment_bytes") for p in (w, b, small))
    lin = torch.nn.Linear(64, 64)
    lin.weight, lin.bias = w, b
    assert mt.pending_step_bytes(lin) == 12 * (w.numel() + b.numel())
    opt = optim.AdamW([w, b, small], moments="fp8")
    assert opt.moments == "fp8" and w._omh_moment_bytes == 2.125
    assert not hasattr(b, "_omh_moment_bytes") and not hasattr(small, "_omh_moment_bytes")
    assert mt.pending_step_bytes(lin) == int(6.125 * w.numel()) + 12 * b.numel()
    # attributes of the optimizer, not hyper-parameters of the groups: the state dict's groups are torch's
    ref = torch.optim.AdamW([w, b, small])
    assert set(opt.state_dict()["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0])
    assert "moments" not in opt.defaults and "min_8bit_size" not in opt.defaults
    opt.load_state_dict(ref.state_dict())
    assert opt.moments == "fp8"
    assert optim.AdamW([small], moments="fp8", min_8bit_size=0)._eligible8(small)
    # a later fp32 optimizer over the same parameters takes the tag away again
    optim.AdamW([w, b, small])
    assert not hasattr(w, "_omh_moment_bytes") and mt.pending_step_bytes(lin) == 12 * (w.numel() + b.numel())
