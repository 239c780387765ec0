"""ops.rope_shift_frames (omh_rope_shift_frames) per element: the frame pairs of every head against the rule in fp64, every
other column and every byte around the destination against the source's bits — over widths of one, two and twelve heads,
row counts below, at and far above a workgroup's 32 rows of 128 columns, one and two batch entries with the destination a
row range of a larger canary-filled tensor (its own batch stride), in place and out of place, delta from 0 to 10^6.

Bound of a rotated element: |err| <= 2^-8 |y| + 2^-20 hypot(x0, x1) — one rounding to bf16 (half an ulp of 8 significant
bits: at most 2^-8 |y|) plus the fp32 slack of two products, a sum and cos / sin rounded to fp32.  An angle formed as an
fp32 product leaves it on 18 % of the elements at delta = 10^6 (tests/test_pinned_sink_host.py)."""
import importlib

import pytest
import torch

import pinned_sink_ref as PR
from conftest import PKG

pytestmark = pytest.mark.gpu
DELTAS = (0, 1, 3, 1000, 10 ** 6)
CANARY = 0x5A5A                                                                  # int16 bits around the destination


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("rows", (1, 3, 56, 1000))
@pytest.mark.parametrize("dim", (128, 256, 1536))
def test_rope_shift_frames(ops, dim, rows):
    g = torch.Generator().manual_seed(1000 * dim + rows)
    for B in (1, 2):
        src_cpu = torch.randn(B, rows, dim, generator=g).to(torch.bfloat16)
        cap = rows + 5
        for delta in DELTAS:
            y, rotated, hyp = PR.shift_exact(src_cpu, delta)
            bound = 2.0 ** -8 * y.abs() + 2.0 ** -20 * hyp
            results = []
            for in_place in (False, True):
                big = torch.full((B, cap, dim), CANARY, dtype=torch.int16, device="cuda").view(torch.bfloat16)
                dst = big[:, 2:2 + rows]
                if in_place:
                    dst.copy_(src_cpu)
                    src = dst
                else:                                                            # the source in a tensor of another pitch
                    src = torch.zeros(B, rows + 3, dim, dtype=torch.bfloat16, device="cuda")[:, 1:1 + rows]
                    src.copy_(src_cpu)
                out = ops.rope_shift_frames(src, dst, delta)
                assert out is dst
                got = dst.cpu()
                err = (got.double() - y).abs()
                worst = float((err - bound)[rotated].max())
                assert bool((err <= bound)[rotated].all()), (B, delta, in_place, worst)
                assert torch.equal(_bits(got)[~rotated], _bits(src_cpu)[~rotated]), (B, delta, in_place)
                edge = _bits(big.cpu())
                assert bool((edge[:, :2] == CANARY).all()) and bool((edge[:, 2 + rows:] == CANARY).all()), (B, delta, in_place)
                if not in_place:
                    assert torch.equal(_bits(src.cpu()), _bits(src_cpu))         # the source is read only
                if delta == 0:
                    assert torch.equal(_bits(got), _bits(src_cpu))
                results.append(got)
            assert torch.equal(_bits(results[0]), _bits(results[1]))             # in place and out of place: the same bits
            again = ops.rope_shift_frames(src_cpu.cuda(), None, delta)            # a fresh destination; a repeated run
            assert torch.equal(_bits(again.cpu()), _bits(results[0]))


def test_rope_shift_continues_the_forward_rotation(ops):
    """Sign, pair layout and frequencies are those of the project's own norm + RoPE kernel: rows it rotates at frame f and
    this entry shifts by delta lie within two roundings, (2^-7 + 2^-20) hypot(x0, x1), of the fp64 rotation at f + delta."""
    model = importlib.import_module(PKG + ".wan.modules.model")
    D, dim, F = 128, 256, 20
    nf = (D - 4 * (D // 6)) // 2
    freqs = torch.cat([model.rope_params(1024, D - 4 * (D // 6)), model.rope_params(1024, 2 * (D // 6)),
                       model.rope_params(1024, 2 * (D // 6))], dim=1)
    cos, sin = (t.to(torch.float32).contiguous().cuda() for t in (freqs.real, freqs.imag))
    x = torch.randn(F, dim, generator=torch.Generator().manual_seed(9))
    grid = torch.tensor([[F, 1, 1]], dtype=torch.int32, device="cuda")             # token r is frame r at h = w = 0
    k = ops.rmsnorm_rope(x.cuda(), None, 1e-6, do_norm=False, rope_cos=cos, rope_sin=sin, head_dim=D, grid=grid, seq_len=F)
    n = D - 4 * (D // 6)
    inv = 1.0 / torch.pow(torch.tensor(10000.0, dtype=torch.float64), torch.arange(0, n, 2, dtype=torch.float64) / n)
    xp = x.double().view(F, dim // D, D // 2, 2)
    hyp = torch.hypot(xp[..., :nf, 0], xp[..., :nf, 1])
    for delta in (0, 7, 1000):
        got = ops.rope_shift_frames(k.view(1, F, dim), None, delta).cpu().double().view(F, dim // D, D // 2, 2)
        ang = torch.outer(torch.arange(F, dtype=torch.float64) + delta, inv).view(F, 1, nf)
        ref0 = xp[..., :nf, 0] * torch.cos(ang) - xp[..., :nf, 1] * torch.sin(ang)
        ref1 = xp[..., :nf, 0] * torch.sin(ang) + xp[..., :nf, 1] * torch.cos(ang)
        bound = (2.0 ** -7 + 2.0 ** -20) * hyp
        e0, e1 = (got[..., :nf, 0] - ref0).abs(), (got[..., :nf, 1] - ref1).abs()
        print(f"delta {delta}: worst error / bound {float(torch.maximum(e0, e1).div(bound).max()):.3f}")
        assert bool((e0 <= bound).all()) and bool((e1 <= bound).all()), delta
        # the h / w pairs sit at position 0: the forward kernel's rounding of x, which the shift leaves alone
        assert torch.equal(got[..., nf:, :], x.to(torch.bfloat16).double().view(F, dim // D, D // 2, 2)[..., nf:, :])


def test_rope_shift_refusals(ops):
    x = torch.zeros(2, 8, 256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ops.OmhError):                                            # partly overlapping rows
        ops.rope_shift_frames(x[:, :6], x[:, 2:8], 1)
    with pytest.raises(ops.OmhError):                                            # a width that is no multiple of 128
        ops.rope_shift_frames(torch.zeros(1, 8, 192, dtype=torch.bfloat16, device="cuda"), None, 1)
    with pytest.raises(ops.OmhError):                                            # heads that do not tile the width
        ops.rope_shift_frames(x, None, 1, head_dim=96)
    with pytest.raises(AssertionError):
        ops.rope_shift_frames(x.float(), None, 1)
