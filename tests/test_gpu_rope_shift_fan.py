"""ops.rope_shift_fan and ops.rope_shift_fold (omh_rope_shift_fan / omh_rope_shift_fold) per element — the fan-out of the
sink keys in front of the attention of teacher forcing under a pinned sink, and the fold behind its backward.

Fan-out: every image against ops.rope_shift_frames of the same source and delta, bit for bit; source and images are row
ranges of ONE canary-filled buffer with its own pitches (the model's layout: the images behind the rows of the sequence), and
every byte around them keeps its canary.  Against the stated arithmetic on the CPU (pinned_sink_ref.shift_emulated), bit
for bit as well, in a test of its own.

Fold: against the fp64 sum of the exactly rotated images.  Bound per element, with image 0 the base rows at delta = 0:

    |err| <= 2^-8 |y| + 2^-19 sum_c hypot(x0_c, x1_c)

— one rounding to bf16 (at most 2^-8 |y|), and in fp32 per image the 2^-20 hypot tests/test_gpu_rope_shift.py grants a
rotation plus one addition to a partial sum that is at most sum_c hypot: 16 additions of 2^-24 each are another 2^-20 of it.
A bf16 rounding of the partial sums leaves it (shown on the CPU below), which is what the bound is there to catch."""
import importlib

import pytest
import torch

import pinned_sink_ref as PR
from conftest import PKG

DELTAS = (1, 3, 1000, 10 ** 6, 0)
CANARY = 0x5A5A                                                                  # int16 bits around the destination
SHAPES = ((1, 16), (2, 3), (2, 1))                                               # (B, copies)


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _deltas(copies):
    return [DELTAS[c % len(DELTAS)] for c in range(copies)]


def _layout(B, rows, dim, copies):
    """One buffer [B, cap, dim]: the base / source rows at [1, 1 + rows), image c at [rows + 3 + c (rows + 1), . + rows) — a
    canary row between any two of them.  Returns (cap, the as_strided arguments of the images)."""
    cap = rows + 3 + copies * (rows + 1) + 2
    return cap, ((B, copies, rows, dim), (cap * dim, (rows + 1) * dim, dim, 1), (rows + 3) * dim)


def _exact_fold(base, images, deltas):
    """(y fp64, sum_c hypot) of base + sum_c R(-delta_c) images[:, c]; ``deltas`` None: the plain sum."""
    y, _, hyp = PR.shift_exact(base, 0)
    y, hyp = y.clone(), hyp.clone()
    for c in range(images.shape[1]):
        yc, _, hc = PR.shift_exact(images[:, c].contiguous(), 0 if deltas is None else -deltas[c])
        y += yc
        hyp += hc
    return y, hyp


@pytest.mark.gpu
@pytest.mark.parametrize("B,copies", SHAPES)
@pytest.mark.parametrize("rows", (1, 56, 1000))
@pytest.mark.parametrize("dim", (128, 256, 1536))
def test_rope_shift_fan(ops, dim, rows, B, copies):
    g = torch.Generator().manual_seed(1000 * dim + 10 * rows + copies)
    src_cpu = torch.randn(B, rows, dim, generator=g).to(torch.bfloat16)
    deltas = _deltas(copies)
    cap, view = _layout(B, rows, dim, copies)
    want = torch.full((B, cap, dim), CANARY, dtype=torch.int16).view(torch.bfloat16)
    want[:, 1:1 + rows] = src_cpu
    big = want.cuda()
    single = {d: ops.rope_shift_frames(src_cpu.cuda(), None, d).cpu() for d in set(deltas)}
    for c, d in enumerate(deltas):                                               # the bits the pinned cache holds at rollout
        torch.as_strided(want, *view)[:, c] = single[d]
    assert torch.equal(_bits(single.get(0, src_cpu)), _bits(src_cpu))
    table = ops.rope_shift_table(deltas, device="cuda")
    dst = torch.as_strided(big, *view)
    assert ops.rope_shift_fan(big[:, 1:1 + rows], dst, table) is dst
    got = big.cpu()
    for c, d in enumerate(deltas):
        assert torch.equal(_bits(torch.as_strided(got, *view)[:, c]), _bits(single[d])), (c, d)
    assert torch.equal(_bits(got), _bits(want))                                  # source, images and every canary around them
    ops.rope_shift_fan(big[:, 1:1 + rows], dst, table)                           # a repeated run
    assert torch.equal(_bits(big.cpu()), _bits(want))
    fresh = torch.empty(B, copies, rows, dim, dtype=torch.bfloat16, device="cuda")   # a destination of its own
    ops.rope_shift_fan(src_cpu.cuda(), fresh, table)
    assert torch.equal(_bits(fresh.cpu()), _bits(torch.as_strided(want, *view)))


@pytest.mark.gpu
@pytest.mark.parametrize("B,copies", SHAPES)
@pytest.mark.parametrize("rows", (1, 56, 1000))
@pytest.mark.parametrize("dim", (128, 256, 1536))
def test_rope_shift_fan_against_the_emulation(ops, dim, rows, B, copies):
    """Every image against pinned_sink_ref.shift_emulated, bit for bit, and within the bound of tests/test_gpu_rope_shift.py.
    (rotate_pair spells its fp32 arithmetic out for this: left to the compiler's contraction of ``x0 c - x1 s``, about one
    rotated element in 10^5 came out one bf16 ulp apart — 12 of 1 056 000 at dim 1 536, 1 000 rows, B 2, delta 1 000 —
    from ops.rope_shift_frames and the fan-out alike.)"""
    g = torch.Generator().manual_seed(1000 * dim + 10 * rows + copies)
    src_cpu = torch.randn(B, rows, dim, generator=g).to(torch.bfloat16)
    deltas = _deltas(copies)
    got = ops.rope_shift_fan(src_cpu.cuda(), torch.empty(B, copies, rows, dim, dtype=torch.bfloat16, device="cuda"),
                             ops.rope_shift_table(deltas, device="cuda")).cpu()
    differ = 0
    for d in sorted(set(deltas)):
        c = deltas.index(d)
        y, rotated, hyp = PR.shift_exact(src_cpu, d)
        err = (got[:, c].double() - y).abs()
        assert bool((err <= 2.0 ** -8 * y.abs() + 2.0 ** -20 * hyp)[rotated].all()), d
        n = int((_bits(got[:, c]) != _bits(PR.shift_emulated(src_cpu, None, d))).sum())
        print(f"dim {dim} rows {rows} B {B} delta {d}: {n} of {int(rotated.sum())} rotated elements differ from shift_emulated")
        differ += n
    assert differ == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,copies", SHAPES)
@pytest.mark.parametrize("rows", (1, 56, 1000))
@pytest.mark.parametrize("dim", (128, 256, 1536))
def test_rope_shift_fold(ops, dim, rows, B, copies):
    g = torch.Generator().manual_seed(7 + 1000 * dim + 10 * rows + copies)
    deltas = _deltas(copies)
    cap, view = _layout(B, rows, dim, copies)
    buf_cpu = torch.randn(B, cap, dim, generator=g).to(torch.bfloat16)
    base_cpu, img_cpu = buf_cpu[:, 1:1 + rows].contiguous(), torch.as_strided(buf_cpu, *view).contiguous()
    table = ops.rope_shift_table(deltas, device="cuda")
    for tab, dl in ((table, deltas), (None, None)):
        y, hyp = _exact_fold(base_cpu, img_cpu, dl)
        bound = 2.0 ** -8 * y.abs() + 2.0 ** -19 * hyp
        results = []
        for in_place in (False, True):
            buf = buf_cpu.cuda()
            base, images = buf[:, 1:1 + rows], torch.as_strided(buf, *view)
            if in_place:
                out, dst = buf, base
            else:
                out = torch.full((B, rows + 5, dim), CANARY, dtype=torch.int16, device="cuda").view(torch.bfloat16)
                dst = out[:, 2:2 + rows]
            assert ops.rope_shift_fold((base, images), dst, tab) is dst
            got = dst.cpu()
            err = (got.double() - y).abs()
            worst = float((err / bound.clamp_min(1e-300)).max())
            assert bool((err <= bound).all()), (tab is None, in_place, worst)
            edge = _bits(out.cpu())
            if in_place:                                                         # nothing but the base rows has changed
                keep = torch.ones(B, cap, dtype=torch.bool)
                keep[:, 1:1 + rows] = False
                assert torch.equal(edge[keep], _bits(buf_cpu)[keep])
            else:
                assert bool((edge[:, :2] == CANARY).all()) and bool((edge[:, 2 + rows:] == CANARY).all())
                assert torch.equal(_bits(buf.cpu()), _bits(buf_cpu))             # the operands are read only
            results.append(got)
        assert torch.equal(_bits(results[0]), _bits(results[1]))                 # in place and out of place: the same bits
        again = ops.rope_shift_fold((base_cpu.cuda(), img_cpu.cuda()), None, tab)    # fresh operands; a repeated run
        assert torch.equal(_bits(again.cpu()), _bits(results[0]))


@pytest.mark.gpu
def test_fold_of_one_image_at_delta_0_keeps_the_bits(ops):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 56, 256, generator=g).to(torch.bfloat16)
    zero = torch.zeros_like(x)
    assert not bool((x == 0).any())
    for tab in (ops.rope_shift_table([0], device="cuda"), None):
        got = ops.rope_shift_fold((zero.cuda(), x.cuda()[:, None]), None, tab)
        assert torch.equal(_bits(got.cpu()), _bits(x))
        got = ops.rope_shift_fold((x.cuda(), zero.cuda()[:, None]), None, tab)
        assert torch.equal(_bits(got.cpu()), _bits(x))


@pytest.mark.gpu
def test_fold_on_column_blocks(ops):
    """The model's layout: dK | dV side by side in one scratch buffer [B, Lk, 2 dim] (the images behind the rows of the
    sequence), the sums written into the dk and dv thirds of the sink rows of [B, S, 3 dim]."""
    B, S, sr, copies, dim = 2, 40, 8, 3, 256
    Lk = S + copies * sr
    g = torch.Generator().manual_seed(31)
    dkv_cpu = torch.randn(B, Lk, 2 * dim, generator=g).to(torch.bfloat16)
    deltas = [2, 4, 6]
    table = ops.rope_shift_table(deltas, device="cuda")
    dkv = dkv_cpu.cuda()
    out = torch.full((B, S, 3 * dim), CANARY, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    image = lambda t, c0: torch.as_strided(t, (B, copies, sr, dim), (Lk * 2 * dim, sr * 2 * dim, 2 * dim, 1), S * 2 * dim + c0)
    ops.rope_shift_fold((dkv[:, :sr, :dim], image(dkv, 0)), out[:, :sr, dim:2 * dim], table)
    ops.rope_shift_fold((dkv[:, :sr, dim:], image(dkv, dim)), out[:, :sr, 2 * dim:], None)
    got = out.cpu()
    for c0, dl in ((0, deltas), (dim, None)):
        y, hyp = _exact_fold(dkv_cpu[:, :sr, c0:c0 + dim].contiguous(), image(dkv_cpu, c0).contiguous(), dl)
        err = (got[:, :sr, dim + c0:2 * dim + c0].double() - y).abs()
        assert bool((err <= 2.0 ** -8 * y.abs() + 2.0 ** -19 * hyp).all()), c0
    edge = _bits(got)
    assert bool((edge[:, :, :dim] == CANARY).all()) and bool((edge[:, sr:] == CANARY).all())
    assert torch.equal(_bits(dkv.cpu()), _bits(dkv_cpu))


def test_bf16_partial_sums_leave_the_bound():
    """On the CPU: the same fold with every partial sum rounded to bf16 (what an accumulation in the gradient's own format
    would do) breaks the bound of test_rope_shift_fold on a good part of the elements; the fp32 sum of the kernel's stated
    arithmetic keeps it."""
    g = torch.Generator().manual_seed(13)
    copies = 16
    deltas = _deltas(copies)
    base = torch.randn(2, 56, 256, generator=g).to(torch.bfloat16)
    images = torch.randn(2, copies, 56, 256, generator=g).to(torch.bfloat16)
    y, hyp = _exact_fold(base, images, deltas)
    bound = 2.0 ** -8 * y.abs() + 2.0 ** -19 * hyp
    acc16, acc32 = base.clone(), base.float()
    for c in range(copies):
        yc = PR.shift_exact(images[:, c].contiguous(), -deltas[c])[0]
        acc16 = (acc16.double() + yc).to(torch.bfloat16)
        acc32 = (acc32.double() + yc.float().double()).float()                   # (a rotated image and a sum, each rounded to fp32)
    frac16 = float(((acc16.double() - y).abs() > bound).double().mean())
    frac32 = float(((acc32.to(torch.bfloat16).double() - y).abs() > bound).double().mean())
    print(f"bf16 partial sums: {100 * frac16:.1f} % of the elements leave the bound; fp32 sums: {100 * frac32:.1f} %")
    assert frac16 > 0.05 and frac32 == 0.0


@pytest.mark.gpu
def test_refusals(ops):
    x = torch.zeros(2, 24, 256, dtype=torch.bfloat16, device="cuda")
    tab = ops.rope_shift_table([1, 2], device="cuda")
    images = lambda t, r0, rows: torch.as_strided(t, (2, 2, rows, 256), (24 * 256, rows * 256, 256, 1), r0 * 256)
    ops.rope_shift_fan(x[:, :8], images(x, 8, 8), tab)                           # rows [0, 8) -> [8, 16), [16, 24) per entry
    with pytest.raises(ops.OmhError):                                            # the first image meets the source rows
        ops.rope_shift_fan(x[:, :8], images(x, 6, 8), tab)
    with pytest.raises(ops.OmhError):                                            # a width that is no multiple of 128
        y = torch.zeros(1, 8, 192, dtype=torch.bfloat16, device="cuda")
        ops.rope_shift_fan(y, y.new_zeros(1, 2, 8, 192), tab)
    with pytest.raises(ops.OmhError):                                            # heads that do not tile the width
        ops.rope_shift_fan(x[:, :8], images(x, 8, 8), tab, head_dim=96)
    with pytest.raises(AssertionError):                                          # one table row per copy
        ops.rope_shift_fan(x[:, :8], images(x, 8, 8), tab[:1])
    with pytest.raises(AssertionError):
        ops.rope_shift_fan(x[:, :8].float(), images(x, 8, 8), tab)
    with pytest.raises(ops.OmhError):                                            # copies < 1
        ops.rope_shift_fan(x[:, :8], x.new_zeros(2, 0, 8, 256), tab[:0])
    with pytest.raises(ops.OmhError):                                            # dst meets the images
        ops.rope_shift_fold((x[:, :8], images(x, 8, 8)), x[:, 4:12], tab)
    with pytest.raises(ops.OmhError):                                            # dst meets the base rows without being them
        ops.rope_shift_fold((x[:, 1:5], images(x, 16, 4)), x[:, :4], None)
    with pytest.raises(AssertionError):
        ops.rope_shift_fold((x[:, :8], images(x, 8, 8)), None, tab[:1])
