"""omh_rmsnorm_rope_bf16_pair_bound in its persistent form (csrc/dit_elementwise.hip: a grid of what the chip holds, every wave
walks rows first, first + grid_waves, ..., the per-(sample, head) maxima live in registers and are flushed at a sample
boundary and at the end of the walk) against its one-wave-per-row form (option RMS_PAIR_BOUND = "0") and against the plain
omh_rmsnorm_rope_bf16_pair, on the same inputs.  Every case asserts
  q and k            torch.equal across the three
  norm2_max          bit-equal between the two bound forms; in the integer-valued construction of norm_exact_ref (every sum
                     of squares exact in fp32) also equal to norm2_max() of the stored values
  repeatability      a second run of the persistent form into a fresh zeroed buffer gives the same bits
and that whatever lies behind the maxima stays as it was."""
import math

import pytest
import torch

import norm_exact_ref as R
from conftest import set_option

pytestmark = pytest.mark.gpu

D = 128
QS = float(torch.tensor(D ** -0.5 * math.log2(math.e), dtype=torch.float32))
WG_PER_CU = 4                  # csrc/dit_elementwise.hip: PAIR_BOUND_WG_PER_CU
GUARD = 7.0                    # behind the maxima: nothing may write there


def grid_waves():
    """Waves of a launch of the persistent form, restated from its launcher: PAIR_BOUND_WG_PER_CU workgroups of four waves
    on each CU (whole XCDs: omh_cu_count), whatever the row count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cus -= cus % 8
    return 4 * WG_PER_CU * (cus if cus >= 8 else 256)


def takes_persistent_form(dim, option):
    """True when omh_rmsnorm_rope_bf16_pair_bound runs the persistent kernel (RMS_PAIR_BOUND = option)"""
    return dim <= 6 * 256 and option != "0"


def _launch(ops, c, form):
    """One launch of `form` ("persistent" / "row": the bound entry under RMS_PAIR_BOUND unset / "0"; "plain": the pair entry in
    its one-wave-per-row form) on outputs pre-filled with a value no case produces.  -> (q, k, maxima or None, guard)"""
    dev = "cuda"
    q = torch.full((c.rows, c.dim), 3.0e38, dtype=torch.bfloat16, device=dev)
    k = torch.full((c.rows, c.dim), 3.0e38, dtype=torch.bfloat16, device=dev)
    p = ops.ptr
    args = (p(c.xd), 2 * c.dim, c.dim, p(q), p(k), c.rows, c.dim, p(c.wd[0]), p(c.wd[1]), c.eps, c.do_norm, p(c.cosd), p(c.sind),
            c.rope_len, D, p(c.gridd), c.seq_len)
    if form == "plain":
        set_option("RMS_PAIR_ROW", "1")
        ops.rmsnorm_rope_bf16_pair_raw(*args, out_scale0=c.scale[0], out_scale1=c.scale[1])
        set_option("RMS_PAIR_ROW", None)
        torch.cuda.synchronize()
        return q, k, None, None
    n = c.rows // c.seq_len * (c.dim // D) * 2
    buf = torch.cat([torch.zeros(n), torch.full((16,), GUARD)]).to(dev)
    set_option("RMS_PAIR_BOUND", "0" if form == "row" else None)
    ops.rmsnorm_rope_bf16_pair_bound_raw(*args, p(buf), out_scale0=c.scale[0], out_scale1=c.scale[1])
    set_option("RMS_PAIR_BOUND", None)
    torch.cuda.synchronize()
    return q, k, buf[:n].view(c.rows // c.seq_len, c.dim // D, 2), buf[n:]


def _to_device(c):
    c.xd = torch.cat([c.x[0].to(torch.bfloat16), c.x[1].to(torch.bfloat16)], 1).contiguous().cuda()
    c.wd = [w.float().cuda() for w in c.w]
    c.cosd, c.sind, c.gridd = c.cos.cuda(), c.sin.cuda(), c.grid.cuda()
    return c


def _three_ways(ops, c, ctx):
    """The assertions of the module docstring; returns (q, k, maxima) of the persistent form on the CPU."""
    qp, kp, _, _ = _launch(ops, c, "plain")
    qr, kr, nr, gr = _launch(ops, c, "row")
    qn, kn, nn, gn = _launch(ops, c, "persistent")
    _, _, n2, _ = _launch(ops, c, "persistent")
    for name, a, b in (("q row/plain", qr, qp), ("k row/plain", kr, kp), ("q persistent/plain", qn, qp), ("k persistent/plain", kn, kp)):
        diff = int((a.view(torch.int16) != b.view(torch.int16)).sum())
        assert diff == 0, f"{ctx} {name}: {diff} of {a.numel()} elements differ"
    assert bool((qn.float().abs() < 1.0e38).all()) and bool((kn.float().abs() < 1.0e38).all()), f"{ctx} rows left unwritten"
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(nn), bits(nr)), f"{ctx} maxima persistent / row:\n{nn.cpu()}\n{nr.cpu()}"
    assert torch.equal(bits(nn), bits(n2)), f"{ctx} maxima of a second run differ"
    assert bool((gn == GUARD).all()) and bool((gr == GUARD).all()), f"{ctx} wrote behind the maxima"
    nn = nn.cpu()
    if c.exact:
        want = torch.stack([R.norm2_max(c, y.cpu()) for y in (qn, kn)], -1)
        assert torch.equal(nn.double(), want.double()), f"{ctx} maxima against the stored values:\n{nn}\n{want}"
    return qn.cpu(), kn.cpu(), nn


def _exact_case(dim, seq_len, grids, seed, rope_len=5):
    return R.rms_case(dim, D, seq_len=seq_len, grids=grids, rope_len=rope_len, seed=seed, exact=True, nseg=2, xmax=3)


def _float_case(dim, seq_len, grids, seed, do_norm=1, scale=(QS, 1.0)):
    """N(0, 1) inputs, trained-like gains, a table of real rotations (norm_exact_ref's bounded mode) at the model's output scales"""
    c = R.rms_case(dim, D, seq_len=seq_len, grids=grids, rope_len=64, seed=seed, exact=False, nseg=2)
    c.do_norm, c.scale = do_norm, list(scale)
    return c


# ------------------------------------------------------------------ sample boundaries
@pytest.mark.parametrize("dim", [256, 1536])
@pytest.mark.parametrize("seq_len", [5, 7])
def test_sample_boundaries(ops, dim, seq_len):
    """Three samples of 5 or 7 rows: consecutive rows of a wave's walk (had it more than one) lie grid_waves apart, and here
    every sample boundary lies inside the first 21 rows.  Sample 0 is 8 x the others and nothing is normalised, so a maximum
    carried from sample 0 into another sample's slot is 64 x too large."""
    c = _float_case(dim, seq_len, ((1, 1, seq_len), (1, 2, 2), (1, 1, 3)), 11 + dim + seq_len, do_norm=0, scale=(1.0, 1.0))
    for s in range(2):
        c.x[s] = c.x[s].float()
        c.x[s][:seq_len] *= 8.0
        c.x[s] = c.x[s].to(torch.bfloat16)
    _, _, nm = _three_ways(ops, _to_device(c), f"boundaries dim={dim} seq_len={seq_len}:")
    assert float(nm[1:].max()) * 8.0 < float(nm[0].min()), f"a maximum of sample 0 in another sample's slot?\n{nm}"


@pytest.mark.parametrize("dim", [256, 1536])
def test_sample_boundaries_inside_a_walk(ops, dim):
    """The same hazard where a wave really has a second row, grid_waves behind its first and in another sample.  dim 256:
    five samples of grid_waves / 2 + 1 rows, every step of every walk crosses a boundary.  dim 1 536: samples of 5 rows,
    64 rows more than grid_waves.  Integer-valued; every third sample reaches |x| = 3 and the others 1, so neighbouring
    samples have different maxima."""
    gw = grid_waves()
    seq_len, B = (gw // 2 + 1, 5) if dim == 256 else (5, (gw + 64) // 5 + 1)
    grids = tuple((1, 1, 3) if b % 2 else (1, 1, seq_len) for b in range(B))
    c = _exact_case(dim, seq_len, grids, 31 + dim)
    for s in range(2):
        x = c.x[s].float().view(B, seq_len, dim)
        low = torch.arange(B) % 3 != 0
        x[low] = x[low].clamp(-1, 1)
        c.x[s] = x.view(B * seq_len, dim).to(torch.bfloat16)
    _three_ways(ops, _to_device(c), f"boundaries inside a walk dim={dim}:")


# ------------------------------------------------------------------ fewer rows than waves
@pytest.mark.parametrize("rows", [1, 3, "grid_waves-1"])
def test_fewer_rows_than_waves(ops, rows):
    """Waves without a row must leave the buffer as it was (and read nothing): one sample of `rows` rows."""
    rows = grid_waves() - 1 if rows == "grid_waves-1" else rows
    c = _exact_case(256, rows, ((1, 1, rows),), 50 + rows % 7)
    _three_ways(ops, _to_device(c), f"rows={rows} < waves:")


# ------------------------------------------------------------------ uneven walk
def _planted(c, row, hq, hk):
    """|x| <= 1 everywhere, gains one, and `row` holds (3, 0) pairs in head hq of q and head hk of k: with c^2 + s^2 in
    [1/2, 5/4] for every table entry a planted head sums to at least 64 * 9 / 2 scale^2 and any other to at most
    64 * 2 * 5/4 scale^2 — the row carries the launch maximum of exactly those two (head, segment) slots."""
    for s, h in ((0, hq), (1, hk)):
        x = c.x[s].float().clamp(-1, 1)
        x[row, h * D:(h + 1) * D] = torch.tensor([3.0, 0.0]).repeat(D // 2)
        c.x[s] = x.to(torch.bfloat16)
        c.w[s] = torch.ones_like(c.w[s])
    return c


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("k", [1, 2])
def test_uneven_walk(ops, k, where):
    """rows = k grid_waves + 1: one wave has a row more than the others; that row (or the first one) carries the maximum of
    head 1 of q and of head 0 of k."""
    rows = k * grid_waves() + 1
    row = rows - 1 if where == "last" else 0
    c = _planted(_exact_case(256, rows, ((1, 1, rows),), 70 + k), row, 1, 0)
    qn, kn, nm = _three_ways(ops, _to_device(c), f"rows={rows} planted row {row}:")
    for y, h, seg in ((qn, 1, 0), (kn, 0, 1)):
        sums = (y.double().view(rows, 2, D) ** 2).sum(-1)[:, h]
        assert int(sums.argmax()) == row and float(sums[row]) == float(nm[0, h, seg])
        assert float(sums[row]) > float(torch.cat([sums[:row], sums[row + 1:]]).max()), "the planted row must be the strict maximum"


# ------------------------------------------------------------------ head layout, pad tokens
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normed"])
@pytest.mark.parametrize("dim", [128, 256, 1408, 1536])
def test_head_layout_and_pad_tokens(ops, dim, exact):
    """1 head (the upper half-wave holds nothing), 2, 11 (the last vector half filled) and 12 heads; two samples of 13 rows
    with 12 and 10 tokens: the pad rows are not rotated and still count toward the maximum."""
    grids = ((2, 2, 3), (1, 2, 5))
    c = _exact_case(dim, 13, grids, 90 + dim) if exact else _float_case(dim, 13, grids, 90 + dim)
    if exact:                  # the pad rows of sample 1 carry its maxima (3 against at most 2 in the other rows)
        for s in range(2):
            x = c.x[s].float()
            x[13:23] = x[13:23].clamp(-2, 2)
            x[23:26] = 3.0
            c.x[s] = x.to(torch.bfloat16)
    qn, kn, nm = _three_ways(ops, _to_device(c), f"heads dim={dim} exact={exact}:")
    if exact:
        for y, seg in ((qn, 0), (kn, 1)):
            sums = (y.double().view(2, 13, dim // D, D) ** 2).sum(-1)[1]            # [13, heads] of sample 1
            assert bool((sums.argmax(0) >= 10).all()), "the construction puts sample 1's maxima in its pad rows"


# ------------------------------------------------------------------ bit drift at workload statistics
def test_no_bit_drift_at_workload_statistics(ops):
    """2 048 rows x 1 536, N(0, 1) inputs, gains 1 + 0.3 N(0, 1), out_scale0 = 128^-1/2 log2 e: 6.3 M stored elements (a
    drift at the 1e-5 rate once recorded for a shared body would move 60 of them)."""
    c = _float_case(1536, 2048, ((8, 16, 16),), 123)
    _three_ways(ops, _to_device(c), "2048 x 1536:")


# ------------------------------------------------------------------ wide instance
def test_wide_instance(ops):
    """dim 5 120, 64 rows: the one-wave-per-row form under either option value"""
    assert not takes_persistent_form(5120, None)
    c = _float_case(5120, 32, ((2, 3, 5), (1, 4, 8)), 321)
    _three_ways(ops, _to_device(c), "64 x 5120:")
