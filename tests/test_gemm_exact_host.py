"""The exact-integer GEMM tests can fail: a torch stand-in for omh_gemm_bf16 goes through the comparer and the canvas of
tests/gemm_exact_ref.py (the ones tests/test_gpu_gemm_exact.py holds the HIP kernels to) with seven defects planted one at
a time.  Each must be reported and the clean stand-in must pass.  Next to it, the written reason for the method: at
1560 x 1536 three of the defects pass ``rel_rms`` at the bounds the suite used so far.  No GPU."""
import pytest
import torch

import gemm_exact_ref as R
from conftest import rel_rms

BF16_BOUND = 4e-3            # tests/test_gpu_kernels.py, tests/test_gpu_train.py: rel_rms of a bf16 GEMM output against fp32 torch


def standin(c, pitch=None, defect=None):
    """What the entry leaves behind for case ``c``, computed by fp32 torch on the CPU into canvases; ``defect`` plants one
    of the bugs the exact tests are there to find.  Returns (C canvas, aux tensor or None)."""
    a, b = c.a.float(), c.b.float()
    acc = a @ b.t()                                                       # integer products: exact in any order
    M, N, K = c.M, c.N, c.K
    if defect == "k_tail_dropped_in_a_strip":                             # one wave's 64 x 64 strip loses the last 8 k
        acc[64:128, 128:192] -= a[64:128, K - 8:] @ b[128:192, K - 8:].t()
    if defect == "k_group_doubled_at_a_slice_boundary":                   # slice 1 starts 8 columns early in one tile
        k0 = K // 2
        acc[:128, :128] += a[:128, k0 - 8:k0] @ b[:128, k0 - 8:k0].t()
    lin = acc.clone()
    if c.bias is not None:
        by_n = (c.bias_mode == R.BIAS_N) != (defect == "bias_by_m_instead_of_n")
        lin = lin + (c.bias[None, :N] if by_n else c.bias[:M, None])
    if c.epilogue == R.EPI_RESID:
        g = torch.full((M, N), c.gate_const)
        if c.gate0 is not None:
            g = g + c.gate0[None, :]
        if c.gate1 is not None:
            rows = torch.arange(M)
            rows = (rows + 1 if defect == "gate_row_off_by_one" else rows) // c.gate_rows
            g = g + c.gate1[rows.clamp_max(c.gate1.shape[0] - 1), :N]
        val = c.c_old + lin * g
    elif c.epilogue == R.EPI_F32_ACCUM:
        val = c.c_old + lin
    else:
        val = lin
    if defect == "adjacent_columns_swapped_in_the_ragged_tile":           # the 4 rows one lane holds, last (ragged) m-tile
        r0 = (M - 1) // 256 * 256
        val[r0:r0 + 4, [8, 9]] = val[r0:r0 + 4, [9, 8]]
    if c.epilogue == R.EPI_BF16:
        val = R.truncate_bf16(val.double()) if defect == "truncation_on_the_bf16_store" else R.rne_bf16(val.double())
    cv = R.Canvas(M, N, pitch or N + 3, val.dtype, sentinel=float("nan")).arm()
    cv.window().copy_(val)
    if defect == "one_element_past_N":
        cv.buf[cv.start + 5 * cv.pitch + N] = 1.0
    aux = R.rne_bf16(lin.double()) if c.with_aux else None
    return cv, aux


def reports(c, cv, aux, tile=("small", 128, 128)):
    ref = R.reference(c)
    out = [R.mismatch_report(cv.window(), ref["C"], tile), cv.guard_report()]
    if "aux" in ref:
        out.append(R.mismatch_report(aux, ref["aux"], tile, what="aux"))
    return [m for m in out if m is not None]


CASES = {
    "k_tail_dropped_in_a_strip": dict(M=200, N=264, K=72, epilogue=R.EPI_F32),
    "k_group_doubled_at_a_slice_boundary": dict(M=136, N=200, K=256, epilogue=R.EPI_F32, bias_mode=R.BIAS_N),
    "adjacent_columns_swapped_in_the_ragged_tile": dict(M=261, N=40, K=64, epilogue=R.EPI_BF16),
    "one_element_past_N": dict(M=33, N=9, K=40, epilogue=R.EPI_F32_ACCUM),
    "bias_by_m_instead_of_n": dict(M=72, N=72, K=40, epilogue=R.EPI_F32, bias_mode=R.BIAS_N),
    "gate_row_off_by_one": dict(M=70, N=24, K=40, epilogue=R.EPI_RESID, bias_mode=R.BIAS_N, gate_rows=33, use_gate0=True,
                                with_aux=True),
    "truncation_on_the_bf16_store": dict(M=64, N=64, K=1024, epilogue=R.EPI_BF16),
}


@pytest.mark.parametrize("defect", sorted(CASES))
def test_a_planted_defect_is_reported_and_the_clean_stand_in_passes(defect):
    c = R.make_case(seed=11, **CASES[defect])
    assert reports(c, *standin(c)) == []
    found = reports(c, *standin(c, defect=defect))
    assert found, f"{defect} went unnoticed"
    print("[report]", defect, "->", found[0][:300])
    if defect == "one_element_past_N":
        assert "outside the [33, 9] window" in found[0] and "(row 5, col 9)" in found[0]
    else:
        assert "elements differ" in found[0] and "tile(s) of small 128 x 128" in found[0]
    if defect == "k_tail_dropped_in_a_strip":                             # the report names the tile: no debugger needed
        assert "tm 0, tn 1" in found[0] and "row 64, col 128" in found[0]
    if defect == "gate_row_off_by_one":                                   # rows 32 and 65: the last row before each boundary
        assert "row 32, col" in found[0]


@pytest.fixture(scope="module")
def production_shape():
    """1560 x 1536 (one training clip x dim), K = 2048, bf16 output, and its fp32 torch reference (computed once)."""
    c = R.make_case(1560, 1536, 2048, epilogue=R.EPI_BF16, seed=3)
    return c, c.a.float() @ c.b.float().t()


@pytest.mark.parametrize("defect,wrong", [("k_tail_dropped_in_a_strip", 64 * 64), ("adjacent_columns_swapped_in_the_ragged_tile", 8),
                                          ("truncation_on_the_bf16_store", None)])
def test_rel_rms_at_the_existing_bound_misses_what_the_exact_comparer_reports(production_shape, defect, wrong):
    """Why this file exists.  One norm over 1560 x 1536 outputs cannot see
      - a 64 x 64 strip that lost 8 of 2048 k terms: sqrt(64 * 64 * 8 / (1560 * 1536 * 2048)) = 2.6e-3 on top of the
        rounding's own share,
      - 8 elements swapped with their neighbours: sqrt(2 * 8 / (1560 * 1536)) = 2.6e-3,
      - truncation instead of RNE on the store (integers up to 256 are exact in bf16 either way),
    at the 4e-3 the suite allows a bf16 output; the per-element comparison reports every one of them."""
    c, ref32 = production_shape
    cv, _ = standin(c, pitch=c.N, defect=defect)
    err = rel_rms(cv.window().float(), ref32)
    clean = rel_rms(R.reference(c)["C"].float(), ref32)
    print(f"[measured] {defect}: rel_rms {err:.3e} (clean {clean:.3e}) against the bound {BF16_BOUND:.0e}")
    assert clean < err < BF16_BOUND
    found = reports(c, cv, None, tile=("big", 256, 256))
    assert found and "elements differ" in found[0]
    if wrong is not None:
        n = int(found[0].split(":")[1].split("of")[0])
        assert 0 < n <= wrong


def test_the_exactness_condition_at_the_largest_contraction():
    """9 K + 8 = 80 648 at K = 8960 before the gate; 9 (9 K + 8) + 128 = 725 960 half-units after gate and residual: both
    below 2^24.  The generator asserts it for every case, refuses a longer contraction, and the extreme operands (all
    +-3, bias +-8, gate 4.5, residual 64) really are exact in fp32."""
    assert R.check_exact(8960) == 80648
    assert R.check_exact(8960, gated=True, accumulates=True) == 80648
    assert int(2 * R.GATE_MAX * 80648) + 2 * R.C_MAX == 725960 < R.F32_EXACT
    with pytest.raises(AssertionError):
        R.check_exact(8968)
    assert 9 * ((R.F32_EXACT - 8) // 9 + 1) + 8 >= R.F32_EXACT              # ... and the first condition does bind eventually
    a = torch.full((1, 8960), 3.0)
    acc = torch.zeros(())
    for k in range(0, 8960, 8):                                           # sequential fp32 sums in 8-wide groups: still exact
        acc = acc + (a[0, k:k + 8] * 3.0).sum()
    lin = acc + 8.0
    assert float(lin) == 80648.0
    out = 64.0 + lin * torch.tensor(4.5)
    assert out.dtype == torch.float32 and float(out) == 64.0 + 80648.0 * 4.5
    c = R.make_case(8, 8, 8960, epilogue=R.EPI_RESID, bias_mode=R.BIAS_N, use_gate0=True, gate_rows=3, seed=1)
    assert R.reference(c)["C"].dtype == torch.float32
    g = R.make_case(8, 8, 8960, epilogue=R.EPI_GELU_BF16, bias_mode=R.BIAS_N, with_aux=True, seed=1)
    assert g.scale_exp == 9 and float(R.linear_part(g).abs().max()) < 8.0     # pre-activations of order 1, still exact
    assert R.reference(g)["aux"].dtype == torch.bfloat16


def test_rne_and_the_transcendental_bound():
    x = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 1.0, 0.0], dtype=torch.float64)
    assert R.rne_bf16(x).tolist() == [256.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0, 1.0, 0.0]      # ties to even
    assert torch.equal(R.rne_bf16(x), x.float().to(torch.bfloat16))
    assert R.truncate_bf16(x).tolist() == [256.0, 256.0, 258.0, 258.0, 260.0, -256.0, -258.0, 1.0, 0.0]
    assert R.ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6,
                                                                                                2.0 ** -8, 2.0 ** -133]
    # a correctly rounded bf16 GELU of an fp32-accurate value sits inside the bound; a one-ulp-off neighbour plus more does not
    x = torch.linspace(-6, 6, 4001, dtype=torch.float64)
    ref = R.gelu_tanh64(x)
    good = ref.float().to(torch.bfloat16)
    worst, msg = R.bound_report(good[None], ref[None], x.abs()[None])
    assert msg is None and worst <= 0.5 + 1e-9
    bad = (ref + 2.5 * R.bound_of(ref, x.abs())).float().to(torch.bfloat16)
    worst, msg = R.bound_report(bad[None], ref[None], x.abs()[None])
    assert msg is not None and worst > 1.0
    nan = good.clone()
    nan[7] = float("nan")
    assert R.bound_report(nan[None], ref[None], x.abs()[None])[1] is not None
    # the derivative's reference against autograd of the formula
    xg = x.clone().requires_grad_(True)
    R.gelu_tanh64(xg).sum().backward()
    assert float((xg.grad - R.gelu_tanh_grad64(x)).abs().max()) < 1e-14


def test_canvas_guards_and_hostile_pads():
    cv = R.Canvas(5, 7, 9, torch.float32, lead=1, trail=3, sentinel=-7.0, offset_bytes=4)
    assert cv.ptr % 16 == 4 and cv.ptr % 4 == 0
    cv.put(torch.ones(5, 7)).arm()
    assert cv.guard_report() is None
    cv.window()[2, 3] = 5.0                                               # inside: not the guard's business
    assert cv.guard_report() is None
    cv.buf[cv.start + 2 * 9 + 7] = 0.0                                    # a pad column
    assert "(row 2, col 7)" in cv.guard_report()
    op = R.Canvas(3, 8, 16, torch.bfloat16, trail=128).put(torch.ones(3, 8)).arm()      # an operand: NaN all round
    assert op.ptr % 16 == 0 and bool(torch.isnan(op.buf[~op.inside]).all()) and int(op.inside.sum()) == 24
    assert op.buf.numel() >= (3 + 128) * 16
    bt = R.Canvas(4, 8, 8, torch.float32, blocks=3, block_stride=44, sentinel=float("nan")).arm()
    assert tuple(bt.window().shape) == (3, 4, 8) and int(bt.inside.sum()) == 96
    bt.window()[1].fill_(2.0)
    assert bt.guard_report() is None
    bt.buf[bt.start + 44 + 32] = 1.0                                      # between two batch blocks
    assert bt.guard_report() is not None
