"""References, cases, bounds and planted defects for the index, reduction and step kernels of the DiT side
(include/omh.h: omh_transpose_bf16, omh_colsum_accum[_multi], omh_cast_f32_bf16, omh_patchify, omh_unpatchify[_bwd],
omh_softmax_bwd_rows, the four GELU entries, omh_dense_f32[_bwd], omh_sinusoidal_embedding[_bwd], omh_cfg_unipc_step,
omh_flow_x0_step).  Test infrastructure, not a test module; plain torch, importable without a GPU.  Canvases, RNE to
bf16, ulp_bf16, ``compare`` and the WORST / COUNTS bookkeeping (printed per file, filtered by its entries) are those of tests/norm_exact_ref.py.

Every reference is written from the formula in omh.h, in float64 (``dt`` = float32 gives the restatement of the kernel's
arithmetic that tests/test_aux_exact_host.py holds against the bounds), and takes a ``defect`` out of DEFECTS.

A. Exact outputs.  ``compare_bits`` on the bit pattern: -0 is not +0, and where the reference is a NaN any NaN passes.
  moves and roundings  transpose, patchify, unpatchify, unpatchify_bwd, cast: bf16 payloads are random finite 16-bit
                       patterns, fp32 payloads random finite 32-bit patterns with SPECIAL_F32 planted (RNE ties under an
                       even and an odd upper half, 0x7f7fffff -> inf, subnormals, -0, +-inf, NaNs).  An output element
                       that a defect leaves unwritten keeps the canvas' NaN.
  column sums          |x| <= 8 integers, out pre-filled with |o| <= 1000 integers, R <= 4100: every partial sum is an
                       integer of magnitude <= 1000 + 8 R <= 33 800 < 2^24, whatever the order of the atomics.
  softmax_bwd_rows     p = k / 16 (k = 0 .. 16), dp integers |dp| <= 8, L <= 1000, scale a power of two: products are
                       multiples of 1/16, the row sum delta <= 8 L = 128 000 sixteenths; (dp - delta) is a multiple of
                       1/16 of magnitude <= 8 + 8 L, its product with p a multiple of 1/256 of magnitude <= 8 008, that
                       is 2 050 048 units < 2^24; the scale moves the exponent.  One RNE on both sides.
  dense, act 0         x, W, bias, dy integers |.| <= 4, K <= 300, N <= 130, B <= 3, accumulators pre-filled with
                       integers |.| <= 64: |y| <= 16 K + 4, |dW| <= 64 + 16 B, |db| <= 64 + 4 B, |dx| <= 64 + 16 N.
  cfg_unipc_step       tensors integers |.| <= 8, guide, sigma and the seven coefficients multiples of 1/2 with
                       |.| <= 4: v = u + g (c - u) a multiple of 1/2, |v| <= 72; m_t = x - sigma v a multiple of 1/4,
                       <= 296; x_c a multiple of 1/8, <= 4 (8 + 8 + 8 + 296) = 1 280; x_next a multiple of 1/16,
                       <= 4 (1 280 + 296 + 8) = 6 336 < 2^14: 101 376 sixteenths.  No operation rounds, so a fused
                       multiply-add gives the bits of the separate operations.
  flow_x0_step         random fp32; the reference is the expression of omh.h op by op in torch fp32 on the CPU (each op
                       rounds once, as the entry promises).

B. Bounded outputs: |got - ref| <= 0.5 ulp_bf16(|ref| + delta) + delta for bf16, delta (+ 0.5 ulp_f32 where the output
is ONE rounding of an fp64 value) for fp32.  S is the formula with every factor in absolute value and every subtraction
turned into an addition; eps = 2^-24.  For the GELU entries the derivations below give D, the first-order worst case of
the kernel's arithmetic; delta = MARGIN D with MARGIN = 4, the factor the project's k rule leaves between a measured
error and its bound, so that "the fp32 restatement stays below delta / 4" says: the restatement stays below D.
  GELU-tanh forward   y = x s, s = 1 / (1 + 2^t), t = -2 c log2(e) x (1 + a x^2).  t carries N_T = 7 roundings (x^2,
                       the fma and the x^2 it inherits, k x, the product, and two for the constant k evaluated in fp32),
                       so |dt| <= 7 eps |t|: the relative error of 2^t is 7 ln 2 eps |t| < 5 eps |t| plus 2 eps for
                       v_exp_f32 (1 ulp).  With q = 2^t / (1 + 2^t) = 1 - s the share of 2^t in the denominator:
                         r_s = (3 + q (2 + 5 |t|)) eps          (1 + 2^t rounds once, v_rcp_f32 is 1 ulp = 2 eps)
                       D = (r_s + 2 eps) S,  S = |x| s.  In the deep negative tail q = 1 and |t| reaches 128:
                       D / S = 645 eps = 2^-14.7, which the project's 2^-16 S does not cover.  The flush: a v_rcp_f32
                       result below the smallest normal number 2^-126 comes back as 0, and 2^t overflows at t = 128
                       where the true s is 2^-128.  That can happen only for t > T_FLUSH = 125 (s < 2^-125; one unit
                       of room for the error of t); there, and only there, the whole of S is added to delta (the
                       result may be lost entirely; it is below 2^-125 |x|).  Every GELU delta also carries SUBN = 2^-146: a product with a
                       tiny dy or x is rounded to fp32's subnormal grid (spacing 2^-149, half of it per rounding, two
                       such roundings, times MARGIN), not relatively; 2^-13 of the smallest bf16 step.
  GELU-tanh backward   dx = dy (s + P s (1 - s)), P = x 2c (1 + 3 a x^2); S = |dy| (s + |P| s (1 - s)).  1 - s is a
                       subtraction of two fp32 values: its absolute error is a = r_s s (+ eps (1 - s)), which P s
                       multiplies.  For t < -26 the sum 1 + 2^t is 1.0f, s = rcp(1.0f) must be exactly 1 and the
                       computed 1 - s exactly 0: there a = 1 - s itself (< 2^-26, vanishing like 2^t), not 3 eps —
                       with 3 eps the bound would grow like |P| and hold nothing for x above 20.
                         D = |dy| ((r_s + 9 eps) S + |P| s a)
                       (9: five roundings of P, s (1 - s), the fma, the product with dy, the rounding of 1 - s).
                       The flush as in the forward: S is added for t > T_FLUSH alone (there S < 2^-116 |dy|).  No term
                       of delta is absolute in |P|: for |x| up to the domain's edge delta stays below 2^-9 |dy|.
                       Domain: P overflows fp32 for |x| > 1.17e13 where s (1 - s) is exactly 0; the entry returns NaN
                       there (``tanh_grad_nan_set``), and include/omh.h says so.
  GELU-erf forward     y = 0.5 z (1 + erf(z / sqrt 2)), S = 0.5 |z| (1 + |erf|).  z / sqrt 2 carries 1.5 roundings: erf
                       moves by at most 0.484 of that (max of u erf'(u)); erff is taken as U_ERF = 4 ulp of a value
                       below 1, the sum rounds once below 2: |d(1 + erf)| <= (0.73 + 4 + 1) eps <= 6 eps (1 + |erf|);
                       two products: D = 8 eps S.
  GELU-erf backward    dx = dy (0.5 (1 + erf) + z phi0 exp(-z^2 / 2)); T2 = |z| phi0 exp(-z^2 / 2).  The argument of
                       exp carries 2 roundings (relative error of exp: eps z^2), expf is 1 ulp, z phi0 1.5, the
                       products and the sum one each: D = |dy| (9 eps S + eps z^2 T2).  expf gives a result below
                       2^-126 (which may come back as 0) only for z^2 / 2 > Z_FLUSH = 86: there, and only there, the
                       whole of |dy| T2 is added (below 2^-121 |dy|); beyond z^2 / 2 = 104 it vanishes by itself.
  dense with SiLU      delta = k eps S with k from K_AUX: four times the worst ratio of the fp32 restatement (lane sums
                       k = lane, lane + 64, ... then wave_sum's butterfly) to eps S, rounded up to a power of two.
                       S of y: S1 D + |y| with S1 = sum |silu x| |W| + |bias|, D = sigma + |z| sigma (1 - sigma) the
                       magnitude of silu'.
  sinusoid forward     0.5 ulp_f32(ref) + 2^-40 for |t| <= 1000.  The exponent -k / half is the same IEEE quotient on
                       both sides; pow within 2 ulp on each side and the product's rounding leave the fp64 angle
                       (<= 1000 < 2^10) off by at most 2^10 (2 + 2 + 1/2) 2^-53 < 2^-40.6; cos and sin have slope <= 1
                       and err by about 2^-52 themselves: below 2^-40 before the ONE rounding to fp32.
  sinusoid backward    0.5 ulp_f32(ref) + 2^-40 S, S = sum_k w_k (|cos| |g1| + |sin| |g0|): an fp64 sum of at most 513
                       terms in a fixed order (513 2^-53 S) and the angle errors above, which a term near a zero of cos
                       passes to the other half of the same k.
  column sums, randn   deterministic mode: two runs give equal bits, each sum within R eps S (R additions: one of them may
                       use the whole of its own eps S, so the restatement is held to a quarter from R = 8 on).
  cfg_unipc_step       coefficients of a real schedule: n_r eps S with n_r the count of roundings on the longest path of
                       the uncontracted expression: m_t 5 (three of v, sigma v, the difference), x_c 12 (m_t's five,
                       four products, three sums), x_next 15 (x_c's twelve, its product, two sums).  A worst case: the
                       fp32 restatement reaches 0.62 of it (m_t at guide 5), so the host test holds the restatement
                       to the bound itself, not to a quarter of it."""
import math
from types import SimpleNamespace as NS

import torch

from norm_exact_ref import (Canvas, rne_bf16, truncate_bf16, ulp_bf16, compare, ratio_to_bound,  # noqa: F401
                            bad_fraction, WORST, COUNTS, _gen, _ints, _randn, _up)
from gemm_exact_ref import exact_f32

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS24 = 2.0 ** -24
F32_EXACT = 1 << 24
T_FLUSH, Z_FLUSH = 125.0, 86.0                              # where v_rcp_f32 / expf may flush a result below 2^-126 to 0
SUBN = 2.0 ** -146                                          # MARGIN x two roundings to fp32's subnormal grid (spacing 2^-149)
U_ERF = 4.0
MARGIN = 4.0                                                # delta = MARGIN x the derived first-order error D of a GELU entry
# measured by tests/test_aux_exact_host.py (restatement / (eps S), worst over the cases): y 1.236, dW 3.345, db 1.603,
# dx 3.081; times four, rounded up to a power of two
K_AUX = {"dense_y": 8.0, "dense_dW": 16.0, "dense_db": 8.0, "dense_dx": 16.0}
N_R = {"mt": 5.0, "xc": 12.0, "xn": 15.0}

DEFECTS = ("transpose_drop_partial_group", "colsum_drop_block_last_row", "colsum_chunk_edge", "patchify_swap_i_j",
           "unpatchify_swap_a_i", "patchify_pad_nonzero", "cast_truncates", "softmax_sum_over_pitch", "dense_bias_after_act",
           "dense_db_times_K", "sinusoid_halves_swapped", "unipc_cond_uncond_swapped", "unipc_m1_dropped_without_m2",
           "flow_one_sigma_per_vector", "gelu_grad_without_s")

NAN = float("nan")


def check_exact(kind, **kw):
    """Assert the exactness condition of the module docstring for one case; returns the largest partial sum in units."""
    if kind == "colsum":
        assert kw["R"] <= 4100
        top = 1000 + 8 * kw["R"]
    elif kind == "softmax":
        assert kw["L"] <= 1000 and math.log2(kw["scale"]) % 1 == 0
        top = 256 * (8 + 8 * kw["L"])                       # (dp - delta) p in units of 1/256, p <= 1
        assert 16 * 8 * kw["L"] < F32_EXACT
    elif kind == "dense":
        assert kw["K"] <= 300 and kw["N"] <= 130 and kw["B"] <= 3
        top = max(16 * kw["K"] + 4, 64 + 16 * kw["B"], 64 + 16 * kw["N"])
    elif kind == "unipc":
        v = 8 + 4 * (8 + 8)                                 # |v|, a multiple of 1/2
        mt = 8 + 4 * v                                      # a multiple of 1/4
        xc = 4 * (8 + 8 + 8 + mt)                           # a multiple of 1/8
        top = 16 * 4 * (xc + mt + 8)                        # x_next in sixteenths
        assert (v, mt, xc, top) == (72, 296, 1280, 101376) and top / 16 < 2 ** 14
    else:
        raise ValueError(kind)
    assert top < F32_EXACT, f"{kind}: the largest partial sum can reach {top} units >= 2^24"
    return top


# ----------------------------------------------------------------------------------------------------------------------
# payloads, bits
# ----------------------------------------------------------------------------------------------------------------------
# RNE ties under an even and an odd upper half (both signs), the largest finite value (rounds to inf), subnormals (the
# smallest, a tie at the bottom of bf16's subnormals, an odd one, the largest), -0, +-inf, a quiet and a signalling NaN
# whose upper half alone is inf, the all-ones NaN
SPECIAL_F32 = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00008000, 0x00018000,
               0x807FFFFF, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF)


def _i16(u):
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)


def _i32(u):
    return torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32)


def bf16_patterns(g, shape):
    """random finite 16-bit patterns: a swap of any two elements changes bits"""
    u = torch.randint(0, 1 << 16, shape, generator=g, dtype=torch.int64)
    u = torch.where((u & 0x7F80) == 0x7F80, u ^ 0x0080, u)
    return _i16(u).view(BF16)


def all_bf16_patterns():
    return _i16(torch.arange(1 << 16, dtype=torch.int64)).view(BF16)


def f32_patterns(g, shape, special=True):
    """random finite 32-bit patterns; ``special``: SPECIAL_F32 planted at random places (as many as fit)"""
    n = int(torch.tensor(shape).prod()) if len(shape) else 1
    u = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    u = torch.where((u & 0x7F800000) == 0x7F800000, u ^ 0x00800000, u)
    if special:
        k = min(n, len(SPECIAL_F32))
        u[torch.randperm(n, generator=g)[:k]] = torch.tensor(SPECIAL_F32[:k], dtype=torch.int64)
    return _i32(u).view(F32).reshape(shape)


def as_bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def rne_any(x, defect=None):
    """fp32 -> bf16 by RNE; a NaN gives a NaN (rne_bf16 takes the rest: +-inf and subnormals are exact in float64)"""
    nan = torch.isnan(x)
    fin = torch.where(nan, torch.zeros_like(x), x).double()
    out = truncate_bf16(fin) if defect == "cast_truncates" else rne_bf16(fin)
    return torch.where(nan, torch.full_like(out, NAN), out)


def compare_bits(entry, what, got, want, context="", record=True):
    """``compare`` on the bit patterns; where ``want`` is a NaN, ``got`` must be a NaN (of any payload)"""
    got = got.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"[{entry}] {context} {what}: got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    nan = torch.isnan(want)
    if bool(nan.any()):
        bad = nan & ~torch.isnan(got)
        if bool(bad.any()):
            return f"[{entry}] {context} {what}: {int(bad.sum())} elements must be NaN and are not; first at flat index {int(bad.flatten().nonzero()[0])}"
        got = torch.where(nan, want, got)
    return compare(entry, what, as_bits(got), as_bits(want), None, context, record)


def ulp_f32(x):
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 23.0)


def bound_bf16(ref, delta):
    return 0.5 * ulp_bf16(ref.abs() + delta) + delta


# ----------------------------------------------------------------------------------------------------------------------
# transpose
# ----------------------------------------------------------------------------------------------------------------------
TR_SIZES = (1, 3, 4, 63, 64, 65, 67, 130)
TR_SCALAR = ("odd_ld_in", "odd_ld_out", "offset")


def transpose_cases():
    """dict(R, C, batch, scalar, seed): the sizes crosswise, the four named shapes; ``scalar`` names how the scalar route is
    forced on the same data"""
    pairs = list(zip(TR_SIZES, reversed(TR_SIZES))) + [(TR_SIZES[i], TR_SIZES[(i + 3) % 8]) for i in range(8)]
    pairs += [(67, 5), (5, 67), (64, 64), (65, 130)]
    return [dict(R=r, C=c, batch=3 if i % 3 == 0 else 1, scalar=TR_SCALAR[i % 3], seed=i)
            for i, (r, c) in enumerate(dict.fromkeys(pairs))]


def transpose_geometry(cs, route):
    """pitches (ld_out > R: a pad), batch strides larger than a matrix, the byte offset of both pointers"""
    g = NS(ld_in=_up(cs["C"], 4) + 4, ld_out=_up(cs["R"], 4) + 4, off=0)
    if route == "odd_ld_in":
        g.ld_in += 1
    elif route == "odd_ld_out":
        g.ld_out += 1
    elif route == "offset":
        g.off = 2
    else:
        assert route == "vec"
    g.bs_in, g.bs_out = cs["R"] * g.ld_in + 8, cs["C"] * g.ld_out + 12
    return g


def transpose_takes_vec(ld_in, ld_out, bs_in, bs_out, p_in, p_out):
    """omh_transpose_bf16's choice, restated from csrc/dit_backward.hip"""
    return not ((ld_in | ld_out | bs_in | bs_out) & 3) and not ((p_in | p_out) & 7)


def transpose_input(cs):
    return bf16_patterns(_gen(11, cs["seed"], cs["R"], cs["C"]), (cs["batch"], cs["R"], cs["C"]))


def transpose_ref(x, defect=None):
    out = x.transpose(-1, -2).clone(memory_format=torch.contiguous_format)
    R = x.shape[-2]
    if defect == "transpose_drop_partial_group" and R % 4:
        out[..., R - R % 4:] = NAN
    return out


# ----------------------------------------------------------------------------------------------------------------------
# column sums
# ----------------------------------------------------------------------------------------------------------------------
def colsum_single_cases():
    cs, rs = (1, 255, 256, 257, 600), (1, 31, 32, 33, 65)
    out = []
    for i in range(5):
        for r in (rs[i], rs[(i + 2) % 5]):
            for bf in (0, 1):
                out.append(dict(R=r, C=cs[i], ld=cs[i] + (3 if bf else 8), bf16=bf, off=0, seed=len(out)))
    return out


def colsum_multi_cases():
    """name -> entries dict(R, C, ld, bf16, off, seed[, wide]); ``off``: elements the pointer is moved off its 16-byte
    boundary; ``wide`` = (columns of the shared matrix, first column): a column block of one wide matrix"""
    cv, rv = (8, 248, 256, 264), (1, 7, 8, 9, 127, 128, 129, 300)

    def ent(i, R, C, ld=None, bf16=None, off=0, wide=None):
        return dict(R=R, C=C, ld=ld or _up(C, 8) + 8, bf16=(i // 2) % 2 if bf16 is None else bf16, off=off, seed=100 + i, wide=wide)

    sixteen = [ent(i, rv[i % 8], cv[(i + i // 8) % 4]) for i in range(16)]
    return {
        "n1": [ent(20, 300, 264)],
        "n2_one_block_beside_six": [ent(21, 1, 8, bf16=1), ent(22, 300, 264, bf16=0)],
        "n16_mixed": sixteen,
        "n17_two_launches": sixteen + [ent(23, 129, 248, bf16=1)],
        "column_blocks_of_a_wide_matrix": [ent(24 + j, 129, c, ld=784, bf16=1, wide=(776, c0))
                                           for j, (c0, c) in enumerate(((0, 256), (256, 264), (520, 248), (768, 8)))],
        "scalar_by_C": [ent(30, 33, 257, ld=264), ent(31, 128, 256)],
        "scalar_by_odd_ld": [ent(32, 9, 8, ld=13), ent(33, 65, 264)],
        "scalar_by_pointer": [ent(34, 127, 248, bf16=1, off=1), ent(35, 8, 8)],
    }


def colsum_multi_takes_vec(entries, ptrs):
    """omh_colsum_accum_multi's choice for ONE launch, restated from csrc/dit_backward.hip"""
    return all(e["C"] % 8 == 0 and e["ld"] % 8 == 0 and p % 16 == 0 for e, p in zip(entries, ptrs))


def colsum_data(e, exact=True):
    """(x [R, C] or, for a column block, the whole wide matrix; out0 [C])"""
    g = _gen(13, e["seed"], e["R"], e["C"], exact)
    cols = e["wide"][0] if e.get("wide") else e["C"]
    if e.get("wide"):
        g = _gen(13, 999, e["R"], cols, exact)              # the blocks of one matrix share its data
    if exact:
        check_exact("colsum", R=e["R"])
        x = _ints(g, (e["R"], cols), 8)
    else:
        x = _randn(g, (e["R"], cols))
    x = x.to(BF16 if e["bf16"] else F32)
    g2 = _gen(14, e["seed"], exact)
    out0 = (_ints(g2, (e["C"],), 1000) if exact else _randn(g2, (e["C"],))).float()
    return x, out0


def colsum_block(e, x):
    return x[:, e["wide"][1]:e["wide"][1] + e["C"]] if e.get("wide") else x


def colsum_ref(x, out0, dt=F64, defect=None, rpb=32):
    """out0 + column sums of x [R, C] and the condition sum; fp32: the rows in sequential order"""
    xs = x.to(dt)
    if defect == "colsum_drop_block_last_row" and xs.shape[0] >= rpb:
        xs = torch.cat([xs[:rpb - 1], xs[rpb:]])
    if dt == F64:
        s = xs.sum(0)
    else:
        s = torch.zeros(xs.shape[1], dtype=dt)
        for r in range(xs.shape[0]):
            s = s + xs[r]
    out = out0.to(dt) + s
    if defect == "colsum_chunk_edge":
        out[255::256] = out0.to(dt)[255::256]
    return NS(out=out, S=out0.double().abs() + x.double().abs().sum(0))


# ----------------------------------------------------------------------------------------------------------------------
# cast, patchify, unpatchify and its adjoint
# ----------------------------------------------------------------------------------------------------------------------
CAST_N = (1, 3, 4, 5, 1027, 8388608 + 3)
PATCHES = ((1, 2, 2), (2, 2, 2), (1, 1, 1), (2, 3, 1))
GRID_V = (1, 2, 3, 5)


def _patch_cases(channels, big_grid):
    """dict(C, patch, grid (f, h, w), pad, seed); the last one crosses the grid cap of its kernel"""
    out = []
    for p in PATCHES:
        for c in channels:
            i = len(out)
            out.append(dict(C=c, patch=p, grid=(GRID_V[i % 4], GRID_V[(i // 2 + 1) % 4], GRID_V[(3 * i + 2) % 4]), pad=24 * (i % 2), seed=i))
    out.append(dict(C=16, patch=(1, 2, 2), grid=big_grid, pad=0, seed=90))
    return out


def patchify_cases():
    return _patch_cases((1, 16, 36), (3, 105, 105))         # 33 075 tokens x 64 columns = 2 116 800 > 8192 x 256


def unpatchify_cases():
    return _patch_cases((1, 16), (3, 105, 105))             # 16 x 3 x 210 x 210 = 2 116 800 > 8192 x 256


def unpatchify_bwd_cases():
    return _patch_cases((1, 16), (6, 105, 105))             # 4 233 600 > 16384 x 256


def patch_dims(cs):
    (pt, ph, pw), (f, h, w) = cs["patch"], cs["grid"]
    return NS(pt=pt, ph=ph, pw=pw, f=f, h=h, w=w, F=f * pt, H=h * ph, W=w * pw, tokens=f * h * w, valid=cs["C"] * pt * ph * pw,
              Kp=cs["C"] * pt * ph * pw + cs["pad"])


def patchify_ref(x, cs, defect=None):
    """x fp32 [C, F, H, W] -> bf16 [tokens, Kp]: column (c pt + a) ph pw + i pw + j = x[c, f pt + a, h ph + i, w pw + j]"""
    d = patch_dims(cs)
    v = x.reshape(cs["C"], d.f, d.pt, d.h, d.ph, d.w, d.pw)
    order = (1, 3, 5, 0, 2, 6, 4) if defect == "patchify_swap_i_j" else (1, 3, 5, 0, 2, 4, 6)
    tok = torch.zeros((d.tokens, d.Kp), dtype=F32)
    tok[:, :d.valid] = v.permute(*order).reshape(d.tokens, d.valid)
    out = rne_any(tok)
    if defect == "patchify_pad_nonzero":
        out[:, d.valid:] = NAN
    return out


def unpatchify_ref(tok, cs, defect=None):
    """tok [tokens, pt ph pw C] -> [C, F, H, W]: out[c, f pt + a, h ph + i, w pw + j] = tok[(f, h, w), ((a ph + i) pw + j) C + c]"""
    d = patch_dims(cs)
    if defect == "unpatchify_swap_a_i":
        return tok.reshape(d.f, d.h, d.w, d.ph, d.pt, d.pw, cs["C"]).permute(6, 0, 4, 1, 3, 2, 5).reshape(cs["C"], d.F, d.H, d.W)
    return tok.reshape(d.f, d.h, d.w, d.pt, d.ph, d.pw, cs["C"]).permute(6, 0, 3, 1, 4, 2, 5).reshape(cs["C"], d.F, d.H, d.W)


def unpatchify_bwd_ref(g, cs):
    """the adjoint: g [C, F, H, W] fp32 -> bf16 [tokens, pt ph pw C]"""
    d = patch_dims(cs)
    v = g.reshape(cs["C"], d.f, d.pt, d.h, d.ph, d.w, d.pw).permute(1, 3, 5, 2, 4, 6, 0)
    return rne_any(v.reshape(d.tokens, d.valid).contiguous())


# ----------------------------------------------------------------------------------------------------------------------
# softmax backward
# ----------------------------------------------------------------------------------------------------------------------
def softmax_cases():
    return [dict(L=L, R=R, scale=(1.0, 0.25)[(i + j) % 2], seed=10 * i + j)
            for i, L in enumerate((1, 63, 64, 255, 256, 257, 1000)) for j, R in enumerate((1, 5))]


def softmax_data(cs):
    g = _gen(17, cs["seed"], cs["L"], cs["R"])
    check_exact("softmax", L=cs["L"], scale=cs["scale"])
    p = (torch.randint(0, 17, (cs["R"], cs["L"]), generator=g).double() / 16.0).to(BF16)
    return p, _ints(g, (cs["R"], cs["L"]), 8).float()


def softmax_bwd_ref(p, dp, scale, defect=None):
    """dS = P (dP - sum_j P dP) scale before its rounding; the defect adds the pad columns (NaN) to the row sum"""
    pd, dd = p.double(), dp.double()
    delta = (pd * dd).sum(-1, keepdim=True)
    if defect == "softmax_sum_over_pitch":
        delta = delta + NAN
    return pd * (dd - delta) * scale


# ----------------------------------------------------------------------------------------------------------------------
# GELU
# ----------------------------------------------------------------------------------------------------------------------
C_T, A_T = 0.7978845608028654, 0.044715
K_T = -2.0 * C_T * 1.4426950408889634
PHI0 = 0.3989422804014327
RSQRT2 = 0.7071067811865476


def _tanh_parts(x, dt):
    """t, s = 1 / (1 + 2^t), q = 1 - s, P — float64: q from 2^t s, which keeps its digits where s rounds to 1"""
    if dt == F32:
        x2 = x * x
        t = (torch.tensor(K_T, dtype=F32) * x) * (torch.tensor(A_T, dtype=F32) * x2 + 1.0)
        s = 1.0 / (1.0 + torch.exp2(t))
        p = (x * torch.tensor(2.0 * C_T, dtype=F32)) * (torch.tensor(3.0 * A_T, dtype=F32) * x2 + 1.0)
        return t, s, 1.0 - s, p
    x2 = x * x
    t = K_T * x * (A_T * x2 + 1.0)
    e = torch.exp2(t)
    s = 1.0 / (1.0 + e)
    q = torch.where(torch.isinf(e), torch.ones_like(e), e * s)
    return t, s, q, x * (2.0 * C_T) * (3.0 * A_T * x2 + 1.0)


def _r_s(t, q):
    return (3.0 + q * (2.0 + 5.0 * t.abs().clamp_max(2000.0))) * EPS24


def gelu_tanh_fwd(x, dt=F64):
    """x: the exact bf16 values as ``dt``; returns (y before its rounding, delta)"""
    t, s, q, _ = _tanh_parts(x, dt)
    if dt == F32:
        return x * s, None
    S = x.abs() * s
    return x * s, MARGIN * (_r_s(t, q) + 2.0 * EPS24) * S + torch.where(t > T_FLUSH, S, torch.zeros_like(S)) + SUBN


def gelu_tanh_bwd(dy, x, dt=F64, defect=None):
    t, s, q, p = _tanh_parts(x, dt)
    g = p * (s * q) if defect == "gelu_grad_without_s" else s + p * (s * q)
    if dt == F32:
        return dy * g, None
    S = s + p.abs() * s * q
    rs = _r_s(t, q)
    a = torch.where(t < -26.0, q, s * rs)                   # the error of the computed 1 - s: all of it where s is exactly 1.0f
    flush = torch.where(t > T_FLUSH, S, torch.zeros_like(S))
    return dy * g, dy.abs() * (MARGIN * ((rs + 9.0 * EPS24) * S + p.abs() * s * a) + flush) + SUBN


def tanh_grad_nan_set(x32):
    """the finite patterns at which the fp32 restatement of the tanh gradient is a NaN: P overflows and s (1 - s) = 0"""
    g, _ = gelu_tanh_bwd(torch.ones_like(x32), x32, F32)
    return torch.isnan(g) & torch.isfinite(x32)


def tanh_grad_nan_count():
    """the count that follows from the threshold: finite bf16 values whose P = x 2c (1 + 3 a x^2), evaluated in float64,
    reaches the fp32 overflow threshold 2^128 (1 - 2^-25), both signs"""
    x = all_bf16_patterns()[:0x7F80].double()               # the non-negative finite values, ascending
    p = x * (2.0 * C_T) * (3.0 * A_T * x * x + 1.0)
    return 2 * int((p >= 2.0 ** 128 * (1.0 - 2.0 ** -25)).sum())


def gelu_erf_fwd(z, dt=F64):
    if dt == F32:
        return 0.5 * z * (1.0 + torch.erf(z * torch.tensor(RSQRT2, dtype=F32))), None
    one_plus = torch.special.erfc(-z * RSQRT2)              # 1 + erf, with its digits in the negative tail
    S = 0.5 * z.abs() * (1.0 + torch.erf(z * RSQRT2).abs())
    return 0.5 * z * one_plus, MARGIN * (U_ERF + 4.0) * EPS24 * S + SUBN


def gelu_erf_bwd(dy, z, dt=F64):
    if dt == F32:
        g = 0.5 * (1.0 + torch.erf(z * torch.tensor(RSQRT2, dtype=F32))) + (z * torch.tensor(PHI0, dtype=F32)) * torch.exp((-0.5 * z) * z)
        return dy * g, None
    t2 = z * PHI0 * torch.exp(-0.5 * z * z)
    g = 0.5 * torch.special.erfc(-z * RSQRT2) + t2
    S = 0.5 * (1.0 + torch.erf(z * RSQRT2).abs()) + t2.abs()
    zz = (z * z).clamp_max(1e6)                             # beyond, T2 is 0 in float64
    flush = torch.where(0.5 * z * z > Z_FLUSH, t2.abs(), torch.zeros_like(t2))
    return dy * g, dy.abs() * (MARGIN * ((U_ERF + 5.0) * EPS24 * S + EPS24 * zz * t2.abs()) + flush) + SUBN


def gelu_classes(kind, x, ref):
    """masks over the patterns for the separate worst figures: results below fp32's normal range (bf16's smallest
    subnormals, where RNE's own tie uses the half ulp), the flush range (tanh: t > T_FLUSH; erf: z^2 / 2 > Z_FLUSH), the
    tail (tanh: |t| > 26, where 1 + 2^t or its reciprocal is 1.0f; erf: z^2 / 2 > 18, the same 2^-26) and the normal
    range, which is the rest"""
    if kind == "tanh":
        t = _tanh_parts(x, F64)[0]
        far, flush = t.abs() > 26.0, t > T_FLUSH
    else:
        far, flush = 0.5 * x * x > 18.0, 0.5 * x * x > Z_FLUSH
    sub = (ref.abs() < 2.0 ** -126) & ~flush
    return {"subnormal": sub, "flush": flush, "tail": far & ~sub & ~flush, "normal": ~far & ~sub & ~flush}


def delta_used(got, ref, delta):
    """the worst (|got - ref| - 0.5 ulp_bf16(|ref| + delta)) / delta, floor 0: what a bf16 result needs of its delta once
    the half ulp of its one rounding is taken off — the ratio to the whole bound is close to 1 for any rounded value"""
    over = (got.double() - ref).abs() - 0.5 * ulp_bf16(ref.abs() + delta)
    return float((over / delta.clamp_min(2.0 ** -300)).clamp_min(0.0).max()) if ref.numel() else 0.0


GELU_DY = ("one", "minus_one", "half", "random")


def gelu_dy(kind):
    if kind == "random":                                    # finite patterns below 2^127: dy gelu' (|gelu'| < 1.13) stays finite
        u = as_bits(bf16_patterns(_gen(19), (1 << 16,))).to(torch.int64) & 0xFFFF
        return _i16(torch.where((u & 0x7F80) == 0x7F00, u ^ 0x4000, u)).view(BF16)
    return torch.full((1 << 16,), {"one": 1.0, "minus_one": -1.0, "half": 0.5}[kind], dtype=BF16)


# ----------------------------------------------------------------------------------------------------------------------
# the tiny dense layer
# ----------------------------------------------------------------------------------------------------------------------
def dense_fwd_cases():
    """dict(B, N, K, bias, act_in, act_out, seed): exact for act 0 / 0, bounded otherwise"""
    out = []
    for i, K in enumerate((1, 63, 64, 65, 300)):
        for j, N in enumerate((1, 5, 70)):
            a = (i + j) % 4
            out.append(dict(B=(1, 3)[(i + j) % 2], N=N, K=K, bias=(i + 2 * j) % 3 != 0, act_in=a & 1, act_out=a >> 1, seed=10 * i + j))
    for a in range(4):                                      # the four combinations at one shape, with and without a bias
        out.append(dict(B=3, N=70, K=300, bias=a % 2 == 0, act_in=a & 1, act_out=a >> 1, seed=80 + a))
    return out


def dense_bwd_cases():
    """dict(B, N, K, act_in, want ('dW' / 'dx' / 'both'), db, acc, seed)"""
    out = []
    for i, N in enumerate((1, 63, 64, 65, 130)):
        for j, K in enumerate((1, 65, 300)):
            out.append(dict(B=(1, 3)[(i + j) % 2], N=N, K=K, act_in=(i + j) % 2, want=("both", "dW", "dx")[(i + 2 * j) % 3],
                            db=(i + j) % 3 != 0, acc=(i + j) % 2, seed=10 * i + j))
    out.append(dict(B=3, N=130, K=300, act_in=0, want="both", db=True, acc=0, seed=70))
    out.append(dict(B=3, N=130, K=300, act_in=1, want="both", db=True, acc=1, seed=71))
    return out


def dense_data(cs, backward=False):
    exact = not (cs["act_in"] or cs.get("act_out"))
    g = _gen(23, cs["seed"], cs["B"], cs["N"], cs["K"], backward)
    B, N, K = cs["B"], cs["N"], cs["K"]
    if exact:
        check_exact("dense", B=B, N=N, K=K)
    mk = (lambda shape, hi=4: _ints(g, shape, hi).float()) if exact else (lambda shape, hi=4: _randn(g, shape).float())
    c = NS(x=mk((B, K)), W=mk((N, K)) if exact else (mk((N, K)) / math.sqrt(K)), bias=mk((N,)), exact=exact)
    if backward:
        c.dy, c.dW0, c.db0, c.dx0 = mk((B, N)), mk((N, K), 64), mk((N,), 64), mk((B, K), 64)
    return c


def wave_strided_sum(t):
    """[..., K] -> [...]: fp32 in dense_f32_kernel's order — lane l adds k = l, l + 64, ..., then wave_sum's butterfly"""
    if t.dtype == F64:
        return t.sum(-1)
    K = t.shape[-1]
    v = torch.zeros(t.shape[:-1] + (_up(K, 64),), dtype=t.dtype)
    v[..., :K] = t
    lanes = torch.zeros(t.shape[:-1] + (64,), dtype=t.dtype)
    for chunk in v.reshape(t.shape[:-1] + (-1, 64)).unbind(-2):
        lanes = lanes + chunk
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., lane ^ o]
    return lanes[..., 0]


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _seq_sum(t, dim):
    """sum along ``dim``; fp32 in index order"""
    if t.dtype == F64:
        return t.sum(dim)
    s = torch.zeros_like(t.select(dim, 0))
    for u in t.unbind(dim):
        s = s + u
    return s


def dense_fwd_ref(c, cs, dt=F64, defect=None):
    x, W = c.x.to(dt), c.W.to(dt)
    a = _silu(x) if cs["act_in"] else x
    z = wave_strided_sum(a[:, None, :] * W[None])
    s1 = (a.abs()[:, None, :] * W.abs()[None]).sum(-1)
    late = defect == "dense_bias_after_act" and cs["bias"]
    if cs["bias"] and not late:
        z, s1 = z + c.bias.to(dt), s1 + c.bias.to(dt).abs()
    if not cs["act_out"]:
        return NS(y=z + c.bias.to(dt) if late else z, S=s1)
    sg = 1.0 / (1.0 + torch.exp(-z))
    y = z * sg
    return NS(y=y + c.bias.to(dt) if late else y, S=s1 * (sg + z.abs() * sg * (1.0 - sg)) + y.abs())


def dense_bwd_ref(c, cs, dt=F64, defect=None):
    """dW, db (from their starts), dx (from dx0 when cs['acc']) and their condition sums"""
    x, W, dy = c.x.to(dt), c.W.to(dt), c.dy.to(dt)
    a = _silu(x) if cs["act_in"] else x
    o = NS()
    o.dW = c.dW0.to(dt) + _seq_sum(dy[:, :, None] * a[:, None, :], 0)
    o.S_dW = c.dW0.to(dt).abs() + (dy.abs()[:, :, None] * a.abs()[:, None, :]).sum(0)
    o.db = c.db0.to(dt) + _seq_sum(dy, 0) * (cs["K"] if defect == "dense_db_times_K" else 1)
    o.S_db = c.db0.to(dt).abs() + dy.abs().sum(0)
    s = _seq_sum(dy[:, :, None] * W[None], 1)
    sa = (dy.abs()[:, :, None] * W.abs()[None]).sum(1)
    if cs["act_in"]:
        sg = 1.0 / (1.0 + torch.exp(-x))
        s, sa = s * (sg * (1.0 + x * (1.0 - sg))), sa * (sg * (1.0 + x.abs() * (1.0 - sg)))
    start = c.dx0.to(dt) if cs["acc"] else torch.zeros_like(s)
    o.dx, o.S_dx = start + s, start.abs() + sa
    return o


# ----------------------------------------------------------------------------------------------------------------------
# sinusoidal embedding
# ----------------------------------------------------------------------------------------------------------------------
SIN_T = (0.0, 0.5, 1.0, 999.0, 1000.0, 637.318)


def sinusoid_cases():
    return [dict(B=B, dim=dim, first=i + j, seed=10 * i + j) for i, dim in enumerate((2, 254, 256, 258, 1026)) for j, B in enumerate((1, 4))] + \
           [dict(B=4, dim=258, first=4, seed=77)]


def sinusoid_t(cs):
    return torch.tensor([SIN_T[(cs["first"] + b) % len(SIN_T)] for b in range(cs["B"])], dtype=F32)


def _angles(t, dim):
    half = dim // 2
    w = torch.pow(torch.tensor(10000.0, dtype=F64), -torch.arange(half, dtype=F64) / half)
    return t.double()[:, None] * w[None], w


def sinusoid_fwd_ref(t, dim, defect=None):
    """float64 [B, dim]: cos | sin; bound 0.5 ulp_f32(ref) + 2^-40"""
    assert float(t.abs().max()) <= 1000.0
    ang, _ = _angles(t, dim)
    a, b = torch.cos(ang), torch.sin(ang)
    ref = torch.cat([b, a] if defect == "sinusoid_halves_swapped" else [a, b], 1)
    return ref, 0.5 * ulp_f32(ref) + 2.0 ** -40


def sinusoid_bwd_ref(dsin, t, defect=None):
    dim = dsin.shape[1]
    half = dim // 2
    ang, w = _angles(t, dim)
    g0, g1 = dsin.double()[:, :half], dsin.double()[:, half:]
    if defect == "sinusoid_halves_swapped":
        g0, g1 = g1, g0
    ref = (w * (torch.cos(ang) * g1 - torch.sin(ang) * g0)).sum(1)
    S = (w * (torch.cos(ang).abs() * g1.abs() + torch.sin(ang).abs() * g0.abs())).sum(1)
    return ref, 0.5 * ulp_f32(ref) + 2.0 ** -40 * S


# ----------------------------------------------------------------------------------------------------------------------
# CFG + UniPC step
# ----------------------------------------------------------------------------------------------------------------------
UNIPC_N = (1, 255, 256, 257)
UNIPC_BIG = 2097152 + 5


def unipc_cases():
    """dict(n, use_corr, m1, m2, outs, last, alias, off, seed): every combination of use_corr x m1 x m2 x (mt_out, xc_out),
    the sizes by turns; then the aliases, the 4-byte offset and the size above the grid cap"""
    out = []
    for k in range(16):
        uc, m1, m2, outs = k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1
        out.append(dict(n=UNIPC_N[(k + k // 4) % 4], use_corr=uc, m1=m1, m2=m2, outs=outs, last=bool(uc) or k % 4 == 2, alias=None, off=0, seed=k))
    out.append(dict(n=257, use_corr=1, m1=1, m2=1, outs=1, last=True, alias="xc_is_last", off=0, seed=20))
    out.append(dict(n=257, use_corr=1, m1=1, m2=0, outs=1, last=True, alias="xnext_is_x", off=0, seed=21))
    out.append(dict(n=255, use_corr=0, m1=1, m2=1, outs=1, last=False, alias="xnext_is_x", off=0, seed=22))
    out.append(dict(n=257, use_corr=1, m1=1, m2=1, outs=1, last=True, alias=None, off=4, seed=23))
    out.append(dict(n=UNIPC_BIG, use_corr=1, m1=1, m2=1, outs=1, last=True, alias=None, off=0, seed=24))
    return out


def unipc_data(cs, exact=True, coef=None):
    """tensors and scalars of one call.  exact: integers and multiples of 1/2; else randn and ``coef`` =
    (sigma, (ca_last, ca_m1, ca_m2, ca_mt) or None, (pb_x, pb_mt, pb_m1)) of a real schedule, guide 5"""
    g = _gen(29, cs["seed"], cs["n"], exact)
    n = cs["n"]
    mk = (lambda: _ints(g, (n,), 8).float()) if exact else (lambda: _randn(g, (n,)).float())
    c = NS(cond=mk(), uncond=mk(), x=mk(), last=mk() if cs["last"] else None, m1=mk() if cs["m1"] else None, m2=mk() if cs["m2"] else None)
    if exact:
        check_exact("unipc")
        h = [0.5 * float(v) for v in torch.randint(-8, 9, (9,), generator=g)]
        h = [v if v else 1.5 for v in h]                    # a zero coefficient would hide its term
        c.guide, c.sigma, c.ca, c.pb = h[0], h[1], h[2:6], h[6:9]
    else:
        c.guide, c.sigma = 5.0, coef[0]
        c.ca, c.pb = list(coef[1] or (0.0, 0.0, 0.0, 0.0)), list(coef[2])
    if not cs["m1"]:                                        # omh.h: a tensor may be NULL when its coefficient is 0
        c.ca[1], c.pb[2] = 0.0, 0.0
    if not cs["m2"]:
        c.ca[2] = 0.0
    if not cs["use_corr"]:
        c.ca = [0.0, 0.0, 0.0, 0.0]
    return c


def unipc_ref(c, cs, dt=F64, defect=None):
    """m_t, x_c, x_next of omh.h and their condition sums"""
    f = lambda t: None if t is None else t.to(dt)                                   # noqa: E731
    cond, unc, x, last, m1, m2 = f(c.cond), f(c.uncond), f(c.x), f(c.last), f(c.m1), f(c.m2)
    if defect == "unipc_cond_uncond_swapped":
        cond, unc = unc, cond
    sc = (lambda v: torch.tensor(v, dtype=dt)) if dt == F32 else (lambda v: v)
    v = unc + sc(c.guide) * (cond - unc)
    sv = unc.abs() + abs(c.guide) * (cond.abs() + unc.abs())
    o = NS()
    o.mt, o.S_mt = x - sc(c.sigma) * v, x.abs() + abs(c.sigma) * sv
    if cs["use_corr"]:
        o.xc, o.S_xc = sc(c.ca[0]) * last + sc(c.ca[3]) * o.mt, abs(c.ca[0]) * last.abs() + abs(c.ca[3]) * o.S_mt
        if m1 is not None and not (defect == "unipc_m1_dropped_without_m2" and m2 is None):
            o.xc = o.xc + sc(c.ca[1]) * m1
        if m1 is not None:
            o.S_xc = o.S_xc + abs(c.ca[1]) * m1.abs()
        if m2 is not None:
            o.xc, o.S_xc = o.xc + sc(c.ca[2]) * m2, o.S_xc + abs(c.ca[2]) * m2.abs()
    else:
        o.xc, o.S_xc = x, x.abs()
    o.xn, o.S_xn = sc(c.pb[0]) * o.xc + sc(c.pb[1]) * o.mt, abs(c.pb[0]) * o.S_xc + abs(c.pb[1]) * o.S_mt
    if m1 is not None:
        o.xn, o.S_xn = o.xn + sc(c.pb[2]) * m1, o.S_xn + abs(c.pb[2]) * m1.abs()
    return o


def unipc_schedule(mod):
    """(sigma, corr, pred) of steps 0, 1 and 2 of a 4-step schedule (shift 3), from the scheduler module ``mod``
    (wan/utils/fm_solvers_unipc.py): order 1 without a corrector, order 2 behind an order-1 corrector, order 2 / 2"""
    sch = mod.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1.0)
    sch.set_timesteps(4, shift=3.0)
    return [mod.unipc_coefficients(sch.sigmas, i, op, oc) for i, op, oc in ((0, 1, None), (1, 2, 1), (2, 2, 2))]


# ----------------------------------------------------------------------------------------------------------------------
# flow_x0_step
# ----------------------------------------------------------------------------------------------------------------------
FLOW_SHAPES = ((1, 1), (1, 5), (2, 3), (3, 7), (3, 1001), (2, 4096))
FLOW_BIG = (3, 2796203)                                     # 8 388 609 elements > 8192 x 256 x 4


def flow_takes_vec(backward, pv, px, pe, p0, pn):
    """omh_flow_x0_step's choice, restated from csrc/dit_elementwise.hip (a NULL pointer is 0)"""
    al = pv | p0
    if not backward:
        al |= px | ((pn | pe) if pn else 0)
    return (al & 15) == 0


def flow_data(B, n, seed=0):
    g = _gen(31, seed, B, n)
    mk = lambda: torch.randn((B, n), generator=g, dtype=F32)                        # noqa: E731
    return NS(v=mk(), x=mk(), eps=mk(), sigma=torch.rand((B,), generator=g, dtype=F32), sigma_next=torch.rand((B,), generator=g, dtype=F32))


def flow_ref(c, backward=False, defect=None):
    """(x0, x_next) in torch fp32, one rounding per operation, left to right as omh.h writes it"""
    B, n = c.v.shape
    b = torch.arange(B * n) // n
    if defect == "flow_one_sigma_per_vector":
        b = (torch.arange(B * n) // 4 * 4) // n
    s, s2 = c.sigma[b].reshape(B, n), c.sigma_next[b].reshape(B, n)
    if backward:
        return (-s) * c.v, None
    sv = s * c.v
    x0 = c.x - sv
    a, e = (1.0 - s2) * x0, s2 * c.eps
    return x0, a + e
