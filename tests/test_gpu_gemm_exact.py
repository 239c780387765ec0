"""Every route of the GEMM family (include/omh.h: omh_gemm_bf16, omh_gemm_bf16_tn, omh_gemm_bf16_tn_grouped) element for
element against the exact references of tests/gemm_exact_ref.py, at tile, K-tail and pitch edges.

Operands are small integers, so fp32 accumulation is exact and ``torch.equal`` holds whatever the summation order: the
8-wave tiles, the one-wave-per-SIMD streams, split K in 2 / 3 / 4 slices and the atomically accumulated TN split are all
held to the same float64 reference, bf16 outputs included (one RNE of an exact value).  The three transcendental
epilogues are held per element to ulp_bf16(ref) + 2^-16 |multiplier| of the fp64 formula; their linear part is exact.

Operand pads (columns [K, lda) / [N, ldb) / [M, lda), and the rows past the logical end that the entry's own
32-bit-offset rule lets a kernel touch: 128 for omh_gemm_bf16, 64 for k-major operands) are allocated and hold NaN.
Every output sits in a canvas whose guard rows and pad columns must keep their bits.

A route is forced through ``set_option`` and each case first asserts, in Python, the precondition under which the
dispatch of csrc/gemm_bf16.hip, csrc/gemm_w64.hip and csrc/gemm_tn.hip really takes that route: a case that would fall
back to another kernel fails instead of counting as coverage.  The ``[routes]`` line printed at the end counts them."""
import collections
import ctypes as C

import pytest
import torch

import gemm_exact_ref as R
from conftest import set_option

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTES = collections.Counter()
WORST = collections.defaultdict(float)      # epilogue name -> worst |got - ref| / bound seen
E_BADARG, E_ALIGN, E_SHAPE = -1, -2, -3
EPI_NAME = {R.EPI_GELU_BF16: "GELU_BF16", R.EPI_GELU_ERF_BF16: "GELU_ERF_BF16", R.EPI_GELU_BWD_BF16: "GELU_BWD_BF16"}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[routes] " + "  ".join(f"{k}={v}" for k, v in sorted(ROUTES.items())))
    print("[measured] worst ratio to ulp_bf16 + 2^-16 s: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))


def _up(x, m):
    return (x + m - 1) // m * m


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch preconditions, restated from csrc/gemm_w64.hip, csrc/gemm_bf16.hip, csrc/gemm_tn.hip, csrc/gemm_tn_w64.hip
# ----------------------------------------------------------------------------------------------------------------------
def _al(p, m=15):
    return p is not None and (p & m) == 0


def w64_takes(a):
    e = a.epilogue
    gbwd = e == R.EPI_GELU_BWD_BF16
    if gbwd and (not a.aux or a.ldaux != a.ldc or not _al(a.aux)):
        return False
    if e == R.EPI_GELU_BF16 and a.aux and (a.ldaux != a.ldc or not _al(a.aux)):
        return False
    bf16_out = e in (R.EPI_BF16, R.EPI_GELU_BF16) or gbwd
    if not (bf16_out or e in (R.EPI_F32, R.EPI_RESID)):
        return False
    if a.bias and a.bias_mode == R.BIAS_M:
        return False
    if e == R.EPI_RESID and a.gate1 and (a.gate_rows < 128 or a.gate1_stride * 4 >= 0x7fffffff or
                                         ((a.M // a.gate_rows) * a.gate1_stride + a.N) * 4 >= 0x7fffffff):
        return False
    es = 2 if bf16_out else 4
    return (a.batch == 1 and not a.b_kmajor and a.K % 64 == 0 and a.K >= 256 and a.N % 8 == 0 and a.M >= 256 and
            a.ldc % (16 // es) == 0 and _al(a.C) and a.lda % 8 == 0 and a.ldb % 8 == 0 and _al(a.A) and _al(a.B) and
            (a.M + 256) * a.lda * 2 < 0x7fffffff and (a.N + 384) * a.ldb * 2 < 0x7fffffff and (a.M + 256) * a.ldc * es < 0xffffffff)


def r192_takes(a):
    if a.aux and (a.ldaux != a.ldc or not _al(a.aux)):
        return False
    if a.c_in and not _al(a.c_in):
        return False
    return a.epilogue == R.EPI_RESID and w64_takes(a) and a.K >= 16 * 64


def n192_takes(a):
    return a.epilogue in (R.EPI_F32, R.EPI_BF16) and w64_takes(a)


def bf16m_takes(a):
    if a.epilogue != R.EPI_BF16 or not a.bias or a.bias_mode != R.BIAS_M:
        return False
    a.bias_mode = R.BIAS_N
    ok = w64_takes(a)
    a.bias_mode = R.BIAS_M
    return ok


def qkv_takes(a):
    if a.epilogue != R.EPI_BF16_SPLIT_T or not a.aux or a.n_split <= 0 or a.n_split >= a.N:
        return False
    if a.n_split % 384 or a.M % 8 or a.ldaux < a.M or a.ldaux % 8 or not _al(a.aux):
        return False
    a.epilogue, aux = R.EPI_BF16, a.aux
    a.aux = None
    ok = w64_takes(a)
    a.epilogue, a.aux = R.EPI_BF16_SPLIT_T, aux
    return ok


def splitk_slices(a):
    """omh_gemm_splitk_slices with GEMM_SPLITK, GEMM_TILE and GEMM_KERNEL unset."""
    if a.batch != 1 or a.b_kmajor or a.epilogue not in (R.EPI_RESID, R.EPI_F32):
        return 1
    if a.bias and (a.bias_mode != R.BIAS_N or not _al(a.bias)):
        return 1
    if a.K < 4096 or a.M < 256 or a.N % 8 or a.ldc % 4 or not _al(a.C):
        return 1
    if a.epilogue == R.EPI_RESID:
        if (a.gate0 and not _al(a.gate0)) or (a.gate1 and (not _al(a.gate1) or a.gate1_stride % 4 or a.gate_rows <= 0)):
            return 1
        if (a.c_in and not _al(a.c_in)) or (a.aux and (a.ldaux % 4 or not _al(a.aux, 7))):
            return 1
    elif a.aux or a.c_in:
        return 1
    t192 = _up(a.M, 256) // 256 * (_up(a.N, 192) // 192)
    if t192 > 128:
        return 1
    for s in (4, 3, 2):
        if t192 * s <= 256 and a.K % (64 * s) == 0 and a.K // s >= 1024:
            return s                    # (the partial product [M, N, K / s] with ldc = N is one the 256 x 192 stream takes)
    return 1


def tn_w64_takes(a):
    return (a.M % 256 == 0 and a.N % 8 == 0 and a.K >= 192 and a.lda % 8 == 0 and a.ldb % 8 == 0 and a.lda >= a.M and
            a.ldb >= a.N and a.ldc >= a.N and _al(a.A) and _al(a.B) and _al(a.C, 3))


def tn_effective_splits(K, asked):
    """launch_tn of csrc/gemm_tn.hip with GEMM_TN_SPLIT = asked (deterministic mode off)."""
    nk = (K + 63) // 64
    s = min(max(asked, 1), 8)
    if nk < 16 * s:
        s = max(nk // 16, 1)
    per = (nk + s - 1) // s
    return (nk + per - 1) // per


# ----------------------------------------------------------------------------------------------------------------------
# one call of omh_gemm_bf16 on canvases
# ----------------------------------------------------------------------------------------------------------------------
def _operand(t, pitch, trail, stride=0):
    """bf16 operand [.., rows, cols] in a NaN-filled allocation: pad columns, ``trail`` rows past the end."""
    blocks = t.shape[0] if t.dim() == 3 else 1
    cv = R.Canvas(t.shape[-2], t.shape[-1], pitch, torch.bfloat16, DEV, lead=0, trail=trail, blocks=blocks, block_stride=stride)
    return cv.put(t).arm()


def run_nt(ops, c, route, takes, lda, ldb, ldc, ldaux=0, tile=None, slices=0, context=""):
    """Run case ``c`` (gemm_exact_ref.GemmCase) through omh_gemm_bf16 and hold every output to the reference.
    ``takes(args)`` is the route's precondition, asserted before the launch; ``slices`` > 0: with a split-K workspace."""
    lib, binding = ops.lib, ops._lib
    M, N, K, e = c.M, c.N, c.K, c.epilogue
    ctx = f"[{route}] {context} M={M} N={N} K={K} lda={lda} ldb={ldb} ldc={ldc} ldaux={ldaux} epi={e} bias={c.bias_mode} batch={c.batch}:"
    sA = 0 if (c.share_a or c.batch == 1) else (M + 1) * lda
    sB = 0 if c.batch == 1 else ((K if c.b_kmajor else N) + 1) * ldb
    sC = 0 if c.batch == 1 else _up((M + 1) * ldc, 8)
    A = _operand(c.a, lda, 128, sA)
    B = _operand(c.b, ldb, 64 if c.b_kmajor else 128, sB)
    bf16_out = e in R.BF16_OUT
    c_cols = c.n_split if e == R.EPI_BF16_SPLIT_T else N
    Cv = R.Canvas(M, c_cols, ldc, torch.bfloat16 if bf16_out else torch.float32, DEV, blocks=c.batch, block_stride=sC)
    Cin = None
    if c.c_old is not None:
        if c.out_of_place:
            Cin = R.Canvas(M, N, ldc, torch.float32, DEV).put(c.c_old).arm()
        else:
            Cv.put(c.c_old)
    Cv.arm()
    Aux = None
    if e == R.EPI_BF16_SPLIT_T:
        Aux = R.Canvas(N - c.n_split, M, ldaux, torch.bfloat16, DEV).arm()
    elif c.with_aux:
        Aux = R.Canvas(M, N, ldaux, torch.bfloat16, DEV).arm()
    elif c.aux_in is not None:
        Aux = R.Canvas(M, N, ldaux, torch.bfloat16, DEV).put(c.aux_in).arm()
    dev = [t.to(DEV) if t is not None else None for t in (c.bias, c.gate0, c.gate1)]
    p = [t.data_ptr() if t is not None else None for t in dev]
    a = binding.GemmArgs(A.ptr, B.ptr, Cv.ptr, M, N, K, lda, ldb, ldc, c.batch, sA, sB, sC, e, c.bias_mode, p[0],
                         p[1], p[2], c.gate1_stride, max(c.gate_rows, 1), c.gate_const, int(c.b_kmajor),
                         Cin.ptr if Cin else None, Aux.ptr if Aux else None, ldaux if Aux else 0, None, 0, c.n_split)
    assert takes(a), f"{ctx} the route's precondition does not hold: the case would run on another kernel"
    ws = None
    if slices:
        need = lib.omh_gemm_workspace_bytes(C.byref(a))
        assert need == slices * _up(M, 256) * N * 4, f"{ctx} workspace query {need}: not {slices} slices"
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    rc = lib.omh_gemm_bf16(C.byref(a), ops._stream())
    assert rc == 0, f"{ctx} omh_gemm_bf16 returned {rc}"
    _sync()
    ROUTES[route] += 1
    ref = R.reference(c)
    got = Cv.window()
    if "C64" in ref:
        worst, msg = R.bound_report(got.float(), ref["C64"], ref["scale"], tile)
        WORST[EPI_NAME[e]] = max(WORST[EPI_NAME[e]], worst)
        print(f"[measured] {ctx} worst |got - ref| / (ulp_bf16 + 2^-16 s) = {worst:.4f}")
        assert msg is None, f"{ctx} {msg}"
    else:
        R.assert_exact(got, ref["C"], tile, "C", ctx)
    Cv.assert_guard("C", ctx)
    if "aux" in ref:
        R.assert_exact(Aux.window(), ref["aux"], tile, "aux", ctx)
    if Aux is not None:
        Aux.assert_guard("aux", ctx)
        if c.aux_in is not None:
            R.assert_exact(Aux.window(), c.aux_in, None, "aux (an input)", ctx)
    if Cin is not None:
        Cin.assert_guard("c_in", ctx)
        R.assert_exact(Cin.window(), c.c_old, None, "c_in (an input)", ctx)
    return a


def _ldc_of(N, mode):
    """N, the next odd number >= N, N + 8."""
    return (N, N | 1, N + 8)[mode]


# ----------------------------------------------------------------------------------------------------------------------
# 8-wave kernels
# ----------------------------------------------------------------------------------------------------------------------
VARIANTS_8W = {
    "f32": dict(epilogue=R.EPI_F32),
    "bf16": dict(epilogue=R.EPI_BF16),
    "f32_accum": dict(epilogue=R.EPI_F32_ACCUM),
    "resid": dict(epilogue=R.EPI_RESID, use_gate0=True),
    "resid_c_in": dict(epilogue=R.EPI_RESID, out_of_place=True, use_gate0=True),
    "resid_c_in_aux": dict(epilogue=R.EPI_RESID, out_of_place=True, with_aux=True),
    "resid_gate1_aux": dict(epilogue=R.EPI_RESID, with_aux=True, use_gate0=True, gate_rows=13),     # a boundary inside a 32-row strip
    "gelu": dict(epilogue=R.EPI_GELU_BF16),
    "gelu_aux": dict(epilogue=R.EPI_GELU_BF16, with_aux=True),
    "gelu_erf": dict(epilogue=R.EPI_GELU_ERF_BF16),
    "gelu_bwd": dict(epilogue=R.EPI_GELU_BWD_BF16),
    "batch_shared_a": dict(epilogue=R.EPI_F32, batch=2, share_a=True),
    "batch3_bf16": dict(epilogue=R.EPI_BF16, batch=3),
    "batch3_f32_accum": dict(epilogue=R.EPI_F32_ACCUM, batch=3),
}
KS_8W = (8, 40, 64, 72, 200)


def _takes_8w(tile):
    def takes(a):           # GEMM_TILE set, GEMM_KERNEL unset: no stream, no split K; mid192 / tiny have no k-major form
        return not (a.b_kmajor and tile in ("mid192", "tiny"))
    return takes


@pytest.mark.parametrize("variant", sorted(VARIANTS_8W))
@pytest.mark.parametrize("tile", ["big", "mid192", "small", "tiny"])
def test_8_wave_kernels_at_tile_k_tail_and_pitch_edges(ops, tile, variant):
    """M in {BM-1, BM, BM+1, 1, 33} x N in {BN-1, BN, BN+1, 1, 7, 9, 201}; K in {8, 40, 64, 72, 200}; ldc in {N, next odd,
    N + 8}; lda / ldb = K or K + 8 with NaN pads; bias none / by N / by M.  Odd N and odd ldc switch the epilogue to its
    element-wise stores, reads of the old C and aux accesses (vec_ok == false).  Every variant walks all 35 (M, N)
    pairs; K, the pitches and the bias mode cycle with periods 5, 3, 2 and 3 against them."""
    bm, bn = R.TILES_8W[tile]
    kw = VARIANTS_8W[variant]
    v = sorted(VARIANTS_8W).index(variant)
    Ms, Ns = (bm - 1, bm, bm + 1, 1, 33), (bn - 1, bn, bn + 1, 1, 7, 9, 201)
    set_option("GEMM_TILE", tile)
    for i, (M, N) in enumerate([(m, n) for m in Ms for n in Ns]):
        K = KS_8W[(i + v) % 5]
        pad = 8 * ((i + v // 2) % 2)
        ldc = _ldc_of(N, (i + v) % 3)
        bias_mode = (R.BIAS_NONE, R.BIAS_N, R.BIAS_M)[(i // 3 + v) % 3] if variant != "gelu_bwd" else R.BIAS_NONE
        c = R.make_case(M, N, K, bias_mode=bias_mode, seed=100 * v + i, **kw)
        run_nt(ops, c, f"8w/{tile}", _takes_8w(tile), K + pad, K + pad, ldc, ldaux=_up(N, 8) + pad,
               tile=(tile, bm, bn), context=variant)


def test_an_aux_pitch_that_is_no_multiple_of_8_is_refused(ops):
    """The kernels read and write aux rows with 16-byte accesses where C allows it; the entry refuses every other pitch
    (include/omh.h: ldaux a multiple of 8), so the element-wise aux path is reached through an odd N or ldc only."""
    binding = ops._lib
    c = R.make_case(33, 9, 40, epilogue=R.EPI_GELU_BWD_BF16, seed=5)
    A, B = _operand(c.a, 40, 128), _operand(c.b, 40, 128)
    Cv = R.Canvas(33, 9, 9, torch.bfloat16, DEV).arm()
    for ldaux in (9, 12, 20):
        Aux = R.Canvas(33, 9, ldaux, torch.bfloat16, DEV).put(c.aux_in).arm()
        a = binding.GemmArgs(A.ptr, B.ptr, Cv.ptr, 33, 9, 40, 40, 40, 9, 1, 0, 0, 0, R.EPI_GELU_BWD_BF16, 0, None, None, None, 0, 1,
                             0.0, 0, None, Aux.ptr, ldaux, None, 0, 0)
        assert ops.lib.omh_gemm_bf16(C.byref(a), ops._stream()) == E_ALIGN
    _sync()
    Cv.assert_guard()
    assert bool(torch.isnan(Cv.window().float()).all())


# ----------------------------------------------------------------------------------------------------------------------
# k-major B
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["f32", "bf16", "f32_accum", "batch3_f32_accum"])
@pytest.mark.parametrize("tile", ["big", "small"])
def test_k_major_b_at_tile_k_tail_and_pitch_edges(ops, tile, epi):
    """B as [K, N] with ldb = N + 24 (NaN pad, 64 NaN rows past K): M in {BM-1, BM, BM+1, 1, 33}, N in {8, 72, BN-8, BN+8},
    K in {8, 40, 64, 72, 200}; the batched strided call writes into a C that starts inside a larger buffer."""
    bm, bn = R.TILES_8W[tile]
    kw = VARIANTS_8W[epi]
    v = ("f32", "bf16", "f32_accum", "batch3_f32_accum").index(epi)
    Ms, Ns = (bm - 1, bm, bm + 1, 1, 33), (8, 72, bn - 8, bn + 8)
    set_option("GEMM_TILE", tile)
    for i in range(10):
        M, N, K = Ms[i % 5], Ns[(i + i // 5 + v) % 4], KS_8W[(i + v) % 5]
        c = R.make_case(M, N, K, b_kmajor=True, bias_mode=(R.BIAS_NONE, R.BIAS_N, R.BIAS_M)[(i + v) % 3], seed=300 + 10 * v + i, **kw)
        run_nt(ops, c, f"kmajor/{tile}", _takes_8w(tile), K + 8 * (i % 2), N + 24, _ldc_of(N, (i + v) % 3), tile=(tile, bm, bn),
               context=epi)


# ----------------------------------------------------------------------------------------------------------------------
# streams
# ----------------------------------------------------------------------------------------------------------------------
W64 = {"GEMM_KERNEL": "w64"}
STREAMS = {
    # route: (options, takes, tile, make_case keywords, K values)
    "w64/f32": (dict(W64, GEMM_W64_N192="0"), w64_takes, R.TILE_W64, dict(epilogue=R.EPI_F32), None),
    "w64/bf16": (dict(W64, GEMM_W64_N192="0"), w64_takes, R.TILE_W64, dict(epilogue=R.EPI_BF16), None),
    "w64/gelu": (W64, w64_takes, R.TILE_W64, dict(epilogue=R.EPI_GELU_BF16), None),
    "w64/gelu_aux": (W64, w64_takes, R.TILE_W64, dict(epilogue=R.EPI_GELU_BF16, with_aux=True), None),
    "w64/gelu_bwd": (dict(W64, GEMM_W64_GBWD="1"), w64_takes, R.TILE_W64, dict(epilogue=R.EPI_GELU_BWD_BF16, bias_mode=R.BIAS_NONE),
                     None),
    "w64/resid": (dict(W64, GEMM_W64_R192="0"), w64_takes, R.TILE_W64, dict(epilogue=R.EPI_RESID, use_gate0=True, gate_rows=130), None),
    "w64/bf16_bias_m": (dict(W64, GEMM_W64_BF16M="1"), bf16m_takes, R.TILE_W64, dict(epilogue=R.EPI_BF16, bias_mode=R.BIAS_M), None),
    "r192/in_place": (dict(W64, GEMM_W64_R192="1"), r192_takes, R.TILE_W64_192, dict(epilogue=R.EPI_RESID, use_gate0=True, gate_rows=130),
                      (1024, 1088)),
    "r192/c_in": (dict(W64, GEMM_W64_R192="1"), r192_takes, R.TILE_W64_192, dict(epilogue=R.EPI_RESID, out_of_place=True, use_gate0=True),
                  (1024, 1088)),
    "r192/c_in_aux": (dict(W64, GEMM_W64_R192="1"), r192_takes, R.TILE_W64_192,
                      dict(epilogue=R.EPI_RESID, out_of_place=True, with_aux=True, gate_rows=200), (1024, 1088)),
    "n192/f32": (dict(W64, GEMM_W64_N192="1"), n192_takes, R.TILE_W64_192, dict(epilogue=R.EPI_F32), None),
    "n192/bf16": (dict(W64, GEMM_W64_N192="1"), n192_takes, R.TILE_W64_192, dict(epilogue=R.EPI_BF16), None),
}


@pytest.mark.parametrize("route", sorted(STREAMS))
def test_streams_against_the_exact_reference(ops, route):
    """M in {256, 257, 511} x N in {8, 184, 192, 200, 376, 384, 392}, K in {256, 320, 1024, 1088} (even and odd step
    counts; the gated-residual 256 x 192 stream from its minimum of 16 steps), C and aux at a 16-byte-aligned pitch wider
    than N with guards all round — against the float64 reference, not against the 8-wave kernels."""
    opts, takes, tile, kw, ks = STREAMS[route]
    v = sorted(STREAMS).index(route)
    for k_, val in opts.items():
        set_option(k_, val)
    Ms, Ns, Ks = (256, 257, 511), (8, 184, 192, 200, 376, 384, 392), ks or (256, 320, 1024, 1088)
    for i in range(21):                                                   # every (M, N) pair once
        M, N, K = Ms[i // 7], Ns[i % 7], Ks[(i + v + i // 7) % len(Ks)]
        kw2 = dict(kw)
        kw2.setdefault("bias_mode", (R.BIAS_N, R.BIAS_NONE)[(i + v) % 2])
        c = R.make_case(M, N, K, seed=500 + 20 * v + i, **kw2)
        run_nt(ops, c, route, takes, K + 8 * (i % 2), K + 8 * ((i // 2) % 2), N + 8, ldaux=N + 8, tile=(route,) + tile)


@pytest.mark.parametrize("extra", [8, 200])
def test_fused_qkv_stream_against_the_exact_reference(ops, extra):
    """OMH_EPI_BF16_SPLIT_T on the 256 x 384 stream: n_split = 384, N = 384 + {8, 200}, M in {256, 264, 504}, ldaux > M;
    the transposed tail element for element, the pad columns of V^T and the guard rows of q | k untouched."""
    set_option("GEMM_QKV", "1")
    for i, M in enumerate((256, 264, 504)):
        for j, K in enumerate(((256, 1088), (320, 1024))[i % 2]):
            c = R.make_case(M, 384 + extra, K, epilogue=R.EPI_BF16_SPLIT_T, n_split=384, seed=700 + 10 * i + j + extra,
                            bias_mode=(R.BIAS_N, R.BIAS_NONE)[(i + j) % 2])
            run_nt(ops, c, "qkv", qkv_takes, K + 8 * j, K + 8 * (1 - j), 384 + 8, ldaux=M + 8 + 8 * j, tile=("qkv",) + R.TILE_W64)


# ----------------------------------------------------------------------------------------------------------------------
# split K
# ----------------------------------------------------------------------------------------------------------------------
SPLITK = {
    "resid": dict(epilogue=R.EPI_RESID, use_gate0=True, bias_mode=R.BIAS_N),
    "resid_c_in_aux": dict(epilogue=R.EPI_RESID, out_of_place=True, with_aux=True, use_gate0=True, bias_mode=R.BIAS_N),
    "resid_gate1": dict(epilogue=R.EPI_RESID, gate_rows=100, use_gate0=True, bias_mode=R.BIAS_N),      # a boundary inside the rows
    "f32_bias": dict(epilogue=R.EPI_F32, bias_mode=R.BIAS_N),
    "f32": dict(epilogue=R.EPI_F32),
}


@pytest.mark.parametrize("epi", sorted(SPLITK))
@pytest.mark.parametrize("K,S", [(4096, 4), (4224, 3), (4480, 2)])
def test_split_k_is_exact(ops, K, S, epi):
    """S = 4 / 3 / 2 slices on the fp32 256 x 192 stream and the combine launch, M in {256, 300} x N in {192, 200}:
    equality with the unsplit float64 result, which no bound on a norm could ask for.  S is asserted twice: by the rule
    restated here and through omh_gemm_workspace_bytes."""
    for k_ in ("GEMM_KERNEL", "GEMM_TILE", "GEMM_SPLITK"):
        set_option(k_, None)
    for i, (M, N) in enumerate([(256, 192), (256, 200), (300, 192), (300, 200)]):
        c = R.make_case(M, N, K, seed=900 + i, **SPLITK[epi])
        run_nt(ops, c, f"splitk/S{S}", lambda a: splitk_slices(a) == S, K + 8 * (i % 2), K + 8 * (i // 2), N + 8, ldaux=N + 8,
               tile=(f"split-K S={S}",) + R.TILE_W64_192, slices=S, context=epi)


# ----------------------------------------------------------------------------------------------------------------------
# TN
# ----------------------------------------------------------------------------------------------------------------------
def _tn_problem(c, lda, ldb, ldc, c_offset_bytes=4):
    A, B = _operand(c.a, lda, 64), _operand(c.b, ldb, 64)
    Cv = R.Canvas(c.M, c.N, ldc, torch.float32, DEV, offset_bytes=c_offset_bytes)
    if c.accumulate:
        Cv.put(c.c_old)
    return A, B, Cv.arm()


def _tn_check(c, Cv, tile, ctx):
    R.assert_exact(Cv.window(), R.reference(c)["C"], tile, "C", ctx)
    Cv.assert_guard("C", ctx)


def run_tn(ops, c, route, takes, lda, ldb, ldc, tile):
    ctx = f"[{route}] M={c.M} N={c.N} K={c.K} lda={lda} ldb={ldb} ldc={ldc} accumulate={c.accumulate}:"
    A, B, Cv = _tn_problem(c, lda, ldb, ldc)
    assert Cv.ptr % 16 == 4
    a = ops._lib.GemmTnArgs(A.ptr, B.ptr, Cv.ptr, c.M, c.N, c.K, lda, ldb, ldc, int(c.accumulate))
    assert takes(a), f"{ctx} the route's precondition does not hold"
    rc = ops.lib.omh_gemm_bf16_tn(C.byref(a), ops._stream())
    assert rc == 0, f"{ctx} omh_gemm_bf16_tn returned {rc}"
    _sync()
    ROUTES[route] += 1
    _tn_check(c, Cv, tile, ctx)


TN_MN = (8, 120, 128, 136, 384, 392)
TN_KS = (1, 8, 63, 64, 65, 200, 333)
TN_LONG_K = {1: 1100, 3: 3100, 8: 8200}       # 16 k-steps of 64 per slice is the least launch_tn splits at: 49 and 129 steps


@pytest.mark.parametrize("split", [1, 3, 8])
@pytest.mark.parametrize("tile", ["big", "small"])
def test_tn_tiles_store_accumulate_and_atomic_split(ops, tile, split):
    """The tiled TN kernels, M and N in {8, 120, 128, 136, 384, 392}, K in {1, 8, 63, 64, 65, 200, 333} and one contraction
    long enough for GEMM_TN_SPLIT to cut it (the split's partial sums meet in fp32 atomics: exact here, in any order).
    Rows past K and the pad columns of both operands are NaN; C is 4-byte but not 16-byte aligned in a wider canvas."""
    set_option("GEMM_TN_W64", "0")
    set_option("GEMM_TN_TILE", tile)
    set_option("GEMM_TN_SPLIT", str(split))
    bm, bn = R.TILES_TN[tile]
    v = split + (3 if tile == "big" else 0)
    if split == 1:          # all 36 (M, N) pairs, K cycling (a forced count changes nothing below 32 k-steps: once is enough)
        shapes = [(M, N, TN_KS[(6 * i + j + v) % 7]) for i, M in enumerate(TN_MN) for j, N in enumerate(TN_MN)]
    else:
        shapes = [(TN_MN[(i + v) % 6], TN_MN[(2 * i + v + 1) % 6], K) for i, K in enumerate(TN_KS)]
    shapes += [(136, 120, TN_LONG_K[split]), (392, 136, TN_LONG_K[split]), (8, 392, TN_LONG_K[split]), (128, 384, TN_LONG_K[split] + 29),
               (120, 8, TN_LONG_K[split] + 64), (384, 128, TN_LONG_K[split] + 1)]
    for i, (M, N, K) in enumerate(shapes):
        eff = tn_effective_splits(K, split)
        if K >= TN_LONG_K[split]:
            assert eff == split
        c = R.make_case(M, N, K, tn=True, accumulate=bool((i + v) % 2), seed=1100 + 10 * v + i)
        run_tn(ops, c, f"tn/{tile}/split{eff}", lambda a: True, M + 8 * (i % 2), N + 8 * ((i + 1) % 2), N + 5 + i % 3,
               (f"tn {tile}", bm, bn))


def test_tn_stream_store_and_accumulate(ops):
    """The 256 x 384 k-major stream (M a multiple of 256, K >= 192): ragged N and K, store and accumulate."""
    set_option("GEMM_TN_W64", "1")
    for i, N in enumerate(TN_MN):
        for j, M in enumerate((256, 512)):
            K = (192, 200, 256, 333)[(i + 2 * j) % 4]
            c = R.make_case(M, N, K, tn=True, accumulate=bool((i + j) % 2), seed=1300 + 10 * i + j)
            run_tn(ops, c, "tn/w64", tn_w64_takes, M + 8 * (i % 2), N + 8 * (j % 2), N + 3 + i, ("tn w64",) + R.TILE_W64)


@pytest.mark.parametrize("route", ["small", "big", "w64"])
def test_tn_grouped_three_products(ops, route):
    """omh_gemm_bf16_tn_grouped with three products in one launch: one stores, one accumulates, and one writes a column
    block of a wider buffer (its C starts 24 floats into rows that are 40 floats wider than N)."""
    set_option("GEMM_TN_W64", "1" if route == "w64" else "0")
    if route != "w64":
        set_option("GEMM_TN_GROUP_TILE", route)
    shapes = [(256, 392, 333), (512, 120, 200), (256, 136, 192)] if route == "w64" else [(136, 392, 333), (384, 120, 65), (8, 136, 200)]
    tile = ("tn w64",) + R.TILE_W64 if route == "w64" else ("tn grouped " + route,) + R.TILES_TN[route]
    g = ops._lib.GemmTnGroup()
    g.n = 3
    held = []
    for i, (M, N, K) in enumerate(shapes):
        c = R.make_case(M, N, K, tn=True, accumulate=(i == 1), seed=1500 + i)
        A, B, Cv = _tn_problem(c, M + 8 * (i % 2), N + 8, N + 40 if i == 2 else N + 1, c_offset_bytes=96 if i == 2 else 4)
        g.problem[i] = ops._lib.GemmTnArgs(A.ptr, B.ptr, Cv.ptr, M, N, K, A.pitch, B.pitch, Cv.pitch, int(c.accumulate))
        assert route != "w64" or tn_w64_takes(g.problem[i])
        held.append((c, A, B, Cv))
    rc = ops.lib.omh_gemm_bf16_tn_grouped(C.byref(g), ops._stream())
    assert rc == 0
    _sync()
    ROUTES[f"tn_grouped/{route}"] += 3
    for c, _, _, Cv in held:
        _tn_check(c, Cv, tile, f"[tn_grouped/{route}] M={c.M} N={c.N} K={c.K}:")
