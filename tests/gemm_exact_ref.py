"""Exact references for the GEMM family of include/omh.h (omh_gemm_bf16, omh_gemm_bf16_tn, omh_gemm_bf16_tn_grouped).
Test infrastructure, not a test module; plain torch, importable without a GPU.

The method: make fp32 accumulation exact.  Operands are small integers (times one power of two), so every product and
every partial sum of the contraction is an integer (times that power of two) below 2^24 and has ONE fp32 value whatever
the summation order, the tile shape, the number of split-K slices or the order of the atomics.  ``torch.equal`` against
a float64 reference is then the assertion for every route — bf16 outputs included, because one round-to-nearest-even of
an exact value is what both sides do (pack_bf2 / f2bf of csrc/omh_common.h are RNE).

The exactness condition (derived, not measured; asserted by ``check_exact`` for every case that is generated):
  |a|, |b| <= 3 and |bias| <= 8 (integers)  =>  |acc + bias| <= 9 K + 8 =: L, an integer     need  L     < 2^24
  gate = gate_const + gate0 + gate1, multiples of 1/2 with |gate| <= 4.5
      =>  (acc + bias) * gate is a multiple of 1/2 of magnitude <= 4.5 L                      need  9 L   < 2^24
  old C / residual integer, |c| <= 64  =>  c + (acc + bias) * gate: a multiple of 1/2         need  9 L + 128 < 2^24
At the largest K in use, 8 960: L = 80 648, 9 L + 128 = 725 960 < 16 777 216.
A common factor 2^-s on one operand and on the bias (the GELU family wants pre-activations of order 1) only moves the
exponent of every value above: nothing is rounded as long as the smallest unit, 2^-s / 2, stays a normal number.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID, EPI_F32_ACCUM, EPI_GELU_ERF_BF16, EPI_GELU_BWD_BF16, EPI_BF16_SPLIT_T = range(8)
BIAS_NONE, BIAS_N, BIAS_M = 0, 1, 2
BF16_OUT = (EPI_BF16, EPI_GELU_BF16, EPI_GELU_ERF_BF16, EPI_GELU_BWD_BF16, EPI_BF16_SPLIT_T)
TRANSCENDENTAL = (EPI_GELU_BF16, EPI_GELU_ERF_BF16, EPI_GELU_BWD_BF16)

AB_MAX, BIAS_MAX, C_MAX, GATE_MAX = 3, 8, 64, 4.5
K_MAX = 8960
F32_EXACT = 1 << 24

# tile configurations of csrc/gemm_bf16.hip (OMH_GEMM_TILE), csrc/gemm_w64.hip and csrc/gemm_tn.hip: (rows, columns)
TILES_8W = {"big": (256, 256), "mid192": (192, 256), "small": (128, 128), "tiny": (64, 64)}
TILE_W64, TILE_W64_192 = (256, 384), (256, 192)
TILES_TN = {"big": (256, 256), "small": (128, 128)}


def check_exact(K, gated=False, accumulates=False, scale_exp=0):
    """Assert the condition of the module docstring for one case; returns the bound on |acc + bias| (unscaled)."""
    L = AB_MAX * AB_MAX * K + BIAS_MAX
    assert K <= K_MAX, f"K = {K}: the bound was derived up to K = {K_MAX}"
    assert L < F32_EXACT, f"K = {K}: |acc + bias| can reach {L} >= 2^24"
    top = L
    if gated:
        top = int(2 * GATE_MAX * L)                 # in units of 1/2
        assert top < F32_EXACT, f"K = {K}: the gated value needs {top} half-units"
    if accumulates or gated:
        top = top + 2 * C_MAX
        assert top < F32_EXACT, f"K = {K}: old C + value needs {top} (half-)units"
    assert 0 <= scale_exp <= 100, "the unit 2^-s / 2 must stay a normal fp32 number"
    return L


def order_one_scale_exp(K):
    """s with 2^-s * (standard deviation of acc) of order 1: products of two uniform integers in [-3, 3] have variance 16."""
    return max(0, round(math.log2(4.0 * math.sqrt(K))))


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return g


def _ints(g, shape, hi):
    return torch.randint(-hi, hi + 1, shape, generator=g, dtype=torch.int64)


@dataclass
class GemmCase:
    """One call of omh_gemm_bf16 (or of the TN entries: ``tn``), all tensors on the CPU, values exact in their dtype.
    a: [batch, M, K] (tn: [K, M]); b: [batch, N, K] (b_kmajor / tn: [K, N]); shapes without the batch axis when batch == 1."""
    M: int
    N: int
    K: int
    epilogue: int = EPI_F32
    bias_mode: int = BIAS_NONE
    batch: int = 1
    b_kmajor: bool = False
    tn: bool = False
    accumulate: bool = False           # tn only
    out_of_place: bool = False         # RESID: old values from c_in
    with_aux: bool = False             # RESID / GELU_BF16: aux OUT
    gate_const: float = 0.0
    gate_rows: int = 0                 # > 0: gate1 [ceil(M / gate_rows), gate1_stride] is used
    gate1_stride: int = 0
    use_gate0: bool = False
    n_split: int = 0
    scale_exp: int = 0
    share_a: bool = False              # batched: strideA = 0
    seed: int = 0
    a: torch.Tensor = field(default=None, repr=False)
    b: torch.Tensor = field(default=None, repr=False)
    bias: Optional[torch.Tensor] = field(default=None, repr=False)
    c_old: Optional[torch.Tensor] = field(default=None, repr=False)
    gate0: Optional[torch.Tensor] = field(default=None, repr=False)
    gate1: Optional[torch.Tensor] = field(default=None, repr=False)
    aux_in: Optional[torch.Tensor] = field(default=None, repr=False)


def make_case(M, N, K, epilogue=EPI_F32, bias_mode=BIAS_NONE, seed=0, batch=1, b_kmajor=False, tn=False, accumulate=False,
              out_of_place=False, with_aux=False, gate_const=None, use_gate0=False, gate_rows=0, gate1_stride=0, n_split=0,
              share_a=False):
    """Seeded operands: bf16 A, B integer in [-3, 3] (B times 2^-s for the GELU family), fp32 bias integer in [-8, 8]
    (times 2^-s), old C / residual integer in [-64, 64], gate tables multiples of 1/2 in [-2, 2], gate_const in
    {-1/2, 0, 1/2}.  The exactness condition is asserted here, for every case."""
    g = _gen(seed * 1000003 + M * 7919 + N * 104729 + K)
    gated = epilogue == EPI_RESID
    accum = epilogue in (EPI_RESID, EPI_F32_ACCUM) or (tn and accumulate)
    s = order_one_scale_exp(K) if epilogue in TRANSCENDENTAL else 0
    check_exact(K, gated=gated, accumulates=accum, scale_exp=s)
    c = GemmCase(M, N, K, epilogue, bias_mode, batch, b_kmajor, tn, accumulate, out_of_place, with_aux,
                 0.0, gate_rows, gate1_stride, use_gate0, n_split, s, share_a, seed)
    bsh = (batch,) if batch > 1 else ()
    ash = () if share_a else bsh
    if tn:
        c.a = _ints(g, (K, M), AB_MAX).to(torch.bfloat16)
        c.b = _ints(g, (K, N), AB_MAX).to(torch.bfloat16)
    else:
        c.a = _ints(g, ash + (M, K), AB_MAX).to(torch.bfloat16)
        bb = _ints(g, bsh + ((K, N) if b_kmajor else (N, K)), AB_MAX).double() * 2.0 ** -s
        c.b = bb.to(torch.bfloat16)
        assert torch.equal(c.b.double(), bb)
    if bias_mode != BIAS_NONE:
        c.bias = (_ints(g, (N if bias_mode == BIAS_N else M,), BIAS_MAX).double() * 2.0 ** -s).float()
    if accum:
        c.c_old = _ints(g, bsh + (M, N), C_MAX).float()
    if gated:
        c.gate_const = 0.5 * float(torch.randint(-1, 2, (1,), generator=g)) if gate_const is None else float(gate_const)
        assert abs(c.gate_const) <= 0.5 and c.gate_const * 2 == int(c.gate_const * 2)
        if use_gate0:
            c.gate0 = (_ints(g, (N,), 4).double() * 0.5).float()
        if gate_rows > 0:
            c.gate1_stride = gate1_stride or N
            assert c.gate1_stride >= N
            c.gate1 = (_ints(g, ((M + gate_rows - 1) // gate_rows, c.gate1_stride), 4).double() * 0.5).float()
        if not use_gate0 and gate_rows <= 0 and c.gate_const == 0.0:
            c.gate_const = 0.5                      # a gate of exactly zero everywhere would hide the product
    if epilogue == EPI_GELU_BWD_BF16:               # the forward's pre-activations: multiples of 1/16 in [-4, 4], exact in bf16
        c.aux_in = (_ints(g, (M, N), 64).double() / 16.0).to(torch.bfloat16)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# references (float64 on the CPU: every value is an integer times a power of two far below 2^53, so exact)
# ----------------------------------------------------------------------------------------------------------------------
def rne_bf16(x):
    """float64 values that are exact in fp32 -> bf16 by round-to-nearest-even on the fp32 bit pattern, spelled out."""
    f = x.float()
    assert torch.equal(f.double(), x.double()), "the value is not exact in fp32: the case breaks the exactness condition"
    u = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    u = torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)
    return u.view(torch.bfloat16)


def truncate_bf16(x):
    """The wrong conversion (drop the low 16 bits): what test_gemm_exact_host.py plants."""
    u = (x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) >> 16
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(torch.bfloat16)


def exact_f32(x):
    f = x.float()
    assert torch.equal(f.double(), x), "the value is not exact in fp32: the case breaks the exactness condition"
    return f


def linear_part(c):
    """acc + bias in float64, [batch,] M, N."""
    a, b = c.a.double(), c.b.double()
    if c.tn:
        acc = a.t() @ b
    elif c.b_kmajor:
        acc = a @ b
    else:
        acc = a @ b.transpose(-1, -2)
    if c.bias is not None:
        acc = acc + (c.bias.double()[None, :] if c.bias_mode == BIAS_N else c.bias.double()[:, None])
    return acc


def gate_of(c):
    """[M, N] float64 gate of OMH_EPI_RESID: gate_const + gate0[n] + gate1[(m / gate_rows) * gate1_stride + n]."""
    g = torch.full((c.M, c.N), c.gate_const, dtype=torch.float64)
    if c.gate0 is not None:
        g = g + c.gate0.double()[None, :]
    if c.gate1 is not None:
        rows = torch.arange(c.M) // c.gate_rows
        g = g + c.gate1.double()[rows, :c.N]
    assert float(g.abs().max()) <= GATE_MAX
    return g


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_tanh_grad64(x):
    cc, aa = 0.7978845608028654, 0.044715
    t = torch.tanh(cc * (x + aa * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * cc * (1.0 + 3.0 * aa * x * x)


def reference(c):
    """dict of what the entry must leave behind.
    exact outputs      "C" (fp32 or bf16 tensor, compared with torch.equal), "aux" (bf16; for BF16_SPLIT_T the transposed
                       columns from n_split on, [N - n_split, M])
    transcendental     "C64" (float64 formula on the exact pre-activation) and "scale" (|x| / |dy|) for ``bound_of``"""
    lin = linear_part(c)
    e = c.epilogue
    out = {}
    if c.tn:
        out["C"] = exact_f32(lin + (c.c_old.double() if c.accumulate else 0.0))
    elif e == EPI_F32:
        out["C"] = exact_f32(lin)
    elif e == EPI_BF16:
        out["C"] = rne_bf16(lin)
    elif e == EPI_F32_ACCUM:
        out["C"] = exact_f32(c.c_old.double() + lin)
    elif e == EPI_RESID:
        out["C"] = exact_f32(c.c_old.double() + exact_f32(lin * gate_of(c)).double())
        if c.with_aux:
            out["aux"] = rne_bf16(lin)
    elif e == EPI_BF16_SPLIT_T:
        out["C"] = rne_bf16(lin[:, :c.n_split])
        out["aux"] = rne_bf16(lin[:, c.n_split:].t().contiguous())
    elif e in (EPI_GELU_BF16, EPI_GELU_ERF_BF16):
        exact_f32(lin)
        out["C64"] = gelu_tanh64(lin) if e == EPI_GELU_BF16 else gelu_erf64(lin)
        out["scale"] = lin.abs()
        if c.with_aux:
            out["aux"] = rne_bf16(lin)
    elif e == EPI_GELU_BWD_BF16:
        exact_f32(lin)
        out["C64"] = lin * gelu_tanh_grad64(c.aux_in.double())
        out["scale"] = lin.abs()
    else:
        raise ValueError(e)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# bounds and comparers
# ----------------------------------------------------------------------------------------------------------------------
def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 7); subnormal spacing 2^-133 below 2^-126."""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7.0)


def bound_of(ref64, scale):
    """ulp_bf16(ref) + 2^-16 * scale, floor 2^-126.  A value with fp32-level relative error rounds to one of the two bf16
    neighbours of the exact value (one ulp); 2^-16 * |multiplier| leaves 2^8 over fp32 epsilon for the conditioning of
    the formula (gelu_tanh' near its zero, 1 + tanh near -1)."""
    return (ulp_bf16(ref64) + 2.0 ** -16 * scale).clamp_min(2.0 ** -126)


def _tile_note(rows, cols, tile):
    if tile is None:
        return ""
    name, bm, bn = tile
    tiles = sorted({(int(r) // bm, int(q) // bn) for r, q in zip(rows.tolist(), cols.tolist())})
    head = ", ".join(f"(tm {a}, tn {b}: rows {a * bm}..{a * bm + bm - 1}, cols {b * bn}..{b * bn + bn - 1})" for a, b in tiles[:4])
    return f"; {len(tiles)} tile(s) of {name} {bm} x {bn} hold them: {head}{' ...' if len(tiles) > 4 else ''}"


def mismatch_report(got, want, tile=None, what="C", limit=6):
    """None when ``got`` equals ``want`` element for element (same dtype and shape; a NaN never equals), else a line
    that names the count of wrong elements, the first few (row, col, got, want) and the tiles of ``tile`` =
    (name, BM, BN) they fall in."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{what}: got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = ~(g2 == w2)
    rows, cols = bad.nonzero(as_tuple=True)
    per = got.shape[-2] if got.dim() >= 2 else 1
    first = ", ".join(f"({'b %d, ' % (int(r) // per) if got.dim() > 2 else ''}row {int(r) % per}, col {int(q)}: got "
                      f"{float(g2[r, q])!r}, want {float(w2[r, q])!r})" for r, q in zip(rows[:limit], cols[:limit]))
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first: {first}"
            f"{_tile_note(rows % per, cols, tile)}")


def assert_exact(got, want, tile=None, what="C", context=""):
    msg = mismatch_report(got, want, tile, what)
    assert msg is None, f"{context} {msg}"


def bound_report(got, ref64, scale, tile=None, what="C", limit=6):
    """(worst |got - ref| / bound, None or the report of the elements over the bound)."""
    got = got.detach().cpu().double()
    bound = bound_of(ref64, scale)
    ratio = (got - ref64).abs() / bound
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    if not bool(bad.any()):
        return worst, None
    rows, cols = bad.nonzero(as_tuple=True)
    first = ", ".join(f"(row {int(r)}, col {int(q)}: got {float(got[r, q])!r}, want {float(ref64[r, q])!r}, bound "
                      f"{float(bound[r, q]):.3e})" for r, q in zip(rows[:limit], cols[:limit]))
    return worst, (f"{what}: {int(bad.sum())} of {bad.numel()} elements miss ulp_bf16 + 2^-16 s (worst ratio {worst:.3f}); "
                   f"first: {first}{_tile_note(rows, cols, tile)}")


# ----------------------------------------------------------------------------------------------------------------------
# canvases
# ----------------------------------------------------------------------------------------------------------------------
class Canvas:
    """A logical [rows, cols] window inside a larger allocation: row pitch ``pitch`` >= cols, ``lead`` guard rows before
    and ``trail`` guard rows after it, the window's first element on a 16-byte boundary plus ``offset_bytes``.  Every
    element outside the window holds ``sentinel`` (NaN for operands: pad columns and the rows a kernel may touch past the
    logical end are really allocated and hostile); ``assert_guard`` proves that no byte outside the window changed.
    ``blocks`` > 1: that many windows, ``block_stride`` elements apart (the batched strided form)."""

    def __init__(self, rows, cols, pitch, dtype, device="cpu", lead=2, trail=2, sentinel=float("nan"), offset_bytes=0,
                 blocks=1, block_stride=0):
        assert pitch >= cols and rows >= 1 and blocks >= 1
        es = torch.empty((), dtype=dtype).element_size()
        assert offset_bytes % es == 0
        self.rows, self.cols, self.pitch, self.blocks = rows, cols, pitch, blocks
        self.block_stride = block_stride if blocks > 1 else 0
        assert blocks == 1 or block_stride >= (rows - 1) * pitch + cols
        span = (blocks - 1) * self.block_stride + (rows - 1) * pitch + cols
        a16 = 16 // es
        self.start = (lead * pitch + a16 - 1) // a16 * a16 + offset_bytes // es
        self.buf = torch.full((self.start + span + trail * pitch + a16,), sentinel, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.start * es
        self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        for w in self._windows(self.inside):
            w.fill_(True)
        self._bits0 = None

    def _windows(self, flat):
        return [flat[self.start + i * self.block_stride:].as_strided((self.rows, self.cols), (self.pitch, 1))
                for i in range(self.blocks)]

    def window(self, block=None):
        """The strided [rows, cols] view ([blocks, rows, cols] as a list-free view when blocks > 1 and block is None)."""
        if block is None and self.blocks > 1:
            return self.buf[self.start:].as_strided((self.blocks, self.rows, self.cols), (self.block_stride, self.pitch, 1))
        return self._windows(self.buf)[block or 0]

    def put(self, values):
        self.window().copy_(values.to(self.buf.device))
        return self

    def _bits(self):
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        return self.buf.view(it)

    def arm(self):
        """Remember the bit pattern of everything (call after ``put``, before the kernel runs)."""
        self._bits0 = self._bits().clone()
        return self

    def guard_report(self, what="C"):
        assert self._bits0 is not None, "arm() the canvas before the call"
        changed = (self._bits() != self._bits0) & ~self.inside
        if not bool(changed.any()):
            return None
        idx = changed.nonzero().flatten()[:6].cpu() - self.start
        where = ", ".join(f"(row {int(i) // self.pitch if i >= 0 else -((-int(i) + self.pitch - 1) // self.pitch)}, "
                          f"col {int(i) % self.pitch})" for i in idx)
        return (f"{what}: {int(changed.sum())} elements outside the [{self.rows}, {self.cols}] window (pitch {self.pitch}) "
                f"were written; first (relative to the window's origin): {where}")

    def assert_guard(self, what="C", context=""):
        msg = self.guard_report(what)
        assert msg is None, f"{context} {msg}"
