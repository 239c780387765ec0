"""References, cases, bounds and the comparison function for the row kernels of the DiT block (include/omh.h:
omh_layernorm_modulate, omh_rmsnorm_rope*, omh_gated_residual_*, and their backward forms in csrc/dit_backward.hip and
csrc/dit_backward2.hip).  Test infrastructure, not a test module; plain torch, importable without a GPU.  The exact
machinery (RNE to bf16, ulp_bf16, canvases with guards) is that of tests/gemm_exact_ref.py.

Every formula below is written ONCE and evaluated in two precisions: float64 is the reference, float32 (``dt``) is a
restatement of the kernel's arithmetic: sums along a row in the kernels' own order (``_rowsum``), sums over rows in
sequential order — both loops are spelled out because torch.cumsum carries its running sum in double on the CPU even
for fp32 tensors and would hide every rounding of an addition.  The restatement takes a ``defect`` (DEFECTS) so that the
host test can show that the comparison reports each of them at the shapes the GPU test runs.

A. Exact outputs (``torch.equal`` against float64) — the index test: which element, which batch element's vector,
which table entry.  The exactness condition, derived (asserted by ``check_exact`` for every generated case):
  gated residual     |xi|, |dx|, |dgate0| <= 64 and |y| <= 8 integers, gate = const + gate0 + gate1 a multiple of 1/2 with
                     |gate| <= 4.5  =>  xo = xi + y gate and dx gate are multiples of 1/2 below 2 (64 + 36) and 576
                     half-units; dgate = dgate0 + sum over a group's rows of dx y: an integer <= 64 + 512 rows_per_batch,
                     need < 2^24.  dy is ONE RNE of an exact value on both sides.
  RMSNorm, do_norm 0 |x| <= XMAX (8; 3 where norm2_max is emitted) and |dy| <= 8 integers, gain in {+-1/2, +-1, +-2},
                     out_scale in {1, 1/2, 1/4}, table entries (cos, sin) from PAIRS: multiples of 1/2 with
                     |cos| + |sin| <= 3/2.  x scale w is a multiple of 1/8 below 16; each product with a table entry a
                     multiple of 1/16 and the two-term sum at most 24 = 384 sixteenths: exact, then one RNE.
                     backward: unrope(dy) a multiple of 1/2 below 12; its product with x at most 96 = 192 half-units per
                     row, dweight = dw0 + sum over all rows: need 128 + 192 rows < 2^24; dx = g w a multiple of 1/4.
                     norm2_max: the stored values are multiples of 1/16 below 24 XMAX / 8, their squares multiples of
                     1/256, 128 of them per head: need 128 (48 XMAX)^2 < 2^24 — XMAX = 3 gives 2 654 208.
  LayerNorm dadd     |dy| <= 8 and |dadd0| <= 64 integers: need 64 + 8 (rows of a group) < 2^24.

B. Bounded outputs, where rsqrtf and the means make exactness impossible.  ``ref`` is the float64 formula; the condition
sum S is the same formula with every factor in absolute value and every subtraction turned into an addition (a sum of
signed terms becomes the sum of their magnitudes; ``x - mean`` becomes |x| + |mean|; the means of the backward become
means of magnitudes; rstd, a positive factor, stays): the magnitude the fp32 errors scale with.  delta = 2^-16 S.
  bf16 outputs       |got - ref| <= 0.5 ulp_bf16(|ref| + delta) + delta      (the half ulp is what one RNE costs)
  fp32 row outputs   |got - ref| <= delta                                     (LayerNorm dx)
  fp32 sums over rows|got - ref| <= k 2^-24 S, S summed over the rows         (dmul, fused dgate, normed dweight)
k per output (K_SUM) is four times the worst ratio of the fp32 restatement to float64 at the GPU test's shapes, rounded
up to a power of two: the GPU adds in another order, partly by atomics, and the error grows like a random walk.
tests/test_norm_exact_host.py measures the ratio again and asserts that K_SUM still covers it four times."""
import collections
import math
from types import SimpleNamespace as NS

import torch

import gemm_exact_ref as G
from gemm_exact_ref import Canvas, rne_bf16, truncate_bf16, ulp_bf16, assert_exact, mismatch_report  # noqa: F401

F64, F32 = torch.float64, torch.float32
SLACK = 2.0 ** -16
F32_EXACT = 1 << 24
EPS = float(torch.tensor(1e-6, dtype=F32))                  # the fp32 value the kernels receive
# measured by tests/test_norm_exact_host.py (restatement / (2^-24 S), worst over the cases): dmul 4.149, dgate 2.390,
# dweight 4.262; times four, rounded up to a power of two
K_SUM = {"dmul": 32.0, "dgate": 16.0, "dweight": 32.0}
WIDTHS = (4, 252, 256, 260, 1536, 1540, 5120, 5124, 8192)
PAIRS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.5, 0.5), (-0.5, 0.5), (1.0, -0.5), (0.5, -1.0))
GAINS = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
SCALES = (1.0, 0.5, 0.25)
XI_MAX, Y_MAX, DY_MAX, ACC0_MAX, GATE_MAX = 64, 8, 8, 64, 4.5
DEFECTS = ("neighbour_modulation", "stale_last_chunk", "no_eps", "mean_over_padded_width", "swap_h_w", "rotate_pad",
           "clamp_at_rope_len", "second_pair_first_entry", "drop_last_row", "dgate_wrong_group")

WORST = collections.defaultdict(float)      # entry -> worst |got - ref| / bound over its bounded outputs
COUNTS = collections.Counter()              # entry -> elements compared


def _up(x, m):
    return (x + m - 1) // m * m


def _gen(*seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(hash(tuple(int(s) for s in seed)) & 0x7FFFFFFF)
    return g


def _ints(g, shape, hi):
    return torch.randint(-hi, hi + 1, shape, generator=g, dtype=torch.int64).double()


def _pick(g, shape, values):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), shape, generator=g)]


def _randn(g, shape):
    return torch.randn(shape, generator=g, dtype=F64)


def check_exact(kind, rows_summed=0, xmax=8, bound=False):
    """Assert the exactness condition of the module docstring for one case; returns the largest partial sum in units."""
    if kind == "gated":
        top = ACC0_MAX + XI_MAX * Y_MAX * rows_summed
        assert 2 * (XI_MAX + Y_MAX * GATE_MAX) < F32_EXACT and 2 * XI_MAX * GATE_MAX < F32_EXACT
    elif kind == "rms":
        assert max(abs(a) + abs(b) for a, b in PAIRS) <= 1.5 and all((2 * a) % 1 == 0 and (2 * b) % 1 == 0 for a, b in PAIRS)
        assert 16 * (xmax * 2 * 1.5) < F32_EXACT
        top = 2 * ACC0_MAX + 2 * int(DY_MAX * 1.5 * xmax) * rows_summed          # half-units
        if bound:
            assert 128 * (48 * xmax) ** 2 < F32_EXACT, f"norm2_max: 128 squares of {48 * xmax} sixteenths"
    elif kind == "dadd":
        top = ACC0_MAX + DY_MAX * rows_summed
    else:
        raise ValueError(kind)
    assert top < F32_EXACT, f"{kind}: the largest partial sum can reach {top} units >= 2^24"
    return top


# ----------------------------------------------------------------------------------------------------------------------
# sums: float64 at once, float32 in sequential order
# ----------------------------------------------------------------------------------------------------------------------
def _rowsum(t):
    """[rows, n] -> [rows, 1].  fp32: in the order of the kernels — lane l of 64 adds the four elements of its float4
    chunks l, l + 64, ... one chunk after the other, then wave_sum's butterfly (lane distance 32, 16, ... 1).  A plain
    sequential fp32 sum over 5124 terms of one sign (the variance of the small-variance case) errs by 0.75 delta on its
    own, which no kernel here does: a lane adds at most 32 chunks."""
    if t.dtype == F64:
        return t.sum(-1, keepdim=True)
    rows, n = t.shape
    nv = n // 4
    v = t.reshape(rows, nv, 4)
    v4 = torch.zeros((rows, _up(nv, 64)), dtype=t.dtype)
    v4[:, :nv] = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    lanes = torch.zeros((rows, 64), dtype=t.dtype)
    for chunk in v4.reshape(rows, -1, 64).unbind(1):
        lanes = lanes + chunk
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, lane ^ o]
    return lanes[:, :1]


def _groupsum(t, b, ng, drop_last=False):
    """sum of the rows of t [rows, n] by group b [rows] -> [ng, n]"""
    if drop_last:
        t, b = t[:-1], b[:-1]
    out = torch.zeros((ng, t.shape[1]), dtype=t.dtype)
    if t.dtype == F64:
        return out.index_add_(0, b, t)
    for r, bb in enumerate(b.tolist()):
        out[bb] += t[r]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm + modulation, forward and backward (+ the next branch's gated residual backward)
# ----------------------------------------------------------------------------------------------------------------------
def ln_case(rows, dim, rpb, seed=0, small=False, dy_bf16=False, shared=False, wide=True):
    """x ~ 3 N(0, 1) + 0.5, or (small) k 2^-12 with |k| <= 8 so that eps = 1e-6 is of the size of the variance; modulation
    and gate vectors ~ N(0, 1/4) around mul_const = 1 / gate_const = 1/2; dy and the start of dadd integers (dadd exact);
    the starts of dx, dmul and dgate ~ N(0, 1).  shared: dmul / dadd are one vector for all row groups (dstride 0).
    wide: the strides of the per-group vectors are larger than the width."""
    g = _gen(seed, rows, dim, rpb, small)
    nb = (rows + rpb - 1) // rpb
    ng = 1 if shared else nb
    check_exact("dadd", rows if shared else min(rows, rpb))
    c = NS(rows=rows, dim=dim, rpb=rpb, nb=nb, ng=ng, small=small, dy_bf16=dy_bf16, shared=shared, eps=EPS, seed=seed,
           stride=dim + (8 if wide else 0), mul_const=1.0, gate_const=0.5)
    c.x = (_ints(g, (rows, dim), 8) * 2.0 ** -12 if small else 3.0 * _randn(g, (rows, dim)) + 0.5).float()
    for name, shape in (("mul0", (dim,)), ("mul1", (nb, dim)), ("add0", (dim,)), ("add1", (nb, dim)), ("gate0", (dim,)),
                        ("gate1", (nb, dim))):
        setattr(c, name, (0.5 * _randn(g, shape)).float())
    c.dy = _ints(g, (rows, dim), DY_MAX).to(torch.bfloat16 if dy_bf16 else F32)
    c.dx0 = _randn(g, (rows, dim)).float()
    c.y_next = _ints(g, (rows, dim), 4).to(torch.bfloat16)
    c.dmul0, c.dgate0 = _randn(g, (ng, dim)).float(), _randn(g, (nb, dim)).float()
    c.dadd0 = _ints(g, (ng, dim), ACC0_MAX).float()
    return c


def _batch_of(c, defect=None):
    b = torch.arange(c.rows) // c.rpb
    if defect == "neighbour_modulation" and c.rows > c.rpb:
        b[c.rpb] = 0                                        # the one row behind the first boundary
    return b


def _vec_sum(c, const, v0, v1, b, dt):
    """const + v0[col] + v1[b, col] per row, in the kernel's order, and the sum of the magnitudes"""
    m = torch.full((c.rows, c.dim), const, dtype=dt)
    a = m.abs()
    if v0 is not None:
        m, a = m + v0.to(dt)[None], a + v0.to(dt).abs()[None]
    if v1 is not None:
        m, a = m + v1.to(dt)[b], a + v1.to(dt).abs()[b]
    return m, a


def _ln_stats(c, dt, defect):
    x = c.x.to(dt)
    n = _up(c.dim, 256) if defect == "mean_over_padded_width" else c.dim
    mean = _rowsum(x) / n
    xc = x - mean
    rstd = torch.rsqrt(_rowsum(xc * xc) / c.dim + (0.0 if defect == "no_eps" else c.eps))
    return xc * rstd, (x.abs() + mean.abs()) * rstd, rstd


def ln_forward(c, dt=F64, defect=None, mul0=True, mul1=True, add0=True, add1=True):
    """y before the rounding to bf16, and its condition sum"""
    b = _batch_of(c, defect)
    xhat, sx, _ = _ln_stats(c, dt, defect)
    mul, amul = _vec_sum(c, c.mul_const, c.mul0 if mul0 else None, c.mul1 if mul1 else None, b, dt)
    add, aadd = _vec_sum(c, 0.0, c.add0 if add0 else None, c.add1 if add1 else None, b, dt)
    y, s = xhat * mul + add, sx * amul + aadd
    if defect == "stale_last_chunk":
        y = y.clone()
        y[:, -4:] = y[:, -8:-4]
    return NS(y=y, S=s)


def ln_backward(c, dt=F64, defect=None, nxt=False, gate=False, mul0=True, mul1=True):
    """dx (from dx0), dmul, dadd (from their starts) and, nxt / gate, dy_next before its rounding and dgate; S_* beside"""
    b = _batch_of(c)
    gb = torch.zeros_like(b) if c.shared else b
    xhat, sx, rstd = _ln_stats(c, dt, defect)
    mul, amul = _vec_sum(c, c.mul_const, c.mul0 if mul0 else None, c.mul1 if mul1 else None, b, dt)
    d = c.dy.to(dt)
    g, sg = d * mul, d.abs() * amul
    mg, smg = _rowsum(g) / c.dim, _rowsum(sg) / c.dim
    mgx, smgx = _rowsum(g * xhat) / c.dim, _rowsum(sg * sx) / c.dim
    drop = defect == "drop_last_row"
    o = NS()
    o.dx = c.dx0.to(dt) + rstd * (g - mg - xhat * mgx)
    o.S_dx = c.dx0.to(dt).abs() + rstd * (sg + smg + sx * smgx)
    o.dmul = c.dmul0.to(dt) + _groupsum(d * xhat, gb, c.ng, drop)
    o.S_dmul = c.dmul0.to(dt).abs() + _groupsum(d.abs() * sx, gb, c.ng)
    o.dadd = c.dadd0.to(dt) + _groupsum(d, gb, c.ng, drop)
    if nxt:
        gt, agt = _vec_sum(c, c.gate_const, c.gate0, c.gate1, b, dt)
        o.dy_next, o.S_dy_next = o.dx * gt, o.S_dx * agt
    if gate:
        yn = c.y_next.to(dt)
        bg = (b + 1) % c.nb if defect == "dgate_wrong_group" else b
        o.dgate = c.dgate0.to(dt) + _groupsum(o.dx * yn, bg, c.nb)
        o.S_dgate = c.dgate0.to(dt).abs() + _groupsum(o.S_dx * yn.abs(), b, c.nb)
    return o


def ln_rows_per_wave(rows, forced=None):
    """omh_layernorm_modulate's choice, restated from csrc/dit_elementwise.hip"""
    if forced is not None:
        return forced if forced in (1, 2, 8, 16) else 4
    return 1 if rows <= 4096 else (2 if rows < 16384 else (4 if rows < 24576 else 16))


def ln_bwd2_rows_per_wg(rows):
    """ln_rows_per_wg of csrc/dit_backward2.hip"""
    return 16 if rows >= 4096 else 8


def ln_bwd2_geometry(rows, rpb):
    """(row groups, workgroups per group) of ln_bwd2_kernel; the workspace holds groups * workgroups * 3 * dim floats"""
    return (rows + rpb - 1) // rpb, (rpb + ln_bwd2_rows_per_wg(rows) - 1) // ln_bwd2_rows_per_wg(rows)


# ----------------------------------------------------------------------------------------------------------------------
# RMSNorm + 3-axis RoPE, forward and backward
# ----------------------------------------------------------------------------------------------------------------------
def rms_case(dim, hd=0, seq_len=13, grids=((2, 2, 3), (1, 1, 13)), rope_len=5, seed=0, exact=True, x_bf16=True,
             dy_bf16=False, nseg=1, xmax=8, rows=None, wide=True):
    """hd == 0: no rotary table (rows free).  Else rows = len(grids) * seq_len; the table has rope_len rows and ONE MORE
    that holds NaN (what a clamp at rope_len instead of rope_len - 1 would read).
    exact: the integer inputs and the table of exactly representable pairs of the module docstring (do_norm = 0);
    otherwise x, dy ~ N(0, 1) (rounded to bf16 where the entry reads bf16), gains ~ 1 + 0.3 N(0, 1), a table of real
    rotations and out_scale in {1, 128^-1/2 log2 e} (do_norm = 1)."""
    g = _gen(seed, dim, hd, seq_len, rope_len, exact, nseg)
    rows = len(grids) * seq_len if hd else rows
    if hd:
        assert hd % 4 == 0 and dim % hd == 0 and all(f * h * w <= seq_len for f, h, w in grids)
    c = NS(rows=rows, dim=dim, hd=hd, seq_len=seq_len, rope_len=rope_len, exact=exact, x_bf16=x_bf16, dy_bf16=dy_bf16,
           nseg=nseg, eps=EPS, do_norm=0 if exact else 1, seed=seed, xmax=xmax, pad=8 if wide else 0)
    c.grid = torch.tensor(grids, dtype=torch.int32) if hd else None
    if exact:
        check_exact("rms", rows, xmax, bound=xmax < 8)
    xt, gt = (torch.bfloat16 if x_bf16 else F32), (torch.bfloat16 if dy_bf16 else F32)
    c.x, c.dy, c.w, c.scale, c.dw0 = [], [], [], [], []
    for s in range(nseg):
        c.x.append((_ints(g, (rows, dim), xmax) if exact else _randn(g, (rows, dim))).to(xt))
        c.dy.append((_ints(g, (rows, dim), DY_MAX) if exact else _randn(g, (rows, dim))).to(gt))
        c.w.append((_pick(g, (dim,), GAINS) if exact else 1.0 + 0.3 * _randn(g, (dim,))).float())
        c.scale.append(SCALES[(seed + s) % 3] if exact else (1.0, float(torch.tensor(128 ** -0.5 * math.log2(math.e), dtype=F32)))[(seed + s) % 2])
        c.dw0.append((_ints(g, (dim,), ACC0_MAX) if exact else _randn(g, (dim,))).float())
    if hd:
        hc = hd // 2
        if exact:
            pr = torch.tensor(PAIRS, dtype=F64)[torch.randint(0, len(PAIRS), (rope_len, hc), generator=g)]
            cos, sin = pr[..., 0], pr[..., 1]
        else:
            ang = 6.283185307179586 * torch.rand((rope_len, hc), generator=g, dtype=F64)
            cos, sin = torch.cos(ang), torch.sin(ang)
        nan = torch.full((1, hc), float("nan"), dtype=F64)
        c.cos, c.sin = torch.cat([cos, nan]).float(), torch.cat([sin, nan]).float()
    return c


def rope_entries(c, dt=F64, defect=None):
    """(cos, sin) per (row, complex pair) [rows, dim / 2], restated from rmsnorm_rope_row: (1, 0) where a token is not
    rotated"""
    if not c.hd:
        return None
    r = torch.arange(c.rows)
    b, s = r // c.seq_len, r % c.seq_len
    gf, gh, gw = (c.grid[b, i].long() for i in range(3))
    rot = torch.ones_like(s, dtype=torch.bool) if defect == "rotate_pad" else s < gf * gh * gw
    pos = torch.stack([s // (gh * gw), (s // gw) % gh, s % gw], 1)              # [rows, 3]: f, h, w
    if defect == "swap_h_w":
        pos = pos[:, [0, 2, 1]]
    hc = c.hd // 2
    c3 = hc // 3
    cf = hc - 2 * c3
    pc = (torch.arange(c.dim // 2) * 2 % c.hd) // 2                             # pair within its head
    if defect == "second_pair_first_entry":
        pc = pc - (torch.arange(c.dim // 2) % 2)
    axis = torch.where(pc < cf, 0, torch.where(pc < cf + c3, 1, 2))
    p = pos[:, axis]                                                            # [rows, dim / 2]
    idx = torch.clamp(p, max=c.rope_len if defect == "clamp_at_rope_len" else c.rope_len - 1) * hc + pc[None]
    one, zero = torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
    cs = torch.where(rot[:, None], c.cos.to(dt).flatten()[idx], one)
    sn = torch.where(rot[:, None], c.sin.to(dt).flatten()[idx], zero)
    return cs, sn


def _rotate(t, st, cs, sn, sign):
    """rotate the pairs (t[2p], t[2p + 1]) by sign * theta; st: magnitudes"""
    re, im, sre, sim = t[:, 0::2], t[:, 1::2], st[:, 0::2], st[:, 1::2]
    nr, ni = re * cs - sign * (im * sn), sign * (re * sn) + im * cs
    out = torch.stack([nr, ni], -1).reshape(t.shape)
    sout = torch.stack([sre * cs.abs() + sim * sn.abs(), sre * sn.abs() + sim * cs.abs()], -1).reshape(t.shape)
    return out, sout


def rms_forward(c, seg=0, dt=F64, defect=None, out_scale=None, gain=True):
    """y of one segment before the rounding to bf16, and its condition sum"""
    x = c.x[seg].to(dt)
    scale = c.scale[seg] if out_scale is None else out_scale
    rinv = (torch.rsqrt(_rowsum(x * x) / c.dim + c.eps) if c.do_norm else torch.ones((c.rows, 1), dtype=dt)) * scale
    t, st = x * rinv, x.abs() * rinv
    if gain:
        t, st = t * c.w[seg].to(dt), st * c.w[seg].to(dt).abs()
    if c.hd:
        cs, sn = rope_entries(c, dt, defect)
        t, st = _rotate(t, st, cs, sn, 1.0)
    return NS(y=t, S=st)


def norm2_max(c, y_bf16):
    """[samples, heads, 1]: the maximum over a sample's rows of the per-head sum of squares of the stored values"""
    v = y_bf16.double().reshape(c.rows // c.seq_len, c.seq_len, c.dim // 128, 128)
    return G.exact_f32((v * v).sum(-1).amax(1))


def rms_backward(c, seg=0, dt=F64, defect=None, gain=True):
    """dx before its rounding to bf16 and dweight (from dw0), with their condition sums"""
    x, d = c.x[seg].to(dt), c.dy[seg].to(dt)
    r = torch.rsqrt(_rowsum(x * x) / c.dim + c.eps) if c.do_norm else torch.ones((c.rows, 1), dtype=dt)
    g, sg = d, d.abs()
    if c.hd:
        cs, sn = rope_entries(c, dt, defect)
        g, sg = _rotate(g, sg, cs, sn, -1.0)
    z = torch.zeros(c.rows, dtype=torch.long)
    o = NS()
    o.dw = c.dw0[seg].to(dt)[None] + _groupsum(g * x * r, z, 1, defect == "drop_last_row")
    o.S_dw = c.dw0[seg].to(dt).abs()[None] + _groupsum(sg * x.abs() * r, z, 1)
    if gain:
        g, sg = g * c.w[seg].to(dt), sg * c.w[seg].to(dt).abs()
    if c.do_norm:
        coef, scoef = _rowsum(x * g) / c.dim * r * r * r, _rowsum(x.abs() * sg) / c.dim * r * r * r
        o.dx, o.S_dx = r * g - x * coef, r * sg + x.abs() * scoef
    else:
        o.dx, o.S_dx = g, sg
    return o


def pair_takes_row_form(rows, dim, hd, option):
    """omh_rmsnorm_rope_bf16_pair with a rotary table: True when the one-wave-per-row kernel runs (RMS_PAIR_ROW = option)"""
    off, on = option == "0", option == "1"
    return (not off) and hd > 0 and 256 % hd == 0 and dim <= 20 * 256 and (on or rows >= 8192)


# ----------------------------------------------------------------------------------------------------------------------
# gated residual
# ----------------------------------------------------------------------------------------------------------------------
def gated_case(rows, dim, rpb, seed=0, wide=True):
    g = _gen(seed, rows, dim, rpb, 77)
    nb = (rows + rpb - 1) // rpb
    check_exact("gated", min(rows, rpb))
    c = NS(rows=rows, dim=dim, rpb=rpb, nb=nb, seed=seed, stride=dim + (12 if wide else 0))
    c.xi = _ints(g, (rows, dim), XI_MAX).float()
    c.y = _ints(g, (rows, dim), Y_MAX).to(torch.bfloat16)
    c.gate_const = 0.5 * float(torch.randint(-1, 2, (1,), generator=g))
    c.gate0, c.gate1 = (0.5 * _ints(g, (dim,), 4)).float(), (0.5 * _ints(g, (nb, dim), 4)).float()
    c.dgate0 = _ints(g, (nb, dim), ACC0_MAX).float()
    return c


def gated_reference(c, defect=None):
    """xo (xi as the input), and dy (bf16) / dgate with xi as the incoming gradient dx: all exact"""
    b = torch.arange(c.rows) // c.rpb
    if defect == "neighbour_modulation" and c.rows > c.rpb:
        b[c.rpb] = 0
    gate = c.gate_const + c.gate0.double()[None] + c.gate1.double()[b]
    assert float(gate.abs().max()) <= GATE_MAX
    xi, y = c.xi.double(), c.y.double()
    bg = (b + 1) % c.nb if defect == "dgate_wrong_group" else b
    return NS(xo=G.exact_f32(xi + y * gate), dy=rne_bf16(xi * gate),
              dgate=G.exact_f32(c.dgate0.double() + _groupsum(xi * y, bg, c.nb)))


# ----------------------------------------------------------------------------------------------------------------------
# bounds and the comparison
# ----------------------------------------------------------------------------------------------------------------------
def bound_bf16(ref, S):
    d = SLACK * S
    return 0.5 * ulp_bf16(ref.abs() + d) + d


def bound_row(S):
    return SLACK * S


def bound_sum(S, what):
    return K_SUM[what] * 2.0 ** -24 * S


def ratio_to_bound(got, ref, bound):
    """|got - ref| / bound per element: 0 where they agree exactly, inf where got is not finite"""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(2.0 ** -300))
    return torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))


def compare(entry, what, got, ref, bound=None, context="", record=True):
    """None when ``got`` holds: equal to ``ref`` element for element (bound None: same dtype, a NaN never equals), or
    |got - ref| <= bound per element.  Else one line that names the count of wrong elements and the worst one: its index,
    values and ratio to the bound.  The worst ratio per entry is kept in WORST."""
    got = got.detach().cpu()
    if record:
        COUNTS[entry] += got.numel()
    if bound is None:
        msg = mismatch_report(got, ref, None, what)
        return None if msg is None else f"[{entry}] {context} {msg}"
    assert got.shape == ref.shape, f"[{entry}] {context} {what}: got {tuple(got.shape)}, want {tuple(ref.shape)}"
    ratio = ratio_to_bound(got, ref, bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if record:
        WORST[entry] = max(WORST[entry], worst)
    if worst <= 1.0:
        return None
    idx = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), got.shape))
    return (f"[{entry}] {context} {what}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements miss their bound; worst at "
            f"{idx}: got {float(got[idx])!r}, want {float(ref[idx])!r}, bound {float(bound[idx]):.3e}, ratio {worst:.3f}")


def bad_fraction(got, ref, bound):
    return float((ratio_to_bound(got, ref, bound) > 1.0).double().mean())


def summary_line():
    return "[measured] worst ratio to the bound: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items()))


# ----------------------------------------------------------------------------------------------------------------------
# the cases: one list per family, shared by tests/test_norm_exact_host.py and tests/test_gpu_norm_exact.py
# ----------------------------------------------------------------------------------------------------------------------
# (rows, rows_per_batch): a batch boundary inside a wave's rows and an incomplete last batch element (17 = 7 + 7 + 3), one
# row per batch element, a batch element longer than the input, one row, one complete batch element in two workgroups
ROWS_RPB = ((17, 7), (5, 1), (3, 37), (1, 1), (17, 37))


def _shape_cases():
    out = []
    for i, dim in enumerate(WIDTHS):
        out.append(dict(dim=dim, rows=17, rpb=7, seed=i))
        rows, rpb = ROWS_RPB[1 + i % 4]
        out.append(dict(dim=dim, rows=rows, rpb=rpb, seed=100 + i))
    for i, dim in enumerate((260, 1540, 5124)):             # one small-variance case per width class
        out.append(dict(dim=dim, rows=17, rpb=7, seed=200 + i, small=True))
    return out


def ln_fwd_cases():
    """dict(dim, rows, rpb, seed[, small][, forced]); ``forced``: the LN_RPW option"""
    out = _shape_cases()
    for rows in (4096, 4097, 16383, 16384, 24575, 24576):   # the automatic choice of rows per wave, both sides
        out.append(dict(dim=8, rows=rows, rpb=101, seed=300))
    for dim in (260, 5124):
        for f in (1, 2, 4, 8, 16):
            out.append(dict(dim=dim, rows=303, rpb=37, seed=400, forced=f))
    return out


def ln_bwd_cases():
    return _shape_cases() + [dict(dim=260, rows=17, rpb=7, seed=500, shared=True)]


LN2_VARIANTS = ("plain", "next", "gate")


def ln_bwd2_cases():
    """dict(dim, rows, rpb, seed, variant, dy_bf16, deferred[, small][, shared][, long]).  Partials per column of the second stage:
    113 | 128 | 129 | 300 workgroups of 8 rows in one row group (the 8-deep unrolled loop needs more than 112)."""
    out = []
    for i, cs in enumerate(_shape_cases()):
        out.append(dict(cs, variant=LN2_VARIANTS[i % 3], dy_bf16=bool((i // 3) % 2), deferred=bool((i // 2) % 2)))
    for i, rows in enumerate((4095, 4096)):                 # 8 -> 16 rows per workgroup
        for j, rpb in enumerate((8, 9, 16, 17)):
            out.append(dict(dim=8, rows=rows, rpb=rpb, seed=600 + j, variant=LN2_VARIANTS[(i + j) % 3], dy_bf16=bool(j % 2), deferred=False))
    out.append(dict(dim=260, rows=17, rpb=7, seed=610, variant="gate", dy_bf16=False, deferred=False, shared=True))
    out.append(dict(dim=8, rows=3 * 904, rpb=904, seed=611, variant="next", dy_bf16=True, deferred=False, shared=True))   # 3 x 113
    for i, n in enumerate((113, 128, 129, 300)):
        out.append(dict(dim=8, rows=8 * n + (3 if i % 2 else 0), rpb=8 * n, seed=620 + i, variant=LN2_VARIANTS[i % 3], dy_bf16=bool(i % 2),
                        deferred=False))
    for i, dim in enumerate((5460, 5464, 8192)):            # the fused gate gradient: 3 * dim * 4 bytes of LDS, above 64 KB from 5464
        out.append(dict(dim=dim, rows=17, rpb=7, seed=630 + i, variant="gate", dy_bf16=bool(i % 2), deferred=False))
    # every instantiation the dispatcher can pick (chunks x dy type x variant x rows per workgroup) is launched: the full
    # cross at one width per chunk class and at 8192, and, for the 32-chunk kernels, at the fewest rows (4096) that take
    # 16 rows per workgroup (three full row groups of 1365 rows and one of a single row).  ``long`` marks those.
    for k, dim in enumerate((260, 1540, 5124, 8192)):
        for j, variant in enumerate(LN2_VARIANTS):
            for bf in (False, True):
                out.append(dict(dim=dim, rows=17, rpb=7, seed=640 + 10 * k + 2 * j + bf, variant=variant, dy_bf16=bf, deferred=False))
    for j, variant in enumerate(LN2_VARIANTS):
        for bf in (False, True):
            out.append(dict(dim=5124, rows=4096, rpb=1365, seed=690 + 2 * j + bf, variant=variant, dy_bf16=bf, deferred=False, long=True))
    return out


def host_cases(cases):
    """what tests/test_norm_exact_host.py restates of a case list: everything but the long cases that another long case
    of the same shape contains (the gate variant computes dx, dmul, dadd, dy_next and dgate, a superset, and dy holds the
    same integers in fp32 and in bf16)"""
    return [cs for cs in cases if not cs.get("long") or (cs["variant"] == "gate" and cs["dy_bf16"])]


ROPE_SHAPES = ((256, 128), (384, 128), (128, 64), (192, 64), (16, 8), (24, 8), (192, 96), (288, 96), (24, 12), (36, 12), (4, 4),
               (252, 12), (260, 52), (1536, 128), (1540, 20), (5120, 128), (5124, 12), (8192, 128))
GRIDS = (dict(seq_len=13, grids=((2, 2, 3), (1, 1, 13)), rope_len=5),     # a pad token; 1 x 1 x n = seq_len; w past rope_len
         dict(seq_len=12, grids=((3, 2, 2), (2, 3, 2)), rope_len=2))      # f h w = seq_len twice; f and h past rope_len


def rms_cases(exact, nseg=1):
    """keyword sets for rms_case: every ROPE_SHAPES entry with one of GRIDS, and every width without a rotary table"""
    out = []
    for i, (dim, hd) in enumerate(ROPE_SHAPES):
        out.append(dict(dim=dim, hd=hd, seed=i, exact=exact, nseg=nseg, **GRIDS[i % 2]))
    for i, dim in enumerate(WIDTHS):
        out.append(dict(dim=dim, hd=0, rows=(17, 5, 3, 1)[i % 4], seed=50 + i, exact=exact, nseg=nseg))
    return out
