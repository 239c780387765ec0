"""Exact reference, cases and assertions for the VAE convolution entry (include/omh.h: omh_conv_cl_bf16) and the per-voxel
RMS norm + SiLU behind it (omh_rms_silu_cl, _f32in, _split3, _pair and the fused epilogue of the stream kernels).  Test
infrastructure, not a test module; plain torch, importable without a GPU.  RNE to bf16, ulp_bf16, the canvases and the
bounded comparison are those of tests/gemm_exact_ref.py and tests/norm_exact_ref.py.

A. The convolution, exact.  The reference is the formula of omh_conv_args written with index arithmetic (``gather``): the
source index S(i), zero outside the (upsampled) image, stride_t, stride_hw and the split_n frame interleave — no padded
tensor and no torch convolution, so it states the contract and not torch's padding.  Operands make fp32 accumulation exact
(asserted per case by ``check_exact``):
  plain   x, w integers in [-3, 3], bias in [-8, 8], residual in [-64, 64]  =>  |acc + bias + resid| <= 9 K + 72 < 2^24
          with K = KT KH KW Cin: every partial sum is an integer below 2^24 in any order.
  pair    x and w are built directly in the pair layout [hi(16) | lo(16)] per 16 real channels, hi an integer in [-2, 2], lo a
          multiple of 2^-9 in [-2, 2] 2^-9 (integers alone would make lo = 0 and the test blind).  The contract is
          x_hi w_hi + x_lo w_hi + x_hi w_lo on whatever pairs are given; all terms are multiples of 2^-9 and one real channel of
          one tap contributes at most 4 + 2 (2 * 2) 2^-9 = 2056 units of 2^-9: K_real 2056 + 72 * 512 < 2^24  (K_real < 8 158:
          384 real channels x 9 taps fit, 384 x 27 do not).
``torch.equal`` against float64 (one RNE for bf16 outputs) is then the assertion for every route.

B. The norm, bounded.  ref = x / max(||x||, 1e-12) sqrt(C) gamma (then SiLU) in float64; S is the same formula with every
factor in absolute value (|x| inv |gamma|, times sigmoid(z), a positive factor, with SiLU); delta = K_NORM 2^-16 S.
  bf16 outputs         |got - ref| <= 0.5 ulp_bf16(|ref| + delta) + delta        (norm_exact_ref.bound_bf16's form)
  hi + lo of a split   |got - ref| <= delta
K_NORM per kind is four times the worst ratio to 2^-16 S of ``norm_restated`` — the kernel's arithmetic in fp32 on the CPU, in
its summation order, SiLU as x * rcp(1 + exp2(-log2(e) x)) — rounded up to a power of two.  The kernel takes the raw
v_sqrt_f32 / v_rcp_f32 / v_exp_f32 (documented to 1 ulp); the restatement evaluates them correctly rounded and again with
every one of them displaced by one ulp in the directions that add up.  tests/test_conv_exact_host.py asserts the derivation.
Where do_silu = 0 and ||x|| C^-1/2 is a power of two the quotient is a power of two up to a few fp32 ulps and x inv gamma
lies that close to a bf16 value: those are held with ``torch.equal``."""
import math
from types import SimpleNamespace as NS

import torch

import gemm_exact_ref as G
import norm_exact_ref as N
from gemm_exact_ref import Canvas, rne_bf16, truncate_bf16, ulp_bf16, exact_f32      # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
F32_EXACT = 1 << 24
XW_MAX, BIAS_MAX, RES_MAX = 3, 8, 64
PAIR_HI_MAX, PAIR_LO_MAX, PAIR_UNIT = 2, 2, 2.0 ** -9
PAIR_TERM_UNITS = PAIR_HI_MAX * PAIR_HI_MAX * 512 + 2 * PAIR_HI_MAX * PAIR_LO_MAX       # 2056 units of 2^-9
# measured by tests/test_conv_exact_host.py (worst restatement / (2^-16 S) over the GPU test's shapes): bf16 0.0736,
# split 0.5343 (of which 0.5 is the rounding of lo: 2^-8 of 2^-8); times four, rounded up to a power of two
K_NORM = {"bf16": 0.5, "split": 4.0}


def _gen(*seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(hash(tuple(int(s) for s in seed)) & 0x7FFFFFFF)
    return g


def _ints(g, shape, hi):
    return torch.randint(-hi, hi + 1, shape, generator=g, dtype=torch.int64).double()


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def make_case(Cin, Cout, T, H, W, KT=3, KH=3, KW=3, kind="same", out_f32=False, bias=False, resid=None, split_n=0, pair=False,
              norm=False, norm_only=False, surplus=0, odd=False, seed=0):
    """One call of omh_conv_cl_bf16, tensors on the CPU.  ``kind``:
      same    stride 1, pad K // 2 in h and w, Tin = T + KT - 1 (the history frames first); H, W are the output's
      down    stride_hw 2, no pad: Hin = 2 H (the last tap is the zero pad) or, ``odd``, 2 H + 1 (it is a real row)
      tstride stride_t 2, Tin = 2 (T - 1) + KT
      up2     the folded nearest-2x upsample: H, W are the INPUT's, the output is 2 H x 2 W
    ``Cin`` is the channel count the entry sees (pair: twice the real one).  ``resid``: None, "bf16" or "f32".
    ``surplus`` frames of NaN follow the frames the contract reads.  ``norm``: norm_gamma / norm_out are passed."""
    c = NS(Cin=Cin, Cout=Cout, KT=KT, KH=KH, KW=KW, stride_t=1, stride_hw=1, pad_h=KH // 2, pad_w=KW // 2, up2=0,
           out_f32=int(out_f32), split_n=split_n, pair=int(pair), has_bias=bool(bias), resid_kind=resid, norm=bool(norm),
           norm_only=bool(norm_only), kind=kind, seed=seed, Tout=T, Hout=H, Wout=W, Hin=H, Win=W)
    if kind == "down":
        c.stride_hw, c.pad_h, c.pad_w = 2, 0, 0
        c.Hin, c.Win = 2 * H + int(odd), 2 * W + int(odd)
    elif kind == "tstride":
        c.stride_t = 2
    elif kind == "up2":
        c.up2, c.Hout, c.Wout = 1, 2 * H, 2 * W
    else:
        assert kind == "same"
    used = (T - 1) * c.stride_t + KT
    c.Tin, c.used_frames = used + surplus, used
    c.taps = KT * KH * KW
    c.K = c.taps * Cin
    c.M = c.Tout * c.Hout * c.Wout
    c.fmul = Cout // split_n if split_n else 1
    c.cch = split_n if split_n else Cout
    c.out_shape = (c.Tout * c.fmul, c.Hout, c.Wout, c.cch)
    c.resid_f32 = int(resid == "f32")
    g = _gen(seed, Cin, Cout, T, H, W, KT, KH, KW, split_n, pair)
    if pair:
        assert Cin % 32 == 0
        c.x = _pair_operand(g, (used, c.Hin, c.Win), Cin)
        c.w = _pair_operand(g, (Cout, c.taps), Cin).reshape(Cout, c.K)
    else:
        c.x = _ints(g, (used, c.Hin, c.Win, Cin), XW_MAX).to(BF16)
        c.w = _ints(g, (Cout, c.K), XW_MAX).to(BF16)
    if surplus:
        c.x = torch.cat([c.x, torch.full((surplus, c.Hin, c.Win, Cin), float("nan"), dtype=BF16)])
    c.bias = _ints(g, (Cout,), BIAS_MAX).float() if bias else None
    c.resid = None if resid is None else _ints(g, c.out_shape, RES_MAX).to(F32 if resid == "f32" else BF16)
    c.gamma = ((torch.rand(Cout, generator=g, dtype=F64) + 0.5) * (1 - 2 * torch.randint(0, 2, (Cout,), generator=g))).float() if norm else None
    check_exact(c)
    return c


def _pair_operand(g, lead, Cin2):
    """[*lead, Cin2] bf16 in the pair layout: per 16 real channels [hi(16) | lo(16)]"""
    cr = Cin2 // 2
    hi = _ints(g, lead + (cr // 16, 1, 16), PAIR_HI_MAX)
    lo = _ints(g, lead + (cr // 16, 1, 16), PAIR_LO_MAX) * PAIR_UNIT
    t = torch.cat([hi, lo], -2).reshape(lead + (Cin2,))
    out = t.to(BF16)
    assert torch.equal(out.double(), t)
    return out


def pair_halves(t):
    """[..., Cin2] in the pair layout -> (hi, lo), each [..., Cin2 / 2]"""
    v = t.reshape(t.shape[:-1] + (t.shape[-1] // 32, 2, 16))
    return v[..., 0, :].reshape(t.shape[:-1] + (-1,)), v[..., 1, :].reshape(t.shape[:-1] + (-1,))


def check_exact(c):
    """Assert the exactness condition of the module docstring for one case; returns the largest partial sum in units."""
    assert c.Cin % 8 == 0 and c.used_frames <= c.Tin
    used = c.x[:c.used_frames].double()
    tail = BIAS_MAX * c.has_bias + RES_MAX * (c.resid_kind is not None)
    if c.pair:
        (xh, xl), (wh, wl) = pair_halves(used), pair_halves(c.w.double())
        for hi, lo in ((xh, xl), (wh, wl)):
            assert float(hi.abs().max()) <= PAIR_HI_MAX and torch.equal(hi, hi.round())
            assert float(lo.abs().max()) <= PAIR_LO_MAX * PAIR_UNIT and torch.equal(lo / PAIR_UNIT, (lo / PAIR_UNIT).round())
        top = c.K // 2 * PAIR_TERM_UNITS + tail * 512
        assert top < F32_EXACT, f"pair: {c.K // 2} real products of {PAIR_TERM_UNITS} units of 2^-9 reach {top} >= 2^24"
    else:
        for t in (used, c.w.double()):
            assert float(t.abs().max()) <= XW_MAX and torch.equal(t, t.round())
        top = XW_MAX * XW_MAX * c.K + tail
        assert top < F32_EXACT, f"K = {c.K}: |acc + bias + resid| can reach {top} >= 2^24"
    if c.bias is not None:
        assert float(c.bias.abs().max()) <= BIAS_MAX and torch.equal(c.bias, c.bias.round())
    if c.resid is not None:
        assert float(c.resid.double().abs().max()) <= RES_MAX and torch.equal(c.resid.double(), c.resid.double().round())
    return top


# ----------------------------------------------------------------------------------------------------------------------
# the float64 reference, from the formula of omh_conv_args
# ----------------------------------------------------------------------------------------------------------------------
def gather(c, x64, kt, dy, dx, defect=None):
    """x[to stride_t + kt][S(yo stride_hw + dy - pad_h)][S(xo stride_hw + dx - pad_w)][:] for every output voxel,
    [Tout, Hout, Wout, C], zero where the tap lies outside the (upsampled) image.  ``defect``: see DEFECTS."""
    up = 1 if c.up2 else 0
    heff, weff = c.Hin << up, c.Win << up
    ti = torch.arange(c.Tout) * c.stride_t + kt
    iy = torch.arange(c.Hout) * c.stride_hw + dy - c.pad_h
    ix = torch.arange(c.Wout) * c.stride_hw + dx - c.pad_w
    oky, okx = (iy >= 0) & (iy < heff), (ix >= 0) & (ix < weff)
    if defect == "pad_row_read":
        oky = iy >= 0                                       # the row past the image: what lies there instead of zero
    sh = up if defect == "up2_plus_one" else 0
    sy, sx = ((iy + sh) >> up).clamp(0, c.Hin - 1), ((ix + sh) >> up).clamp(0, c.Win - 1)
    assert int(ti.max()) < c.used_frames, "a frame past the ones the contract reads"
    g = x64[ti][:, sy][:, :, sx]
    return torch.where((oky[:, None] & okx[None, :])[None, :, :, None], g, torch.zeros((), dtype=F64))


def _contract(c, x64, w64, defect=None):
    """sum over taps and channels, [Tout, Hout, Wout, Cout]"""
    w5 = w64.reshape(c.Cout, c.KT, c.KH, c.KW, -1)
    acc = torch.zeros((c.Tout, c.Hout, c.Wout, c.Cout), dtype=F64)
    for kt in range(c.KT):
        for dy in range(c.KH):
            for dx in range(c.KW):
                acc += gather(c, x64, kt, dy, dx, defect) @ w5[:, kt, dy, dx].t()
    if defect == "row_wrap":                                # voxel (0, 1, 0): its left tap took the previous row's last voxel
        t0, y0 = 0, 1
        for kt in range(c.KT):
            for dy in range(c.KH):
                row = y0 * c.stride_hw + dy - c.pad_h - 1
                if 0 <= row < c.Hin:
                    acc[t0, y0, 0] += w5[:, kt, dy, 0] @ x64[t0 * c.stride_t + kt, row, c.Win - 1]
    if defect == "frame_wrap":                              # voxel (1, 0, 1): the row above the image came from the frame before
        t0, x0 = 1, 1
        for kt in range(c.KT):
            for dx in range(c.KW):
                col = x0 * c.stride_hw + dx - c.pad_w
                if 0 <= col < c.Win:
                    acc[t0, 0, x0] += w5[:, kt, 0, dx] @ x64[t0 * c.stride_t + kt - 1, c.Hin - 1, col]
    if defect == "drop_k_block":                            # 64 k from the centre tap on, missing for voxels 0..31 x couts 0..31
        xk = torch.cat([gather(c, x64, kt, dy, dx) for kt in range(c.KT) for dy in range(c.KH) for dx in range(c.KW)], -1)
        k0 = c.taps // 2 * w5.shape[-1]
        part = xk.reshape(c.M, -1)[:32, k0:k0 + 64] @ w64[:32, k0:k0 + 64].t()
        acc.reshape(c.M, c.Cout)[:32, :32] -= part
    return acc


def accumulate(c, defect=None):
    x64, w64 = c.x[:c.used_frames].double(), c.w.double()
    if not c.pair:
        return _contract(c, x64, w64, defect)
    (xh, xl), (wh, wl) = pair_halves(x64), pair_halves(w64.reshape(c.Cout, c.taps, c.Cin))
    acc = _contract(c, xh, wh) + _contract(c, xl, wh) + _contract(c, xh, wl)
    if defect == "lo_lo":
        acc = acc + _contract(c, xl, wl)
    return acc


def interleave(c, v, defect=None):
    """[Tout, Hout, Wout, Cout] -> out_shape: output frame to * f + j holds channels [j split_n, (j + 1) split_n)"""
    if not c.split_n:
        return v
    v = v.reshape(c.Tout, c.Hout, c.Wout, c.fmul, c.split_n).permute(0, 3, 1, 2, 4)
    if defect == "split_swap":
        v = v.flip(1)
    return v.reshape(c.out_shape)


def reference(c, defect=None):
    """NS(y: what the entry must leave in y, in y's dtype; y64: the same before the store's rounding)"""
    v = accumulate(c, defect)
    if c.bias is not None:
        b = c.bias.double()
        v = v + (b.roll(-1) if defect == "bias_next" else b)
    v = interleave(c, v, defect)
    if c.resid is not None:
        v = v + c.resid.double()
        if defect == "resid_twice":                         # on the last, ragged 128-voxel tile
            flat = v.reshape(-1, c.cch)
            m0 = (flat.shape[0] - 1) // 128 * 128
            flat[m0:] += c.resid.double().reshape(-1, c.cch)[m0:]
    if c.out_f32:
        return NS(y=exact_f32(v), y64=v)
    return NS(y=truncate_bf16(v) if defect == "truncate" else rne_bf16(v), y64=v)


DEFECTS = ("row_wrap", "frame_wrap", "drop_k_block", "truncate", "bias_next", "resid_twice", "up2_plus_one", "pad_row_read",
           "split_swap", "lo_lo")


def mismatch(got, want, c=None, what="y", limit=4):
    """None when ``got`` equals ``want`` element for element (dtype and shape too; a NaN never equals), else a line with the
    count of wrong elements and the first ones as (t, y, x, co) with got and want."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{what}: got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = ~(got == want)
    idx = bad.nonzero()[:limit]
    first = ", ".join(f"(t {i[0]}, y {i[1]}, x {i[2]}, co {i[3]}: got {float(got[tuple(i)])!r}, want {float(want[tuple(i)])!r})"
                      for i in idx.tolist())
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first: {first}"


def assert_exact(got, want, c=None, what="y", context=""):
    msg = mismatch(got, want, c, what)
    assert msg is None, f"{context} {msg}"


class Frozen:
    """An input whose bits must not change: ``check`` names the first changed element."""

    def __init__(self, t, what):
        self.t, self.what = t, what
        self.bits = self._bits().clone()

    def _bits(self):
        return self.t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.t.element_size()]).flatten()

    def report(self):
        ch = self._bits() != self.bits
        if not bool(ch.any()):
            return None
        return f"{self.what} (an input): {int(ch.sum())} elements changed, first at flat index {int(ch.nonzero()[0])}"

    def check(self, context=""):
        msg = self.report()
        assert msg is None, f"{context} {msg}"


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch of csrc/vae_conv.hip and csrc/conv_w64.hip, restated
# ----------------------------------------------------------------------------------------------------------------------
def w64_takes(c, resid_ptr=0, bias_ptr=0):
    """omh_conv_w64_takes"""
    up = 1 if c.up2 else 0
    es = 4 if c.out_f32 else 2
    return (c.KW == 3 and c.KH == 3 and c.KT in (1, 3) and c.stride_hw == 1 and c.stride_t == 1 and c.pad_h == 1 and c.pad_w == 1 and
            c.Hout == c.Hin << up and c.Wout == c.Win << up and c.Cin % 32 == 0 and c.split_n == 0 and c.Wout >= 3 and
            (c.Cout == 96 or c.Cout % 192 == 0) and c.KT * 3 * (c.Cin >> 5) >= 15 and
            (c.resid_kind is None or bool(c.resid_f32) == bool(c.out_f32)) and resid_ptr % 16 == 0 and bias_ptr % 16 == 0 and
            c.Win * c.Cin * 2 < 1 << 24 and c.Hin << up < 16384 and c.M < 1 << 24 and (c.M + 1024) * c.Cout * es < 0x7fffffff and
            c.Tin * c.Hin * c.Win * c.Cin * 2 < 0x7fffffff and c.Cout * c.KT * 9 * c.Cin * 2 < 0x7fffffff)


def pair_takes(c, resid_ptr=0, bias_ptr=0):
    """omh_conv_w64_pair_takes"""
    ns = c.KT * 3 * (c.Cin >> 5)
    return bool(c.pair and c.out_f32 and (not c.norm or c.Cout == 96) and ns % 2 == 0 and ns >= 16 and w64_takes(c, resid_ptr, bias_ptr))


def kw3_takes(c):
    """the kw-shared condition of omh_conv_cl_bf16 (CONV_KW3 not "0")"""
    return (c.KW == 3 and c.KH == 3 and c.KT in (1, 3) and c.stride_hw == 1 and c.stride_t == 1 and not c.up2 and c.pad_h == 1 and
            c.pad_w == 1 and c.Hout == c.Hin and c.Wout == c.Win and c.Cin % 32 == 0 and c.split_n == 0 and c.Wout >= 3)


def wide_tiles(c):
    mn = 2 * c.Hout * c.Wout
    return (mn + 511) // 512 if c.Cout <= 96 else ((mn + 255) // 256) * ((c.Cout + 191) // 192)


def route_of(c, tile=None, wide_min=None, kw3=True, fuse=True, resid_ptr=0, bias_ptr=0):
    """(kernel, fused): the instantiation omh_conv_cl_bf16 launches for the convolution and whether the norm runs in its
    epilogue; "E_SHAPE" where a pair call is refused.  ``tile`` / ``wide_min`` / ``kw3`` / ``fuse``: the options CONV_TILE,
    CONV_WIDE_MIN, CONV_KW3, CONV_FUSE_NORM."""
    out = "f32" if c.out_f32 else "bf16"
    misaligned = resid_ptr % 16 != 0 or bias_ptr % 4 != 0
    wide = wide_tiles(c) >= (96 if wide_min is None else wide_min)
    if tile in ("wide", "w64"):
        wide = True
    if tile == "small":
        wide = False
    if misaligned:
        wide = False
    forced = tile == "w64"
    w64 = (forced or (tile is None and wide)) and w64_takes(c, resid_ptr, bias_ptr)
    if forced:
        wide = not misaligned
    if c.norm and not (c.Cout == 96 and fuse and (c.pair or w64)):
        plain = NS(**{**vars(c), "norm": False})
        return route_of(plain, tile, wide_min, kw3, fuse, resid_ptr, bias_ptr)[0], False
    if c.pair:
        if not (w64 and pair_takes(c, resid_ptr, bias_ptr)):
            return "E_SHAPE", False
        return ("pairPn" if c.norm else "pairP" if c.Cout == 96 else "pairQ") + "/f32", bool(c.norm)
    if w64:
        return ("w64Pn" if c.norm else "w64P" if c.Cout == 96 else "w64Q") + "/" + out, bool(c.norm)
    if wide:
        if kw3 and kw3_takes(c):
            return ("kw3<8,1,1>" if c.Cout <= 32 else "kw3<8,1>" if c.Cout <= 96 else "kw3<4,2>") + "/" + out, False
        return ("wide<8,1>" if c.Cout <= 96 else "wide<4,2>") + "/" + out, False
    return "128x128/" + out, False


ALL_ROUTES = tuple(f"{k}/{o}" for k in ("128x128", "wide<8,1>", "wide<4,2>", "kw3<8,1,1>", "kw3<8,1>", "kw3<4,2>", "w64P", "w64Q", "w64Pn")
                   for o in ("bf16", "f32")) + ("pairP/f32", "pairQ/f32", "pairPn/f32")
COLUMN_TILE = {"128x128": 128, "wide<8,1>": 96, "wide<4,2>": 192, "kw3<8,1,1>": 32, "kw3<8,1>": 96, "kw3<4,2>": 192, "w64P": 96,
               "w64Q": 192, "w64Pn": 96, "pairP": 96, "pairQ": 192, "pairPn": 96}


# ----------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_conv_exact.py: dict(args of make_case) + tile (CONV_TILE) + kw3 (CONV_KW3) + route
# ----------------------------------------------------------------------------------------------------------------------
def _c(route, tile, Cin, Cout, T, H, W, kw3=True, **kw):
    return dict(route=route, tile=tile, kw3=kw3, Cin=Cin, Cout=Cout, T=T, H=H, W=W, **kw)


_EPI = [dict(bias=b, resid=r, out_f32=o) for b in (False, True) for r in (None, "bf16", "f32") for o in (False, True)]


def _o(route, f32):
    return route + ("/f32" if f32 else "/bf16")


def tiling_cases():
    """M on both sides of every tile's row count; tile boundaries on the last voxel of an image row, in mid row and inside
    a frame's first row (a tile that spans two frames); W = 3, 2, 1; H = 1; one voxel."""
    out = []
    for i, (T, H, W) in enumerate(((1, 1, 127), (1, 8, 16), (1, 3, 43), (2, 8, 8), (1, 1, 1))):        # 128 x 128: 127 | 128 | 129
        f = bool(i % 2)
        out.append(_c(_o("128x128", f), "small", (8, 24, 40, 32, 8)[i], (33, 128, 136, 3, 1)[i], T, H, W, out_f32=f, bias=True, resid="f32" if f else "bf16"))
    for i, (T, H, W) in enumerate(((1, 7, 73), (1, 16, 32), (1, 27, 19), (2, 16, 16), (1, 1, 1), (1, 5, 2), (3, 7, 1))):      # 512 rows: 511 | 512 | 513
        f = bool(i % 2)
        out.append(_c(_o("wide<8,1>", f), "wide", (8, 24, 40, 32, 32, 32, 32)[i], (96, 96, 33, 32, 1, 96, 3)[i], T, H, W, kw3=i >= 5, out_f32=f,
                      bias=True, resid="bf16" if i % 3 == 0 else None))
    for i, (T, H, W) in enumerate(((1, 15, 17), (1, 16, 16), (1, 1, 257), (2, 8, 16), (1, 1, 1), (1, 5, 2), (3, 7, 1))):      # 256 rows: 255 | 256 | 257
        f = bool(i % 2)
        out.append(_c(_o("wide<4,2>", f), "wide", (8, 24, 40, 32, 32, 32, 32)[i], (97, 192, 200, 384, 136, 192, 128)[i], T, H, W, kw3=i >= 5, out_f32=f,
                      bias=True, resid="f32" if f and i % 2 else None))
    # the kw-shared tiles advance by 510 / 254 voxels
    p_shapes = ((1, 1, 509), (1, 15, 34), (1, 7, 73), (2, 15, 20), (3, 34, 5), (1, 5, 3), (2, 1, 3), (1, 1, 3), (2, 17, 30))
    q_shapes = ((1, 11, 23), (1, 2, 127), (1, 15, 17), (2, 10, 20), (3, 17, 5), (1, 5, 3), (2, 1, 3), (1, 1, 3), (4, 127, 3))
    for i, (T, H, W) in enumerate(p_shapes):
        f = bool(i % 2)
        e = dict(out_f32=f, bias=True, resid=("f32" if f else "bf16") if i % 3 else None)
        out.append(_c(_o("kw3<8,1,1>", f), "wide", 32, (1, 3, 32)[i % 3], T, H, W, KT=(1, 3)[i % 2], **e))
        out.append(_c(_o("kw3<8,1>", f), "wide", (32, 96)[i % 2], (33, 96, 64)[i % 3], T, H, W, KT=(3, 1)[i % 2], **e))
        out.append(_c(_o("w64P", f), "w64", (160, 64)[i % 2], 96, T, H, W, KT=(1, 3)[i % 2], **e))
    for i, (T, H, W) in enumerate(q_shapes):
        f = bool(i % 2)
        e = dict(out_f32=f, bias=True, resid=("f32" if f else "bf16") if i % 3 else None)
        out.append(_c(_o("kw3<4,2>", f), "wide", (32, 96)[i % 2], (97, 192, 200, 384)[i % 4], T, H, W, KT=(3, 1)[i % 2], **e))
        out.append(_c(_o("w64Q", f), "w64", (160, 64)[i % 2], (192, 384)[i % 2], T, H, W, KT=(1, 3)[i % 2], **e))
    return out


def channel_cases():
    """Cin 8 | 24 | 40 (a K tail against BK = 64, no kw-shared route) and 32 | 96 | 160 | 384; Cout 1, 3, 32 | 33, 96 | 97,
    128 | 136, 192 | 200, 384; the stream's stage counts 15 | 18 | 21 | 24 (3 KT Cin / 32: 16 cannot occur)."""
    out = []
    couts = (1, 3, 32, 33, 96, 97, 128, 136, 192, 200, 384)
    for i, Cout in enumerate(couts):
        f = bool(i % 2)
        for j, Cin in enumerate((8, 24, 40)):
            tile = ("small", "wide")[(i + j) % 2]
            r = "128x128" if tile == "small" else ("wide<8,1>" if Cout <= 96 else "wide<4,2>")
            out.append(_c(_o(r, f), tile, Cin, Cout, 1, 5, 7, KT=(3, 1)[j % 2], out_f32=f, bias=bool(j % 2)))
        Cin = (32, 96, 160, 384)[i % 4]
        KT = 1 if Cin == 384 else (1, 3)[i % 2]
        r = "kw3<8,1,1>" if Cout <= 32 else ("kw3<8,1>" if Cout <= 96 else "kw3<4,2>")
        out.append(_c(_o(r, f), "wide", Cin, Cout, 2, 6, 9, KT=KT, out_f32=f, bias=True))
        out.append(_c(_o("128x128", not f), "small", Cin, Cout, 2, 6, 9, KT=KT, out_f32=not f, bias=True))
        out.append(_c(_o("wide<8,1>" if Cout <= 96 else "wide<4,2>", f), "wide", Cin, Cout, 2, 6, 9, KT=KT, kw3=False, out_f32=f))
    for i, Cin in enumerate((160, 192, 224, 256, 384)):     # 15 | 18 | 21 | 24 | 36 stages with KT = 1
        for f in (False, True):
            out.append(_c(_o("w64P", f), "w64", Cin, 96, 2, 6, 9, KT=1, out_f32=f, bias=True))
            out.append(_c(_o("w64Q", f), "w64", Cin, (192, 384)[i % 2], 2, 6, 9, KT=1, out_f32=f, bias=True))
    out.append(_c("w64Q/f32", "w64", 384, 384, 1, 6, 9, KT=3, out_f32=True))                # 108 stages, K = 10 368
    out.append(_c("kw3<8,1>/bf16", "w64", 128, 96, 2, 6, 9, KT=1))                           # 12 stages: below the stream's 15
    return out


def geometry_cases():
    """3x3x3, 1x3x3, 3x1x1, 1x1x1; stride 2 with and without a real last row; temporal stride; the folded upsample at odd input
    sizes; the frame interleave with the split boundary on and inside a column tile — on every tile family that accepts it."""
    out = []
    for tile, kw3, name in (("small", True, "128x128"), ("wide", True, None), ("wide", False, None)):
        for i, Cout in enumerate((96, 200)):
            wide = "wide<8,1>" if Cout <= 96 else "wide<4,2>"
            k3 = ("kw3<8,1>" if Cout <= 96 else "kw3<4,2>") if kw3 else wide
            f = bool(i)
            e = dict(out_f32=f, bias=True, surplus=1)
            out.append(_c(_o(name or k3, f), tile, 32, Cout, 2, 5, 7, kw3=kw3, KT=3, **e))
            out.append(_c(_o(name or k3, not f), tile, 32, Cout, 2, 5, 7, kw3=kw3, KT=1, out_f32=not f))
            out.append(_c(_o(name or wide, f), tile, 32, Cout, 2, 5, 7, kw3=kw3, KT=3, KH=1, KW=1, **e))
            out.append(_c(_o(name or wide, f), tile, 40, Cout, 2, 5, 7, kw3=kw3, KT=1, KH=1, KW=1, **e))
            for odd in (False, True):
                out.append(_c(_o(name or wide, f), tile, 32, Cout, 2, 4, 5, kw3=kw3, KT=1, kind="down", odd=odd, **e))
            out.append(_c(_o(name or wide, f), tile, 32, Cout, 3, 4, 5, kw3=kw3, KT=3, KH=1, KW=1, kind="tstride", **e))
            out.append(_c(_o(name or wide, f), tile, 32, Cout, 2, 5, 7, kw3=kw3, KT=1, kind="up2", **e))
        for split_n, Cout in ((32, 64), (96, 192), (192, 384), (40, 80)):
            wide = "wide<8,1>" if Cout <= 96 else "wide<4,2>"
            for f in (False, True):
                out.append(_c(_o(name or wide, f), tile, 32, Cout, 2, 5, 7, kw3=kw3, KT=3, KH=1, KW=1, split_n=split_n, out_f32=f, bias=True,
                              resid=("f32" if f else "bf16") if kw3 else None))
    for f in (False, True):                                 # the folded upsample on the stream, odd input sizes
        out.append(_c(_o("w64P", f), "w64", 160, 96, 2, 5, 7, KT=1, kind="up2", out_f32=f, bias=True))
        out.append(_c(_o("w64Q", f), "w64", 192, 192, 1, 9, 13, KT=1, kind="up2", out_f32=f, bias=True, resid="f32" if f else "bf16"))
        out.append(_c(_o("w64P", f), "w64", 64, 96, 2, 5, 7, KT=3, out_f32=f, bias=True, surplus=2))
    return out


def epilogue_cases():
    """bias x residual kind x output type on every family; the combinations the stream refuses run on the 8-wave kernel"""
    out = []
    for e in _EPI:
        f = e["out_f32"]
        out.append(_c(_o("128x128", f), "small", 32, 136, 1, 9, 15, KT=1, **e))
        out.append(_c(_o("wide<8,1>", f), "wide", 32, 96, 1, 9, 15, KT=1, kw3=False, **e))
        out.append(_c(_o("wide<4,2>", f), "wide", 32, 200, 1, 9, 15, KT=1, kw3=False, **e))
        out.append(_c(_o("kw3<8,1,1>", f), "wide", 32, 3, 1, 9, 15, KT=1, **e))
        out.append(_c(_o("kw3<8,1>", f), "wide", 32, 96, 1, 9, 15, KT=1, **e))
        out.append(_c(_o("kw3<4,2>", f), "wide", 32, 200, 1, 9, 15, KT=1, **e))
        mixed = e["resid"] is not None and (e["resid"] == "f32") != f
        out.append(_c(_o("kw3<8,1>" if mixed else "w64P", f), "w64", 160, 96, 1, 9, 15, KT=1, **e))
        out.append(_c(_o("kw3<4,2>" if mixed else "w64Q", f), "w64", 160, 192, 1, 9, 15, KT=1, **e))
    return out


def pair_cases():
    """real channels x KT chosen so that K_real 2056 + 72 * 512 < 2^24; 18 and 24 stages are the shortest the pair stream
    takes (3 KT Cin2 / 32, even, >= 16)"""
    out = []
    for i, (Cin2, KT, T, H, W) in enumerate(((192, 1, 1, 5, 3), (256, 1, 1, 7, 5), (192, 3, 2, 12, 20), (768, 1, 1, 9, 29), (384, 1, 2, 15, 34),
                                             (192, 1, 1, 1, 509), (64, 3, 2, 15, 20))):
        e = dict(out_f32=True, bias=bool(i % 2), resid="f32" if i % 3 else None, pair=True, KT=KT)
        out.append(_c("pairP/f32", "w64", Cin2, 96, T, H, W, **e))
        out.append(_c("pairQ/f32", "w64", Cin2, (192, 384)[i % 2], T, H, W, **e))
        out.append(_c("pairPn/f32", "w64", Cin2, 96, T, H, W, norm=True, **e))
    out.append(_c("pairP/f32", "w64", 192, 96, 1, 5, 7, KT=1, kind="up2", out_f32=True, bias=True, pair=True))
    out.append(_c("pairQ/f32", "w64", 384, 192, 1, 5, 7, KT=1, kind="up2", out_f32=True, bias=True, resid="f32", pair=True))
    return out


def fused_norm_cases():
    out = []
    for i, (Cin, KT, T, H, W) in enumerate(((160, 1, 1, 5, 3), (64, 3, 2, 12, 20), (96, 3, 2, 15, 34), (192, 1, 1, 1, 509))):
        for f in (False, True):
            out.append(_c(_o("w64Pn", f), "w64", Cin, 96, T, H, W, KT=KT, norm=True, out_f32=f, bias=bool(i % 2),
                          resid=(("f32" if f else "bf16") if i % 2 == 0 else None)))
    out.append(_c("w64Pn/bf16", "w64", 160, 96, 2, 7, 9, KT=1, norm=True, norm_only=True, bias=True))
    return out


def all_cases():
    return tiling_cases() + channel_cases() + geometry_cases() + epilogue_cases() + pair_cases() + fused_norm_cases()


def build(cs, seed=0):
    kw = {k: v for k, v in cs.items() if k not in ("route", "tile", "kw3")}
    return make_case(seed=seed, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# the norm behind the convolution
# ----------------------------------------------------------------------------------------------------------------------
NORM_C = (16, 96, 192, 384)
NORM_P = (1, 63, 64, 65, 77)            # 77: no multiple of the voxels a workgroup takes


def rows_per_workgroup(C):
    """rms_silu_launch of csrc/vae_elementwise.hip: 256 threads, G lanes per voxel with G = 4 up to 16 chunks of 8 channels,
    16 up to 64 chunks, 64 beyond"""
    return 256 // lanes_per_voxel(C)


def lanes_per_voxel(C):
    nch = C // 8
    return 4 if nch <= 16 else (16 if nch <= 64 else 64)


def norm_input(C, P, seed=0, bf16=False):
    """[P, C] float64: the first P voxels of an exact convolution's output (1x3x3, 8 channels in, bias: integers up to
    9 * 72 + 8), voxel P // 2 all zero (the 1e-12 clamp).  ``bf16``: rounded as the bf16 entry reads them."""
    c = make_case(8, C, 1, 7, 11, KT=1, bias=True, out_f32=not bf16, seed=1000 + seed)
    v = reference(c).y.double().reshape(-1, C)[:P].clone()
    v[P // 2] = 0.0
    return v


def norm_input_pow2(C, P, seed=0):
    """[P, C] float64 with ||x|| C^-1/2 = 2^j per voxel: all channels +-2^j, or +-2^(j+1) on one channel in four and zero on the rest"""
    g = _gen(seed, C, P, 5)
    j = torch.randint(-3, 6, (P, 1), generator=g).double()
    sign = 1.0 - 2.0 * torch.randint(0, 2, (P, C), generator=g).double()
    flat = torch.ones((P, C), dtype=F64)
    sparse = torch.zeros((P, C // 4, 4), dtype=F64)
    sparse.scatter_(2, torch.randint(0, 4, (P, C // 4, 1), generator=g), 2.0)
    pick = torch.randint(0, 2, (P, 1), generator=g).bool()
    return torch.where(pick, flat, sparse.reshape(P, C)) * sign * torch.exp2(j)


def norm_gamma(C, seed=0, pow2=False):
    g = _gen(seed, C, 9)
    if pow2:                                                # multiples of 1/8 in [-2, 2] without zero: x inv gamma is a bf16 value
        v = _ints(g, (C,), 16)
        return (torch.where(v == 0, torch.ones_like(v), v) / 8.0).float()
    return ((torch.rand(C, generator=g, dtype=F64) + 0.5) * (1 - 2 * torch.randint(0, 2, (C,), generator=g))).float()


def norm_reference(x64, gamma, do_silu=True):
    """NS(y, S): the formula of include/omh.h in float64 and its condition sum"""
    C = x64.shape[-1]
    inv = math.sqrt(C) / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    z = x64 * inv * gamma.double()
    if not do_silu:
        return NS(y=z, S=z.abs())
    sg = torch.sigmoid(z)
    return NS(y=z * sg, S=z.abs() * sg)


def _ulps(t, n):
    return t if n == 0 else (t.double() * (1.0 + n * 2.0 ** -23)).float()


def norm_restated(x, gamma, do_silu=True, nudge=(0, 0, 0, 0)):
    """rms_silu_kernel of csrc/vae_elementwise.hip in fp32 on the CPU: lane l of a voxel's G lanes takes the 8-channel
    chunks l, l + G, ... and adds their squares by one fma per value in channel order, then the butterfly over lane
    distances G / 2 .. 1; inv = sqrtf(C) * rcp(max(sqrt(ss), 1e-12)); (x * inv) * gamma; silu(a) = a * rcp(1 + exp2(-log2(e) * a)).
    ``nudge``: ulps by which the raw sqrt, rcp, exp2 and the second rcp are displaced (the hardware's are 1-ulp class)."""
    x = x.float()
    P, C = x.shape
    nch, Gl = C // 8, lanes_per_voxel(C)
    ss = torch.zeros((P, Gl), dtype=F32)
    xc = x.reshape(P, nch, 8)
    for i in range(4):
        ch = torch.arange(Gl) + Gl * i
        ok = ch < nch
        if not bool(ok.any()):
            break
        v = xc[:, ch[ok]].double()
        s = ss[:, ok]
        for e in range(8):
            s = (v[..., e] * v[..., e] + s.double()).float()            # fmaf: one rounding
        ss[:, ok] = s
    lane = torch.arange(Gl)
    o = Gl // 2
    while o:
        ss = ss + ss[:, lane ^ o]
        o //= 2
    root = _ulps(torch.sqrt(ss[:, :1]), nudge[0])
    rcp = _ulps(1.0 / torch.clamp_min(root, torch.tensor(1e-12, dtype=F32)), nudge[1])
    inv = torch.sqrt(torch.tensor(float(C), dtype=F32)) * rcp
    a = (x * inv) * gamma.float()
    if do_silu:
        t = torch.tensor(-1.4426950408889634, dtype=F32) * a
        e = _ulps(torch.exp2(t.double()).float(), nudge[2])
        a = a * _ulps(1.0 / (1.0 + e), nudge[3])
    return a


NUDGES = ((0, 0, 0, 0), (-1, 1, -1, 1), (1, -1, 1, -1))


def split_pair(a):
    """fp32 -> (hi, lo) as the kernels write them: hi = bf16(a), lo = bf16(a - hi)"""
    a = a.float()
    hi = a.to(BF16)
    return hi, (a - hi.float()).to(BF16)


def norm_bound(ref, kind):
    d = K_NORM[kind] * N.SLACK * ref.S
    return d if kind == "split" else 0.5 * ulp_bf16(ref.y.abs() + d) + d


def unpack_split(t, C, layout):
    """(hi, lo) [P, C] from a [P, 3 C] pattern-0 result [hi | lo | hi] ("split3": the two hi blocks must agree) or a
    [P, 2 C] pair result [hi(16) | lo(16)] per 16 channels ("pair")"""
    if layout == "pair":
        return pair_halves(t)
    assert torch.equal(t[:, :C].view(torch.int16), t[:, 2 * C:].view(torch.int16)), "the two hi blocks of [hi | lo | hi] differ"
    return t[:, :C], t[:, C:2 * C]
