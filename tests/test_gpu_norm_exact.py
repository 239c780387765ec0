"""The row kernels of the DiT block (csrc/dit_elementwise.hip, csrc/dit_backward.hip, csrc/dit_backward2.hip) element for
element against the float64 references of tests/norm_exact_ref.py, at the edges of their register-array templates
(6 / 20 / 32 float4 chunks per lane: widths 1536 | 1540 and 5120 | 5124, 8192, partly filled last chunks), of their row
dispatch (rows per wave, rows per workgroup, batch boundaries inside a wave's rows, an incomplete last batch element)
and of the RoPE index arithmetic (heads that share a lane's table entries and heads that do not, pad tokens, the clamp
at rope_len - 1, two samples with different grids).

Two kinds of assertion.  Where the arithmetic can be made exact (the gated residual, every RMSNorm entry with
do_norm = 0 on integer inputs and a rotary table of exactly representable pairs, dadd of the LayerNorm backwards)
``torch.equal`` against float64 is the index test.  Where rsqrtf and means forbid that, every element is held to the
bound of its own condition sum (norm_exact_ref: 0.5 ulp_bf16 + 2^-16 S for bf16, 2^-16 S for fp32 rows, k 2^-24 S for
sums over rows).  Input pads hold NaN, every output sits in a canvas whose guard rows and pad columns must keep their
bits, modulation and gate vectors are slices 4 elements into larger NaN-filled buffers.

Each omh_rmsnorm_rope_bf16_pair case first asserts, in Python, the dispatch condition restated from the .hip file; the
``[routes]`` line printed at the end counts the kernels that ran, ``[measured]`` the worst ratio to the bound per entry.

Not here: omh_rmsnorm_rope_bwd2 (one and two segments, dx aliasing dy).  Its cases were written with the others; the
20-chunk kernel with fp32 x and bf16 dy at width 1540 ended in a GPU fault on its first run, the cause is not found, and
the cases stay out until it is ("The norm kernels held per element")."""
import collections
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

import norm_exact_ref as R
from conftest import set_option

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTES = collections.Counter()
E_BADARG, E_SHAPE = -1, -3
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[routes] " + "  ".join(f"{k}={v}" for k, v in sorted(ROUTES.items())))
    print(R.summary_line())
    print("[compared] " + "  ".join(f"{k}={v}" for k, v in sorted(R.COUNTS.items())))


def _sync():
    torch.cuda.synchronize()


def _nv(dim):
    return 6 if dim <= 1536 else (20 if dim <= 5120 else 32)


def _in(t, pitch=None):
    """an input [rows, cols] at row pitch ``pitch`` in a NaN-filled allocation, armed: it must not change"""
    return R.Canvas(t.shape[0], t.shape[1], pitch or t.shape[1], t.dtype, DEV, lead=1, trail=1).put(t).arm()


def _out(rows, cols, pitch, dtype, init=None):
    cv = R.Canvas(rows, cols, pitch, dtype, DEV)
    if init is not None:
        cv.put(init)
    return cv.arm()


class Vec:
    """a [dim] vector or [n, dim] vectors ``stride`` apart, 4 elements into a larger NaN-filled buffer (as the model passes
    slices of its modulation tensor)"""

    def __init__(self, t, stride=None, use=True):
        self.ptr, self.stride = None, 0
        if not use or t is None:
            return
        dim = t.shape[-1]
        if t.dim() == 1:
            self.buf = torch.full((4 + dim + 4,), NAN, dtype=F32, device=DEV)
            self.buf[4:4 + dim] = t.to(DEV)
        else:
            self.stride = stride or dim
            assert self.stride >= dim and self.stride % 4 == 0
            self.buf = torch.full((4 + t.shape[0] * self.stride + 4,), NAN, dtype=F32, device=DEV)
            self.buf[4:4 + t.shape[0] * self.stride].view(t.shape[0], self.stride)[:, :dim] = t.to(DEV)
        self.ptr = self.buf.data_ptr() + 16
        self._bits0 = self.buf.view(torch.int32).clone()

    def assert_unchanged(self, ctx):
        if self.ptr is not None:
            assert torch.equal(self.buf.view(torch.int32), self._bits0), f"{ctx} a modulation / gate / gain vector was written"


def _hold(entry, what, cv, ref, bound, ctx):
    """the window of canvas ``cv`` against the reference (bound None: exact), and its guards"""
    got = cv.window()
    msg = R.compare(entry, what, got if bound is None else got.float(), ref, bound, ctx)
    assert msg is None, msg
    cv.assert_guard(what, ctx)


def _ln(cs):
    return R.ln_case(cs["rows"], cs["dim"], cs["rpb"], cs["seed"], small=cs.get("small", False), dy_bf16=cs.get("dy_bf16", False),
                     shared=cs.get("shared", False))


def _ids(cases):
    return ["-".join(f"{k}{v}" for k, v in cs.items() if k not in ("seed", "grids")) for cs in cases]


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm + modulation, forward
# ----------------------------------------------------------------------------------------------------------------------
LN_FWD = R.ln_fwd_cases()
RPW_AT = {4096: 1, 4097: 2, 16383: 2, 16384: 4, 24575: 4, 24576: 16}


@pytest.mark.parametrize("cs", LN_FWD, ids=_ids(LN_FWD))
def test_layernorm_modulate(ops, cs):
    c = _ln(cs)
    ctx = f"{cs}:"
    forced = cs.get("forced")
    if forced is not None:
        set_option("LN_RPW", str(forced))
    rpw = R.ln_rows_per_wave(c.rows, forced)
    assert rpw == (forced if forced is not None else RPW_AT.get(c.rows, 1)), f"{ctx} the case would run {rpw} rows per wave"
    use = ((1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0))[cs["seed"] % 4]           # which of mul0, mul1, add0, add1 are passed
    x, y = _in(c.x), _out(c.rows, c.dim, c.dim, BF16)
    m0, m1, a0, a1 = Vec(c.mul0, use=use[0]), Vec(c.mul1, c.stride, use[1]), Vec(c.add0, use=use[2]), Vec(c.add1, c.stride + 4, use[3])
    rc = ops.lib.omh_layernorm_modulate(x.ptr, y.ptr, c.rows, c.dim, c.eps, c.mul_const, m0.ptr, m1.ptr, m1.stride, a0.ptr, a1.ptr,
                                        a1.stride, c.rpb, ops._stream())
    assert rc == 0, f"{ctx} omh_layernorm_modulate returned {rc}"
    _sync()
    ROUTES[f"ln/chunks{_nv(c.dim)}/rpw{rpw}"] += 1
    ref = R.ln_forward(c, mul0=use[0], mul1=use[1], add0=use[2], add1=use[3])
    _hold("layernorm_modulate", "y", y, ref.y, R.bound_bf16(ref.y, ref.S), ctx)
    x.assert_guard("x", ctx)
    for v in (m0, m1, a0, a1):
        v.assert_unchanged(ctx)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm + modulation, backward: the atomics form and the two-stage form
# ----------------------------------------------------------------------------------------------------------------------
LN_BWD = R.ln_bwd_cases()


def _param_canvases(c):
    """dmul, dadd [groups, dim] at pitch dstride (0: one shared vector) and dgate [row groups, dim], holding their starts"""
    ds = 0 if c.shared else c.stride
    return (_out(c.ng, c.dim, ds or c.dim, F32, c.dmul0), _out(c.ng, c.dim, ds or c.dim, F32, c.dadd0),
            _out(c.nb, c.dim, c.stride + 4, F32, c.dgate0), ds)


@pytest.mark.parametrize("cs", LN_BWD, ids=_ids(LN_BWD))
def test_layernorm_modulate_bwd(ops, cs):
    c = _ln(cs)
    ctx = f"{cs}:"
    x, dy, dx = _in(c.x), _in(c.dy.float()), _out(c.rows, c.dim, c.dim, F32, c.dx0)
    dmul, dadd, _, ds = _param_canvases(c)
    m0, m1 = Vec(c.mul0), Vec(c.mul1, c.stride)
    rc = ops.lib.omh_layernorm_modulate_bwd(x.ptr, dy.ptr, dx.ptr, c.rows, c.dim, c.eps, c.mul_const, m0.ptr, m1.ptr, m1.stride, dmul.ptr,
                                            dadd.ptr, ds, c.rpb, ops._stream())
    assert rc == 0, f"{ctx} omh_layernorm_modulate_bwd returned {rc}"
    _sync()
    ROUTES[f"ln_bwd/chunks{_nv(c.dim)}"] += 1
    ref = R.ln_backward(c)
    _hold("layernorm_modulate_bwd", "dx", dx, ref.dx, R.bound_row(ref.S_dx), ctx)
    _hold("layernorm_modulate_bwd", "dmul", dmul, ref.dmul, R.bound_sum(ref.S_dmul, "dmul"), ctx)
    _hold("layernorm_modulate_bwd", "dadd", dadd, R.G.exact_f32(ref.dadd), None, ctx)
    for cv, what in ((x, "x"), (dy, "dy")):
        cv.assert_guard(what, ctx)


def run_ln_bwd2(ops, cs, deferred=None):
    """one omh_layernorm_modulate_bwd2 call on canvases; ``deferred``: a PartialReduce to fill instead of the second stage.
    Returns the case and what has to be held afterwards."""
    binding = ops._lib
    c = _ln(cs)
    ctx = f"{cs}:"
    v = cs["variant"]
    x, dy, dx = _in(c.x), _in(c.dy), _out(c.rows, c.dim, c.dim, F32, c.dx0)
    dmul, dadd, dgate, ds = _param_canvases(c)
    m0, m1, g0, g1 = Vec(c.mul0), Vec(c.mul1, c.stride), Vec(c.gate0), Vec(c.gate1, c.stride + 8)
    dyn = _out(c.rows, c.dim, c.dim, BF16) if v != "plain" else None
    yn = _in(c.y_next) if v == "gate" else None
    nb, nj = R.ln_bwd2_geometry(c.rows, c.rpb)
    need = ops.lib.omh_layernorm_modulate_bwd2_workspace(c.rows, c.dim, c.rpb)
    assert need == nb * nj * 3 * c.dim, f"{ctx} workspace query {need}, geometry {nb} x {nj} x 3 x {c.dim}"
    ws = torch.full((need + 64,), NAN, dtype=F32, device=DEV)
    a = binding.LnBwdArgs(x.ptr, dy.ptr, int(c.dy_bf16), dx.ptr, c.rows, c.dim, c.eps, c.mul_const, m0.ptr, m1.ptr, m1.stride, dmul.ptr,
                          dadd.ptr, ds, c.rpb, dyn.ptr if dyn else None, yn.ptr if yn else None, c.gate_const, g0.ptr, g1.ptr, g1.stride,
                          dgate.ptr if v == "gate" else None, c.stride + 4, ws.data_ptr(), need,
                          C.pointer(deferred) if deferred is not None else None)
    rc = ops.lib.omh_layernorm_modulate_bwd2(C.byref(a), ops._stream())
    assert rc == 0, f"{ctx} omh_layernorm_modulate_bwd2 returned {rc}"
    ROUTES[f"ln_bwd2/chunks{_nv(c.dim)}/{v}/{'bf16' if c.dy_bf16 else 'f32'}/wg{R.ln_bwd2_rows_per_wg(c.rows)}"] += 1
    return NS(c=c, ctx=ctx, v=v, x=x, dy=dy, dx=dx, dmul=dmul, dadd=dadd, dgate=dgate, dyn=dyn, yn=yn, ws=ws, nb=nb, nj=nj,
              keep=(m0, m1, g0, g1))


def hold_ln_bwd2(h):
    c, ctx, e = h.c, h.ctx, "layernorm_modulate_bwd2"
    ref = R.ln_backward(c, nxt=h.v != "plain", gate=h.v == "gate")
    _hold(e, "dx", h.dx, ref.dx, R.bound_row(ref.S_dx), ctx)
    _hold(e, "dmul", h.dmul, ref.dmul, R.bound_sum(ref.S_dmul, "dmul"), ctx)
    _hold(e, "dadd", h.dadd, R.G.exact_f32(ref.dadd), None, ctx)
    if h.v != "plain":
        _hold(e, "dy_next", h.dyn, ref.dy_next, R.bound_bf16(ref.dy_next, ref.S_dy_next), ctx)
    if h.v == "gate":
        _hold(e, "dgate", h.dgate, ref.dgate, R.bound_sum(ref.S_dgate, "dgate"), ctx)
        h.yn.assert_guard("y_next", ctx)
    else:
        h.dgate.assert_guard("dgate", ctx)
        assert torch.equal(h.dgate.window().cpu(), c.dgate0), f"{ctx} dgate was written without y_next"
    for cv, what in ((h.x, "x"), (h.dy, "dy")):
        cv.assert_guard(what, ctx)
    for vec in h.keep:
        vec.assert_unchanged(ctx)
    # the partials: groups x workgroups x (2 or 3) x dim floats from the start of the workspace, nothing behind them
    wrote = h.nb * h.nj * (3 if h.v == "gate" else 2) * c.dim
    ws = h.ws.cpu()
    assert bool(torch.isfinite(ws[:wrote]).all()), f"{ctx} the kernel left part of its {wrote} partials unwritten"
    assert bool(torch.isnan(ws[wrote:]).all()), f"{ctx} the workspace was written behind its {wrote} partials"


LN_BWD2 = R.ln_bwd2_cases()


@pytest.mark.parametrize("cs", LN_BWD2, ids=_ids(LN_BWD2))
def test_layernorm_modulate_bwd2(ops, cs):
    if not cs["deferred"]:
        h = run_ln_bwd2(ops, cs)
    else:
        d = ops._lib.PartialReduce()
        h = run_ln_bwd2(ops, cs, d)
        assert (d.nj, d.nb, d.dim, d.np, d.grid_y) == (h.nj, h.nb, cs["dim"], 3 if h.v == "gate" else 2, h.nb * (3 if h.v == "gate" else 2))
        bt = ops._lib.PartialReduceBatch()
        bt.n, bt.e[0] = 1, d
        assert ops.lib.omh_partial_colsum_multi(C.byref(bt), ops._stream()) == 0
    _sync()
    hold_ln_bwd2(h)


def test_deferred_second_stages_in_one_launch_equal_the_direct_form(ops):
    """three entries of widths 8, 260 and 1540 with different grid_y in one omh_partial_colsum_multi: bit for bit the direct
    form, and inside the bound of the reference"""
    cases = [dict(dim=8, rows=40, rpb=40, seed=700, variant="plain", dy_bf16=False),       # grid_y 2
             dict(dim=260, rows=17, rpb=7, seed=701, variant="gate", dy_bf16=True),        # grid_y 9
             dict(dim=1540, rows=17, rpb=9, seed=702, variant="next", dy_bf16=False)]      # grid_y 4
    direct = [run_ln_bwd2(ops, cs) for cs in cases]
    bt = ops._lib.PartialReduceBatch()
    ds = [ops._lib.PartialReduce() for _ in cases]
    deferred = [run_ln_bwd2(ops, cs, d) for cs, d in zip(cases, ds)]
    bt.n = 3
    for i, d in enumerate(ds):
        bt.e[i] = d
    assert sorted(d.grid_y for d in ds) == [2, 4, 9]
    assert ops.lib.omh_partial_colsum_multi(C.byref(bt), ops._stream()) == 0
    _sync()
    for a, b in zip(direct, deferred):
        hold_ln_bwd2(b)
        for what in ("dx", "dmul", "dadd", "dgate"):
            assert torch.equal(getattr(a, what).window(), getattr(b, what).window()), f"{b.ctx} {what}: deferred differs from direct"
        if a.dyn is not None:
            assert torch.equal(a.dyn.window(), b.dyn.window())


# ----------------------------------------------------------------------------------------------------------------------
# RMSNorm + RoPE, forward
# ----------------------------------------------------------------------------------------------------------------------
class RmsProblem:
    """the operands of one rms_case on the device: x of all segments in ONE canvas, seg_x = dim + 4 apart, at a pitch 8
    wider than its columns (with_dy: dy of segment 0 at the same pitch, for the one-segment backward entries); the rotary
    table with its NaN row behind rope_len; the grids; the gains"""

    def __init__(self, c, with_dy=False):
        self.c = c
        self.seg = c.dim + 4
        cols = self.seg * (c.nseg - 1) + c.dim
        self.ld = cols + c.pad
        self.x = self._pack(c.x, cols)
        self.dy = self._pack(c.dy[:1], cols) if with_dy else None
        self.w = [Vec(w) for w in c.w]
        self.cos = self.sin = self.grid = None
        if c.hd:
            self.cos, self.sin, self.grid = c.cos.to(DEV), c.sin.to(DEV), c.grid.to(DEV).contiguous()
        self.table = (self.cos.data_ptr() if c.hd else None, self.sin.data_ptr() if c.hd else None, c.rope_len, c.hd,
                      self.grid.data_ptr() if c.hd else None, c.seq_len)

    def _pack(self, segs, cols):
        full = torch.full((self.c.rows, cols), NAN, dtype=segs[0].dtype)
        for s, t in enumerate(segs):
            full[:, s * self.seg:s * self.seg + self.c.dim] = t
        return _in(full, self.ld)

    def hold_inputs(self, ctx):
        self.x.assert_guard("x", ctx)
        if self.dy is not None:
            self.dy.assert_guard("dy", ctx)
        for v in self.w:
            v.assert_unchanged(ctx)


def _hold_y(entry, c, seg, cv, ctx, out_scale=None):
    ref = R.rms_forward(c, seg, out_scale=out_scale)
    if c.exact:
        _hold(entry, f"y{seg}", cv, R.rne_bf16(ref.y), None, ctx)
    else:
        _hold(entry, f"y{seg}", cv, ref.y, R.bound_bf16(ref.y, ref.S), ctx)


RMS_FWD = [dict(kw, entry=e) for exact in (True, False) for kw in R.rms_cases(exact) for e in ("f32", "bf16")]


@pytest.mark.parametrize("cs", RMS_FWD, ids=_ids(RMS_FWD))
def test_rmsnorm_rope_one_segment(ops, cs):
    kw = dict(cs)
    entry = kw.pop("entry")
    c = R.rms_case(x_bf16=entry == "bf16", **kw)
    ctx = f"{cs}:"
    p = RmsProblem(c)
    y = _out(c.rows, c.dim, c.dim, BF16)
    if entry == "f32":
        rc = ops.lib.omh_rmsnorm_rope(p.x.ptr, p.ld, y.ptr, c.rows, c.dim, p.w[0].ptr, c.eps, c.do_norm, *p.table, ops._stream())
    else:
        rc = ops.lib.omh_rmsnorm_rope_bf16(p.x.ptr, p.ld, y.ptr, c.rows, c.dim, p.w[0].ptr, c.eps, c.do_norm, *p.table, c.scale[0],
                                           ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ROUTES[f"rms_{entry}/chunks{_nv(c.dim)}/{'shared' if c.hd and 256 % c.hd == 0 else ('per_vector' if c.hd else 'no')}_table"] += 1
    _hold_y("rmsnorm_rope" if entry == "f32" else "rmsnorm_rope_bf16", c, 0, y, ctx, 1.0 if entry == "f32" else None)
    p.hold_inputs(ctx)


# (dim, head_dim, RMS_PAIR_ROW, the form that must run)
PAIR = [(256, 128, "1", "row"), (256, 128, "0", "two_wg"), (384, 128, None, "two_wg"), (128, 64, "1", "row"), (192, 64, "0", "two_wg"),
        (16, 8, "1", "row"), (24, 8, "0", "two_wg"), (192, 96, "1", "two_wg"), (288, 96, None, "two_wg"), (24, 12, "1", "two_wg"),
        (36, 12, "0", "two_wg"), (1536, 128, "1", "row"), (1540, 20, "1", "two_wg"), (5120, 128, "1", "row"), (5120, 128, "0", "two_wg"),
        (5124, 12, "1", "two_wg"), (8192, 128, "1", "two_wg"), (1536, 128, None, "two_wg")]


def _run_pair(ops, c, option, form, ctx, bound=False):
    p = RmsProblem(c)
    y0, y1 = _out(c.rows, c.dim, c.dim, BF16), _out(c.rows, c.dim, c.dim, BF16)
    args = (p.x.ptr, p.ld, p.seg, y0.ptr, y1.ptr, c.rows, c.dim, p.w[0].ptr, p.w[1].ptr, c.eps, c.do_norm, *p.table, c.scale[0], c.scale[1])
    if bound:
        heads = c.dim // 128
        n2 = _out(c.rows // c.seq_len * heads, 2, 2, F32, torch.zeros(c.rows // c.seq_len * heads, 2))
        rc = ops.lib.omh_rmsnorm_rope_bf16_pair_bound(*args, n2.ptr, ops._stream())
        entry = "rmsnorm_rope_bf16_pair_bound"
    else:
        if option is not None:
            set_option("RMS_PAIR_ROW", option)
        took = "row" if R.pair_takes_row_form(c.rows, c.dim, c.hd, option) else "two_wg"
        assert took == form, f"{ctx} the case names the {form} form and would run the {took} form"
        rc = ops.lib.omh_rmsnorm_rope_bf16_pair(*args, ops._stream())
        entry = "rmsnorm_rope_bf16_pair"
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ROUTES[f"pair/{'bound' if bound else form}/chunks{_nv(c.dim)}"] += 1
    _hold_y(entry, c, 0, y0, ctx)
    _hold_y(entry, c, 1, y1, ctx)
    p.hold_inputs(ctx)
    if bound:                   # from the values as stored: exact in the exact mode, 128 fp32 additions of squares otherwise
        want = torch.stack([R.norm2_max(c, y.window().cpu()) if c.exact else
                            (y.window().cpu().double().reshape(c.rows // c.seq_len, c.seq_len, heads, 128) ** 2).sum(-1).amax(1)
                            for y in (y0, y1)], -1).reshape(-1, 2)
        _hold(entry, "norm2_max", n2, want if c.exact else want.double(), None if c.exact else R.bound_row(want.double()), ctx)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normed"])
@pytest.mark.parametrize("dim,hd,option,form", PAIR)
def test_rmsnorm_rope_bf16_pair(ops, dim, hd, option, form, exact):
    i = PAIR.index((dim, hd, option, form))
    c = R.rms_case(dim, hd, seed=900 + i, exact=exact, nseg=2, **R.GRIDS[i % 2])
    _run_pair(ops, c, option, form, f"pair dim={dim} hd={hd} RMS_PAIR_ROW={option} exact={exact}:")


def test_rmsnorm_rope_bf16_pair_takes_the_row_form_by_itself(ops):
    """8192 rows at width 128 with no option set: the one-wave-per-row kernel (1024 samples of 8 tokens, 2 x 2 x 2 or 1 x 1 x 7)"""
    grids = tuple((2, 2, 2) if b % 3 else (1, 1, 7) for b in range(1024))
    for rows, form in ((8192, "row"), (8184, "two_wg")):
        c = R.rms_case(128, 64, seq_len=8, grids=grids[:rows // 8], rope_len=2, seed=950, exact=True, nseg=2)
        _run_pair(ops, c, None, form, f"pair rows={rows} by itself:")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normed"])
@pytest.mark.parametrize("dim", [128, 256, 384, 1536, 1664, 5120])
def test_rmsnorm_rope_bf16_pair_bound(ops, dim, exact):
    c = R.rms_case(dim, 128, seed=960 + dim, exact=exact, nseg=2, xmax=3, **R.GRIDS[dim // 128 % 2])
    _run_pair(ops, c, None, None, f"pair_bound dim={dim} exact={exact}:", bound=True)


# ----------------------------------------------------------------------------------------------------------------------
# RMSNorm + RoPE, backward
# ----------------------------------------------------------------------------------------------------------------------
def _hold_rms_bwd(entry, c, dx, dw, ctx):
    """the dx [rows, dim] and dweight [1, dim] canvases of a one-segment backward against the reference, with their guards"""
    ref = R.rms_backward(c)
    if c.exact:
        _hold(entry, "dx", dx, R.rne_bf16(ref.dx), None, ctx)
        _hold(entry, "dweight", dw, R.G.exact_f32(ref.dw), None, ctx)
    else:
        _hold(entry, "dx", dx, ref.dx, R.bound_bf16(ref.dx, ref.S_dx), ctx)
        _hold(entry, "dweight", dw, ref.dw, R.bound_sum(ref.S_dw, "dweight"), ctx)


RMS_BWD = [dict(kw, types=t) for exact in (True, False) for i, kw in enumerate(R.rms_cases(exact))
           for t in (("f32", "f32", "bwd"), (("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16"), ("f32", "f32"))[i % 4] + ("bwd_t",))]


@pytest.mark.parametrize("cs", RMS_BWD, ids=_ids(RMS_BWD))
def test_rmsnorm_rope_bwd_and_bwd_t(ops, cs):
    kw = dict(cs)
    xt, gt, entry = kw.pop("types")
    c = R.rms_case(x_bf16=xt == "bf16", dy_bf16=gt == "bf16", **kw)
    ctx = f"{cs}:"
    p = RmsProblem(c, with_dy=True)
    dx = _out(c.rows, c.dim, c.dim + 12, BF16)
    dw = _out(1, c.dim, c.dim, F32, c.dw0[0][None])
    if entry == "bwd":
        rc = ops.lib.omh_rmsnorm_rope_bwd(p.x.ptr, p.ld, p.dy.ptr, p.ld, dx.ptr, c.dim + 12, dw.ptr, c.rows, c.dim, p.w[0].ptr, c.eps,
                                          c.do_norm, *p.table, ops._stream())
    else:
        rc = ops.lib.omh_rmsnorm_rope_bwd_t(p.x.ptr, int(c.x_bf16), p.ld, p.dy.ptr, int(c.dy_bf16), p.ld, dx.ptr, c.dim + 12, dw.ptr, c.rows,
                                            c.dim, p.w[0].ptr, c.eps, c.do_norm, *p.table, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ROUTES[f"rms_{entry}/chunks{_nv(c.dim)}/x_{xt}/dy_{gt}"] += 1
    _hold_rms_bwd("rmsnorm_rope_" + entry, c, dx, dw, ctx)
    p.hold_inputs(ctx)


# ----------------------------------------------------------------------------------------------------------------------
# gated residual
# ----------------------------------------------------------------------------------------------------------------------
GATED = [(dim, rows, rpb) for i, dim in enumerate(R.WIDTHS) for rows, rpb in (R.ROWS_RPB[i % 5], (100, 33))]


@pytest.mark.parametrize("dim,rows,rpb", GATED)
def test_gated_residual_forward_and_backward_are_exact(ops, dim, rows, rpb):
    c = R.gated_case(rows, dim, rpb, seed=dim)
    ref = R.gated_reference(c)
    ctx = f"gated dim={dim} rows={rows} rpb={rpb}:"
    xi, y = _in(c.xi), _in(c.y)
    g0, g1 = Vec(c.gate0), Vec(c.gate1, c.stride)
    xo = _out(rows, dim, dim, F32)
    rc = ops.lib.omh_gated_residual_fwd(xi.ptr, y.ptr, xo.ptr, rows, dim, c.gate_const, g0.ptr, g1.ptr, g1.stride, rpb, ops._stream())
    assert rc == 0, f"{ctx} omh_gated_residual_fwd returned {rc}"
    _sync()
    _hold("gated_residual_fwd", "xo", xo, ref.xo, None, ctx)
    for mode in ("0", "1"):             # atomics per 32-row block, then one adder per dgate element
        set_option("DETERMINISTIC", mode)
        dy, dgate = _out(rows, dim, dim, BF16), _out(c.nb, dim, dim + 8, F32, c.dgate0)
        rc = ops.lib.omh_gated_residual_bwd(xi.ptr, y.ptr, dy.ptr, dgate.ptr, dim + 8, rows, dim, c.gate_const, g0.ptr, g1.ptr, g1.stride, rpb,
                                            ops._stream())
        assert rc == 0, f"{ctx} omh_gated_residual_bwd returned {rc} (deterministic {mode})"
        _sync()
        ROUTES[f"gated_bwd/deterministic{mode}"] += 1
        _hold("gated_residual_bwd", "dy", dy, ref.dy, None, ctx)
        _hold("gated_residual_bwd", "dgate", dgate, ref.dgate, None, ctx)
    set_option("DETERMINISTIC", None)
    for cv, what in ((xi, "xi"), (y, "y")):
        cv.assert_guard(what, ctx)
    g0.assert_unchanged(ctx)
    g1.assert_unchanged(ctx)


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_widths_8196_and_6_are_refused(ops):
    lib, st = ops.lib, ops._stream()
    t = torch.zeros(4 * 8200, dtype=F32, device=DEV)
    p, z = t.data_ptr(), torch.zeros(8, dtype=torch.int32, device=DEV).data_ptr()
    for dim in (8196, 6):
        ld = 8200
        rope = (p, p, 4, 128, z, 2)
        assert lib.omh_layernorm_modulate(p, p, 2, dim, 1e-6, 1.0, None, None, 0, None, None, 0, 1, st) == E_SHAPE
        assert lib.omh_layernorm_modulate_bwd(p, p, p, 2, dim, 1e-6, 1.0, None, None, 0, None, None, 0, 1, st) == E_SHAPE
        a = ops._lib.LnBwdArgs(p, p, 0, p, 2, dim, 1e-6, 1.0, None, None, 0, None, None, 0, 1, None, None, 0.0, None, None, 0, None, 0, p, 1 << 20, None)
        assert lib.omh_layernorm_modulate_bwd2(C.byref(a), st) == E_SHAPE
        assert lib.omh_rmsnorm_rope(p, ld, p, 2, dim, None, 1e-6, 1, *rope, st) == E_SHAPE
        assert lib.omh_rmsnorm_rope_bf16(p, ld, p, 2, dim, None, 1e-6, 1, *rope, 1.0, st) == E_SHAPE
        assert lib.omh_rmsnorm_rope_bf16_pair(p, ld, 0, p, p, 2, dim, None, None, 1e-6, 1, *rope, 1.0, 1.0, st) == E_SHAPE
        assert lib.omh_rmsnorm_rope_bf16_pair_bound(p, ld, 0, p, p, 2, dim, None, None, 1e-6, 1, *rope, 1.0, 1.0, p, st) == E_SHAPE
        assert lib.omh_rmsnorm_rope_bwd(p, ld, p, ld, p, ld, None, 2, dim, None, 1e-6, 1, *rope, st) == E_SHAPE
        assert lib.omh_rmsnorm_rope_bwd_t(p, 1, ld, p, 1, ld, p, ld, None, 2, dim, None, 1e-6, 1, *rope, st) == E_SHAPE
        r = ops._lib.RmsBwdArgs()
        r.x = r.dy = r.dx = p
        r.ldx = r.lddy = r.lddx = ld
        r.n_seg, r.rows, r.dim, r.do_norm = 1, 2, dim, 1
        assert lib.omh_rmsnorm_rope_bwd2(C.byref(r), st) == E_SHAPE
    _sync()
    assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("dim,hd", [(24, 6), (36, 10), (256, 96), (260, 128), (8, 2)])
def test_a_head_that_splits_a_float4_or_the_width_is_refused(ops, dim, hd):
    """head_dim % 4 != 0 (a float4 would straddle two heads, the pair index would pass head_dim / 2) or dim % head_dim != 0:
    OMH_E_BADARG from the forward entries and from omh_rmsnorm_rope_bwd / _bwd_t alike"""
    lib, st = ops.lib, ops._stream()
    t = torch.zeros(4 * 512, dtype=F32, device=DEV)
    p, z = t.data_ptr(), torch.ones(8, dtype=torch.int32, device=DEV).data_ptr()
    rope = (p, p, 4, hd, z, 2)
    assert lib.omh_rmsnorm_rope(p, dim, p, 2, dim, None, 1e-6, 1, *rope, st) == E_BADARG
    assert lib.omh_rmsnorm_rope_bf16(p, dim, p, 2, dim, None, 1e-6, 1, *rope, 1.0, st) == E_BADARG
    assert lib.omh_rmsnorm_rope_bf16_pair(p, dim, 0, p, p, 2, dim, None, None, 1e-6, 1, *rope, 1.0, 1.0, st) == E_BADARG
    assert lib.omh_rmsnorm_rope_bwd(p, dim, p, dim, p, dim, None, 2, dim, None, 1e-6, 1, *rope, st) == E_BADARG
    assert lib.omh_rmsnorm_rope_bwd_t(p, 1, dim, p, 1, dim, p, dim, None, 2, dim, None, 1e-6, 1, *rope, st) == E_BADARG
    _sync()
    assert float(t.abs().max()) == 0.0
