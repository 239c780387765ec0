"""The index, reduction and step kernels of the DiT side (csrc/dit_elementwise.hip, csrc/dit_backward.hip: transpose,
column sums, cast, patchify / unpatchify and its adjoint, softmax backward, the four GELU entries, the tiny dense layer,
the sinusoidal embedding, the CFG + UniPC step, the flow x0 step) element for element against the float64 references of
tests/aux_exact_ref.py, through the C entries (ops.lib), so that pitches, offsets and aliases the Python wrappers forbid
can be passed.

Two kinds of assertion (aux_exact_ref's docstring derives both).  Where inputs can be chosen so that every evaluation
order gives the same bits — moves and roundings on random bit patterns, sums of small integers, the step kernels on
multiples of 1/2 — the bit patterns are compared.  Elsewhere every element is held to the bound of its own condition
sum.  Every operand sits in a canvas: NaN in pads and guard rows; inputs must keep their bits, outputs every byte
outside the logical window.

omh_transpose_bf16, omh_colsum_accum_multi and omh_flow_x0_step choose between two kernels: each case first asserts, in
Python, the dispatch condition restated from the .hip file; ``[routes]`` counts the kernels that ran, ``[measured]``
the worst ratio to the bound per entry and what is recorded without being asserted."""
import collections
import ctypes as C
import importlib

import pytest
import torch

import aux_exact_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTES = collections.Counter()
MEASURED = {}
GELU_CLASS = {}                                             # entry/class -> (worst ratio to the bound, worst share of delta used)
E_BADARG = -1
BF16, F32 = torch.bfloat16, torch.float32
ENTRIES = ("transpose_bf16", "colsum_accum", "colsum_accum_multi", "cast_f32_bf16", "patchify", "unpatchify", "unpatchify_bwd",
           "softmax_bwd_rows", "gelu_tanh_bf16", "gelu_tanh_bwd_bf16", "gelu_erf_bf16", "gelu_erf_bwd_bf16", "dense_f32",
           "dense_f32_bwd", "sinusoidal_embedding", "sinusoidal_embedding_bwd", "cfg_unipc_step", "flow_x0_step")


@pytest.fixture(scope="module", autouse=True)
def _summary_and_mode(ops):
    """the deterministic mode is process-wide: whatever a test leaves behind, the mode found here comes back"""
    prev = ops.lib.omh_set_deterministic(-1)
    try:
        yield
    finally:
        ops.lib.omh_set_deterministic(prev)
        print("\n[routes] " + "  ".join(f"{k}={v}" for k, v in sorted(ROUTES.items())))
        # WORST and COUNTS are shared with the norm tests of the same session: this file's entries alone
        print("[measured] worst ratio to the bound: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(R.WORST.items()) if k in ENTRIES))
        print("[measured] GELU by class, ratio to the bound | share of delta needed beyond the half ulp: " +
              "  ".join(f"{k}={a:.3f}|{b:.3f}" for k, (a, b) in sorted(GELU_CLASS.items())))
        print("[measured] recorded, not asserted: " + "  ".join(f"{k}={v}" for k, v in sorted(MEASURED.items())))
        print("[compared] " + "  ".join(f"{k}={v}" for k, v in sorted(R.COUNTS.items()) if k in ENTRIES))


def _sync():
    torch.cuda.synchronize()


def _in(t, pitch=None, off=0, **kw):
    """an input [rows, cols] ([n] as one row) in a NaN-filled allocation, armed: it must not change"""
    t = t[None] if t.dim() == 1 else t
    return R.Canvas(t.shape[-2], t.shape[-1], pitch or t.shape[-1], t.dtype, DEV, lead=1, trail=1, offset_bytes=off, **kw).put(t).arm()


def _out(rows, cols, dtype, pitch=None, init=None, off=0, **kw):
    cv = R.Canvas(rows, cols, pitch or cols, dtype, DEV, offset_bytes=off, **kw)
    if init is not None:
        cv.put(init[None] if init.dim() == 1 else init)
    return cv.arm()


def _hold(entry, what, cv, ref, bound, ctx, bits=False):
    """the window of canvas ``cv`` against the reference — bits: bit patterns; bound None: exact values — and its guards"""
    got = cv.window().reshape(ref.shape)
    if bits:
        msg = R.compare_bits(entry, what, got, ref, ctx)
    else:
        msg = R.compare(entry, what, got if bound is None else got.float(), ref, bound, ctx)
    assert msg is None, msg
    cv.assert_guard(what, ctx)


def _keep(ctx, **cvs):
    for what, cv in cvs.items():
        if cv is not None:
            cv.assert_guard(what, ctx)
            assert torch.equal(cv._bits(), cv._bits0), f"{ctx} the input {what} was written"


def _ids(cases):
    return ["-".join(f"{k}{v}" for k, v in cs.items() if k != "seed").replace(" ", "") for cs in cases]


class deterministic:
    def __init__(self, ops, on):
        self.lib, self.on = ops.lib, on

    def __enter__(self):
        self.prev = self.lib.omh_set_deterministic(-1)
        assert self.lib.omh_set_deterministic(self.on) == self.on

    def __exit__(self, *exc):
        self.lib.omh_set_deterministic(self.prev)


# ----------------------------------------------------------------------------------------------------------------------
# transpose
# ----------------------------------------------------------------------------------------------------------------------
TRANSPOSE = R.transpose_cases()


@pytest.mark.parametrize("cs", TRANSPOSE, ids=_ids(TRANSPOSE))
def test_transpose_both_routes(ops, cs):
    x = R.transpose_input(cs)
    want = R.transpose_ref(x)
    rows, cols, nb = cs["R"], cs["C"], cs["batch"]
    seen = {}
    for route in ("vec", cs["scalar"]):
        ctx = f"{cs} {route}:"
        g = R.transpose_geometry(cs, route)
        xin = _in(x if nb > 1 else x[0], g.ld_in, g.off, blocks=nb, block_stride=g.bs_in)
        out = _out(cols, rows, BF16, g.ld_out, off=g.off, blocks=nb, block_stride=g.bs_out)
        vec = R.transpose_takes_vec(g.ld_in, g.ld_out, g.bs_in, g.bs_out, xin.ptr, out.ptr)
        assert vec == (route == "vec"), f"{ctx} the case would run the {'vector' if vec else 'scalar'} kernel"
        rc = ops.lib.omh_transpose_bf16(xin.ptr, out.ptr, rows, cols, g.ld_in, g.ld_out, nb, g.bs_in, g.bs_out, ops._stream())
        assert rc == 0, f"{ctx} returned {rc}"
        _sync()
        ROUTES["transpose/" + ("vec" if vec else "scalar")] += 1
        _hold("transpose_bf16", "out", out, want, None, ctx, bits=True)
        _keep(ctx, x=xin)
        seen[route] = R.as_bits(out.window().reshape(want.shape).cpu())
    assert torch.equal(seen["vec"], seen[cs["scalar"]]), f"{cs}: the two routes differ"


# ----------------------------------------------------------------------------------------------------------------------
# column sums
# ----------------------------------------------------------------------------------------------------------------------
COLSUM1 = R.colsum_single_cases()
COLSUM_MULTI = R.colsum_multi_cases()


def _colsum_single(ops, e, exact, ctx):
    x, out0 = R.colsum_data(e, exact)
    xin, out = _in(x, e["ld"]), _out(1, e["C"], F32, init=out0)
    rc = ops.lib.omh_colsum_accum(xin.ptr, e["bf16"], e["ld"], out.ptr, e["R"], e["C"], ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    _keep(ctx, x=xin)
    return out, R.colsum_ref(x, out0)


@pytest.mark.parametrize("e", COLSUM1, ids=_ids(COLSUM1))
def test_colsum_single(ops, e):
    for mode in (0, 1):
        with deterministic(ops, mode):
            ctx = f"{e} deterministic {mode}:"
            out, ref = _colsum_single(ops, e, True, ctx)
            _hold("colsum_accum", "out", out, R.exact_f32(ref.out)[None], None, ctx)
    with deterministic(ops, 1):                              # randn: two runs give equal bits, each sum within R 2^-24 S
        ctx = f"{e} randn:"
        a, ref = _colsum_single(ops, e, False, ctx)
        b, _ = _colsum_single(ops, e, False, ctx)
        _hold("colsum_accum", "out", a, ref.out[None], (e["R"] * R.EPS24 * ref.S)[None], ctx)
        assert torch.equal(R.as_bits(a.window().cpu()), R.as_bits(b.window().cpu())), f"{ctx} two deterministic runs differ"


def _colsum_multi(ops, entries, exact, ctx, through_wrapper=False):
    """one batch on canvases; returns [(out canvas, reference)] and the input canvases"""
    wide, ins, prob = {}, [], []
    for e in entries:
        x, out0 = R.colsum_data(e, exact)
        if e.get("wide"):
            if "cv" not in wide:
                wide["cv"] = _in(x, e["ld"])
                ins.append(wide["cv"])
            cv, c0 = wide["cv"], e["wide"][1]
        else:
            cv, c0 = _in(x, e["ld"], off=e["off"] * x.element_size()), 0
            ins.append(cv)
        prob.append(R.NS(e=e, cv=cv, c0=c0, ptr=cv.ptr + c0 * x.element_size(), out=_out(1, e["C"], F32, init=out0),
                         ref=R.colsum_ref(R.colsum_block(e, x), out0)))
    for k in range(0, len(prob), 16):                       # one launch per 16 entries: its own choice of kernel
        chunk = prob[k:k + 16]
        vec = R.colsum_multi_takes_vec([p.e for p in chunk], [p.ptr for p in chunk])
        ROUTES["colsum_multi/" + ("vec" if vec else "scalar")] += 1
        if not through_wrapper:
            b = ops._lib.ColsumBatch()
            b.n = len(chunk)
            for i, p in enumerate(chunk):
                b.x[i], b.out[i], b.ld[i], b.R[i], b.C[i], b.is_bf16[i] = p.ptr, p.out.ptr, p.e["ld"], p.e["R"], p.e["C"], p.e["bf16"]
            rc = ops.lib.omh_colsum_accum_multi(C.byref(b), ops._stream())
            assert rc == 0, f"{ctx} returned {rc}"
    if through_wrapper:
        assert len(prob) == 17
        ops.colsum_accum_multi([(p.cv.window()[:, p.c0:p.c0 + p.e["C"]], p.out.window()[0]) for p in prob])
    _sync()
    for i, cv in enumerate(ins):
        _keep(ctx, **{f"x{i}": cv})
    return prob


@pytest.mark.parametrize("name", list(COLSUM_MULTI))
def test_colsum_multi(ops, name):
    entries = COLSUM_MULTI[name]
    wrapper = name == "n17_two_launches"
    ptrs_vec = name.startswith(("n", "column"))
    for mode in (0, 1):
        with deterministic(ops, mode):
            ctx = f"colsum_multi {name} deterministic {mode}:"
            before = ROUTES["colsum_multi/scalar"]
            for p in _colsum_multi(ops, entries, True, ctx, wrapper):
                _hold("colsum_accum_multi", "out", p.out, R.exact_f32(p.ref.out)[None], None, f"{ctx} {p.e}")
            assert (ROUTES["colsum_multi/scalar"] > before) == (not ptrs_vec), f"{ctx} the case names the other kernel"
    with deterministic(ops, 1):
        ctx = f"colsum_multi {name} randn:"
        a, b = _colsum_multi(ops, entries, False, ctx, wrapper), _colsum_multi(ops, entries, False, ctx, wrapper)
        for p, q in zip(a, b):
            _hold("colsum_accum_multi", "out", p.out, p.ref.out[None], (p.e["R"] * R.EPS24 * p.ref.S)[None], f"{ctx} {p.e}")
            assert torch.equal(R.as_bits(p.out.window().cpu()), R.as_bits(q.out.window().cpu())), f"{ctx} {p.e} two deterministic runs differ"


# ----------------------------------------------------------------------------------------------------------------------
# cast, patchify, unpatchify, unpatchify_bwd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_rounds_to_nearest_even(ops, n):
    x = R.f32_patterns(R._gen(45, n), (n,))
    ctx = f"cast n={n}:"
    xin, y = _in(x), _out(1, n, BF16)
    assert n <= 8192 * 256 * 4 or n == R.CAST_N[-1]
    rc = ops.lib.omh_cast_f32_bf16(xin.ptr, y.ptr, n, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    _hold("cast_f32_bf16", "y", y, R.rne_any(x)[None], None, ctx, bits=True)
    _keep(ctx, x=xin)


PATCHIFY, UNPATCHIFY, UNPATCHIFY_BWD = R.patchify_cases(), R.unpatchify_cases(), R.unpatchify_bwd_cases()


@pytest.mark.parametrize("cs", PATCHIFY, ids=_ids(PATCHIFY))
def test_patchify(ops, cs):
    d = R.patch_dims(cs)
    ctx = f"{cs}:"
    x = R.f32_patterns(R._gen(43, cs["seed"]), (cs["C"], d.F, d.H, d.W))
    xin, tok = _in(x.reshape(-1)), _out(d.tokens, d.Kp, BF16)
    rc = ops.lib.omh_patchify(xin.ptr, tok.ptr, cs["C"], d.F, d.H, d.W, d.pt, d.ph, d.pw, d.Kp, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    want = R.patchify_ref(x, cs)
    assert d.Kp == d.valid or bool((R.as_bits(want[:, d.valid:]) == 0).all()), "the pad columns of the reference are +0"
    _hold("patchify", "tokens", tok, want, None, ctx, bits=True)
    _keep(ctx, x=xin)


@pytest.mark.parametrize("cs", UNPATCHIFY, ids=_ids(UNPATCHIFY))
def test_unpatchify(ops, cs):
    d = R.patch_dims(cs)
    ctx = f"{cs}:"
    tok = R.f32_patterns(R._gen(44, cs["seed"]), (d.tokens, d.valid))
    tin, out = _in(tok), _out(1, cs["C"] * d.F * d.H * d.W, F32)
    rc = ops.lib.omh_unpatchify(tin.ptr, out.ptr, cs["C"], d.f, d.h, d.w, d.pt, d.ph, d.pw, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    _hold("unpatchify", "out", out, R.unpatchify_ref(tok, cs).reshape(1, -1), None, ctx, bits=True)
    _keep(ctx, tokens=tin)


@pytest.mark.parametrize("cs", UNPATCHIFY_BWD, ids=_ids(UNPATCHIFY_BWD))
def test_unpatchify_bwd(ops, cs):
    d = R.patch_dims(cs)
    ctx = f"{cs}:"
    g = R.f32_patterns(R._gen(46, cs["seed"]), (cs["C"], d.F, d.H, d.W))
    gin, dtok = _in(g.reshape(-1)), _out(d.tokens, d.valid, BF16)
    rc = ops.lib.omh_unpatchify_bwd(gin.ptr, dtok.ptr, cs["C"], d.f, d.h, d.w, d.pt, d.ph, d.pw, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    _hold("unpatchify_bwd", "dtok", dtok, R.unpatchify_bwd_ref(g, cs), None, ctx, bits=True)
    _keep(ctx, g=gin)


# ----------------------------------------------------------------------------------------------------------------------
# softmax backward
# ----------------------------------------------------------------------------------------------------------------------
SOFTMAX = R.softmax_cases()


@pytest.mark.parametrize("cs", SOFTMAX, ids=_ids(SOFTMAX))
def test_softmax_bwd_rows_is_exact(ops, cs):
    p, dp = R.softmax_data(cs)
    L, rows = cs["L"], cs["R"]
    ctx = f"{cs}:"
    pin, dpin, ds = _in(p, L + 2), _in(dp, L + 5), _out(rows, L, BF16, L + 3)
    rc = ops.lib.omh_softmax_bwd_rows(pin.ptr, L + 2, dpin.ptr, L + 5, ds.ptr, L + 3, rows, L, cs["scale"], ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    _hold("softmax_bwd_rows", "ds", ds, R.rne_bf16(R.softmax_bwd_ref(p, dp, cs["scale"])), None, ctx, bits=True)
    _keep(ctx, p=pin, dp=dpin)


# ----------------------------------------------------------------------------------------------------------------------
# GELU: all 65 536 patterns
# ----------------------------------------------------------------------------------------------------------------------
ALL = R.all_bf16_patterns()
FINITE = torch.isfinite(ALL.float())
NANS = torch.isnan(ALL.float())
GELU_BIG = 65 * 65536 + 3                                   # above the cap of 16384 x 256 threads


def _record_classes(entry, kind, got, ref, delta, keep):
    """the worst figures of one GELU call apart for the normal range, the tail, the flush range and subnormal results"""
    for name, mask in R.gelu_classes(kind, ALL.double(), ref).items():
        m = mask & keep
        if bool(m.any()):
            a = float(R.ratio_to_bound(got[m].float(), ref[m], R.bound_bf16(ref[m], delta[m])).max())
            b = R.delta_used(got[m].float(), ref[m], delta[m])
            old = GELU_CLASS.get(f"{entry}/{name}", (0.0, 0.0))
            GELU_CLASS[f"{entry}/{name}"] = (max(old[0], a), max(old[1], b))


def _record_inf(entry, got):
    f = ALL.float()
    MEASURED[entry + "(+inf)"] = float(got[(f == float("inf")).nonzero()[0, 0]])
    MEASURED[entry + "(-inf)"] = float(got[(f == float("-inf")).nonzero()[0, 0]])


@pytest.mark.parametrize("kind", ["tanh", "erf"])
def test_gelu_forward_on_every_pattern(ops, kind):
    entry = f"gelu_{kind}_bf16"
    fn = getattr(ops.lib, "omh_" + entry)
    ref, delta = (R.gelu_tanh_fwd if kind == "tanh" else R.gelu_erf_fwd)(ALL.double())
    xin, y = _in(ALL), _out(1, 1 << 16, BF16)
    assert fn(xin.ptr, y.ptr, 1 << 16, ops._stream()) == 0
    _sync()
    got = y.window()[0].cpu()
    msg = R.compare(entry, "y", got[FINITE].float(), ref[FINITE], R.bound_bf16(ref, delta)[FINITE], kind)
    assert msg is None, msg
    _record_classes(entry, kind, got, ref, delta, FINITE)
    assert bool(torch.isnan(got[NANS]).all()), f"{entry}: a NaN pattern gave a number"
    _record_inf(entry, got.float())
    y.assert_guard("y", kind)
    _keep(kind, x=xin)
    # the same patterns 65 times and 3 more, 2 bytes off a 16-byte boundary: the grid-stride loop makes a second trip
    big = torch.cat([ALL.repeat(65), ALL[:3]])
    xin, y2 = _in(big, off=2), _out(1, GELU_BIG, BF16, off=2)
    assert fn(xin.ptr, y2.ptr, GELU_BIG, ops._stream()) == 0
    _sync()
    want = torch.cat([got.repeat(65), got[:3]])
    assert torch.equal(R.as_bits(y2.window()[0].cpu()), R.as_bits(want)), f"{entry}: n = {GELU_BIG} differs from the single trip"
    y2.assert_guard("y", kind + " big")
    _keep(kind + " big", x=xin)


@pytest.mark.parametrize("dyk", R.GELU_DY)
@pytest.mark.parametrize("kind", ["tanh", "erf"])
def test_gelu_backward_on_every_pattern(ops, kind, dyk):
    entry = f"gelu_{kind}_bwd_bf16"
    fn = getattr(ops.lib, "omh_" + entry)
    dy = R.gelu_dy(dyk)
    ref, delta = (R.gelu_tanh_bwd if kind == "tanh" else R.gelu_erf_bwd)(dy.double(), ALL.double())
    keep = FINITE.clone()
    if kind == "tanh":                                      # the domain of omh.h: the fp32 overflow of P, from the restatement alone
        nan_set = R.tanh_grad_nan_set(ALL.float())
        assert int(nan_set.sum()) == R.tanh_grad_nan_count()
        keep &= ~nan_set
    off = 2 if dyk == "random" else 0
    dyin, xin, dx = _in(dy, off=off), _in(ALL, off=off), _out(1, 1 << 16, BF16, off=off)
    assert fn(dyin.ptr, xin.ptr, dx.ptr, 1 << 16, ops._stream()) == 0
    _sync()
    got = dx.window()[0].cpu()
    msg = R.compare(entry, "dx", got[keep].float(), ref[keep], R.bound_bf16(ref, delta)[keep], f"{kind} dy {dyk}")
    assert msg is None, msg
    _record_classes(entry, kind, got, ref, delta, keep)
    assert bool(torch.isnan(got[NANS]).all()), f"{entry}: a NaN pattern gave a number"
    if kind == "tanh":
        MEASURED["gelu_tanh_bwd_nan_set"] = int(nan_set.sum())
        MEASURED[f"gelu_tanh_bwd_nan_set_gave_nan({dyk})"] = int(torch.isnan(got[nan_set]).sum())
    if dyk == "one":
        _record_inf(entry, got.float())
    dx.assert_guard("dx", kind)
    _keep(kind, dy=dyin, x=xin)


# ----------------------------------------------------------------------------------------------------------------------
# the tiny dense layer
# ----------------------------------------------------------------------------------------------------------------------
DENSE_FWD, DENSE_BWD = R.dense_fwd_cases(), R.dense_bwd_cases()


@pytest.mark.parametrize("cs", DENSE_FWD, ids=_ids(DENSE_FWD))
def test_dense_f32(ops, cs):
    c = R.dense_data(cs)
    ctx = f"{cs}:"
    x, w, b, y = _in(c.x), _in(c.W), _in(c.bias) if cs["bias"] else None, _out(cs["B"], cs["N"], F32)
    rc = ops.lib.omh_dense_f32(x.ptr, w.ptr, b.ptr if b else None, y.ptr, cs["B"], cs["N"], cs["K"], cs["act_in"], cs["act_out"], ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ref = R.dense_fwd_ref(c, cs)
    if c.exact:
        _hold("dense_f32", "y", y, R.exact_f32(ref.y), None, ctx)
    else:
        _hold("dense_f32", "y", y, ref.y, R.K_AUX["dense_y"] * R.EPS24 * ref.S, ctx)
    _keep(ctx, x=x, W=w, bias=b)


@pytest.mark.parametrize("mode", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("cs", DENSE_BWD, ids=_ids(DENSE_BWD))
def test_dense_f32_bwd(ops, cs, mode):
    c = R.dense_data(cs, backward=True)
    ctx = f"{cs} deterministic {mode}:"
    B, N, K = cs["B"], cs["N"], cs["K"]
    x, w, dy = _in(c.x), _in(c.W), _in(c.dy)
    dW, db = _out(N, K, F32, init=c.dW0), _out(1, N, F32, init=c.db0)
    dx = _out(B, K, F32, init=c.dx0 if cs["acc"] else None)  # acc 0: the window holds NaN, the entry zeroes it itself
    want_w, want_x = cs["want"] != "dx", cs["want"] != "dW"
    use_db = cs["db"] and want_w
    with deterministic(ops, mode):
        rc = ops.lib.omh_dense_f32_bwd(x.ptr, w.ptr, dy.ptr, dW.ptr if want_w else None, db.ptr if use_db else None, dx.ptr if want_x else None,
                                       cs["acc"], B, N, K, cs["act_in"], ops._stream())
        assert rc == 0, f"{ctx} returned {rc}"
        _sync()
    ref = R.dense_bwd_ref(c, cs)
    for what, cv, used, start in (("dW", dW, want_w, c.dW0), ("db", db, use_db, c.db0), ("dx", dx, want_x, None)):
        r, S = getattr(ref, what).reshape(cv.rows, cv.cols), getattr(ref, "S_" + what).reshape(cv.rows, cv.cols)
        if not used:                                        # a NULL output: nothing moved
            _keep(ctx, **{what: cv})
        elif c.exact:
            _hold("dense_f32_bwd", what, cv, R.exact_f32(r), None, ctx)
        else:
            _hold("dense_f32_bwd", what, cv, r, R.K_AUX["dense_" + what] * R.EPS24 * S, ctx)
    _keep(ctx, x=x, W=w, dy=dy)


def test_dense_f32_bwd_refuses_a_bias_gradient_without_the_weight_gradient(ops):
    """db is summed by the launch that forms dW: with dW NULL it would silently stay as it was, so the entry refuses"""
    cs = dict(B=3, N=5, K=7, act_in=0, want="dx", db=True, acc=0, seed=99)
    c = R.dense_data(cs, backward=True)
    x, w, dy, db, dx = _in(c.x), _in(c.W), _in(c.dy), _out(1, 5, F32, init=c.db0), _out(3, 7, F32)
    assert ops.lib.omh_dense_f32_bwd(x.ptr, w.ptr, dy.ptr, None, db.ptr, dx.ptr, 0, 3, 5, 7, 0, ops._stream()) == E_BADARG
    _sync()
    _keep("refusal", db=db, dx=dx)


# ----------------------------------------------------------------------------------------------------------------------
# sinusoidal embedding
# ----------------------------------------------------------------------------------------------------------------------
SINUSOID = R.sinusoid_cases()


@pytest.mark.parametrize("cs", SINUSOID, ids=_ids(SINUSOID))
def test_sinusoidal_embedding_forward_and_backward(ops, cs):
    t = R.sinusoid_t(cs)
    B, dim = cs["B"], cs["dim"]
    ctx = f"{cs}:"
    tin, out = _in(t), _out(B, dim, F32)
    rc = ops.lib.omh_sinusoidal_embedding(tin.ptr, out.ptr, B, dim, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ref, bound = R.sinusoid_fwd_ref(t, dim)
    _hold("sinusoidal_embedding", "out", out, ref, bound, ctx)
    g = R._randn(R._gen(41, cs["seed"]), (B, dim)).float()
    gin, dt = _in(g), _out(1, B, F32)
    rc = ops.lib.omh_sinusoidal_embedding_bwd(gin.ptr, tin.ptr, dt.ptr, B, dim, ops._stream())
    assert rc == 0, f"{ctx} backward returned {rc}"
    _sync()
    ref, bound = R.sinusoid_bwd_ref(g, t)
    _hold("sinusoidal_embedding_bwd", "dt", dt, ref[None], bound[None], ctx)
    _keep(ctx, t=tin, dsin=gin)


# ----------------------------------------------------------------------------------------------------------------------
# CFG + UniPC step
# ----------------------------------------------------------------------------------------------------------------------
UNIPC = R.unipc_cases()


def _unipc_call(ops, c, cs, ctx):
    """one call on canvases; returns the canvases by name (an alias appears under both names)"""
    n, off = cs["n"], cs["off"]
    cv = R.NS(**{k: (_in(getattr(c, k), off=off) if getattr(c, k) is not None else None) for k in ("cond", "uncond", "x", "last", "m1", "m2")})
    cv.mt = _out(1, n, F32, off=off) if cs["outs"] else None
    cv.xc = cv.last if cs["alias"] == "xc_is_last" else (_out(1, n, F32, off=off) if cs["outs"] else None)
    cv.xn = cv.x if cs["alias"] == "xnext_is_x" else _out(1, n, F32, off=off)
    p = lambda v: v.ptr if v is not None else None                                  # noqa: E731
    rc = ops.lib.omh_cfg_unipc_step(p(cv.cond), p(cv.uncond), p(cv.x), p(cv.last), p(cv.m1), p(cv.m2), p(cv.mt), p(cv.xc), p(cv.xn), n,
                                    c.guide, c.sigma, cs["use_corr"], *c.ca, *c.pb, ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    return cv


def _unipc_hold(cv, cs, ref, ctx, exact):
    for what, out in (("mt", cv.mt), ("xc", cv.xc), ("xn", cv.xn)):
        if out is None:
            continue
        r = getattr(ref, what)[None]
        bound = None if exact else (R.N_R[what] * R.EPS24 * getattr(ref, "S_" + what))[None]
        _hold("cfg_unipc_step", what, out, R.exact_f32(r) if exact else r, bound, ctx)
    aliased = {"xc_is_last": "last", "xnext_is_x": "x"}.get(cs["alias"])
    _keep(ctx, **{k: getattr(cv, k) for k in ("cond", "uncond", "x", "last", "m1", "m2") if k != aliased})


@pytest.mark.parametrize("cs", UNIPC, ids=_ids(UNIPC))
def test_cfg_unipc_step_is_exact_on_multiples_of_a_half(ops, cs):
    c = R.unipc_data(cs)
    ctx = f"{cs}:"
    _unipc_hold(_unipc_call(ops, c, cs, ctx), cs, R.unipc_ref(c, cs), ctx, True)


@pytest.mark.parametrize("cs", UNIPC[:-1], ids=_ids(UNIPC[:-1]))
def test_cfg_unipc_step_on_a_real_schedule(ops, cs):
    coefs = R.unipc_schedule(importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc"))
    coef = coefs[0] if not cs["use_corr"] else coefs[2 if cs["m2"] else 1]         # order 1 | order 2 behind order 1 | order 2 / 2
    c = R.unipc_data(cs, exact=False, coef=coef)
    ctx = f"{cs} schedule:"
    _unipc_hold(_unipc_call(ops, c, cs, ctx), cs, R.unipc_ref(c, cs), ctx, False)


def test_cfg_unipc_step_refusals_leave_the_outputs_alone(ops):
    cs = dict(n=257, use_corr=1, m1=1, m2=1, outs=1, last=True, alias=None, off=0, seed=50)
    c = R.unipc_data(cs)
    ins = [_in(getattr(c, k)) for k in ("cond", "uncond", "x", "last", "m1", "m2")]
    outs = [_out(1, 257, F32) for _ in range(3)]
    pi, po = [v.ptr for v in ins], [v.ptr for v in outs]
    tail = (c.guide, c.sigma, 1, *c.ca, *c.pb, ops._stream())
    assert ops.lib.omh_cfg_unipc_step(pi[0], pi[1], pi[2], None, pi[4], pi[5], *po, 257, *tail) == E_BADARG        # use_corr, last NULL
    assert ops.lib.omh_cfg_unipc_step(*pi, *po, 0, *tail) == E_BADARG                                               # n = 0
    _sync()
    _keep("refusal", **{f"t{i}": v for i, v in enumerate(ins + outs)})


# ----------------------------------------------------------------------------------------------------------------------
# flow x0 step
# ----------------------------------------------------------------------------------------------------------------------
def _flow_call(ops, c, ctx, backward=False, nxt=True, off_v=0, alias=None, nulls=False):
    """one call on canvases: returns (x0 bits, x_next bits or None).  alias: 'x0_is_v' | 'x0_is_x' | 'xn_is_x' | 'xn_is_eps';
    nulls: x, eps, sigma_next NULL (backward)"""
    B, n = c.v.shape
    flat = lambda t: t.reshape(-1)                                                  # noqa: E731
    v, x, eps = _in(flat(c.v), off=off_v), None if nulls else _in(flat(c.x)), None if (nulls or not nxt) else _in(flat(c.eps))
    sg, sn = _in(c.sigma), None if (nulls or not nxt) else _in(c.sigma_next)
    x0 = {"x0_is_v": v, "x0_is_x": x}.get(alias) or _out(1, B * n, F32)
    xn = None if not nxt or backward else ({"xn_is_x": x, "xn_is_eps": eps}.get(alias) or _out(1, B * n, F32))
    p = lambda t: t.ptr if t is not None else None                                  # noqa: E731
    vec = R.flow_takes_vec(backward, p(v), p(x) or 0, p(eps) or 0, p(x0), p(xn) or 0)
    assert vec == (off_v == 0), f"{ctx} the case would run the {'vector' if vec else 'scalar'} route"
    rc = ops.lib.omh_flow_x0_step(p(v), p(x), p(eps), p(sg), p(sn), p(x0), p(xn), B, n, int(backward), ops._stream())
    assert rc == 0, f"{ctx} returned {rc}"
    _sync()
    ROUTES[f"flow_x0{'_bwd' if backward else ''}/" + ("vec" if vec else "scalar")] += 1
    want0, want1 = R.flow_ref(c, backward)
    _hold("flow_x0_step", "x0", x0, want0.reshape(1, -1), None, ctx, bits=True)
    if xn is not None:
        _hold("flow_x0_step", "x_next", xn, want1.reshape(1, -1), None, ctx, bits=True)
    written = {id(x0), id(xn)}
    _keep(ctx, **{k: t for k, t in (("v", v), ("x", x), ("eps", eps), ("sigma", sg), ("sigma_next", sn)) if id(t) not in written})
    return R.as_bits(x0.window().cpu()), None if xn is None else R.as_bits(xn.window().cpu())


@pytest.mark.parametrize("B,n", R.FLOW_SHAPES + (R.FLOW_BIG,))
def test_flow_x0_step_bit_for_bit_on_both_routes(ops, B, n):
    c = R.flow_data(B, n)
    ctx = f"flow B={B} n={n}"
    a = _flow_call(ops, c, ctx + " vec:")
    if (B, n) == R.FLOW_BIG:
        return
    b = _flow_call(ops, c, ctx + " scalar:", off_v=4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"{ctx}: the two routes differ"
    _flow_call(ops, c, ctx + " no x_next:", nxt=False)
    _flow_call(ops, c, ctx + " backward, NULLs:", backward=True, nulls=True)
    _flow_call(ops, c, ctx + " backward, scalar:", backward=True, off_v=4)


@pytest.mark.parametrize("alias", ["x0_is_v", "x0_is_x", "xn_is_x", "xn_is_eps"])
def test_flow_x0_step_permitted_aliases(ops, alias):
    for B, n in ((3, 7), (2, 4096)):
        _flow_call(ops, R.flow_data(B, n, seed=1), f"flow B={B} n={n} {alias}:", alias=alias)


def test_flow_x0_step_refusals(ops):
    c = R.flow_data(2, 3)
    t = [_in(v.reshape(-1)) for v in (c.v, c.x, c.eps)] + [_in(c.sigma), _in(c.sigma_next)]
    x0, xn = _out(1, 6, F32), _out(1, 6, F32)
    v, x, eps, sg, sn = (q.ptr for q in t)
    assert ops.lib.omh_flow_x0_step(v, None, eps, sg, sn, x0.ptr, xn.ptr, 2, 3, 0, ops._stream()) == E_BADARG      # forward without x
    assert ops.lib.omh_flow_x0_step(v, x, None, sg, sn, x0.ptr, xn.ptr, 2, 3, 0, ops._stream()) == E_BADARG        # x_next without eps
    _sync()
    _keep("refusal", x0=x0, xn=xn)


# ----------------------------------------------------------------------------------------------------------------------
def test_every_route_ran_and_every_entry_was_compared():
    """runs last in the file: each of the two kernels of the three dispatching entries was chosen at least once"""
    for r in ("transpose/vec", "transpose/scalar", "colsum_multi/vec", "colsum_multi/scalar", "flow_x0/vec", "flow_x0/scalar",
              "flow_x0_bwd/vec", "flow_x0_bwd/scalar"):
        assert ROUTES[r] > 0, f"route {r} never ran: {dict(ROUTES)}"
    for e in ENTRIES:
        assert R.COUNTS[e] > 0, f"entry {e} was never compared"
        assert R.WORST.get(e, 0.0) <= 1.0
