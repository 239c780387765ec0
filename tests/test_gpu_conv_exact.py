"""Every route of omh_conv_cl_bf16 (include/omh.h) element for element against the float64 reference of
tests/conv_exact_ref.py, and the RMS norm + SiLU behind it per element against float64 of its formula.

Operands are small integers (pair mode: integer hi, lo a multiple of 2^-9), so fp32 accumulation is exact in any order
and ``torch.equal`` holds for the 128 x 128 tile, the wide and the kw-shared 8-wave kernels, the one-wave-per-SIMD stream
with its fused-norm, pair and folded-upsample forms — bf16 outputs included (one RNE of an exact value).

Memory: x lies between a NaN frame before and one after it (and NaN frames past the ones the contract reads), w is
followed by NaN rows up to the column tile, bias / gamma / residuals are slices of NaN-filled buffers, y and norm_out
sit in canvases whose guard rows must keep their bits (the stream relies on buffer descriptors that drop the stores of
rows past M), and every input must keep its bits.

A route is forced through ``set_option``; before a case counts, the dispatch restated in conv_exact_ref.route_of (from
conv_route, the kw-shared condition and omh_conv_w64_takes / _pair_takes) must name the instantiation the case is
listed under, with the pointers of this very call.  The ``[routes]`` line at the end counts them."""
import collections
import ctypes as C

import pytest
import torch

import conv_exact_ref as R
from conftest import set_option

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTES = collections.Counter()
E_BADARG, E_ALIGN, E_SHAPE = -1, -2, -3
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[routes] " + "  ".join(f"{k}={ROUTES[k]}" for k in R.ALL_ROUTES))
    # (bf16 outputs sit at ~1 whenever a value lies next to a rounding midpoint: half an ulp of the 0.5 ulp + delta allowed;
    # the ":hi+lo" entries are held to delta alone and show what the fp32-class arithmetic uses of it)
    print("[measured] worst ratio to the bound: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(R.N.WORST.items()) if k.startswith("conv/")))


def _up(x, m):
    return (x + m - 1) // m * m


def _padded(t, lead, trail, what, off=0):
    """``t`` (flattened) inside a NaN-filled allocation with ``lead`` / ``trail`` elements around it, its first element
    16-byte aligned plus ``off`` bytes; returns (pointer, Frozen over the whole allocation)"""
    es = t.element_size()
    a16 = 16 // es
    start = _up(lead, a16) + off // es
    buf = torch.full((start + t.numel() + trail + a16,), float("nan"), dtype=t.dtype, device=DEV)
    buf[start:start + t.numel()] = t.flatten().to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf.data_ptr() + start * es, R.Frozen(buf, what)


def run_conv(ops, cs, c, resid_off=0, bias_off=0, wide_min=None, fuse=True, mutate=None, expect_rc=0, context=""):
    """One call of omh_conv_cl_bf16 for case ``c`` (conv_exact_ref.make_case) listed as ``cs`` (route, tile, kw3)."""
    lib, binding = ops.lib, ops._lib
    set_option("OMH_CONV_TILE", cs["tile"])
    set_option("OMH_CONV_KW3", "1" if cs["kw3"] else "0")
    set_option("OMH_CONV_FUSE_NORM", "1" if fuse else "0")
    set_option("OMH_CONV_WIDE_MIN", None if wide_min is None else str(wide_min))
    geo = {k: v for k, v in cs.items() if k not in ("route", "tile", "kw3")}
    ctx = f"[{cs['route']}] {context} tile={cs['tile']} kw3={cs['kw3']} {geo}:"
    frame = c.Hin * c.Win * c.Cin
    xp, xf = _padded(c.x, frame, frame, "x")
    coltile = R.COLUMN_TILE.get(cs["route"].split("/")[0], 128)
    wp, wf = _padded(c.w, 0, (_up(c.Cout, coltile) - c.Cout) * c.K, "w")
    frozen = [xf, wf]
    bp = gp = None
    if c.bias is not None:
        bp, f = _padded(c.bias, 16, 16, "bias", bias_off)
        frozen.append(f)
    if c.gamma is not None:
        gp, f = _padded(c.gamma, 16, 16, "norm_gamma")
        frozen.append(f)
    rows = c.M * c.fmul
    ydt = F32 if c.out_f32 else BF16
    Res = None
    if c.resid is not None:
        Res = R.Canvas(rows, c.cch, c.cch, c.resid.dtype, DEV, offset_bytes=resid_off).put(c.resid.reshape(rows, c.cch)).arm()
    Y = R.Canvas(rows, c.cch, c.cch, ydt, DEV, lead=4, trail=16).arm()
    yall = R.Frozen(Y.buf, "y")
    Nout = R.Canvas(c.M, c.Cout * (2 if c.pair else 1), c.Cout * (2 if c.pair else 1), BF16, DEV, lead=4, trail=16).arm() if c.norm else None
    a = binding.ConvArgs(xp, wp, bp, Res.ptr if Res else None, Y.ptr, c.Tin, c.Hin, c.Win, c.Cin, c.Tout, c.Hout, c.Wout, c.Cout,
                         c.KT, c.KH, c.KW, c.stride_t, c.stride_hw, c.pad_h, c.pad_w, c.up2, c.out_f32, c.split_n, c.resid_f32,
                         gp, Nout.ptr if Nout else None, int(c.norm_only), c.pair)
    if mutate is not None:
        mutate(a)
    else:
        got = R.route_of(c, cs["tile"], wide_min, cs["kw3"], fuse, Res.ptr if Res else 0, bp or 0)
        want = (cs["route"], c.norm and fuse and cs["route"].split("/")[0] in ("w64Pn", "pairPn"))
        assert got == want, f"{ctx} the route's precondition does not hold: the call would run on {got}, not {want}"
    rc = lib.omh_conv_cl_bf16(C.byref(a), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, f"{ctx} omh_conv_cl_bf16 returned {rc}, expected {expect_rc}"
    for f in frozen:
        f.check(ctx)
    if Res is not None:
        Res.assert_guard("resid", ctx)
        R.assert_exact(Res.window().reshape(c.out_shape), c.resid, c, "resid (an input)", ctx)
    if expect_rc != 0:
        yall.check(ctx + " a refused call wrote")
        if Nout is not None:
            Nout.assert_guard("norm_out", ctx)
            assert bool(torch.isnan(Nout.window()).all()), f"{ctx} a refused call wrote norm_out"
        return None
    ROUTES[cs["route"]] += 1
    ref = R.reference(c)
    Y.assert_guard("y", ctx)
    if c.norm_only and got[1]:
        yall.check(ctx + " norm_only:")                     # the fused kernel's empty descriptor: no y at all
    else:
        R.assert_exact(Y.window().reshape(c.out_shape), ref.y, c, "y", ctx)
    if Nout is not None:
        Nout.assert_guard("norm_out", ctx)
        nref = R.norm_reference(ref.y.double().reshape(c.M, c.Cout), c.gamma, True)
        entry = "conv/" + ("fused" if got[1] else "unfused") + ("_pair" if c.pair else "")
        if c.pair:
            hi, lo = R.unpack_split(Nout.window().cpu(), c.Cout, "pair")
            msgs = [R.N.compare(entry, "norm_out hi", hi.float(), nref.y, R.norm_bound(nref, "bf16"), ctx),
                    R.N.compare(entry + ":hi+lo", "norm_out hi + lo", hi.double() + lo.double(), nref.y, R.norm_bound(nref, "split"), ctx)]
        else:
            msgs = [R.N.compare(entry, "norm_out", Nout.window().float(), nref.y, R.norm_bound(nref, "bf16"), ctx)]
        assert all(m is None for m in msgs), [m for m in msgs if m]
    return Y.window().reshape(c.out_shape).clone()


def _run_family(ops, cases, chunk, nchunks):
    cases = list(enumerate(cases))[chunk::nchunks]
    assert cases
    for i, cs in cases:
        run_conv(ops, cs, R.build(cs, seed=i))


@pytest.mark.parametrize("chunk", range(4))
def test_voxel_tiling(ops, chunk):
    """M at 127 | 128 | 129, 511 | 512 | 513, 255 | 256 | 257, 509 | 510 | 511 and 253 | 254 | 255; tile boundaries on the last
    voxel of an image row, in mid row and inside the second frame; W = 3, 2, 1 (below 3 the kw-shared route is left); H = 1;
    a single voxel."""
    _run_family(ops, R.tiling_cases(), chunk, 4)


@pytest.mark.parametrize("chunk", range(4))
def test_channels_and_stage_counts(ops, chunk):
    _run_family(ops, R.channel_cases(), chunk, 4)


@pytest.mark.parametrize("chunk", range(4))
def test_geometry(ops, chunk):
    _run_family(ops, R.geometry_cases(), chunk, 4)


@pytest.mark.parametrize("chunk", range(4))
def test_epilogue_combinations(ops, chunk):
    _run_family(ops, R.epilogue_cases(), chunk, 4)


@pytest.mark.parametrize("chunk", range(2))
def test_pair_stream(ops, chunk):
    """x_hi w_hi + x_lo w_hi + x_hi w_lo and no lo lo, exactly; the query agrees with the entry"""
    cases = R.pair_cases()
    for i, cs in list(enumerate(cases))[chunk::2]:
        c = R.build(cs, seed=i)
        set_option("OMH_CONV_TILE", "w64")
        assert ops.conv_pair_supported(c.Tin, c.Hin, c.Win, c.Cin, c.Tout, c.Hout, c.Wout, c.Cout, c.KT, 3, 3, pad_h=1, pad_w=1, up2=bool(c.up2))
        run_conv(ops, cs, c)


def test_fused_norm_and_the_unfused_route(ops):
    """y exact and norm_out per element against float64 — in the stream's epilogue and, CONV_FUSE_NORM = 0, as
    omh_rms_silu_cl(_f32in / _pair) behind the same convolution"""
    for i, cs in enumerate(R.fused_norm_cases() + [cs for cs in R.pair_cases() if cs.get("norm")]):
        c = R.build(cs, seed=i)
        run_conv(ops, cs, c)
        plain = dict(cs, route=cs["route"].replace("w64Pn", "w64P").replace("pairPn", "pairP"))
        run_conv(ops, plain, c, fuse=False, context="unfused")


# ----------------------------------------------------------------------------------------------------------------------
# fallbacks, default routing, refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["wide", "w64"])
def test_alignment_fallbacks(ops, tile):
    """A bf16 residual 8 bytes off a 16-byte boundary takes the call to the 128 x 128 tile; a bias 4 bytes off takes it off the
    stream only; a residual 4 bytes off is OMH_E_ALIGN and nothing is written."""
    for Cout in (96, 192):
        wide = "wide<8,1>" if Cout == 96 else "wide<4,2>"
        for f, Cin in ((False, 160), (True, 40)):
            geo = dict(Cin=Cin, Cout=Cout, T=1, H=9, W=15, KT=1, bias=True, out_f32=f, resid="bf16")
            run_conv(ops, dict(geo, route=R._o("128x128", f), tile=tile, kw3=True), R.make_case(**geo, seed=1), resid_off=8, context="resid + 8")
            k3 = ("kw3<8,1>" if Cout == 96 else "kw3<4,2>") if Cin % 32 == 0 else wide
            run_conv(ops, dict(geo, route=R._o(k3, f), tile=tile, kw3=True), R.make_case(**geo, seed=2), bias_off=4, context="bias + 4")
            run_conv(ops, dict(geo, route="refused", tile=tile, kw3=True), R.make_case(**geo, seed=3), resid_off=4, mutate=lambda a: None,
                     expect_rc=E_ALIGN, context="resid + 4")
    # the aligned call of the same layer does take the stream under CONV_TILE = w64
    if tile == "w64":
        geo = dict(Cin=160, Cout=96, T=1, H=9, W=15, KT=1, bias=True, resid="bf16")
        run_conv(ops, dict(geo, route="w64P/bf16", tile=tile, kw3=True), R.make_case(**geo, seed=1))


DEFAULT_LAYERS = (      # (Cin, Cout, CONV_WIDE_MIN, (H, W) with one wide tile less than that, (H, W) with that many, the kernel there)
    (32, 96, 2, (16, 16), (1, 257), "kw3<8,1>"), (160, 96, 2, (16, 16), (1, 257), "w64P"), (40, 96, 2, (16, 16), (1, 257), "wide<8,1>"),
    (32, 192, 2, (8, 16), (3, 43), "kw3<4,2>"), (160, 192, 2, (8, 16), (3, 43), "w64Q"), (40, 200, 4, (8, 16), (3, 43), "wide<4,2>"))


@pytest.mark.parametrize("layer", DEFAULT_LAYERS, ids=lambda l: f"{l[0]}-{l[1]}")
def test_default_routing_counts_two_frames_whatever_tout_is(ops, layer):
    """No CONV_TILE, CONV_WIDE_MIN lowered: wide_tiles = ceil(2 H W / 512) for Cout <= 96, ceil(2 H W / 256) ceil(Cout / 192)
    beyond — H W = 256 | 257 and 128 | 129, one voxel either side of the threshold, for Tout = 1 and Tout = 3 (the count is
    taken for two frames whatever Tout is); frame 0 of the two calls bit for bit."""
    Cin, Cout, wmin, below, above, kernel = layer
    for (H, W), name in ((below, "128x128"), (above, kernel)):
        tiles = R.wide_tiles(R.NS(Hout=H, Wout=W, Cout=Cout))
        step = 1 if Cout <= 192 else 2
        assert tiles == (wmin - step if name == "128x128" else wmin)
        for f in (False, True):
            first = []
            for T in (1, 3):
                geo = dict(Cin=Cin, Cout=Cout, T=T, H=H, W=W, KT=1, bias=True, out_f32=f)
                cs = dict(geo, route=R._o(name, f), tile=None, kw3=True)
                run_conv(ops, cs, R.make_case(**geo, seed=T), wide_min=wmin, context="default routing")
            # values that are NOT exact: another kernel for the longer call would show in the low bits of frame 0
            set_option("OMH_CONV_TILE", None)
            set_option("OMH_CONV_WIDE_MIN", str(wmin))
            g = torch.Generator(device="cpu").manual_seed(Cin + Cout + H)
            x = torch.randn(3, H, W, Cin, generator=g).to(BF16).to(DEV)
            w = (torch.randn(Cout, 9 * Cin, generator=g) / (9 * Cin) ** 0.5).to(BF16).to(DEV)
            for T in (1, 3):
                first.append(ops.conv_cl(x[:T].contiguous(), w, None, T, H, W, Cout, 1, 3, 3, pad_h=1, pad_w=1, out_f32=f)[0])
            assert torch.equal(first[0], first[1]), f"{layer} {name}: frame 0 depends on Tout"


def test_refusals_leave_the_output_untouched(ops):
    geo = dict(Cin=32, Cout=96, T=2, H=5, W=7, KT=3, bias=True, out_f32=True)
    cs = dict(geo, route="refused", tile="wide", kw3=True)

    def cin12(a):
        a.Cin = 12

    def no_history(a):
        a.Tin = a.Tin - 1

    def bad_split(a):
        a.split_n = 40

    run_conv(ops, cs, R.make_case(**geo), mutate=cin12, expect_rc=E_SHAPE, context="Cin % 8")
    run_conv(ops, cs, R.make_case(**geo), mutate=no_history, expect_rc=E_SHAPE, context="history frames")
    run_conv(ops, cs, R.make_case(**geo), mutate=bad_split, expect_rc=E_SHAPE, context="Cout % split_n")
    # norm_gamma with split_n
    gs = dict(Cin=32, Cout=64, T=2, H=5, W=7, KT=3, KH=1, KW=1, norm=True)

    def split(a):
        a.split_n = 32

    run_conv(ops, dict(gs, route="refused", tile="wide", kw3=True), R.make_case(**gs), mutate=split, expect_rc=E_BADARG, context="norm + split_n")
    # pair on layers the query declines: an odd stage count, 48 real channels, a stride
    for Cin2, Cout, kw in ((160, 96, {}), (96, 96, {}), (224, 192, {}), (192, 96, dict(kind="down"))):
        ps = dict(Cin=Cin2, Cout=Cout, T=1, H=5, W=7, KT=1, pair=True, out_f32=True, **kw)
        c = R.make_case(**ps)
        set_option("OMH_CONV_TILE", "w64")
        assert not ops.conv_pair_supported(c.Tin, c.Hin, c.Win, c.Cin, c.Tout, c.Hout, c.Wout, c.Cout, c.KT, 3, 3, stride_hw=c.stride_hw,
                                           pad_h=c.pad_h, pad_w=c.pad_w)
        assert R.route_of(c, "w64")[0] == "E_SHAPE"
        run_conv(ops, dict(ps, route="refused", tile="w64", kw3=True), c, mutate=lambda a: None, expect_rc=E_SHAPE, context="pair declined")
    # ... and without the stream there is no pair kernel at all
    ps = dict(Cin=192, Cout=96, T=1, H=5, W=7, KT=1, pair=True, out_f32=True)
    run_conv(ops, dict(ps, route="refused", tile="wide", kw3=True), R.make_case(**ps), mutate=lambda a: None, expect_rc=E_SHAPE, context="pair, wide")


# ----------------------------------------------------------------------------------------------------------------------
# the norm entries
# ----------------------------------------------------------------------------------------------------------------------
ENTRIES = {"cl": ("omh_rms_silu_cl", BF16, 1, None), "f32in": ("omh_rms_silu_cl_f32in", F32, 1, None),
           "split3": ("omh_rms_silu_cl_split3", F32, 3, "split3"), "pair": ("omh_rms_silu_cl_pair", F32, 2, "pair")}


def _run_norm(ops, entry, x64, gamma, do_silu, exact=False, context=""):
    fn, xdt, nb, layout = ENTRIES[entry]
    P, Cc = x64.shape
    ctx = f"[{fn}] {context} P={P} C={Cc} do_silu={do_silu}:"
    xv = x64.to(xdt)
    assert torch.equal(xv.double(), x64)
    X = R.Canvas(P, Cc, Cc, xdt, DEV).put(xv).arm()
    Y = R.Canvas(P, nb * Cc, nb * Cc, BF16, DEV, lead=4, trail=16).arm()
    gp, gf = _padded(gamma, 16, 16, "gamma")
    rc = getattr(ops.lib, fn)(X.ptr, gp, Y.ptr, P, Cc, int(do_silu), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{ctx} returned {rc}"
    gf.check(ctx)
    X.assert_guard("x", ctx)
    R.G.assert_exact(X.window(), xv, None, "x (an input)", ctx)
    Y.assert_guard("y", ctx)
    ref = R.norm_reference(x64, gamma, do_silu)
    got = Y.window().cpu()
    hi, lo = (got, None) if layout is None else R.unpack_split(got, Cc, layout)
    if exact:
        R.G.assert_exact(hi.contiguous(), R.rne_bf16(ref.y), None, "y" if lo is None else "hi", ctx)
    else:
        msg = R.N.compare("conv/" + entry, "y" if lo is None else "hi", hi.float(), ref.y, R.norm_bound(ref, "bf16"), ctx)
        assert msg is None, msg
    if lo is not None:
        msg = R.N.compare("conv/" + entry + ":hi+lo", "hi + lo", hi.double() + lo.double(), ref.y, R.norm_bound(ref, "split"), ctx)
        assert msg is None, msg


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_rms_silu_entries_per_element(ops, entry):
    """C = 16, 96, 192, 384 x P = 1, 63 | 64 | 65, 77 (a workgroup takes 64 voxels up to 128 channels, 16 beyond) on exact
    convolution outputs with one all-zero voxel, both do_silu values; power-of-two voxels with do_silu = 0 exactly"""
    for Cc in R.NORM_C:
        assert 77 % R.rows_per_workgroup(Cc) != 0
        for P in R.NORM_P:
            gamma = R.norm_gamma(Cc, seed=P)
            x = R.norm_input(Cc, P, seed=Cc + P, bf16=entry == "cl")
            for do_silu in (False, True):
                _run_norm(ops, entry, x, gamma, do_silu)
        _run_norm(ops, entry, R.norm_input_pow2(Cc, 77, seed=Cc), R.norm_gamma(Cc, seed=1, pow2=True), False, exact=True, context="power of two")


def test_every_listed_instantiation_ran(ops):
    """(runs last in this module) the [routes] counts: every instantiation with fp32 and with bf16 output"""
    missing = [k for k in R.ALL_ROUTES if ROUTES[k] == 0]
    if sum(ROUTES.values()) < 300:
        return                                              # only part of this module was selected: nothing to say
    assert not missing, missing
