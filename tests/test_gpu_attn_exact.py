"""The attention entries of include/omh.h (csrc/attention.hip, attention_w64.hip, attention_bwd.hip, attention_bwd2.hip)
element for element against the float64 references of tests/attn_exact_ref.py on CODED inputs: Hadamard keys, integer
values, queries aimed at their own mask edges, 2^14 behind every k_lens and in the pad columns of vt (the construction,
the condition sums and the kappas are described there; tests/test_attn_exact_host.py shows on the CPU that the bound
reports a single leaked or dropped key, a band edge off by one, a wrong bottom-right shift, an unmasked ``whole`` tile, a
block list cut late, the neighbouring head's V and a shifted dk row).

Every element is held to a bound of its own (0.5 ulp_bf16 + kappa S for bf16, kappa S for fp32; flat rows of the forward
at the fp32-class kappa).  Exact, by ``torch.equal``: rows past q_lens, rows with an empty band and rows with k_lens = 0
(zero in o and o32, lse = -inf), dq of rows past q_lens, dk and dv of keys no live query sees, delta past q_lens, and
every result against a second run.  Outputs sit in NaN-filled canvases with guard rows; o / dq inside a buffer of row
stride 3 H 128 (the model's fused qkv / gradient buffers), ldv wider than roundup(Lk, 64); inputs are armed and must not
change.  The backward is fed the float64 forward rounded to fp32, so that a forward defect can neither hide nor fake a
backward one; one chained case per route feeds the forward kernel's own lse / o32.  The split-KV tail of the long-sequence
stream (more workgroups than CUs, 4096 keys) is held to an analytic reference: per-code means, no score matrix.  For the varlen and masked backward
entries the rows past q_lens of q, dout, lse and o32 hold NaN.

Each case first asserts, in Python, the dispatch condition it relies on (restated from the .hip files in
attn_exact_ref); ``[routes]`` counts the kernels that ran, ``[measured]`` the worst ratio to the bound per output."""
import collections
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

import attn_exact_ref as R
from conftest import set_option

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 128
ROUTES = collections.Counter()
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
ATTN_SHORT_KERNEL, ATTN_ALLOW_SPLIT = 1, 2
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[routes] " + "  ".join(f"{k}={v}" for k, v in sorted(ROUTES.items())))
    print(R.summary_line())
    print("[compared] " + "  ".join(f"{k}={v}" for k, v in sorted(R.COUNTS.items())))
    _REF.clear()


def _case(cs, requant=False):
    """the operands and the float64 forward of a case, computed once per module"""
    key = (R.ident(cs), cs.get("seed"), requant)
    if key not in _REF:
        base = _REF.get((R.ident(cs), cs.get("seed"), False))
        c = base[0] if base else R.build(cs)
        _REF[key] = (c, R.reference_forward(c, requant=requant))
    return _REF[key]


def _cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n - n % 8


def _rows(t):
    """[B, L, H, D] -> [B * L, H * D]"""
    return t.reshape(t.shape[0] * t.shape[1], -1)


def _in(t2, pitch=None, blocks=1, block_stride=0):
    """an input [rows, cols] in a NaN-filled allocation, armed: nothing of it may change"""
    return R.Canvas(t2.shape[-2], t2.shape[-1], pitch or t2.shape[-1], t2.dtype, DEV, lead=1, trail=1, blocks=blocks,
                    block_stride=block_stride).put(t2).arm()


def _out(rows, cols, pitch, dtype, guard=2):
    """an output window in a NaN-filled allocation with ``guard`` rows before and after it"""
    return R.Canvas(rows, cols, pitch, dtype, DEV, lead=guard, trail=guard).arm()


def _takes_w64(c, option, **kw):
    """attn_choice restated (attn_exact_ref.takes_w64) at the strides run_fwd uses"""
    return R.takes_w64(c.B, c.H, c.Lq, c.Lk, 3 * c.H * D, c.H * D + 64, 3 * c.H * D, c.ldv, option, **kw)


def _unchanged(cv, what, ctx):
    assert torch.equal(cv._bits(), cv._bits0), f"{ctx} the input {what} was written"


def _lens(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mask_of(ops, c):
    """the resolved ops.AttnMask of the case's mask (tables on the device), (left, right) of a band"""
    m = c.mask
    kw = dict(H=c.H, Lq=c.Lq, Lk=c.Lk, device=torch.device(DEV, torch.cuda.current_device()))
    if m.kind == "full":
        return None, (-1, -1)
    if m.kind == "band":
        return None, (m.left, m.right)
    if m.kind == "chunk":
        return ops.attn_mask(chunk_causal=(m.chunk, m.left_chunks, m.q_offset), **kw), (0, 0)
    if m.kind == "interval":
        from importlib import import_module
        causal = import_module(ops.__name__.rsplit(".", 1)[0] + ".causal")
        return ops.attn_mask(interval_mask=causal.IntervalMask(m.vis, m.group, runs=m.runs, k_group=m.k_group), **kw), (0, 0)
    return ops.attn_mask(block_mask=m.m if m.m.shape[0] > 1 else m.m[0], **kw), (0, 0)


def _mask_route(c):
    m = c.mask
    return {"full": "full", "band": "band", "chunk": "chunk", "block": f"block/heads{m.m.shape[0] if m.kind == 'block' else 0}",
            "interval": "interval" + ("_rect" if getattr(m, "k_group", None) else str(getattr(m, "runs", "")))}[m.kind]


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def run_fwd(ops, c, cs, *, lse=True, o32=False, flags=0, workspace=None, nm=None, bounded_entry=False, q=None):
    """one forward call on canvases -> the output canvases (o, o32, lse) and what must stay unchanged"""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    pq = po = 3 * H * D
    pk = H * D + 64
    r = NS(c=c, ctx=f"{cs}:")
    r.q, r.k, r.vt = _in(_rows(c.q if q is None else q), pq), _in(_rows(c.k), pk), _in(c.vt.reshape(B * H * D, c.ldv))
    r.o = _out(B * Lq, H * D, po, BF16)
    r.o32 = _out(B * Lq, H * D, po, F32) if o32 else None
    r.lse = _out(B * H, Lq, Lq, F32) if lse else None
    r.keep = (_lens(c.k_lens), _lens(c.q_lens), workspace, nm)
    mask, (wl, wr) = _mask_of(ops, c)
    a = ops._lib.AttnArgs(r.q.ptr, r.k.ptr, r.vt.ptr, r.o.ptr, _ptr(r.keep[0]), B, H, Lq, Lk, Lq * pq, pq, Lk * pk, pk, H * D * c.ldv,
                          Lq * po, po, c.ldv, c.scale, r.lse.ptr if lse else None, int(c.prescaled), _ptr(workspace),
                          workspace.numel() * workspace.element_size() if workspace is not None else 0, r.o32.ptr if o32 else None,
                          int(flags), _ptr(r.keep[1]), wl, wr)
    r.args = a
    if mask is not None:
        entry, st = ops._mask_entries(mask)[0], mask.c_struct()
        r.call = lambda: getattr(ops.lib, entry)(C.byref(a), C.byref(st), ops._stream())
        r.keep += (mask, st)
    elif bounded_entry:
        entry = "omh_flash_attn_fwd_d128_bounded"
        r.call = lambda: ops.lib.omh_flash_attn_fwd_d128_bounded(C.byref(a), _ptr(nm), ops._stream())
    else:
        entry = "omh_flash_attn_fwd_d128"
        r.call = lambda: ops.lib.omh_flash_attn_fwd_d128(C.byref(a), ops._stream())
    r.entry = entry
    return r


def launch(r):
    rc = r.call()
    assert rc == 0, f"{r.ctx} {r.entry} returned {rc}"
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                         # a fault: nothing more is started on this device
        pytest.exit(f"{r.ctx} {r.entry}: the GPU reported {e}", returncode=3)


def _bits(r, names):
    return [getattr(r, n)._bits().clone() for n in names if getattr(r, n, None) is not None]


def launch_twice(r, names):
    """run, keep the bits, run again: every result bit for bit"""
    launch(r)
    first = _bits(r, names)
    launch(r)
    for n, a, b in zip([n for n in names if getattr(r, n, None) is not None], first, _bits(r, names)):
        assert torch.equal(a, b), f"{r.ctx} {n}: the second run differs in {int((a != b).sum())} elements"


def hold_fwd(entry, r, ref, flat_ok=True, flat_key="o_flat"):
    c, ctx = r.c, r.ctx
    B, H, Lq = c.B, c.H, c.Lq
    delta = R.fwd_delta(c, ref, flat_ok, flat_key=flat_key)
    dead = c.dead.permute(0, 2, 1)[..., None].expand(B, Lq, H, D)
    for name, cv, is_bf in (("o", r.o, True), ("o32", r.o32, False)):
        if cv is None:
            continue
        got = cv.window().reshape(B, Lq, H, D).cpu()
        msg = R.compare(entry, name, got.float() if is_bf else got, ref.o, R.bound(ref.o, delta, None, is_bf), c, "bihd", ctx)
        assert msg is None, msg
        flat = c.flat.permute(0, 2, 1)[..., None].expand(B, Lq, H, D)
        if bool(flat.any()):                                          # the flat rows on their own line of ``[measured]``
            key = f"{entry}/{name}_flat{'' if flat_ok else '_at_kappa_o'}"
            half = 0.5 * R.ulp_bf16(ref.o.abs() + delta) if is_bf else torch.zeros_like(delta)       # what is left for delta alone
            R.WORST[key] = max(R.WORST[key], float(R.ratio_to_bound(((got.double() - ref.o).abs() - half).clamp_min(0.0), torch.zeros_like(delta), delta)[flat].max()))
        assert bool((got[dead] == 0).all()), f"{ctx} {name}: rows that see no key (past q_lens, empty band, k_lens = 0) must be exact zeros"
        cv.assert_guard(name, ctx)
    if r.lse is not None:
        got = r.lse.window().reshape(B, H, Lq).cpu()
        assert torch.equal(got[c.dead], torch.full_like(got[c.dead], -float("inf"))), f"{ctx} lse of rows that see no key must be -inf"
        live = ~c.dead
        msg = R.compare(entry, "lse", got[live], ref.lse[live], R.KAPPA["lse"] * ref.lse[live].abs().clamp_min(1.0), context=ctx)
        if msg is not None:
            b, h, i = (int(x) for x in live.nonzero()[int(R.ratio_to_bound(got[live], ref.lse[live], R.KAPPA["lse"] * ref.lse[live].abs().clamp_min(1.0)).argmax())])
            msg += " " + R.describe_row(c, b, h, i)
        assert msg is None, msg
        r.lse.assert_guard("lse", ctx)
    for cv, what in ((r.q, "q"), (r.k, "k"), (r.vt, "vt")):
        _unchanged(cv, what, ctx)


FWD_SHORT = R.fwd_short_cases()


@pytest.mark.parametrize("cs", FWD_SHORT, ids=[R.ident(cs) for cs in FWD_SHORT])
def test_forward_short(ops, cs):
    c, ref = _case(cs)
    set_option("ATTN_KERNEL", "base")
    r = run_fwd(ops, c, cs, lse=cs["lse"], o32=cs["o32"])
    assert not _takes_w64(c, "base", o32=cs["o32"], q_lens=c.q_lens is not None), f"{r.ctx} the case would take the long-sequence stream"
    assert R.short_split_plan(cs, _cus(), None)[1] == 0 and ops.lib.omh_flash_attn_workspace_bytes(C.byref(r.args)) == 0, f"{r.ctx} the case would split"
    launch_twice(r, ("o", "o32", "lse"))
    ROUTES["fwd/short/full"] += 1
    hold_fwd("fwd_short", r, ref)


FWD_SPLIT = R.fwd_split_cases()


@pytest.mark.parametrize("cs", FWD_SPLIT, ids=[R.ident(cs) for cs in FWD_SPLIT])
def test_forward_short_split_tail(ops, cs):
    c, ref = _case(cs)
    set_option("ATTN_KERNEL", "base")
    set_option("ATTN_SPLIT", "tail")
    n_regular, n_tail, splits = R.short_split_plan(cs, _cus())
    assert not _takes_w64(c, "base", o32=cs["o32"]), f"{cs}: the case would take the long-sequence stream"
    assert n_tail > 0 and (cs["Lk"] + 63) // 64 // splits >= 4, f"{cs}: the plan does not split ({n_regular}, {n_tail}, {splits})"
    need = n_tail * splits * 128 * (D + 1) * 4
    ws = torch.full((need // 4 + 16,), NAN, dtype=F32, device=DEV) if cs["workspace"] else None
    r = run_fwd(ops, c, cs, lse=cs["lse"], o32=cs["o32"], flags=ATTN_ALLOW_SPLIT, workspace=ws[:need // 4] if ws is not None else None)
    r.args.workspace, r.args.workspace_bytes = None, 0
    assert ops.lib.omh_flash_attn_workspace_bytes(C.byref(r.args)) == need, f"{r.ctx} workspace query against the restated plan {need}"
    if ws is not None:
        r.args.workspace, r.args.workspace_bytes = ws.data_ptr(), need
    launch_twice(r, ("o", "o32", "lse"))
    ROUTES[f"fwd/short/full/{'split' if ws is not None else 'split_withheld'}"] += 1
    hold_fwd("fwd_short_split", r, ref, flat_key="o_flat_split" if ws is not None else "o_flat")
    if ws is not None:
        assert bool(torch.isnan(ws[need // 4:]).all()), f"{r.ctx} the workspace was written past its {need} bytes"


BANDS = R.band_cases()


@pytest.mark.parametrize("cs", BANDS, ids=[R.ident(cs) for cs in BANDS])
def test_forward_band(ops, cs):
    c, ref = _case(cs)
    r = run_fwd(ops, c, cs, lse=cs["lse"], o32=cs["o32"])
    # a bounded side selects the short-sequence kernel's band instantiation, unsplit, whatever ATTN_KERNEL says
    assert (c.mask.left >= 0 or c.mask.right >= 0) and not _takes_w64(c, "w64", o32=cs["o32"], q_lens=c.q_lens is not None, band=True)
    assert R.short_split_plan(cs, _cus(), "tail")[1] == 0
    launch_twice(r, ("o", "o32", "lse"))
    ROUTES["fwd/short/band"] += 1
    hold_fwd("fwd_band", r, ref)


MASKED = R.masked_cases()


@pytest.mark.parametrize("cs", MASKED, ids=[R.ident(cs) for cs in MASKED])
def test_forward_masked(ops, cs):
    c, ref = _case(cs)
    r = run_fwd(ops, c, cs, lse=cs["lse"], o32=cs["o32"])
    assert R.masked_entry_accepts(c) and (r.args.window_left, r.args.window_right) == (0, 0), f"{r.ctx} the masked entry would refuse the call"
    launch_twice(r, ("o", "o32", "lse"))
    ROUTES["fwd/short/" + _mask_route(c)] += 1
    hold_fwd("fwd_" + c.mask.kind, r, ref)


W64 = R.w64_cases()


@pytest.mark.parametrize("cs", W64, ids=[R.ident(cs) for cs in W64])
def test_forward_w64(ops, cs):
    """the long-sequence stream (ATTN_KERNEL = "w64"), both schedules; ``bounded``: also the fixed-m stream through
    omh_flash_attn_fwd_d128_bounded, and, with one (sample, head) whose m > 48 / whose word is NaN, the plain call's bits"""
    requant = not cs["prescaled"]                                     # the stream re-rounds q * scale * log2(e) to bf16
    c, ref = _case(cs, requant)
    set_option("ATTN_KERNEL", "w64")
    set_option("W64_SCHED", cs["sched"])
    n_regular, n_tail, _ = R.w64_plan(c.B, c.H, c.Lq, c.Lk, _cus())
    assert n_tail == 0, f"{cs}: the case would split"
    assert _takes_w64(c, "w64") and not _takes_w64(c, None), f"{cs}: attn_choice: the stream only because ATTN_KERNEL forces it"
    r = run_fwd(ops, c, cs, lse=cs["lse"])
    launch_twice(r, ("o", "lse"))
    ROUTES[f"fwd/w64/v2/sched{cs['sched']}/pre{int(cs['prescaled'])}"] += 1
    hold_fwd("fwd_w64", r, ref)
    if not cs["bounded"]:
        return
    plain = _bits(r, ("o", "lse"))
    assert ops.lib.omh_flash_attn_takes_bounded(C.byref(r.args)) == 1, f"{r.ctx} omh_flash_attn_takes_bounded"
    nm = R.qk_norm2_max(c)
    assert R.bound_m(c, nm) <= 48
    rb = run_fwd(ops, c, cs, lse=cs["lse"], nm=nm.to(DEV), bounded_entry=True)
    launch_twice(rb, ("o", "lse"))
    ROUTES[f"fwd/w64/v4/sched{cs['sched']}/pre{int(cs['prescaled'])}"] += 1
    hold_fwd("fwd_w64_bounded", rb, ref, flat_ok=R.flat_ok(c, "fixed"))
    for what, word in (("m > 48", 1.0e6), ("a NaN word", NAN)):
        bad = nm.clone()
        bad[:, :, 0] = word                                           # every workgroup: the call is the plain one
        rp = run_fwd(ops, c, cs, lse=cs["lse"], nm=bad.to(DEV), bounded_entry=True)
        launch(rp)
        for n, a, b in zip(("o", "lse"), plain, _bits(rp, ("o", "lse"))):
            assert torch.equal(a, b), f"{r.ctx} {n} with {what} in the norm buffer differs from the plain call"
        bad = nm.clone()
        bad[0, 0, 1] = word                                           # one (sample, head): still inside the bound everywhere
        rp = run_fwd(ops, c, cs, lse=cs["lse"], nm=bad.to(DEV), bounded_entry=True)
        launch(rp)
        hold_fwd("fwd_w64_bounded", rp, ref, flat_ok=R.flat_ok(c, "fixed"))
        got, want = rp.o.window().reshape(c.B, c.Lq, c.H, D)[0, :, 0], r.o.window().reshape(c.B, c.Lq, c.H, D)[0, :, 0]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{r.ctx} o of sample 0 head 0 with {what} differs from the plain call"
        if rp.lse is not None:
            got, want = rp.lse.window().reshape(c.B, c.H, c.Lq)[0, 0], r.lse.window().reshape(c.B, c.H, c.Lq)[0, 0]
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{r.ctx} lse of sample 0 head 0 with {what} differs from the plain call"
    ROUTES["fwd/w64/v4/fallback"] += 1


def test_forward_w64_split_kv_tail(ops):
    """the split-KV tail of the long-sequence stream: more workgroups than CUs with a remainder <= 64 and at least 64 key
    tiles (w64_plan, restated); held to the analytic reference (per-code means), the tail tiles' flat rows at the split
    kappa (their slabs are weighted by exp(lse_s - max lse))"""
    cus = _cus()
    B, H, Lk = 2, 3, 4096
    q_tiles = (cus + 2 + B * H - 1) // (B * H)                       # B H q_tiles = cus + r with a small r
    Lq = (q_tiles - 1) * 256 + 100
    n_regular, n_tail, splits = R.w64_plan(B, H, Lq, Lk, cus)
    if n_tail == 0:
        print(f"[skipped] w64 split-KV tail: {B * H * q_tiles} workgroups on {cus} CUs give an empty plan")
        pytest.skip(f"{B * H * q_tiles} workgroups on {cus} CUs: w64_plan does not split")
    c = R.analytic_case(B, H, Lq, Lk, [Lk, Lk - 36])
    ref = R.analytic_forward(c)
    cs = c.cs
    set_option("ATTN_KERNEL", "w64")
    assert _takes_w64(c, "w64"), f"{cs}: attn_choice"
    need = n_tail * splits * 256 * (D + 1) * 4
    ws = torch.full((need // 4 + 16,), NAN, dtype=F32, device=DEV)
    r = run_fwd(ops, c, cs, lse=True, workspace=ws[:need // 4])
    assert ops.lib.omh_flash_attn_workspace_bytes(C.byref(r.args)) == need, f"{r.ctx} workspace query against the restated plan {need}"
    assert ops.lib.omh_flash_attn_takes_bounded(C.byref(r.args)) == 0, f"{r.ctx} a split launch does not look at the norm buffer"
    launch_twice(r, ("o", "lse"))
    ROUTES[f"fwd/w64/v2+v3/tail{n_tail}x{splits}"] += 1
    tail = torch.zeros(B * H * q_tiles, 256, dtype=torch.bool)
    tail[n_regular:] = True
    tail = tail.reshape(B, H, q_tiles * 256)[:, :, :Lq].permute(0, 2, 1)[..., None]                   # [B, Lq, H, 1]
    delta = torch.where(tail, R.fwd_delta(c, ref, flat_key="o_flat_split"), R.fwd_delta(c, ref))
    got = r.o.window().reshape(B, Lq, H, D).cpu().float()
    msg = R.compare("fwd_w64_tail", "o", got, ref.o, R.bound(ref.o, delta, None, True), context=r.ctx)
    if msg is not None:
        rat = R.ratio_to_bound(got, ref.o, R.bound(ref.o, delta, None, True))
        b, i, h, _ = (int(x) for x in torch.unravel_index(rat.argmax(), rat.shape))
        msg += (f" sample {b} head {h} row {i} (workgroup {(b * H + h) * q_tiles + i // 256}, {'tail' if bool(tail[b, i, h]) else 'regular'}) "
                f"code {int(c.qc[b, h, i])}{' graded with ' + str(int(c.qc2[b, h, i])) if bool(c.graded[b, h, i]) else ''}, klen {c.kl[b]}")
    assert msg is None, msg
    got = r.lse.window().reshape(B, H, Lq).cpu()
    msg = R.compare("fwd_w64_tail", "lse", got, ref.lse, R.KAPPA["lse"] * ref.lse.abs().clamp_min(1.0), context=r.ctx)
    assert msg is None, msg
    r.o.assert_guard("o", r.ctx)
    r.lse.assert_guard("lse", r.ctx)
    for cv, what in ((r.q, "q"), (r.k, "k"), (r.vt, "vt")):
        _unchanged(cv, what, r.ctx)
    assert bool(torch.isnan(ws[need // 4:]).all()), f"{r.ctx} the workspace was written past its {need} bytes"


# ----------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------
def run_bwd(ops, c, cs, lse, o32, *, entry="plain", phase=0, out_bf16=False, workspace=None, own_lo=0, nan_rows=False, share=None):
    """one backward call (o32 kernels) on canvases.  lse [B, H, Lq], o32 [B, Lq, H, D] fp32: what the kernel is fed.
    nan_rows: rows past q_lens of q, dout, lse and o32 hold NaN.  share: an earlier call of the same case whose canvases
    (delta included) this phase goes on with."""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    pq, pk, po = 3 * H * D, H * D + 64, H * D + 8
    Lown = Lk - own_lo
    if share is not None:
        r = share
    else:
        r = NS(c=c, ctx=f"{cs}:")
        q, dout, lse_in, o_in = c.q.clone(), c.dout.clone(), lse.clone().float(), o32.clone().float()
        if nan_rows:
            for b in range(B):
                q[b, c.ql[b]:], dout[b, c.ql[b]:], lse_in[b, :, c.ql[b]:], o_in[b, c.ql[b]:] = NAN, NAN, NAN, NAN
        kbs = (Lk + 5) * pk if own_lo else Lk * pk                   # cached: k_bs wider than Lk rows
        r.kbs = kbs
        kv = dict(blocks=B, block_stride=kbs) if own_lo else {}
        r.q, r.dout = _in(_rows(q), pq), _in(_rows(dout), po)
        r.k = _in(c.k.reshape(B, Lk, H * D) if own_lo else _rows(c.k), pk, **kv)
        r.v = _in(c.v.reshape(B, Lk, H * D) if own_lo else _rows(c.v), pk, **kv)
        r.lse_in, r.o32_in = _in(lse_in.reshape(B * H, Lq)), _in(_rows(o_in), po)
        gt = BF16 if out_bf16 else F32
        # cached: own_lo + 2 guard rows around dk / dv, so that a row written at r - own_lo or at own_lo + r lands in the guard
        r.dq, r.dk, r.dv = _out(B * Lq, H * D, pq, gt), _out(B * Lown, H * D, pk, gt, own_lo + 2), _out(B * Lown, H * D, pk, gt, own_lo + 2)
        r.delta = _out(B * H, Lq, Lq, F32)
        r.keep = (_lens(c.k_lens), _lens(c.q_lens), workspace)
        r.mask, (r.wl, r.wr) = _mask_of(ops, c)
    a = ops._lib.AttnBwdArgs(r.q.ptr, r.k.ptr, r.v.ptr, None, r.dout.ptr, None, None, None, r.lse_in.ptr, r.delta.ptr, r.dq.ptr, r.dk.ptr,
                             r.dv.ptr, _ptr(r.keep[0]), B, H, Lq, Lk, Lq * pq, pq, r.kbs, pk, Lq * po, po, Lq * pq, pq, Lown * pk, pk, 0, 0, 0, 0,
                             c.scale, int(c.prescaled), int(out_bf16), r.o32_in.ptr, int(phase), _ptr(workspace),
                             workspace.numel() * workspace.element_size() if workspace is not None else 0)
    r.args, lib, s = a, ops.lib, ops._stream
    ql = _ptr(r.keep[1])
    if r.mask is not None:
        name, st = ops._mask_entries(r.mask)[1], r.mask.c_struct()
        r.keep += (st,)
        r.call = lambda: getattr(lib, name)(C.byref(a), ql, C.byref(st), s())
    elif entry == "varlen":
        name = "omh_flash_attn_bwd_varlen_d128"
        r.call = lambda: lib.omh_flash_attn_bwd_varlen_d128(C.byref(a), ql, r.wl, r.wr, s())
    elif entry == "band":
        name = "omh_flash_attn_bwd_band_d128"
        r.call = lambda: lib.omh_flash_attn_bwd_band_d128(C.byref(a), r.wl, r.wr, s())
    elif entry == "cached":
        name = "omh_flash_attn_bwd_cached_d128"
        r.call = lambda: lib.omh_flash_attn_bwd_cached_d128(C.byref(a), own_lo, s())
    else:
        name = "omh_flash_attn_bwd_d128"
        r.call = lambda: lib.omh_flash_attn_bwd_d128(C.byref(a), s())
    r.entry, r.out_bf16, r.own_lo = name, out_bf16, own_lo
    return r


def hold_bwd(entry, r, ref):
    c, ctx = r.c, r.ctx
    B, H, Lq, Lk, lo = c.B, c.H, c.Lq, c.Lk, r.own_lo
    bf = r.out_bf16
    dead = c.dead.permute(0, 2, 1)[..., None].expand(B, Lq, H, D)
    unseen = (~c.vis.any(2)).permute(0, 2, 1)[:, lo:, :, None].expand(B, Lk - lo, H, D)
    for name, cv, rows, want, S, layout in (("dq", r.dq, Lq, ref.dq, ref.S_dq, "bihd"), ("dk", r.dk, Lk - lo, ref.dk[:, lo:], ref.S_dk[:, lo:], "bjhd"),
                                            ("dv", r.dv, Lk - lo, ref.dv[:, lo:], ref.S_dv[:, lo:], "bjhd")):
        got = cv.window().reshape(B, rows, H, D).cpu()
        msg = R.compare(entry, name + ("_bf16" if bf else ""), got.float() if bf else got, want, R.bound(want, S, R.KAPPA[name], bf), c,
                        layout if not lo or name == "dq" else None, ctx + (f" own_lo {lo}: row r is key {lo} + r;" if lo else ""))
        assert msg is None, msg
        zero = dead if name == "dq" else unseen
        assert bool((got[zero] == 0).all()), f"{ctx} {name}: " + ("rows that see no key" if name == "dq" else "keys no live query sees") + " must be exact zeros"
        cv.assert_guard(name, ctx)
    got = r.delta.window().reshape(B, H, Lq).cpu()
    live = ~c.dead
    msg = R.compare(entry, "delta", got[live], ref.delta[live], R.KAPPA["delta"] * ref.S_delta[live], context=ctx)
    assert msg is None, msg
    past = torch.zeros(B, H, Lq, dtype=torch.bool)
    for b in range(B):
        past[b, :, c.ql[b]:] = True
    if c.q_lens is not None:
        assert bool((got[past] == 0).all()), f"{ctx} delta past q_lens must be exact zeros"
    r.delta.assert_guard("delta", ctx)
    for cv, what in ((r.q, "q"), (r.k, "k"), (r.v, "v"), (r.dout, "dout"), (r.lse_in, "lse"), (r.o32_in, "o32")):
        _unchanged(cv, what, ctx)


def _fed(ref):
    """what the backward is fed: the float64 forward rounded to fp32"""
    return ref.lse.float(), ref.o.float()


def _bwd_twice(r, phases):
    """phase 0, or phases 1, 2 + 3 on the same canvases; twice, bit for bit"""
    names = ("dq", "dk", "dv", "delta")
    for rep in range(2):
        if phases:
            for ph in (1, 2, 3):
                r.args.phase = ph
                launch(r)
        else:
            launch(r)
        if rep == 0:
            first = _bits(r, names)
    for n, a, b in zip(names, first, _bits(r, names)):
        assert torch.equal(a, b), f"{r.ctx} {n}: the second run differs in {int((a != b).sum())} elements"


BWD = R.bwd_cases()


@pytest.mark.parametrize("cs", BWD, ids=[R.ident(cs) for cs in BWD])
def test_backward_o32(ops, cs):
    """omh_flash_attn_bwd_d128 with o32: ATTN_BWD_W64 "0" (both HIP kernels), "k" (the dK / dV stream), default (both
    streams); phases; bf16 gradients; the split tail with and without workspace"""
    c, ref0 = _case(cs)
    if cs["w64"] is not None:
        set_option("ATTN_BWD_W64", cs["w64"])
    split = cs.get("split", False)
    set_option("ATTN_SPLIT", "tail" if split else "0")
    lse, o32 = _fed(ref0)
    ref = R.reference_backward(c, lse, o32)
    ws = None
    if split:
        pq, pk = R.bwd_split_plan(cs, _cus(), True), R.bwd_split_plan(cs, _cus(), False)
        assert pq[1] > 0 and pk[1] > 0, f"{cs}: the plans do not split: dQ {pq}, dK / dV {pk}"
        need = (pq[1] * pq[2] + 2 * pk[1] * pk[2]) * 128 * D * 4
        ws = torch.full((need // 4 + 16,), NAN, dtype=F32, device=DEV)
    r = run_bwd(ops, c, cs, lse, o32, out_bf16=cs["out_bf16"], workspace=ws[:need // 4] if (split and cs["workspace"]) else None)
    if split:
        r.args.phase = 0
        assert ops.lib.omh_flash_attn_bwd_workspace_bytes(C.byref(r.args)) == need, f"{r.ctx} workspace query against the restated plans {need}"
    _bwd_twice(r, cs["phases"])
    dq_stream = cs["w64"] is None
    ROUTES[f"bwd/dq/{'w64' if dq_stream else 'hip'}/pre{int(cs['prescaled'])}" + ("/split" if split and cs["workspace"] else "")] += 1
    ROUTES[f"bwd/dkdv/{'hip' if cs['w64'] == '0' else 'w64'}/pre{int(cs['prescaled'])}" + ("/split" if split and cs["workspace"] else "")] += 1
    ROUTES["bwd/phases123" if cs["phases"] else "bwd/phase0"] += 1
    hold_bwd("bwd_o32", r, ref)
    if ws is not None:
        assert bool(torch.isnan(ws[need // 4:]).all()), f"{r.ctx} the workspace was written past its {need} bytes"


@pytest.mark.parametrize("cs", BANDS + MASKED, ids=[R.ident(cs) for cs in BANDS + MASKED])
def test_backward_masked(ops, cs):
    """band (no q_lens: omh_flash_attn_bwd_band_d128), varlen, and the five masked entries, NaN past q_lens"""
    c, ref0 = _case(cs)
    lse, o32 = _fed(ref0)
    ref = R.reference_backward(c, lse, o32)
    seed = cs["seed"]
    entry = "masked" if c.mask.kind != "band" else ("band" if c.q_lens is None else "varlen")
    r = run_bwd(ops, c, cs, lse, o32, entry=entry, out_bf16=bool(seed % 3 == 0), nan_rows=c.q_lens is not None)
    # the band / varlen / masked entries: o32 set, the HIP kernels' instantiation of the mask kind, the workspace declined
    assert r.args.o32 and not r.args.workspace and (R.masked_entry_accepts(c) if entry == "masked" else (r.wl >= 0 or r.wr >= 0)), r.ctx
    _bwd_twice(r, phases=bool(seed % 2))
    ROUTES[f"bwd/{entry if entry != 'masked' else _mask_route(c)}/pre{int(c.prescaled)}"] += 1
    hold_bwd("bwd_" + (entry if entry != "masked" else c.mask.kind), r, ref)


VARLEN_FULL = [dict(B=2, H=2, Lq=129, Lk=200, q_lens=[129, 65], k_lens=[0, 200], prescaled=True, seed=160),
               dict(B=2, H=3, Lq=257, Lk=65, q_lens=[0, 200], k_lens=[65, 64], prescaled=False, seed=161)]


@pytest.mark.parametrize("cs", VARLEN_FULL, ids=[R.ident(cs) for cs in VARLEN_FULL])
def test_backward_varlen_full(ops, cs):
    """omh_flash_attn_bwd_varlen_d128 with the unbounded band: q_lens 0, k_lens 0"""
    c, ref0 = _case(cs)
    lse, o32 = _fed(ref0)
    r = run_bwd(ops, c, cs, lse, o32, entry="varlen", nan_rows=True)
    _bwd_twice(r, phases=False)
    ROUTES[f"bwd/varlen_full/pre{int(c.prescaled)}"] += 1
    hold_bwd("bwd_varlen", r, R.reference_backward(c, lse, o32))


CACHED = R.cached_cases()


@pytest.mark.parametrize("cs", CACHED, ids=[R.ident(cs) for cs in CACHED])
def test_backward_cached(ops, cs):
    """omh_flash_attn_bwd_cached_d128: row r of dk / dv is key own_lo + r; the canvas in front of dk / dv stays untouched"""
    c, ref0 = _case(cs)
    lse, o32 = _fed(ref0)
    set_option("ATTN_SPLIT", "0")
    r = run_bwd(ops, c, cs, lse, o32, entry="cached", own_lo=cs["own_lo"], out_bf16=cs["out_bf16"])
    _bwd_twice(r, phases=bool(cs["seed"] % 2))
    ROUTES["bwd/cached"] += 1
    hold_bwd("bwd_cached", r, R.reference_backward(c, lse, o32))


OLD = R.bwd_old_cases()


@pytest.mark.parametrize("cs", OLD, ids=[R.ident(cs) for cs in OLD])
def test_backward_without_o32(ops, cs):
    """the kernels of csrc/attention_bwd.hip, through the transposed operands that ops.flash_attn_bwd makes; their delta
    comes from a pass over the keys (rowsum(P dP)), so o32 plays no part.  Going through ops.flash_attn_bwd means its own
    allocations: dq, dk and dv are held per element without guard rows and the inputs must keep their bits; delta, the one
    buffer the caller may hand in, sits in a guarded canvas and is held to sum_j P_ij dP_ij (KAPPA["delta_p"])."""
    c, ref0 = _case(cs)
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    lse = ref0.lse.float()
    ref = R.reference_backward(c, lse, ref0.o)
    ins = [t.to(DEV) for t in (_rows(c.q), _rows(c.k), _rows(c.v), _rows(c.dout), lse)]
    before = [t.clone() for t in ins]
    delta = _out(B * H, Lq, Lq, F32)                                  # the one buffer of this route the caller may supply
    outs, deltas = [], []
    for _ in range(2):
        outs.append(ops.flash_attn_bwd(ins[0], ins[1], ins[2], None, ins[3], ins[4], _lens(c.k_lens), B, H, Lq, Lk, scale=c.scale,
                                       q_prescaled=c.prescaled, delta=delta.window()))
        torch.cuda.synchronize()
        deltas.append(delta._bits().clone())
    assert torch.equal(deltas[0], deltas[1]), f"{cs}: delta: the second run differs"
    msg = R.compare("bwd_without_o32", "delta", delta.window().reshape(B, H, Lq).cpu(), ref.delta_p, R.KAPPA["delta_p"] * ref.S_delta_p, c, "bhi", str(cs))
    assert msg is None, msg
    delta.assert_guard("delta", str(cs))
    for what, a, b2 in zip(("q", "k", "v", "dout", "lse"), ins, before):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32), b2.view(torch.int16 if a.dtype == BF16 else torch.int32)), \
            f"{cs}: the input {what} was written"
    ROUTES["bwd/without_o32"] += 1
    for name, a, b2, rows, want, S, layout in (("dq", outs[0][0], outs[1][0], Lq, ref.dq, ref.S_dq, "bihd"), ("dk", outs[0][1], outs[1][1], Lk, ref.dk, ref.S_dk, "bjhd"),
                                               ("dv", outs[0][2], outs[1][2], Lk, ref.dv, ref.S_dv, "bjhd")):
        assert torch.equal(a, b2), f"{cs}: {name}: the second run differs"
        msg = R.compare("bwd_without_o32", name, a.reshape(B, rows, H, D).cpu(), want, R.bound(want, S, R.KAPPA[name], False), c, layout, str(cs))
        assert msg is None, msg


CHAINED = [next(cs for cs in BWD if cs["Lq"] == 300 and cs["Lk"] == 129), BANDS[3], MASKED[0], MASKED[4], MASKED[7], MASKED[8], MASKED[10]]


@pytest.mark.parametrize("cs", CHAINED, ids=[R.ident(cs) for cs in CHAINED])
def test_chained_forward_backward(ops, cs):
    """one case per backward route fed the forward kernel's own lse and o32 (the reference takes them as they are)"""
    c, ref0 = _case(cs)
    set_option("ATTN_KERNEL", "base")
    f = run_fwd(ops, c, cs, lse=True, o32=True)
    launch(f)
    hold_fwd("chained_fwd", f, ref0)
    lse, o32 = f.lse.window().reshape(c.B, c.H, c.Lq).cpu(), f.o32.window().reshape(c.B, c.Lq, c.H, D).cpu()
    entry = "plain" if c.mask.kind == "full" else ("masked" if c.mask.kind != "band" else "varlen")
    r = run_bwd(ops, c, cs, lse, o32, entry=entry, nan_rows=c.q_lens is not None and entry != "plain")
    launch(r)
    ROUTES["chained/" + _mask_route(c)] += 1
    hold_bwd("chained_bwd", r, R.reference_backward(c, lse, o32))
