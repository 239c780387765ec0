"""CPU only: what tests/test_gpu_attn_exact.py rests on (tests/attn_exact_ref.py), shown without a GPU.

  * the visibility builders agree with a slow per-(i, j) statement of include/omh.h's rule on random small masks;
  * the input conditions hold for every GPU case (equal target scores, gap >= 32 log2 units, at most 1/4 uniform rows,
    m <= 48 for the bounded cases);
  * the fp32 restatements of the kernels' arithmetic (short running-max loop; lazy-max and fixed-m streams; the
    backward with P and dS rounded to bf16) stay below a quarter of the bound on every element at the GPU test's own
    shapes: KAPPA is at least four times their worst ratio to the condition sum (printed as ``[kappa]``);
  * each planted defect is reported: at least one element over the bound in the rows concerned, none elsewhere."""
import collections

import pytest
import torch

import attn_exact_ref as R

F64 = torch.float64
MEASURED = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[kappa] worst |restatement - ref| / S: " + "  ".join(f"{k}={v:.3e} (kappa {R.KAPPA[k]:.3e})" for k, v in sorted(MEASURED.items())))


_CACHE = {}


def _case(cs):
    key = R.ident(cs) + str(cs.get("seed"))
    if key not in _CACHE:
        c = R.build(cs)
        _CACHE[key] = (c, R.reference_forward(c))
    return _CACHE[key]


def _qrows(t):
    """[B, H, Lq] -> [B, Lq, H, 1]"""
    return t.permute(0, 2, 1)[..., None]


def _measure(key, got, ref, S, sel=None):
    """worst |got - ref| / S over the selected elements (S = 0: the values must agree)"""
    err = (got.double() - ref).abs()
    if sel is not None:
        err, S = err[sel.expand_as(err)], S[sel.expand_as(S)]
    if err.numel() == 0:
        return
    assert bool((err[S == 0] == 0).all()), f"{key}: an element with condition sum 0 differs"
    MEASURED[key] = max(MEASURED[key], float((err[S > 0] / S[S > 0]).max()) if bool((S > 0).any()) else 0.0)
    assert 4.0 * MEASURED[key] <= R.KAPPA[key], f"{key}: the restatement's ratio {MEASURED[key]:.3e} times four is above kappa {R.KAPPA[key]:.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# visibility
# ----------------------------------------------------------------------------------------------------------------------
def _random_masks():
    g = torch.Generator().manual_seed(7)
    out = [(R.mask_full(), 13, 21)]
    for l, r in ((-1, 0), (3, 2), (0, -1), (0, 0), (5, -1), (-1, 4)):
        out.append((R.mask_band(l, r), 17, 23))
        out.append((R.mask_band(l, r), 23, 11))
    for ch, left, off in ((5, -1, 0), (4, 1, 3), (7, 0, 9), (1, 2, 0)):
        out.append((R.mask_chunk(ch, left, off), 19, 26))
    for grp, kg in ((8, None), (9, None), (8, 3), (11, 1)):
        for _ in range(2):
            nq, nk = (20 + grp - 1) // grp, (27 + (kg or grp) - 1) // (kg or grp)
            out.append((R.mask_interval(torch.rand(nq, nk, generator=g) < 0.5, grp, kg), 20, 27))
    for heads in (1, 2):
        out.append((R.mask_block(torch.rand(heads, 2, 3, generator=g) < 0.6), 130, 260))
    return out


@pytest.mark.parametrize("n", range(len(_random_masks())))
def test_visibility_agrees_with_the_slow_statement(n):
    mask, Lq, Lk = _random_masks()[n]
    for q_lens, k_lens in ((None, None), ([Lq - 3, 0], [Lk, Lk - 5]), ([1, Lq + 4], [0, 1])):
        a = R.visibility(mask, 2, 2, Lq, Lk, q_lens, k_lens)
        b = R.visibility_slow(mask, 2, 2, Lq, Lk, q_lens, k_lens)
        assert torch.equal(a, b), f"{mask} q_lens {q_lens} k_lens {k_lens}: {int((a != b).sum())} pairs differ"


# ----------------------------------------------------------------------------------------------------------------------
# input conditions and restatements, forward
# ----------------------------------------------------------------------------------------------------------------------
FWD = [("short", cs) for cs in R.fwd_short_cases() + R.fwd_split_cases() + R.band_cases() + R.masked_cases()] + \
      [("w64", cs) for cs in R.w64_cases()]


@pytest.mark.parametrize("family,cs", FWD, ids=[f + "-" + R.ident(cs) for f, cs in FWD])
def test_forward_inputs_and_restatement(family, cs):
    c, ref0 = _case(cs)
    R.check_inputs(c, bounded=bool(cs.get("bounded")))
    forms = ("short",) if family == "short" else (("lazy", "fixed") if cs.get("bounded") else ("lazy",))
    if "workspace" in cs:
        forms += ("split",)
    for form in forms:
        requant = family == "w64" and not c.prescaled
        ref = R.reference_forward(c, requant=True) if requant else ref0
        if form == "split":
            o, lse = R.restate_forward(c, splits=R.short_split_plan(cs, 256)[2])
        else:
            o, lse = R.restate_forward(c, form=form, requant=requant)
        ok = R.flat_ok(c, form)
        flat = _qrows(c.flat) if ok else torch.zeros(c.B, c.Lq, c.H, 1, dtype=torch.bool)
        _measure("o", o, ref.o, ref.S, ~flat)
        tails = R.KAPPA["o"] / 4.0 * (ref.S - ref.S_t)                  # the other codes' 2^-32 tails: P rounded to bf16
        fk = "o_flat_split" if form == "split" else "o_flat"
        _measure(fk, ((o.double() - ref.o).abs() - tails).clamp_min(0.0), torch.zeros_like(ref.o), ref.S_t, flat)
        live = ~c.dead
        assert torch.equal(torch.isinf(lse), c.dead), f"{cs}: lse = -inf exactly on the rows that see nothing"
        _measure("lse", lse[live], ref.lse[live], ref.lse[live].abs().clamp_min(1.0))
        # the bound itself, on the bf16 output, with a quarter of kappa
        msg = R.compare("host", "o", R.bf(o), ref.o, R.bound(ref.o, R.fwd_delta(c, ref, ok, quarter=True, flat_key=fk), None, True), c, "bihd", str(cs),
                        record=False)
        assert msg is None, msg
        dead = _qrows(c.dead).expand_as(o)
        assert bool((o[dead] == 0).all()), f"{cs}: rows that see nothing must be exact zeros"


def test_analytic_reference_agrees_with_the_dense_one():
    """the per-code means that the long split-KV case is held to, against the dense float64 softmax at a small shape; the
    restatements of the stream and of its split tail stay below a quarter of the bound there too"""
    c = R.analytic_case(2, 2, 70, 300, [300, 259])
    c.vis = R.visibility(c.mask, c.B, c.H, c.Lq, c.Lk, None, c.k_lens)
    a, d = R.analytic_forward(c), R.reference_forward(c)
    for what in ("o", "S", "S_t"):
        x, y = getattr(a, what), getattr(d, what)
        assert float(((x - y).abs() / y.abs().clamp_min(1.0)).max()) < 1e-12, what
    assert float((a.lse - d.lse).abs().max()) < 1e-12
    for splits, fk in ((1, "o_flat"), (4, "o_flat_split")):
        o, lse = R.restate_forward(c, form="lazy", splits=splits)
        msg = R.compare("host", "o", R.bf(o), a.o, R.bound(a.o, R.fwd_delta(c, a, quarter=True, flat_key=fk), None, True), record=False)
        assert msg is None, msg
        _measure("lse", lse, a.lse, a.lse.abs().clamp_min(1.0))


# ----------------------------------------------------------------------------------------------------------------------
# restatement, backward
# ----------------------------------------------------------------------------------------------------------------------
BWD = R.bwd_cases() + R.bwd_old_cases() + R.cached_cases() + R.band_cases() + R.masked_cases()


@pytest.mark.parametrize("cs", BWD, ids=[R.ident(cs) for cs in BWD])
def test_backward_restatement(cs):
    c, ref0 = _case(cs)
    lse, o32 = ref0.lse.float(), ref0.o.float()
    ref = R.reference_backward(c, lse, o32)
    got = R.restate_backward(c, lse, o32)
    for what in ("dq", "dk", "dv", "delta"):
        _measure(what, getattr(got, what), getattr(ref, what), getattr(ref, "S_" + what))
    if cs in R.bwd_old_cases():
        _measure("delta_p", got.delta_p, ref.delta_p, ref.S_delta_p)
    dead = _qrows(c.dead).expand_as(got.dq)
    assert bool((ref.dq[dead] == 0).all()) and bool((got.dq[dead] == 0).all())
    unseen = ~c.vis.any(2)                                              # [B, H, Lk]: keys no live query sees
    for t in (ref.dk, ref.dv, got.dk, got.dv):
        assert bool((t[unseen.permute(0, 2, 1)[..., None].expand_as(t)] == 0).all()), f"{cs}: keys no live query sees get zero gradients"


# ----------------------------------------------------------------------------------------------------------------------
# planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _reported(c, ref, o, rows, what, cs):
    """at least one element over the bound in ``rows`` [B, H, Lq], none elsewhere"""
    bad = R.bad_rows(R.bf(o), ref.o, R.bound(ref.o, R.fwd_delta(c, ref), None, True)).permute(0, 2, 1)       # [B, H, Lq]
    assert bool((bad & rows).any()), f"{what} at {cs}: not reported ({int(rows.sum())} rows concerned)"
    assert not bool((bad & ~rows).any()), f"{what} at {cs}: {int((bad & ~rows).sum())} rows reported that the defect does not touch"
    return int((bad & rows).sum())


DEFECT_CASES = [cs for cs in R.fwd_short_cases() if cs["Lk"] >= 129 and cs["Lq"] >= 33] + R.band_cases() + R.masked_cases()


@pytest.mark.parametrize("defect", R.FWD_DEFECTS)
def test_forward_defects_are_reported(defect):
    seen = 0
    for cs in DEFECT_CASES:
        c, ref = _case(cs)
        if defect == "neighbour_head_v":
            o, _ = R.restate_forward(c, neighbour_head_v=True)
            rows = ~c.dead
            bad = R.bad_rows(R.bf(o), ref.o, R.bound(ref.o, R.fwd_delta(c, ref), None, True)).permute(0, 2, 1)
            assert bool(bad[rows].all()) and not bool(bad[~rows].any()), f"{defect} at {cs}: {int(bad[rows].sum())} of {int(rows.sum())} live rows reported"
            seen += 1
            continue
        planted = R.defect_visibility(c, defect)
        if planted is None:
            continue
        vis, rows = planted
        o, _ = R.restate_forward(c, vis=vis)
        _reported(c, ref, o, rows, defect, cs)
        seen += 1
    assert seen >= 2, f"{defect}: applies to {seen} cases"


@pytest.mark.parametrize("defect", R.BWD_DEFECTS)
def test_backward_defects_are_reported(defect):
    seen = 0
    for cs in (R.cached_cases() if defect == "own_lo_ignored" else [cs for cs in R.bwd_cases() if min(cs["Lq"], cs["Lk"]) >= 63][:3] + R.band_cases()[:2] + R.masked_cases()[:2]):
        c, ref0 = _case(cs)
        lse, o32 = ref0.lse.float(), ref0.o.float()
        ref = R.reference_backward(c, lse, o32)
        bnd = {w: R.bound(getattr(ref, w), getattr(ref, "S_" + w), R.KAPPA[w], False) for w in ("dq", "dk", "dv")}
        if defect == "dk_shifted_row":
            got = R.restate_backward(c, lse, o32, dk_shift=1)
            assert bool(R.bad_rows(got.dk, ref.dk, bnd["dk"]).any()), f"{defect} at {cs}: not reported"
            assert not bool(R.bad_rows(got.dq, ref.dq, bnd["dq"]).any()) and not bool(R.bad_rows(got.dv, ref.dv, bnd["dv"]).any())
        elif defect == "own_lo_ignored":        # row r of dk is key r, not key own_lo + r
            lo = cs["own_lo"]
            got = R.restate_backward(c, lse, o32)
            want = ref.dk[:, lo:]
            assert not bool(R.bad_rows(got.dk[:, lo:], want, bnd["dk"][:, lo:]).any())
            assert bool(R.bad_rows(got.dk[:, :c.Lk - lo], want, bnd["dk"][:, lo:]).any()), f"{defect} at {cs}: not reported"
        else:
            planted = R.defect_visibility(c, defect)
            if planted is None:
                continue
            vis, rows = planted
            got = R.restate_backward(c, lse, o32, vis=vis)
            bad = R.bad_rows(got.dq, ref.dq, bnd["dq"]).permute(0, 2, 1)
            # (a row with ONE target has dS = P (dP - delta) = 0 at that key: only dv and dk see its loss)
            assert bool((bad & rows).any()) or bool(R.bad_rows(got.dv, ref.dv, bnd["dv"]).any()), f"{defect} at {cs}: neither dq nor dv reports it"
            assert not bool((bad & ~rows).any()), f"{defect} at {cs}: dq reports rows the defect does not touch"
        seen += 1
    assert seen >= 2, f"{defect}: applies to {seen} cases"
