"""CPU-only checks of tests/norm_exact_ref.py at the shapes tests/test_gpu_norm_exact.py runs: the generators satisfy the
exactness condition, the fp32 restatements (sequential sums) stay below delta / 4 before the rounding and inside the
bound after it, truncation instead of RNE is flagged, K_SUM covers the restatement's sums four times, and each planted
defect of norm_exact_ref.DEFECTS is reported by the comparison function."""
import collections

import pytest
import torch

import norm_exact_ref as R

F32 = R.F32
TRUNC = collections.defaultdict(lambda: [0, 0])        # entry -> [flagged, compared] under truncation


def _ln(cs):
    return R.ln_case(cs["rows"], cs["dim"], cs["rpb"], cs["seed"], small=cs.get("small", False), dy_bf16=cs.get("dy_bf16", False),
                     shared=cs.get("shared", False))


def _hold_bf16(entry, what, ref, S, rest, ctx):
    """the three assertions of a bf16 output: restatement below delta / 4, its RNE inside the bound, its truncation flagged"""
    err = (rest.double() - ref).abs()
    assert bool((err <= 0.25 * R.SLACK * S).all()), f"{entry} {ctx} {what}: restatement at {float((err / (R.SLACK * S)).max()):.3f} delta"
    bound = R.bound_bf16(ref, S)
    msg = R.compare(entry, what, R.rne_bf16(rest.double()).float(), ref, bound, ctx, record=False)
    assert msg is None, msg
    frac = R.bad_fraction(R.truncate_bf16(rest.double()).float(), ref, bound)
    TRUNC[entry][0] += frac * ref.numel()
    TRUNC[entry][1] += ref.numel()
    if ref.numel() >= 1000:
        assert frac > 0.3, f"{entry} {ctx} {what}: truncation is flagged in only {frac:.3f} of the elements"


def _hold_sum(what, ref, S, rest, seen):
    ratio = float(((rest.double() - ref).abs() / (2.0 ** -24 * S)).max())
    seen[what] = max(seen[what], ratio)                     # (asserted against K_SUM once all cases are in)


def test_exact_cases_satisfy_the_condition_and_need_no_rounding():
    """every exact case is generated (check_exact is asserted inside), and its fp32 restatement equals the float64
    reference bit for bit: no operation of the formula rounds"""
    for nseg in (1, 2):
        for kw in R.rms_cases(True, nseg):
            for xb, gb in ((True, False), (False, True)):
                c = R.rms_case(x_bf16=xb, dy_bf16=gb, **kw)
                for s in range(nseg):
                    assert torch.equal(R.rms_forward(c, s, F32).y.double(), R.rms_forward(c, s).y)
                    a, b = R.rms_backward(c, s, F32), R.rms_backward(c, s)
                    assert torch.equal(a.dx.double(), b.dx) and torch.equal(a.dw.double(), b.dw)
    c = R.rms_case(5120, 128, exact=True, nseg=2, xmax=3, **R.GRIDS[0])
    y = R.rne_bf16(R.rms_forward(c, 0).y)
    assert torch.equal(y.double(), R.rms_forward(c, 0).y), "with |x| <= 3 the stored values need no rounding"
    assert R.norm2_max(c, y).shape == (2, 40)
    for cs in R.ln_bwd_cases() + R.host_cases(R.ln_bwd2_cases()):
        c = _ln(cs)
        assert torch.equal(R.ln_backward(c, F32).dadd.double(), R.ln_backward(c).dadd)
    for rows, rpb in R.ROWS_RPB + ((4097, 1111),):
        R.gated_reference(R.gated_case(rows, 260, rpb))
    with pytest.raises(AssertionError):
        R.check_exact("gated", 40000)
    with pytest.raises(AssertionError):
        R.check_exact("rms", 10, xmax=8, bound=True)


def test_layernorm_forward_restatement_rne_and_truncation():
    for cs in R.ln_fwd_cases():
        c = _ln(cs)
        ref, rest = R.ln_forward(c), R.ln_forward(c, F32)
        _hold_bf16("layernorm_modulate", "y", ref.y, ref.S, rest.y, str(cs))
    f, n = TRUNC["layernorm_modulate"]
    assert f / n > 0.3


def test_layernorm_backward_restatement_and_the_measured_k():
    seen = collections.defaultdict(float)
    for cs in R.ln_bwd_cases() + R.host_cases(R.ln_bwd2_cases()):
        c = _ln(cs)
        v = cs.get("variant", "plain")
        ref = R.ln_backward(c, nxt=v != "plain", gate=v == "gate")
        rest = R.ln_backward(c, F32, nxt=v != "plain", gate=v == "gate")
        err = (rest.dx.double() - ref.dx).abs()
        assert bool((err <= 0.25 * R.SLACK * ref.S_dx).all()), f"{cs} dx: {float((err / (R.SLACK * ref.S_dx)).max()):.3f} delta"
        assert torch.equal(rest.dadd.double(), ref.dadd)
        _hold_sum("dmul", ref.dmul, ref.S_dmul, rest.dmul, seen)
        if v != "plain":
            _hold_bf16("layernorm_modulate_bwd2", "dy_next", ref.dy_next, ref.S_dy_next, rest.dy_next, str(cs))
        if v == "gate":
            _hold_sum("dgate", ref.dgate, ref.S_dgate, rest.dgate, seen)
    print("\n[measured] restatement / (2^-24 S): " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(seen.items())))
    for k, v in seen.items():                               # four times the worst ratio, rounded up to a power of two: K in [4 v, 8 v)
        assert 4.0 * v <= R.K_SUM[k] < 8.0 * v, f"K_SUM[{k}] = {R.K_SUM[k]} against a worst ratio of {v:.3f}"


def test_rmsnorm_restatement_rne_truncation_and_the_measured_k():
    seen = collections.defaultdict(float)
    for nseg in (1, 2):
        for kw in R.rms_cases(False, nseg):
            for xb, gb in ((True, True), (False, False)):
                c = R.rms_case(x_bf16=xb, dy_bf16=gb, **kw)
                for s in range(nseg):
                    ref, rest = R.rms_forward(c, s), R.rms_forward(c, s, F32)
                    _hold_bf16("rmsnorm_rope", "y", ref.y, ref.S, rest.y, str(kw))
                    ref, rest = R.rms_backward(c, s), R.rms_backward(c, s, F32)
                    _hold_bf16("rmsnorm_rope_bwd", "dx", ref.dx, ref.S_dx, rest.dx, str(kw))
                    _hold_sum("dweight", ref.dw, ref.S_dw, rest.dw, seen)
    print("\n[measured] restatement / (2^-24 S): " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(seen.items())))
    for e in ("rmsnorm_rope", "rmsnorm_rope_bwd"):
        assert TRUNC[e][0] / TRUNC[e][1] > 0.3
    v = seen["dweight"]
    assert 4.0 * v <= R.K_SUM["dweight"] < 8.0 * v, f"K_SUM[dweight] = {R.K_SUM['dweight']} against a worst ratio of {v:.3f}"


# ----------------------------------------------------------------------------------------------------------------------
# planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _ln_fwd_report(cs, defect):
    c = _ln(cs)
    ref = R.ln_forward(c)
    got = R.rne_bf16(R.ln_forward(c, F32, defect).y.double()).float()
    return R.compare("planted", "y", got, ref.y, R.bound_bf16(ref.y, ref.S), record=False), got, ref


def _bf(t):
    """RNE to bf16 that lets a NaN through (a defect may read the table's NaN row)"""
    return t.float().to(torch.bfloat16)


def _rms_reports(kw, defect):
    """the comparison's verdicts on a defective forward and backward: exact mode, then bounded"""
    out = []
    c = R.rms_case(**dict(kw, exact=True))
    out.append(R.compare("planted", "y", _bf(R.rms_forward(c, 0, F32, defect).y), R.rne_bf16(R.rms_forward(c).y), record=False))
    out.append(R.compare("planted", "dx", _bf(R.rms_backward(c, 0, F32, defect).dx), R.rne_bf16(R.rms_backward(c).dx),
                         record=False))
    c = R.rms_case(**dict(kw, exact=False))
    ref = R.rms_forward(c)
    out.append(R.compare("planted", "y", _bf(R.rms_forward(c, 0, F32, defect).y).float(), ref.y, R.bound_bf16(ref.y, ref.S),
                         record=False))
    ref = R.rms_backward(c)
    out.append(R.compare("planted", "dx", _bf(R.rms_backward(c, 0, F32, defect).dx).float(), ref.dx,
                         R.bound_bf16(ref.dx, ref.S_dx), record=False))
    return out


def _uses_h_w(kw):
    return kw["hd"] // 2 // 3 > 0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_is_reported(defect):
    n = 0
    if defect == "neighbour_modulation":
        for cs in R.ln_fwd_cases():
            if cs["rows"] > cs["rpb"]:
                msg, got, ref = _ln_fwd_report(cs, defect)
                assert msg is not None, cs
                rows = (R.ratio_to_bound(got, ref.y, R.bound_bf16(ref.y, ref.S)) > 1).any(1).nonzero().flatten().tolist()
                assert rows == [cs["rpb"]], f"{cs}: rows {rows} reported"
                n += 1
        g = R.gated_case(17, 260, 7)
        good, bad = R.gated_reference(g), R.gated_reference(g, defect)
        assert R.compare("planted", "xo", bad.xo, good.xo, record=False) and R.compare("planted", "dy", bad.dy, good.dy, record=False)
    elif defect == "stale_last_chunk":
        for cs in R.ln_fwd_cases():
            if cs["dim"] == 1540:
                msg, got, ref = _ln_fwd_report(cs, defect)
                cols = (R.ratio_to_bound(got, ref.y, R.bound_bf16(ref.y, ref.S)) > 1).any(0).nonzero().flatten().tolist()
                assert msg is not None and cols and min(cols) >= 1536, f"{cs}: columns {cols} reported"
                n += 1
    elif defect == "no_eps":
        for cs in R.ln_fwd_cases():
            if cs.get("small"):
                assert _ln_fwd_report(cs, defect)[0] is not None, cs
                c = _ln(cs)
                ref, got = R.ln_backward(c), R.ln_backward(c, F32, defect)
                assert R.compare("planted", "dx", got.dx, ref.dx, R.bound_row(ref.S_dx), record=False) is not None, cs
                n += 1
    elif defect == "mean_over_padded_width":
        for cs in R.ln_fwd_cases():
            if cs["dim"] % 256:
                assert _ln_fwd_report(cs, defect)[0] is not None, cs
                n += 1
    elif defect in ("swap_h_w", "rotate_pad", "clamp_at_rope_len", "second_pair_first_entry"):
        for kw in R.rms_cases(True):
            if not kw["hd"]:
                continue
            if defect == "swap_h_w" and not _uses_h_w(kw):
                continue                                    # head_dim 4: both pairs turn with the frame axis
            if defect == "rotate_pad" and kw["seq_len"] != 13:
                continue                                    # the grids without a pad token
            if defect == "clamp_at_rope_len" and kw["seq_len"] == 13 and not _uses_h_w(kw):
                continue                                    # only w passes rope_len in that grid
            reports = _rms_reports(kw, defect)
            assert all(r is not None for r in reports), f"{kw}: {reports}"
            n += 1
    elif defect == "drop_last_row":
        for cs in R.ln_bwd_cases() + R.host_cases(R.ln_bwd2_cases()):
            c = _ln(cs)
            ref, got = R.ln_backward(c), R.ln_backward(c, F32, defect)
            assert R.compare("planted", "dmul", got.dmul, ref.dmul, R.bound_sum(ref.S_dmul, "dmul"), record=False) is not None, cs
            assert R.compare("planted", "dadd", got.dadd, R.G.exact_f32(ref.dadd), record=False) is not None, cs
            n += 1
        for kw in R.rms_cases(False):
            c = R.rms_case(**kw)
            ref, got = R.rms_backward(c), R.rms_backward(c, 0, F32, defect)
            assert R.compare("planted", "dweight", got.dw, ref.dw, R.bound_sum(ref.S_dw, "dweight"), record=False) is not None, kw
            c = R.rms_case(**dict(kw, exact=True))
            assert R.compare("planted", "dweight", R.rms_backward(c, 0, F32, defect).dw, R.G.exact_f32(R.rms_backward(c).dw), record=False)
            n += 1
    elif defect == "dgate_wrong_group":
        for cs in R.host_cases(R.ln_bwd2_cases()):
            if cs["variant"] == "gate" and cs["rows"] > cs["rpb"]:
                c = _ln(cs)
                ref, got = R.ln_backward(c, nxt=True, gate=True), R.ln_backward(c, F32, defect, nxt=True, gate=True)
                assert R.compare("planted", "dgate", got.dgate, ref.dgate, R.bound_sum(ref.S_dgate, "dgate"), record=False) is not None, cs
                n += 1
        g = R.gated_case(17, 260, 7)
        assert R.compare("planted", "dgate", R.gated_reference(g, defect).dgate, R.gated_reference(g).dgate, record=False)
    assert n >= 3, f"{defect}: planted in {n} cases only"


def test_compare_reports_the_worst_element_and_a_nan():
    ref = torch.zeros(3, 8, dtype=torch.float64)
    got = ref.clone().float()
    got[2, 5] = 3.0
    got[1, 1] = 1.0
    msg = R.compare("planted", "t", got, ref, torch.full_like(ref, 0.5), record=False)
    assert "2 of 24" in msg and "(2, 5)" in msg and "ratio 6.000" in msg
    got[0, 0] = float("nan")
    assert "(0, 0)" in R.compare("planted", "t", got, ref, torch.full_like(ref, 0.5), record=False)
    assert R.compare("planted", "t", ref.float(), ref, torch.zeros_like(ref), record=False) is None
