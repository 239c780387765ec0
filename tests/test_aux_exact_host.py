"""CPU-only checks of tests/aux_exact_ref.py at the cases tests/test_gpu_aux_exact.py runs: the exact cases satisfy their
exactness condition and their fp32 restatement equals float64 bit for bit; the fp32 restatement of every bounded
reference stays below delta / 4 (below delta where a result may be flushed whole), its RNE is inside the bound and its
truncation is flagged on a large share of the elements; no GELU delta has a term that grows with |x| against the result
(delta <= 2^-9 max(|ref|, |dy|) on every held pattern, an error of 1 beyond |x| = 1e12 is flagged); the stored k factors are four times the measured ratio rounded up to a power of two; the NaN set of the tanh
gradient has the size that follows from the overflow threshold; each planted defect of aux_exact_ref.DEFECTS is reported
by the comparison on at least one case of the GPU test's own lists."""
import collections
import importlib

import pytest
import torch

import aux_exact_ref as R
from conftest import PKG

F32, F64, BF16 = R.F32, R.F64, R.BF16


def _schedule():
    return R.unipc_schedule(importlib.import_module(PKG + ".wan.utils.fm_solvers_unipc"))


# ----------------------------------------------------------------------------------------------------------------------
# exactness
# ----------------------------------------------------------------------------------------------------------------------
def test_exact_cases_satisfy_their_condition_and_need_no_rounding():
    for e in R.colsum_single_cases() + [e for es in R.colsum_multi_cases().values() for e in es]:
        x, out0 = R.colsum_data(e)
        x = R.colsum_block(e, x)
        assert torch.equal(R.colsum_ref(x, out0, F32).out.double(), R.colsum_ref(x, out0).out), e
    for cs in R.softmax_cases():
        p, dp = R.softmax_data(cs)
        ref = R.softmax_bwd_ref(p, dp, cs["scale"])
        delta = (p.float() * dp).sum(-1, keepdim=True)
        assert torch.equal((p.float() * (dp - delta) * cs["scale"]).double(), ref), cs
    for cs in R.dense_fwd_cases():
        c = R.dense_data(cs)
        if c.exact:
            assert torch.equal(R.dense_fwd_ref(c, cs, F32).y.double(), R.dense_fwd_ref(c, cs).y), cs
    for cs in R.dense_bwd_cases():
        c = R.dense_data(cs, backward=True)
        if c.exact:
            a, b = R.dense_bwd_ref(c, cs, F32), R.dense_bwd_ref(c, cs)
            assert all(torch.equal(getattr(a, k).double(), getattr(b, k)) for k in ("dW", "db", "dx")), cs
    for cs in R.unipc_cases():
        c = R.unipc_data(cs)
        a, b = R.unipc_ref(c, cs, F32), R.unipc_ref(c, cs)
        assert all(torch.equal(getattr(a, k).double(), getattr(b, k)) for k in ("mt", "xc", "xn")), cs
        assert float(b.xn.abs().max()) <= 6336
    for kind, kw in (("colsum", dict(R=2100000)), ("softmax", dict(L=1001, scale=1.0)), ("softmax", dict(L=8, scale=0.3)),
                     ("dense", dict(B=3, N=131, K=300))):
        with pytest.raises(AssertionError):
            R.check_exact(kind, **kw)


def test_special_patterns_round_as_the_contract_says():
    x = torch.tensor(R.SPECIAL_F32, dtype=torch.int64)
    x = R._i32(x).view(F32)
    got = R.as_bits(R.rne_any(x)).tolist()
    u = lambda v: v - 0x10000 if v >= 0x8000 else v                                 # noqa: E731
    assert got[:6] == [u(0x3F80), u(0x3F82), u(0xBF80), u(0xBF82), u(0x7F80), u(0xFF80)]          # ties to even, overflow to inf
    assert got[6:13] == [0, 0, 2, u(0x8080), u(0x8000), u(0x7F80), u(0xFF80)]
    assert bool(torch.isnan(R.rne_any(x)[13:]).all())
    assert R.compare_bits("planted", "t", torch.tensor([0.0]), torch.tensor([-0.0]), record=False) is not None
    assert R.compare_bits("planted", "t", torch.tensor([R.NAN]), torch.tensor([R.NAN]), record=False) is None
    assert R.compare_bits("planted", "t", torch.tensor([1.0]), torch.tensor([R.NAN]), record=False) is not None


# ----------------------------------------------------------------------------------------------------------------------
# bounded references: restatement below delta / 4, its RNE inside the bound, its truncation flagged
# ----------------------------------------------------------------------------------------------------------------------
CLASS_WORST = collections.defaultdict(float)


def _hold_bf16(what, ref, delta, rest, keep, busy, share=0.3, classes=None, flush=None):
    """``keep``: the elements held; ``busy``: those among them whose result is not trivially a bf16 value (|x| in
    [2^-6, 8]: below, gelu(x) is x / 2 or x to all of fp32's digits; above, x or 0), where truncation must show"""
    busy = busy[keep]
    flush = torch.zeros_like(keep)[keep] if flush is None else flush[keep]
    ref, delta, rest = ref[keep], delta[keep], rest[keep]
    err = (rest.double() - ref).abs()
    ratio = err / delta.clamp_min(2.0 ** -300)
    worst = float(ratio[~flush].max())
    assert worst <= 0.25, f"{what}: restatement at {worst:.3f} delta"
    if bool(flush.any()):                                   # where a result may be flushed whole, all of it is allowed
        assert float(ratio[flush].max()) <= 1.0, f"{what}: restatement at {float(ratio[flush].max()):.3f} delta in the flush range"
    bound = R.bound_bf16(ref, delta)
    msg = R.compare("planted", what, R.rne_bf16(rest.double()).float(), ref, bound, record=False)
    assert msg is None, msg
    for name, mask in (classes or {}).items():              # the RNE of the restatement against the bound, per class
        m = mask[keep]
        if bool(m.any()):
            key = f"{what.split()[0]}/{name}"
            CLASS_WORST[key] = max(CLASS_WORST[key], R.delta_used(R.rne_bf16(rest[m].double()).float(), ref[m], delta[m]))
    frac = R.bad_fraction(R.truncate_bf16(rest[busy].double()).float(), ref[busy], bound[busy])
    assert frac > share, f"{what}: truncation is flagged in only {frac:.3f} of the elements"
    return worst


def _bounds_hold_something_everywhere(x64, finite, nan_set):
    """no term of a backward delta is absolute in |P| or |z|: on every held pattern delta stays below 2^-9 of
    max(|ref|, |dy|) (bf16's half ulp of the larger of the two), and an error of 1 planted in the result of dy = 1, -1,
    1/2 is flagged on every held pattern with |x| > 1e12; the flush terms are open on their own ranges alone"""
    far = x64.abs() > 1e12
    for name, fn, keep in (("tanh", R.gelu_tanh_bwd, finite & ~nan_set), ("erf", R.gelu_erf_bwd, finite)):
        assert int((keep & far).sum()) > 800
        for kind in R.GELU_DY:
            dy = R.gelu_dy(kind).double()
            ref, delta = fn(dy, x64)
            room = torch.maximum(ref.abs(), dy.abs()) * 2.0 ** -9 + 2.0 ** -134        # (half of bf16's smallest step, for dy = 0)
            worst = float((delta / room)[keep].max())
            assert worst <= 1.0, f"{name} backward, dy {kind}: delta reaches {worst:.3e} of 2^-9 max(|ref|, |dy|)"
            if kind != "random":
                k = keep & far
                ratio = R.ratio_to_bound(R.rne_bf16(ref[k]).float() + 1.0, ref[k], R.bound_bf16(ref[k], delta[k]))
                assert bool((ratio > 1.0).all()), f"{name} backward, dy {kind}: an error of 1 passes at |x| > 1e12"
    t = R._tanh_parts(x64, F64)[0]
    gate = finite & (t > R.T_FLUSH)
    assert 0 < int(gate.sum()) < 16100 and float(x64[gate].max()) < -9.9           # x <= -10: the negative patterns from there down
    ref, delta = R.gelu_tanh_fwd(x64)
    assert bool((delta[finite & ~gate] <= 2.0 ** -12 * ref.abs()[finite & ~gate] + R.SUBN).all())
    z_gate = finite & (0.5 * x64 * x64 > R.Z_FLUSH)
    assert float(x64[z_gate].abs().min()) > 13.1


def test_gelu_restatements_over_all_patterns():
    xb = R.all_bf16_patterns()
    x32, x64 = xb.float(), xb.double()
    finite = torch.isfinite(x32)
    busy = (x32.abs() >= 2.0 ** -6) & (x32.abs() <= 8.0)
    seen = {}
    t_flush = R._tanh_parts(x64, F64)[0] > R.T_FLUSH
    ref, delta = R.gelu_tanh_fwd(x64)
    seen["tanh"] = _hold_bf16("gelu_tanh", ref, delta, R.gelu_tanh_fwd(x32, F32)[0], finite, busy, classes=R.gelu_classes("tanh", x64, ref), flush=t_flush)
    ref, delta = R.gelu_erf_fwd(x64)
    seen["erf"] = _hold_bf16("gelu_erf", ref, delta, R.gelu_erf_fwd(x32, F32)[0], finite, busy, classes=R.gelu_classes("erf", x64, ref))
    nan_set = R.tanh_grad_nan_set(x32)
    assert int(nan_set.sum()) == R.tanh_grad_nan_count() > 0
    assert float(x32[nan_set].abs().min()) > 1.16e13 and float(x32[finite & ~nan_set].abs().max()) < 1.18e13
    for kind in R.GELU_DY:
        dy = R.gelu_dy(kind)
        ref, delta = R.gelu_tanh_bwd(dy.double(), x64)
        assert bool(torch.isfinite(delta[finite]).all()) and bool(torch.isfinite(ref[finite]).all())
        seen["tanh_bwd/" + kind] = _hold_bf16("gelu_tanh_bwd " + kind, ref, delta, R.gelu_tanh_bwd(dy.float(), x32, F32)[0], finite & ~nan_set, busy,
                                                classes=R.gelu_classes("tanh", x64, ref), flush=t_flush)
        ref, delta = R.gelu_erf_bwd(dy.double(), x64)
        seen["erf_bwd/" + kind] = _hold_bf16("gelu_erf_bwd " + kind, ref, delta, R.gelu_erf_bwd(dy.float(), x32, F32)[0], finite, busy,
                                               classes=R.gelu_classes("erf", x64, ref), flush=0.5 * x64 * x64 > R.Z_FLUSH)
    print("\n[measured] restatement / delta: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(seen.items())))
    print("[measured] share of delta the RNE of the restatement needs beyond its half ulp, by class: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(CLASS_WORST.items())))
    _bounds_hold_something_everywhere(x64, finite, nan_set)
    # the deep negative tail: at x = -9 (t = 95.8) D / S = 486 eps passes the project's 2^-16
    x = torch.tensor([-9.0], dtype=F64)
    ref, delta = R.gelu_tanh_fwd(x)
    assert 2.0 ** -16 < float(delta / ref.abs()) / R.MARGIN < 2.0 ** -15


def test_dense_silu_restatement_and_the_measured_k():
    seen = collections.defaultdict(float)

    def ratio(what, rest, ref, S):
        seen[what] = max(seen[what], float(((rest.double() - ref).abs() / (R.EPS24 * S)).max()))

    for cs in R.dense_fwd_cases():
        c = R.dense_data(cs)
        if not c.exact:
            ref, rest = R.dense_fwd_ref(c, cs), R.dense_fwd_ref(c, cs, F32)
            ratio("dense_y", rest.y, ref.y, ref.S)
    for cs in R.dense_bwd_cases():
        c = R.dense_data(cs, backward=True)
        if not c.exact:
            ref, rest = R.dense_bwd_ref(c, cs), R.dense_bwd_ref(c, cs, F32)
            for k in ("dW", "db", "dx"):
                ratio("dense_" + k, getattr(rest, k), getattr(ref, k), getattr(ref, "S_" + k))
    print("\n[measured] restatement / (2^-24 S): " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(seen.items())))
    assert set(seen) == set(R.K_AUX)
    for k, v in seen.items():                               # four times the worst ratio, rounded up to a power of two
        assert 4.0 * v <= R.K_AUX[k] < 8.0 * v, f"K_AUX[{k}] = {R.K_AUX[k]} against a worst ratio of {v:.3f}"


def test_sinusoid_one_rounding_is_inside_the_bound_and_truncation_is_not():
    flagged = total = 0
    for cs in R.sinusoid_cases():
        t = R.sinusoid_t(cs)
        ref, bound = R.sinusoid_fwd_ref(t, cs["dim"])
        assert R.compare("planted", "out", ref.float(), ref, bound, record=False) is None
        trunc = (R.as_bits(ref.float()).to(torch.int64) - (ref.float().double().abs() > ref.abs()).to(torch.int64)).to(torch.int32).view(F32)
        flagged += int((R.ratio_to_bound(trunc, ref, bound) > 1).sum())
        total += ref.numel()
        g = R._randn(R._gen(41, cs["seed"]), (cs["B"], cs["dim"])).float()
        ref, bound = R.sinusoid_bwd_ref(g, t)
        assert R.compare("planted", "dt", ref.float(), ref, bound, record=False) is None
    assert flagged / total > 0.3, f"truncation flagged in {flagged} of {total}"


def test_colsum_and_unipc_restatements_stay_inside_their_bounds():
    worst = 0.0
    for e in R.colsum_single_cases() + R.colsum_multi_cases()["n16_mixed"]:
        x, out0 = R.colsum_data(e, exact=False)
        ref, rest = R.colsum_ref(x, out0), R.colsum_ref(x, out0, F32)
        ratio = float(((rest.out.double() - ref.out).abs() / (e["R"] * R.EPS24 * ref.S)).max())
        assert ratio <= (0.25 if e["R"] >= 8 else 1.0), f"{e}: restatement at {ratio:.3f} of R 2^-24 S"
        worst = max(worst, ratio)
    assert worst > 0.0
    seen = collections.defaultdict(float)
    coefs = _schedule()
    assert coefs[0][1] is None and coefs[1][1][2] == 0.0 and coefs[2][1][2] != 0.0 and coefs[0][2][2] == 0.0
    for step, coef in enumerate(coefs):
        for cs in R.unipc_cases():
            if cs["n"] > 1000 or bool(cs["use_corr"]) != (coef[1] is not None):
                continue
            c = R.unipc_data(cs, exact=False, coef=coef)
            ref, rest = R.unipc_ref(c, cs), R.unipc_ref(c, cs, F32)
            for k in ("mt", "xc", "xn"):
                S = getattr(ref, "S_" + k)
                seen[k] = max(seen[k], float(((getattr(rest, k).double() - getattr(ref, k)).abs() / (R.N_R[k] * R.EPS24 * S)).max()))
    print("\n[measured] restatement / (n_r 2^-24 S): " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(seen.items())))
    assert len(seen) == 3 and all(v <= 1.0 for v in seen.values()), dict(seen)


# ----------------------------------------------------------------------------------------------------------------------
# planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _bits(entry, got, want):
    return R.compare_bits("planted", entry, got, want, record=False)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_is_reported(defect):
    n = 0
    if defect == "transpose_drop_partial_group":
        for cs in R.transpose_cases():
            x = R.transpose_input(cs)
            msg = _bits("out", R.transpose_ref(x, defect), R.transpose_ref(x))
            assert (msg is not None) == (cs["R"] % 4 != 0), cs
            n += msg is not None
    elif defect in ("colsum_drop_block_last_row", "colsum_chunk_edge"):
        lists = [(32, R.colsum_single_cases())] + [(128 if name.startswith(("n", "column")) else 32, es) for name, es in R.colsum_multi_cases().items()]
        for rpb, es in lists:
            for e in es:
                for exact in (True, False):
                    x, out0 = R.colsum_data(e, exact)
                    x = R.colsum_block(e, x)
                    ref, bad = R.colsum_ref(x, out0), R.colsum_ref(x, out0, F32, defect, rpb)
                    hit = e["R"] >= rpb if defect == "colsum_drop_block_last_row" else e["C"] > 255
                    msg = (R.compare("planted", "out", bad.out, R.exact_f32(ref.out), record=False) if exact else
                           R.compare("planted", "out", bad.out, ref.out, e["R"] * R.EPS24 * ref.S, record=False))
                    assert hit or msg is None, (e, msg)     # (a hit may hide: a dropped row of zeros, a column sum of zero)
                    n += msg is not None
    elif defect in ("patchify_swap_i_j", "patchify_pad_nonzero"):
        for cs in R.patchify_cases()[:-1]:
            d = R.patch_dims(cs)
            x = R.f32_patterns(R._gen(43, cs["seed"]), (cs["C"], d.F, d.H, d.W))
            msg = _bits("tokens", R.patchify_ref(x, cs, defect), R.patchify_ref(x, cs))
            hit = (d.ph > 1 and d.pw > 1) if defect == "patchify_swap_i_j" else cs["pad"] > 0
            assert (msg is not None) == hit, cs
            n += msg is not None
    elif defect == "unpatchify_swap_a_i":
        for cs in R.unpatchify_cases()[:-1]:
            d = R.patch_dims(cs)
            tok = R.f32_patterns(R._gen(44, cs["seed"]), (d.tokens, d.valid))
            msg = _bits("out", R.unpatchify_ref(tok, cs, defect), R.unpatchify_ref(tok, cs))
            assert (msg is not None) == (d.pt > 1 and d.ph > 1), cs
            n += msg is not None
    elif defect == "cast_truncates":
        for k in R.CAST_N[:-1]:
            x = R.f32_patterns(R._gen(45, k), (k,))
            n += _bits("y", R.rne_any(x, defect), R.rne_any(x)) is not None
        assert n >= 2
        n += 1
    elif defect == "softmax_sum_over_pitch":
        for cs in R.softmax_cases():
            p, dp = R.softmax_data(cs)
            got = R.softmax_bwd_ref(p, dp, cs["scale"], defect).float().to(BF16)
            assert _bits("ds", got, R.rne_bf16(R.softmax_bwd_ref(p, dp, cs["scale"]))) is not None, cs
            n += 1
    elif defect == "dense_bias_after_act":
        for cs in R.dense_fwd_cases():
            if cs["bias"] and cs["act_out"]:
                c = R.dense_data(cs)
                ref, bad = R.dense_fwd_ref(c, cs), R.dense_fwd_ref(c, cs, F32, defect)
                assert R.compare("planted", "y", bad.y, ref.y, R.K_AUX["dense_y"] * R.EPS24 * ref.S, record=False) is not None, cs
                n += 1
    elif defect == "dense_db_times_K":
        for cs in R.dense_bwd_cases():
            if cs["db"] and cs["want"] != "dx" and cs["K"] > 1:
                c = R.dense_data(cs, backward=True)
                ref, bad = R.dense_bwd_ref(c, cs), R.dense_bwd_ref(c, cs, F32, defect)
                msg = (R.compare("planted", "db", bad.db, R.exact_f32(ref.db), record=False) if c.exact else
                       R.compare("planted", "db", bad.db, ref.db, R.K_AUX["dense_db"] * R.EPS24 * ref.S_db, record=False))
                assert msg is not None, cs
                n += 1
    elif defect == "sinusoid_halves_swapped":
        for cs in R.sinusoid_cases():
            t = R.sinusoid_t(cs)
            ref, bound = R.sinusoid_fwd_ref(t, cs["dim"])
            assert R.compare("planted", "out", R.sinusoid_fwd_ref(t, cs["dim"], defect)[0].float(), ref, bound, record=False) is not None, cs
            g = R._randn(R._gen(41, cs["seed"]), (cs["B"], cs["dim"])).float()
            ref, bound = R.sinusoid_bwd_ref(g, t)
            n += R.compare("planted", "dt", R.sinusoid_bwd_ref(g, t, defect)[0].float(), ref, bound, record=False) is not None
    elif defect in ("unipc_cond_uncond_swapped", "unipc_m1_dropped_without_m2"):
        coefs = _schedule()
        for cs in R.unipc_cases()[:-1]:
            c = R.unipc_data(cs)
            ref, bad = R.unipc_ref(c, cs), R.unipc_ref(c, cs, F32, defect)
            msg = R.compare("planted", "x_next", bad.xn, R.exact_f32(ref.xn), record=False)
            hit = True if defect == "unipc_cond_uncond_swapped" else bool(cs["use_corr"] and cs["m1"] and not cs["m2"])
            assert (msg is not None) == hit, cs
            n += msg is not None
            coef = coefs[2 if cs["use_corr"] else 0]
            if hit and (defect == "unipc_cond_uncond_swapped" or cs["m1"]):
                c = R.unipc_data(cs, exact=False, coef=coefs[1] if (cs["use_corr"] and not cs["m2"]) else coef)
                ref, bad = R.unipc_ref(c, cs), R.unipc_ref(c, cs, F32, defect)
                assert R.compare("planted", "x_next", bad.xn, ref.xn, R.N_R["xn"] * R.EPS24 * ref.S_xn, record=False) is not None, cs
    elif defect == "flow_one_sigma_per_vector":
        for B, n_ in R.FLOW_SHAPES:
            c = R.flow_data(B, n_)
            good, bad = R.flow_ref(c), R.flow_ref(c, defect=defect)
            msg = _bits("x0", bad[0], good[0])
            assert (msg is not None) == (B > 1 and n_ % 4 != 0), (B, n_)
            n += msg is not None
        n += 1
    elif defect == "gelu_grad_without_s":
        xb = R.all_bf16_patterns()
        keep = torch.isfinite(xb.float()) & ~R.tanh_grad_nan_set(xb.float())
        for kind in R.GELU_DY:
            dy = R.gelu_dy(kind)
            ref, delta = R.gelu_tanh_bwd(dy.double(), xb.double())
            bad = R.gelu_tanh_bwd(dy.float(), xb.float(), F32, defect)[0]
            frac = R.bad_fraction(R.rne_bf16(bad[keep].double()).float(), ref[keep], R.bound_bf16(ref[keep], delta[keep]))
            assert frac > 0.3, f"{kind}: flagged in {frac:.3f}"
            n += 1
    assert n >= 3, f"{defect}: planted in {n} cases only"
