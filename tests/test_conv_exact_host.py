"""tests/conv_exact_ref.py checked on the CPU: the index-arithmetic reference against torch's float64 convolution on the
padded / upsampled tensor, the exactness condition of every case the GPU test runs, a plain fp32 convolution passing the
exact assertion, planted defects reported per element (and whether rel_rms at the tolerance of tests/test_gpu_vae.py would
have seen them), and the restatement of the norm kernel from which K_NORM is derived."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R
from conftest import rel_rms

F64 = torch.float64


def _torch_conv(c, dtype=F64):
    """[Tout, Hout, Wout, Cout] from torch's convolution on the explicitly upsampled and padded tensor (plain layers only)"""
    x = c.x[:c.used_frames].to(dtype).permute(3, 0, 1, 2)[None]                        # [1, C, T, H, W]
    w = c.w.to(dtype).reshape(c.Cout, c.KT, c.KH, c.KW, c.Cin).permute(0, 4, 1, 2, 3)
    if c.up2:
        x = x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    if c.kind == "down":                                    # ZeroPad2d((0, 1, 0, 1)) only where the last tap has no real row
        need_h, need_w = 2 * (c.Hout - 1) + 3, 2 * (c.Wout - 1) + 3
        x = F.pad(x, (0, need_w - x.shape[4], 0, need_h - x.shape[3]))
    else:
        x = F.pad(x, (c.pad_w, c.pad_w, c.pad_h, c.pad_h))
    return F.conv3d(x, w, stride=(c.stride_t, c.stride_hw, c.stride_hw))[0].permute(1, 2, 3, 0)


def _torch_full(c, dtype=F64):
    v = _torch_conv(c, dtype)
    if c.bias is not None:
        v = v + c.bias.to(dtype)
    if c.split_n:                                           # the reshape of test_conv_cl_upsample_downsample_stride_split
        r = v.permute(3, 0, 1, 2).reshape(c.fmul, c.split_n, c.Tout, c.Hout, c.Wout)
        v = torch.stack(tuple(r[j] for j in range(c.fmul)), 2).reshape(c.split_n, c.Tout * c.fmul, c.Hout, c.Wout).permute(1, 2, 3, 0)
    if c.resid is not None:
        v = v + c.resid.to(dtype)
    return v


@pytest.fixture(scope="module")
def cases():
    return [(cs, R.build(cs, seed=i)) for i, cs in enumerate(R.all_cases())]


def test_every_listed_instantiation_has_a_case_of_both_output_types():
    routes = {cs["route"] for cs in R.all_cases()}
    assert set(R.ALL_ROUTES) <= routes, sorted(set(R.ALL_ROUTES) - routes)
    assert max(R.build(cs).M for cs in R.all_cases()) <= 2100


def test_each_case_names_the_route_the_restated_dispatch_gives(cases):
    for cs, c in cases:
        got, fused = R.route_of(c, cs["tile"], kw3=cs["kw3"])
        assert got == cs["route"], (cs, got)
        assert fused == (c.norm and cs["route"].split("/")[0] in ("w64Pn", "pairPn"))


def test_check_exact_holds_for_every_gpu_case_and_refuses_what_does_not_fit(cases):
    top = max(R.check_exact(c) for _, c in cases)
    assert top < R.F32_EXACT
    with pytest.raises(AssertionError):                     # 384 real channels x 27 taps: 21 M units of 2^-9
        R.make_case(768, 96, 1, 3, 3, KT=3, pair=True, out_f32=True)
    R.make_case(768, 96, 1, 3, 3, KT=1, pair=True, out_f32=True)


def test_reference_equals_torch_float64_on_the_padded_and_upsampled_tensor(cases):
    seen = set()
    for cs, c in cases:
        if c.pair:
            continue
        seen.add((c.kind, c.KT, c.KH, bool(c.split_n)))
        want = _torch_full(c)
        got = R.reference(c).y64
        assert got.shape == want.shape == c.out_shape and torch.equal(got, want), cs
    assert {k[0] for k in seen} == {"same", "down", "tstride", "up2"} and any(k[3] for k in seen)


def test_a_plain_fp32_convolution_passes_the_exact_assertion(cases):
    for cs, c in cases:
        if c.pair:
            (xh, xl), (wh, wl) = R.pair_halves(c.x.float()), R.pair_halves(c.w.float().reshape(c.Cout, c.taps, c.Cin))
            v = sum(_torch_conv(R.NS(**{**vars(c), "x": a, "w": b.reshape(c.Cout, -1), "Cin": c.Cin // 2}), torch.float32)
                    for a, b in ((xh, wh), (xl, wh), (xh, wl)))
            v = v + (c.bias if c.bias is not None else 0.0) + (c.resid if c.resid is not None else 0.0)
        else:
            v = _torch_full(c, torch.float32)
        got = v if c.out_f32 else v.to(torch.bfloat16)
        assert R.mismatch(got.contiguous(), R.reference(c).y, c) is None, cs


def _first(cases, **want):
    for cs, c in cases:
        if all((cs.get(k) if k in cs else getattr(c, k)) == v for k, v in want.items()):
            return c
    raise LookupError(want)


# tolerances of tests/test_gpu_vae.py's rel_rms assertions on the convolution: its kernels at large, the folded upsample
# on the stream before this file existed
REL_RMS_TOL, REL_RMS_TOL_UP2 = 2e-5, 2e-3


def test_planted_defects_are_reported_per_element(cases):
    """Each defect, applied to a correct result at a shape the GPU test runs, is named with its count and first (t, y, x, co).
    ``seen_by_rel_rms`` records what the tolerance of tests/test_gpu_vae.py would have noticed."""
    picks = {
        "row_wrap": _first(cases, route="w64P/f32", Tout=2, Hout=15, KT=3),
        "frame_wrap": _first(cases, route="w64P/f32", Tout=2, Hout=15, KT=3),
        "drop_k_block": _first(cases, route="kw3<4,2>/f32", Cin=96),
        "truncate": _first(cases, route="w64Q/bf16"),
        "bias_next": _first(cases, route="wide<4,2>/f32", has_bias=True),
        "resid_twice": _first(cases, route="128x128/f32", resid_kind="f32", Cout=136),
        "up2_plus_one": _first(cases, kind="up2", route="w64P/f32"),
        "pad_row_read": _first(cases, kind="down", Hin=8),
        "split_swap": _first(cases, split_n=40, out_f32=1),
        "lo_lo": _first(cases, route="pairQ/f32"),
    }
    assert set(picks) == set(R.DEFECTS)
    seen_by_rel_rms = {}
    for name, c in picks.items():
        good, bad = R.reference(c), None
        try:
            bad = R.reference(c, defect=name)
        except AssertionError:                              # lo_lo: multiples of 2^-18 may even leave fp32's exact range
            bad = R.NS(y=R.accumulate(c, defect=name).float())
        msg = R.mismatch(bad.y, good.y, c)
        assert msg is not None and "elements differ; first: (t " in msg and "got" in msg and "want" in msg, (name, msg)
        rr = rel_rms(bad.y, good.y)
        seen_by_rel_rms[name] = rr >= REL_RMS_TOL
        print(f"[defect] {name}: {msg[:150]} ...  rel_rms {rr:.2e}: {'seen' if rr >= REL_RMS_TOL else 'NOT seen'} at 2e-5, "
              f"{'seen' if rr >= REL_RMS_TOL_UP2 else 'NOT seen'} at 2e-3")
    # one wrong voxel of ~2 000, or an RNE / truncation difference, is below 2e-5 of the whole tensor or not: recorded, and at
    # least the single-voxel and the pair defects must be among those the old assertion could not be trusted with
    assert not seen_by_rel_rms["lo_lo"]


def test_a_reference_with_lo_lo_differs_from_the_contract(cases):
    c = _first(cases, route="pairP/f32")
    a, b = R.accumulate(c), R.accumulate(c, defect="lo_lo")
    d = (a - b).abs()
    assert float(d.max()) > 0 and float(d.max()) <= c.K // 2 * 4 * 2.0 ** -18
    assert bool((d > 0).float().mean() > 0.5)


def test_a_store_past_m_and_a_changed_input_bit_are_reported():
    c = R.make_case(32, 96, 1, 5, 7, bias=True)
    cv = R.Canvas(c.M, c.cch, c.cch, torch.float32, lead=4, trail=16).arm()
    cv.window().copy_(R.reference(R.make_case(32, 96, 1, 5, 7, bias=True, out_f32=True)).y.reshape(c.M, c.cch))
    assert cv.guard_report("y") is None
    cv.buf[cv.start + c.M * c.cch + 5] = 1.0                # row M, column 5
    msg = cv.guard_report("y")
    assert msg is not None and f"(row {c.M}, col 5)" in msg
    x = c.x.clone()
    fz = R.Frozen(x, "x")
    assert fz.report() is None
    x.view(torch.int16)[2, 2, 1, 0] ^= 1
    assert "1 elements changed" in fz.report()


# ----------------------------------------------------------------------------------------------------------------------
# the norm: the restatement, K_NORM, the exact cases
# ----------------------------------------------------------------------------------------------------------------------
def _norm_ratios():
    worst = {"bf16": 0.0, "split": 0.0}
    for C in R.NORM_C:
        for P in R.NORM_P:
            gamma = R.norm_gamma(C, seed=P)
            for bf in (False, True):
                x = R.norm_input(C, P, seed=C + P, bf16=bf)
                for do_silu in (False, True):
                    ref = R.norm_reference(x, gamma, do_silu)
                    unit = (R.N.SLACK * ref.S).clamp_min(2.0 ** -300)
                    for nudge in R.NUDGES:
                        a = R.norm_restated(x, gamma, do_silu, nudge)
                        err = (a.double() - ref.y).abs()
                        worst["bf16"] = max(worst["bf16"], float((err / unit).max()))
                        hi, lo = R.split_pair(a)
                        err = (hi.double() + lo.double() - ref.y).abs()
                        worst["split"] = max(worst["split"], float((err / unit).max()))
    return worst


def test_k_norm_is_four_times_the_restatements_worst_ratio_rounded_up_to_a_power_of_two():
    worst = _norm_ratios()
    print("\n[measured] restatement / (2^-16 S): " + "  ".join(f"{k}={v:.4f}" for k, v in sorted(worst.items())))
    for kind, ratio in worst.items():
        assert ratio > 0 and R.K_NORM[kind] == 2.0 ** math.ceil(math.log2(4.0 * ratio)), (kind, ratio, R.K_NORM[kind])


def test_the_restatement_holds_the_bounds_it_derives_and_a_defect_does_not():
    for C in R.NORM_C:
        gamma = R.norm_gamma(C, seed=3)
        x = R.norm_input(C, 77, seed=C)
        for do_silu in (False, True):
            ref = R.norm_reference(x, gamma, do_silu)
            a = R.norm_restated(x, gamma, do_silu)
            assert R.N.compare("host", "y", a.to(torch.bfloat16).float(), ref.y, R.norm_bound(ref, "bf16"), record=False) is None
            hi, lo = R.split_pair(a)
            assert R.N.compare("host", "hi + lo", hi.double() + lo.double(), ref.y, R.norm_bound(ref, "split"), record=False) is None
            # a norm over C + 8 channels' worth (sqrt(C) off by 4 %), gamma of the next channel, truncation
            for bad in (a * math.sqrt((C + 8) / C), R.norm_restated(x, gamma.roll(-1), do_silu)):
                assert R.N.compare("host", "y", bad.to(torch.bfloat16).float(), ref.y, R.norm_bound(ref, "bf16"), record=False) is not None
            assert R.N.compare("host", "y", R.truncate_bf16(a).float(), ref.y, R.norm_bound(ref, "bf16"), record=False) is not None
            # a split whose lo is dropped misses the fp32 bound
            assert R.N.compare("host", "hi + lo", hi.double(), ref.y, R.norm_bound(ref, "split"), record=False) is not None


def test_power_of_two_voxels_are_exact_up_to_one_rounding():
    for C in R.NORM_C:
        gamma = R.norm_gamma(C, seed=1, pow2=True)
        x = R.norm_input_pow2(C, 77, seed=C)
        ref = R.norm_reference(x, gamma, do_silu=False)
        want = R.rne_bf16(ref.y)                            # asserts that ref.y is exact in fp32
        assert torch.equal(want.double(), ref.y), "x inv gamma is not a bf16 value"
        for nudge in R.NUDGES:
            assert torch.equal(R.norm_restated(x, gamma, False, nudge).to(torch.bfloat16), want)


def test_rows_per_workgroup_restated():
    assert [R.rows_per_workgroup(C) for C in R.NORM_C] == [64, 64, 16, 16]
    assert all(77 % R.rows_per_workgroup(C) for C in R.NORM_C)
