"""Interval masks with one group size per axis and frame-aligned condition tokens, the part that needs no GPU: the
declared / exported symbols and the struct, ``causal.IntervalMask(k_group=)`` against its matrix, ``interval_visible``
against loops, ``causal.condition_window_visible`` against a brute-force statement of the rule, the model's token order,
the ValueErrors, ``condition_frames`` and the fp32 restatement tests/condition_window_ref.py against the oracle."""
import ctypes
import importlib
import inspect
import os
import re

import pytest
import torch

import condition_window_ref as CR
import make_golden_chunk_causal as MC
from conftest import PKG
from oracle import wan_dit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("omh_flash_attn_fwd_interval_rect_d128", "omh_flash_attn_bwd_interval_rect_d128")


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


@pytest.fixture(scope="module")
def model_mod(omh):
    return importlib.import_module(PKG + ".wan.modules.model")


def _runs(values):
    out, start = [], None
    for i, v in enumerate(list(values) + [False]):
        if v and start is None:
            start = i
        if not v and start is not None:
            out.append((start, i))
            start = None
    return out


def test_symbols_and_struct(omh):
    binding = importlib.import_module(PKG + "._lib")
    header = open(os.path.join(ROOT, "include", "omh.h")).read()
    for name in ENTRIES:
        assert name in binding.EXPORTED and hasattr(binding.lib, name)
        assert re.search(r"\bint " + name + r"\(", header)
    assert "typedef struct omh_interval_rect_mask" in header
    assert re.search(r"#define OMH_ABI_VERSION\s+12\b", header) and binding.lib.omh_abi_version() == 12
    A = binding.IntervalRectMaskArgs
    assert [f[0] for f in A._fields_] == ["q_group", "k_group", "q_groups", "k_groups", "q_iv", "k_iv"]
    assert ctypes.sizeof(A) == 32
    assert [getattr(A, n).offset for n in ("q_group", "k_group", "q_groups", "k_groups", "q_iv", "k_iv")] == [0, 4, 8, 12, 16, 24]


def test_entries_validate_without_gpu(omh):
    """The refusals of the two-run interval entries, in their order, with their codes (fake, aligned pointers)."""
    binding = importlib.import_module(PKG + "._lib")
    lib, by = binding.lib, ctypes.byref
    P = 4096

    def fwd_args(**kw):
        a = binding.AttnArgs(P, P, P, P, None, 1, 2, 256, 384, 0, 256, 0, 256, 0, 0, 256, 384, 0.1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def bwd_args(**kw):
        a = binding.AttnBwdArgs()
        for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv", "o32"):
            setattr(a, name, P)
        a.B, a.H, a.Lq, a.Lk = 1, 2, 256, 384
        for name in ("q_rs", "k_rs", "o_rs", "dq_rs", "dk_rs"):
            setattr(a, name, 256)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def mask(qg=64, kg=3, nq=4, nk=128, q_iv=P, k_iv=P):
        return binding.IntervalRectMaskArgs(qg, kg, nq, nk, q_iv, k_iv)

    bad, align, shape = -1, -2, -3
    fwd = lambda a, m: lib.omh_flash_attn_fwd_interval_rect_d128(by(a), None if m is None else by(m), None)
    bwd = lambda a, m: lib.omh_flash_attn_bwd_interval_rect_d128(by(a), None, None if m is None else by(m), None)
    assert lib.omh_flash_attn_fwd_interval_rect_d128(None, by(mask()), None) == bad
    assert lib.omh_flash_attn_bwd_interval_rect_d128(None, None, by(mask()), None) == bad
    for entry, args in ((fwd, fwd_args), (bwd, bwd_args)):
        assert entry(args(), None) == bad                                        # a null struct
        assert entry(args(), mask(qg=7, nq=37)) == bad                           # q_group < 8
        assert entry(args(), mask(kg=0)) == bad                                  # k_group < 1
        assert entry(args(), mask(nq=5)) == bad                                  # not ceil(Lq / q_group)
        assert entry(args(), mask(nk=127)) == bad                                # not ceil(Lk / k_group)
        assert entry(args(), mask(kg=64, nk=128)) == bad                         # the query group's size on the key axis
        assert entry(args(), mask(q_iv=None)) == bad
        assert entry(args(), mask(k_iv=None)) == bad
        assert entry(args(), mask(q_iv=P + 2)) == align
        assert entry(args(), mask(k_iv=P + 1)) == align
    g = 2 ** 20
    assert fwd(fwd_args(Lq=2 ** 28, Lk=64, ldv=64), mask(qg=g, kg=1, nq=256, nk=64)) == shape
    for wl, wr in ((16, 16), (-1, 0), (0, 5), (3, -1)):                          # a band beside the mask
        assert fwd(fwd_args(window_left=wl, window_right=wr), mask()) == bad
    for wl, wr in ((0, 0), (-1, -1)):                                            # these pass THAT check: q_lens' alignment stops them
        assert fwd(fwd_args(window_left=wl, window_right=wr, q_lens=P + 2), mask()) == align
    assert bwd(bwd_args(o32=None), mask()) == bad                                # the backward needs the fp32 output
    assert lib.omh_flash_attn_bwd_interval_rect_d128(by(bwd_args()), P + 2, by(mask()), None) == align
    assert bwd(bwd_args(phase=4, o_rs=256), mask()) == bad


def test_rect_mask_tables_and_visible(causal):
    vis = torch.tensor([[1, 1, 0, 0, 0, 1, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0, 0]]).bool()
    m = causal.IntervalMask(vis, 10, k_group=3)
    assert (m.group, m.k_group, m.q_groups, m.k_groups, m.runs) == (10, 3, 4, 7, 2)
    assert m.q_iv.shape == (4, 4) and m.k_iv.shape == (7, 4) and m.q_iv.dtype == torch.int32
    for table, lines in ((m.q_iv, vis.tolist()), (m.k_iv, vis.t().tolist())):
        for (lo0, hi0, lo1, hi1), line in zip(table.tolist(), lines):
            assert lo0 <= hi0 <= lo1 <= hi1
            assert [(a, b) for a, b in ((lo0, hi0), (lo1, hi1)) if b > a] == _runs(line)
    s = m.c_struct()
    assert (s.q_group, s.k_group, s.q_groups, s.k_groups) == (10, 3, 4, 7)
    assert type(s).__name__ == "IntervalRectMaskArgs"
    assert m.to("cpu") is m
    Lq, Lk, qlen, klen = 37, 20, 33, 19                                          # partial last groups on both axes
    got = causal.interval_visible(m, Lq, Lk, qlen, klen)
    assert got.shape == (Lq, Lk) and got.dtype == torch.bool
    for i in range(Lq):
        for j in range(Lk):
            assert bool(got[i, j]) == (i < qlen and j < klen and bool(vis[i // 10, j // 3]))
    with pytest.raises(ValueError):
        causal.interval_visible(m, Lq, Lk + 3)
    with pytest.raises(ValueError):
        causal.interval_visible(m, Lq + 10, Lk)
    # k_group=None is the square object, unchanged
    sq = causal.IntervalMask(causal.teacher_forcing_groups(2), 64)
    assert sq.k_group is None and type(sq.c_struct()).__name__ == "IntervalMaskArgs"
    for bad in (dict(k_group=0), dict(k_group=1, runs=3)):
        with pytest.raises(ValueError):
            causal.IntervalMask(vis, 10, **bad)
    with pytest.raises(ValueError):
        causal.IntervalMask(vis, 7, k_group=1)
    with pytest.raises(ValueError):
        causal.IntervalMask([[1, 0, 1, 0, 1]], 8, k_group=1)                     # three runs
    assert "k_group" in inspect.signature(causal.IntervalMask.__init__).parameters


def test_attn_mask_routes_the_rect_form(omh, causal):
    ops = importlib.import_module(PKG + ".ops")
    vis = causal.condition_window_visible(4, torch.tensor([0, 1, 2, 3]), 60, 0, 0)
    m = causal.IntervalMask(vis, 64, k_group=1)
    am = ops.attn_mask(interval_mask=m, H=2, Lq=256, Lk=64, device=torch.device("cpu"))
    assert am.kind == "interval" and am.rule is m
    assert ops._mask_entries(am) == ENTRIES
    sq = ops.attn_mask(interval_mask=causal.IntervalMask(causal.teacher_forcing_groups(2), 64), H=2, Lq=256, Lk=256,
                       device=torch.device("cpu"))
    assert ops._mask_entries(sq) == ("omh_flash_attn_fwd_interval_d128", "omh_flash_attn_bwd_interval_d128")
    for Lq, Lk in ((320, 64), (256, 65), (256, 128)):
        with pytest.raises(ValueError):
            ops.attn_mask(interval_mask=m, H=2, Lq=Lq, Lk=Lk, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        ops.attn_mask((16, -1), interval_mask=m, H=2, Lq=256, Lk=64, device=torch.device("cpu"))


def test_tile_counts_of_the_skipping_case(causal):
    """Case 3 of tests/test_gpu_attn_interval_rect.py: 40 frames of 24 queries on one key group of 8 each, then 8 text
    groups.  The first query workgroup runs key tiles 0 and 5 and skips 1 - 4; ``tiles()`` agrees with a count on the
    dense matrix."""
    tf = [f for f in range(40) for _ in range(8)]
    vis = causal.condition_window_visible(40, torch.tensor(tf), 64, 0, 0)[:, ::8]
    m = causal.IntervalMask(vis, 24, k_group=8)
    dense = causal.interval_visible(m, 960, 384)
    per_wg = [[t for t in range(6) if bool(dense[q0:q0 + 128, 64 * t:64 * t + 64].any())] for q0 in range(0, 960, 128)]
    assert per_wg[0] == [0, 5]
    assert m.tiles(960, 384) == sum(len(t) for t in per_wg) < 8 * 6
    assert causal.IntervalMask(torch.ones(1, 1), 960, k_group=384).tiles(960, 384) == 8 * 6


def _brute(q_frames, token_frames, n_text, back, ahead, fpc, segments, offset):
    rows = []
    for r in range(segments * q_frames):
        f = offset + r % q_frames
        row = []
        for g in token_frames:
            if g == -1:
                row.append(True)
                continue
            hi = None if ahead < 0 else f + ahead
            if fpc is not None:
                E = (f // fpc) * fpc + fpc - 1
                hi = E if hi is None else min(hi, E)
            row.append((back < 0 or g >= f - back) and (hi is None or g <= hi))
        rows.append(row + [True] * n_text)
    return torch.tensor(rows, dtype=torch.bool).view(segments * q_frames, len(token_frames) + n_text)


SHUFFLED = [3, 0, -1, 2, 2, 5, 1, 1, -1, 4, 0, 3, 5, 2]


@pytest.mark.parametrize("back,ahead", [(0, 0), (1, 1), (2, 0), (-1, 0)])
@pytest.mark.parametrize("fpc", [None, 1, 2])
@pytest.mark.parametrize("segments", [1, 2])
def test_condition_window_rule(causal, back, ahead, fpc, segments):
    for offset in (0, 2):
        got = causal.condition_window_visible(6, torch.tensor(SHUFFLED), 3, back, ahead, fpc, segments, offset)
        assert got.dtype == torch.bool and got.shape == (segments * 6, len(SHUFFLED) + 3)
        assert torch.equal(got, _brute(6, SHUFFLED, 3, back, ahead, fpc, segments, offset))


def test_condition_window_refusals(causal):
    for bad in (dict(q_frames=0), dict(n_text=-1), dict(segments=0), dict(frame_offset=-1), dict(frames_per_chunk=0),
                dict(token_frames=torch.tensor([0, -2])), dict(token_frames=torch.tensor([0.0, 1.0])),
                dict(token_frames=torch.tensor([[0, 1]]))):
        kw = dict(q_frames=4, token_frames=torch.tensor([0, 1]), n_text=2, back=0, ahead=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            causal.condition_window_visible(**kw)


def _cpu_model(model_mod, **kw):
    return model_mod.WanModel(num_layers=2, **dict(MC.make_golden.TINY, **kw))


def test_model_order_gives_two_runs(causal, model_mod):
    """After the model's stable sort (frame tokens ascending, then the -1 tokens, then the text) every row is
    [window] U [global | text] and every column one run, two under teacher forcing; the tokens move with their frames."""
    m = _cpu_model(model_mod)
    tok = torch.arange(len(SHUFFLED), dtype=torch.float32).view(1, -1, 1).expand(2, -1, 64).contiguous()
    for back, ahead in ((0, 0), (1, 1), (2, 0), (-1, 0), (-1, -1)):
        n = m._normal_conditions({"tokens": tok, "frames": torch.tensor(SHUFFLED), "window": (back, ahead)})
        order = sorted(range(len(SHUFFLED)), key=lambda j: (SHUFFLED[j] < 0, SHUFFLED[j]))
        assert list(n["frames"]) == [SHUFFLED[j] for j in order] and n["window"] == (back, ahead)
        assert n["tokens"][0, :, 0].tolist() == [float(j) for j in order]            # stable, and the tokens follow
        assert m._normal_conditions(n) is n
        for fpc in (None, 1, 2):
            for segments in (1, 2):
                vis = causal.condition_window_visible(6, torch.tensor(n["frames"]), 5, back, ahead, fpc, segments)
                assert all(len(_runs(r)) <= 2 for r in vis.tolist())
                assert all(len(_runs(c)) <= segments for c in vis.t().tolist())
                causal.IntervalMask(vis, 56, k_group=1)                              # the tables build
    # a chunk keeps what one of its queries sees: frames 2, 3 under (1, 0) see the frames 1 .. 3 and the -1 tokens
    n = m._normal_conditions({"tokens": tok, "frames": torch.tensor(SHUFFLED), "window": (1, 0)}, chunk=(2, 2))
    assert list(n["frames"]) == [1, 1, 2, 2, 2, 3, 3, -1, -1] and n["chunk"] == (2, 2)
    assert m._normal_conditions({"tokens": tok, "frames": torch.tensor(SHUFFLED), "window": (0, 0)}, chunk=(7, 1)) is not None
    only = {"tokens": tok[:, :2], "frames": torch.tensor([0, 1]), "window": (0, 0)}
    assert m._normal_conditions(only, chunk=(3, 1)) is None                          # nothing left for frame 3
    plain = {"tokens": tok}
    assert m._normal_conditions(plain) is plain and m._normal_conditions(tok) is tok and m._normal_conditions(None) is None


def test_model_refusals_before_any_device_call(causal, model_mod):
    """On a CPU model: the ValueErrors come before the 'runs on the MI355X only' error of the first device call."""
    m = _cpu_model(model_mod)
    x = [torch.zeros(16, 4, 14, 16)] * 2
    ctx = [torch.zeros(8, 64)] * 2
    t = torch.tensor([1.0, 2.0])
    tok = torch.zeros(2, 5, MC.make_golden.TINY["dim"])
    good = {"tokens": tok, "frames": torch.tensor([0, 1, 2, 3, -1]), "window": (0, 0)}
    for bad in (dict(frames=torch.tensor([0, 1, 2, 3])),                          # another length
                dict(frames=torch.tensor([0., 1., 2., 3., -1.])),                  # another dtype
                dict(frames=[0, 1, 2, 3, -1]),                                     # no tensor
                dict(frames=torch.tensor([0, 1, 2, 3, -2])),
                dict(window=None)):
        ec = dict(good, **bad)
        for call in (lambda: m(x, t, ctx, 224, extra_conditions=ec), lambda: m.encode_context(ctx, extra_conditions=ec)):
            with pytest.raises(ValueError):
                call()
    missing = {k: v for k, v in good.items() if k != "window"}
    with pytest.raises(ValueError):
        m(x, t, ctx, 224, extra_conditions=missing)
    i2v = _cpu_model(model_mod, model_type="i2v")
    with pytest.raises(ValueError):
        i2v(x, t, ctx, 224, extra_conditions=good)
    ops = importlib.import_module(PKG + ".ops")
    with pytest.raises(ops.OmhError):                                              # a good dict reaches the device check
        m(x, t, ctx, 224, extra_conditions=good)
    for fn in (m.forward_chunk, causal.sample, causal.self_forcing_rollout):
        assert "extra_conditions" in inspect.signature(fn).parameters
    assert "interval_mask" in inspect.signature(model_mod.WanT2VCrossAttention.forward).parameters


def test_condition_frames():
    """9 video frames behind one reference frame: 8 audio pairs (frames t, t + 1), then 9 pose tokens; video frame v sits
    at latent frame (v + 3) // 4 + 1."""
    mod = importlib.import_module(PKG + ".omnihuman_wan_t2v")
    got = mod.OmniHumanWanT2V.condition_frames(8, 9, ref_frames=1)
    lat = lambda v: (v + 3) // 4 + 1
    want = [lat(t + k) for t in range(8) for k in (0, 1)] + [lat(v) for v in range(9)]
    assert got.dtype == torch.int64 and got.tolist() == want
    assert [lat(v) for v in range(9)] == [1, 2, 2, 2, 2, 3, 3, 3, 3]
    assert mod.OmniConditionsModule.condition_frames(0, 5).tolist() == [0, 1, 1, 1, 1]


def test_restatement_is_pinned_to_the_oracle(causal):
    """tests/condition_window_ref.py with every token visible is O.dit_forward(extra_tokens=) to fp32 rounding; on the
    inputs of tests/test_gpu_condition_window_model.py its windowed and unwindowed outputs differ by >= 5e-2 rel-RMS."""
    cfg, clean, _, _, ctx, t_frames, tok, frames = CR.case()
    sd = O.synth_state_dict(cfg, MC.TAG)
    S = CR.F_LATENT * CR.TOKENS_PER_FRAME
    t = torch.tensor([900., 300.])
    every = torch.ones(S, len(CR.FRAMES) + cfg.text_len, dtype=torch.bool)
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, clean, t, ctx, S, extra_tokens=tok)
        for got in (CR.forward(sd, cfg, clean, t[:, None].expand(2, 4), ctx, S, extra_tokens=tok),
                    CR.forward(sd, cfg, clean, t[:, None].expand(2, 4), ctx, S, extra_tokens=tok, cross_mask=every)):
            for a, b in zip(got, ref):
                assert float((a.double() - b.double()).norm() / b.double().norm()) < 1e-6
        base = CR.forward(sd, cfg, clean, t_frames, ctx, S, extra_tokens=tok)
        for back, ahead in ((0, 0), (1, 1), (-1, 0)):
            vis = causal.condition_window_visible(CR.F_LATENT, frames, cfg.text_len, back, ahead)
            out = CR.forward(sd, cfg, clean, t_frames, ctx, S, extra_tokens=tok,
                             cross_mask=vis.repeat_interleave(CR.TOKENS_PER_FRAME, 0))
            for a, b in zip(out, base):
                diff = float((a - b).norm() / b.norm())
                print(f"window ({back}, {ahead}): windowed against unwindowed rel-RMS {diff:.3f}")
                assert diff >= 5e-2
