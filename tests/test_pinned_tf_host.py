"""Host checks for teacher forcing under a pinned sink (no GPU): the extended-key restatement tests/pinned_tf_ref.py against
tests/pinned_sink_ref.py, the rectangular mask of causal.teacher_forcing_groups(pin_sink=True) against the rule,
causal.sink_copy_deltas, the (cos, sin) tables of omh_rope_shift_table, the refusals and the header entries."""
import importlib
import os
import re

import pytest
import torch

import make_golden_chunk_causal as MC
import pinned_sink_ref as PR
import pinned_tf_ref as PT
import teacher_forcing_ref as R
from conftest import PKG, rel_rms
from oracle import wan_dit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPF = MC.TOKENS_PER_FRAME
SETTINGS = ((1, 1, 1, 6), (2, 1, 1, 8), (1, 0, 2, 6))                            # fpc, W, S, F
GEOMETRIES = ((4, 1, 1), (7, 1, 1), (7, 2, 1), (8, 1, 2), (12, 1, 1), (21, 2, 1), (6, 0, 1), (5, 0, 2))     # n, W, S


@pytest.fixture(scope="module")
def causal():
    return importlib.import_module(PKG + ".causal")


def _inputs(F):
    """The inputs of tests/test_gpu_sink_model.py::_inputs."""
    cfg, _, ctx, _, _ = MC.case()
    g = torch.Generator().manual_seed(17)
    clean = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    noisy = [torch.randn(16, F, 14, 16, generator=g) for _ in range(2)]
    t_frames = torch.stack([torch.linspace(900., 100., F), torch.linspace(50., 950., F)])
    return cfg, clean, noisy, ctx, t_frames


@pytest.mark.parametrize("fpc,W,S,F", SETTINGS)
def test_extended_keys_are_the_pinned_restatement(causal, fpc, W, S, F):
    """Dense attention over the extended key axis computes what pinned_sink_ref.forward(pinned=True) computes by
    overwriting scores: < 1e-6 rel-RMS (fp32 summation order is all that differs)."""
    cfg, clean, noisy, ctx, t_frames = _inputs(F)
    sd = O.synth_state_dict(cfg, MC.TAG)
    t = t_frames[:, ::fpc].clone()
    assert any(PR.sink_deltas(F // fpc, W, S, fpc))                             # the clip outlasts the ring
    ref = PR.forward(sd, cfg, clean, noisy, t, ctx, causal, fpc, W, S, pinned=True)
    with torch.no_grad():
        got = PT.forward(sd, cfg, clean, noisy, t, ctx, causal, fpc, W, S)
    for a, b in zip(got, ref):
        err = rel_rms(a, b)
        print(f"({fpc}, {W}, {S}, {F}): extended keys against the pinned restatement rel-RMS {err:.2e}")
        assert a.shape == b.shape and err < 1e-6


def test_extended_keys_without_a_copy_are_teacher_forcing(causal):
    """A clip that does not outlast the ring has no copy: the operations of teacher_forcing_ref.forward under the square
    mask, hence its result exactly."""
    fpc, W, S, F = 1, 1, 1, 3
    cfg, clean, noisy, ctx, t = _inputs(F)
    sd = O.synth_state_dict(cfg, MC.TAG)
    assert causal.sink_copy_deltas(F, W, S, fpc) == []
    m = causal.IntervalMask(causal.teacher_forcing_groups(F, W, S), TPF, runs=3)
    mask = causal.interval_visible(m, 2 * F * TPF, 2 * F * TPF)[None].expand(2, -1, -1)
    with torch.no_grad():
        got = PT.forward(sd, cfg, clean, noisy, t, ctx, causal, fpc, W, S)
        ref = R.forward(sd, cfg, [torch.cat([c, n], 1) for c, n in zip(clean, noisy)], torch.cat([torch.zeros(2, F), t], 1),
                        ctx, 2 * F * TPF, mask=mask, segments=2, out_from=F)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_sink_copy_deltas(causal):
    assert causal.sink_copy_deltas(7, 1, 1, 1) == [(3, 1), (4, 2), (5, 3), (6, 4)]
    assert causal.sink_copy_deltas(7, 1, 2, 2) == [(4, 2), (5, 4), (6, 6)]
    assert causal.sink_copy_deltas(3, 1, 1, 1) == [] and causal.sink_copy_deltas(1, 0, 1, 4) == []
    for n, W, S in GEOMETRIES:
        for fpc in (1, 3):
            deltas = PR.sink_deltas(n, W, S, fpc)
            assert causal.sink_copy_deltas(n, W, S, fpc) == [(I, d) for I, d in enumerate(deltas) if d > 0]
            assert len(causal.sink_copy_deltas(n, W, S, fpc)) == max(0, n - S - W - 1)
    for bad in ((4, 1, 0, 1), (4, -1, 1, 1), (0, 1, 1, 1), (4, 1, 1, 0)):
        with pytest.raises(ValueError):
            causal.sink_copy_deltas(*bad)


@pytest.mark.parametrize("n,W,S", GEOMETRIES)
def test_pinned_mask_selects_the_rule(causal, n, W, S):
    """Expanded densely, query chunk I (clean and noisy) sees exactly the (key chunk, Delta) pairs of the rule: what
    teacher_forcing_groups(n, W, S) shows it, the sink chunks at Delta_I, everything else at 0 — and the three-run tables
    take the matrix."""
    fpc = 2
    vis = causal.teacher_forcing_groups(n, W, S, pin_sink=True)
    square = causal.teacher_forcing_groups(n, W, S)
    deltas = PR.sink_deltas(n, W, S, fpc)
    copies = causal.sink_copy_deltas(n, W, S, fpc)
    C = max(0, n - S - W - 1)
    assert vis.dtype == torch.bool and vis.shape == (2 * n, 2 * n + C * S) and len(copies) == C
    # what a column of the extended axis is: (column of the square axis, shift of its keys)
    column = [(j, 0) for j in range(2 * n)] + [(j, d) for _, d in copies for j in range(S)]
    for r in range(2 * n):
        I = r % n
        want = {(j, deltas[I] if j < S else 0) for j in range(2 * n) if square[r, j]}
        got = {column[j] for j in range(vis.shape[1]) if vis[r, j]}
        assert got == want, (r, sorted(got), sorted(want))
        assert int(vis[r].sum()) == int(square[r].sum())                         # (no key twice)
    m = causal.IntervalMask(vis, 8, runs=3)
    assert (m.q_groups, m.k_groups) == tuple(vis.shape)
    runs = lambda row: int((row[1:] & ~row[:-1]).sum()) + int(row[0])
    assert max(runs(r) for r in vis) <= 3 and max(runs(c) for c in vis.t()) <= 2
    dense = causal.interval_visible(m, 2 * n * 8, vis.shape[1] * 8)
    assert torch.equal(dense, vis.repeat_interleave(8, 0).repeat_interleave(8, 1))
    # pin_sink=False is today's matrix
    assert torch.equal(causal.teacher_forcing_groups(n, W, S, pin_sink=False), square)
    assert torch.equal(causal.teacher_forcing_groups(n, W, S, False), square)
    if C == 0:
        assert torch.equal(vis, square)


def test_mask_refusals(causal):
    for n, W, S in ((6, 1, 0), (6, -1, 1), (6, -1, 0)):
        with pytest.raises(ValueError, match="pin_sink"):
            causal.teacher_forcing_groups(n, W, S, pin_sink=True)
    causal.teacher_forcing_groups(6, -1, 1)                                     # (without a pin every one of them stands)


def test_shift_table_is_the_restatement_bit_for_bit():
    """omh_rope_shift_table against pinned_sink_ref._frame_angles -> fp32: the numbers ops.rope_shift_frames hands its kernel."""
    ops = importlib.import_module(PKG + ".ops")
    deltas = (0, 1, 3, 1000, 10 ** 6)
    tab = ops.rope_shift_table(deltas)
    assert tab.shape == (5, ops.ROPE_SHIFT_MAX_PAIRS, 2) and tab.dtype == torch.float32 and tab.device.type == "cpu"
    for c, delta in enumerate(deltas):
        a = PR._frame_angles(delta, 128, 10000.0)
        nf = a.numel()
        assert nf == 22
        assert torch.equal(tab[c, :nf, 0], torch.cos(a).float()) and torch.equal(tab[c, :nf, 1], torch.sin(a).float())
        assert bool((tab[c, nf:, 0] == 1).all()) and bool((tab[c, nf:, 1] == 0).all())
    assert bool((tab[0, :, 0] == 1).all()) and bool((tab[0, :, 1] == 0).all())   # delta = 0: the identity everywhere
    a = PR._frame_angles(7, 64, 500.0)                                          # another head size and base
    t = ops.rope_shift_table([7], head_dim=64, theta=500.0)
    assert torch.equal(t[0, :a.numel(), 0], torch.cos(a).float()) and torch.equal(t[0, :a.numel(), 1], torch.sin(a).float())
    with pytest.raises(ops.OmhError):
        ops.rope_shift_table([1], head_dim=12)


def test_model_and_loss_refusals(causal):
    """pin_sink=True without a sink (or without a window) is refused before anything touches a device."""
    model_mod = importlib.import_module(PKG + ".wan.modules.model")
    m = model_mod.WanModel(num_layers=2, **MC.make_golden.TINY)
    x = [torch.zeros(16, 6, 14, 16)]
    t = torch.zeros(1, 6)
    for setting in ((1, 1), (1, 1, 0), (1, -1, 1)):
        m.set_causal_chunks(*setting)
        with pytest.raises(ValueError, match="pin_sink"):
            m.forward_teacher_forcing(x, x, t, [torch.zeros(4, 64)], pin_sink=True)
        with pytest.raises(ValueError, match="pin_sink"):
            causal.forcing_loss(m, x, x, t, t, [torch.zeros(4, 64)], pin_sink=True)
    m.set_causal_chunks(1, 1, 1)
    with pytest.raises(ValueError, match="pin_sink"):                            # diffusion forcing has no clean sink to pin
        causal.forcing_loss(m, x, x, t, t, [torch.zeros(4, 64)], mode="diffusion", pin_sink=True)
    cache = causal.RollingKVCache(m, 1, TPF, 1, 1, "cpu", pin_sink=True)
    with pytest.raises(ValueError, match="self forcing under a pinned sink"):
        m.forward_chunk([torch.zeros(16, 1, 14, 16)], torch.zeros(1), [torch.zeros(4, 64)], cache, grad=True)


def test_header_and_binding():
    lib = importlib.import_module(PKG + "._lib")
    ops = importlib.import_module(PKG + ".ops")
    text = open(os.path.join(ROOT, "include", "omh.h")).read()
    for name in ("omh_rope_shift_table", "omh_rope_shift_fan", "omh_rope_shift_fold"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and name in lib.EXPORTED
    assert lib.ABI_VERSION == 12 and lib.lib.omh_abi_version() == 12
    assert int(re.search(r"#define\s+OMH_ROPE_SHIFT_MAX_PAIRS\s+(\d+)", text).group(1)) == ops.ROPE_SHIFT_MAX_PAIRS
    for name in ("rope_shift_table", "rope_shift_fan", "rope_shift_fold"):
        assert name in ops.__all__
    x = torch.zeros(1, 8, 128, dtype=torch.bfloat16)
    with pytest.raises(ops.OmhError):                                            # no CPU fallback
        ops.rope_shift_fan(x, x.new_zeros(1, 2, 8, 128), ops.rope_shift_table([1, 2]))
    with pytest.raises(ops.OmhError):
        ops.rope_shift_fold((x, x.new_zeros(1, 2, 8, 128)), None, None)
