"""Attention backward with q_lens: omh_flash_attn_bwd_varlen_d128 through ops.flash_attn_bwd(q_lens=, window=) after the
product forward with the same q_lens / window, against autograd through an fp32 masked softmax built per sample with
shift = klen - qlen (the formula of test_gpu_kernels.py's _band_ref).  dout rows past q_lens hold NaN in every call:
those rows do not exist and must not be read."""
import ctypes as C
import importlib

import pytest
import torch

from conftest import PKG, rel_rms

pytestmark = pytest.mark.gpu

CASES = [
    # B, H, Lq, Lk, q_lens, k_lens, window
    (2, 2, 200, 200, [200, 77], None, (-1, 0)),              # causal, one ragged sample, positive shift
    (2, 2, 300, 300, [300, 130], [288, 120], (40, 25)),      # both lens, negative and positive shift, band across tile edges
    (3, 1, 129, 64, [0, 129, 1], None, (-1, 0)),             # qlen 0 and 1, one row past a workgroup
    (1, 2, 333, 130, [260], None, (10, 5)),                  # klen < qlen: the first live rows see nothing
    (1, 2, 700, 700, [650], [690], (128, 128)),              # whole key tiles skipped on both sides
    (2, 2, 260, 260, [260, 100], None, (-1, -1)),            # full attention with q_lens through the new entry
]


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def _mask(Lq, Lk, qlen, klen, left, right):
    """[Lq, Lk] bool: query i < qlen sees key j < klen iff i + klen - qlen - left <= j <= i + klen - qlen + right."""
    i = torch.arange(Lq, device="cuda")[:, None]
    j = torch.arange(Lk, device="cuda")[None, :]
    ok = (i < qlen) & (j < klen)
    s = i + (klen - qlen)
    if left >= 0:
        ok = ok & (j >= s - left)
    if right >= 0:
        ok = ok & (j <= s + right)
    return ok


class _Problem:
    """Inputs, the product forward and the fp32 reference of one case — built once, shared by the tests, never modified."""

    def __init__(self, ops, B, H, Lq, Lk, qlens, klens, window, seed):
        self.shape = (B, H, Lq, Lk)
        self.window = window
        d = H * 128
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.q = torch.randn(B * Lq, d, device="cuda", generator=g).bfloat16()
        self.k = torch.randn(B * Lk, d, device="cuda", generator=g).bfloat16()
        self.v = torch.randn(B * Lk, d, device="cuda", generator=g).bfloat16()
        do = torch.randn(B * Lq, d, device="cuda", generator=g).bfloat16()
        self.ql = None if qlens is None else torch.tensor(qlens, dtype=torch.int32, device="cuda")
        self.kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device="cuda")
        qlens = [Lq] * B if qlens is None else qlens
        klens = [Lk] * B if klens is None else klens
        self.masks = torch.stack([_mask(Lq, Lk, qlens[b], klens[b], *window) for b in range(B)])       # [B, Lq, Lk]
        past = (torch.arange(Lq, device="cuda")[None, :] >= torch.tensor(qlens, device="cuda")[:, None]).reshape(B * Lq)
        self.do = do.clone()
        self.do[past] = float("nan")                                  # what the product sees
        do_ref = do.clone()
        do_ref[past] = 0
        # the product forward: o, lse, fp32 o
        Lp = (Lk + 63) // 64 * 64
        vt = torch.zeros(B, d, Lp, device="cuda", dtype=torch.bfloat16)
        vt[:, :, :Lk] = self.v.view(B, Lk, d).transpose(1, 2)
        self.o = torch.empty(B * Lq, d, device="cuda", dtype=torch.bfloat16)
        self.o32 = torch.empty(B * Lq, d, device="cuda", dtype=torch.float32)
        self.lse = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
        ops.flash_attn_raw(ops.ptr(self.q), ops.ptr(self.k), ops.ptr(vt), ops.ptr(self.o),
                           ops.ptr(self.kl) if self.kl is not None else None, B, H, Lq, Lk, Lq * d, d, Lk * d, d, d * Lp,
                           Lq * d, d, Lp, 128 ** -0.5, lse=ops.ptr(self.lse), o32=ops.ptr(self.o32),
                           q_lens=ops.ptr(self.ql) if self.ql is not None else None, window=window)
        # autograd through the masked fp32 softmax on the same bf16 inputs
        qr, kr, vr = (t.float().view(B, -1, H, 128).transpose(1, 2).detach().requires_grad_(True)
                      for t in (self.q, self.k, self.v))
        s = torch.einsum("bhid,bhjd->bhij", qr, kr) * 128 ** -0.5
        s = s.masked_fill(~self.masks[:, None], float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)      # rows past q_lens / rows whose band is empty
        out = torch.einsum("bhij,bhjd->bhid", p, vr)
        out.backward(do_ref.float().view(B, Lq, H, 128).transpose(1, 2))
        self.ref = [t.grad.transpose(1, 2).reshape(B * L, d) for t, L in ((qr, Lq), (kr, Lk), (vr, Lk))]

    def bwd(self, ops, q_lens="own", **kw):
        B, H, Lq, Lk = self.shape
        ql = self.ql if isinstance(q_lens, str) else q_lens
        return ops.flash_attn_bwd(self.q, self.k, self.v, self.o, self.do, self.lse, self.kl, B, H, Lq, Lk, o32=self.o32,
                                  window=self.window, q_lens=ql, **kw)


_problems = {}


def _problem(ops, idx, qlens="case"):
    key = (idx, None if qlens is None else "case")
    if key not in _problems:
        B, H, Lq, Lk, ql, kl, window = CASES[idx]
        _problems[key] = _Problem(ops, B, H, Lq, Lk, ql if qlens == "case" else None, kl, window, 100 + idx)
    return _problems[key]


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_varlen_backward_matches_autograd(ops, idx):
    pr = _problem(ops, idx)
    B, H, Lq, Lk = pr.shape
    qlens = CASES[idx][4]
    # a case cannot pass by being all zeros: every sample but a deliberate qlen = 0 has a live row with a non-empty band
    for b in range(B):
        assert bool(pr.masks[b].any()) == (qlens[b] != 0)
    dq, dk, dv = pr.bwd(ops)
    for name, got, ref in (("dq", dq, pr.ref[0]), ("dk", dk, pr.ref[1]), ("dv", dv, pr.ref[2])):
        assert torch.isfinite(got).all(), name
        err = rel_rms(got, ref)
        print(f"case {idx} {name}: rel_rms {err:.3e}")
        assert err < 1.2e-2, name
    # rows past q_lens / rows with an empty band, and keys no live query reaches: exactly zero, written
    dead_q = ~pr.masks.any(2).reshape(B * Lq)
    dead_k = ~pr.masks.any(1).reshape(B * Lk)
    assert float(dq[dead_q].abs().sum()) == 0.0
    assert float(dk[dead_k].abs().sum()) == 0.0 and float(dv[dead_k].abs().sum()) == 0.0
    # no atomics: repeatable bit for bit
    dq2, dk2, dv2 = pr.bwd(ops)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)


def _entry_direct(ops, pr, q_lens):
    """omh_flash_attn_bwd_varlen_d128 itself (ops.flash_attn_bwd takes the band entry when q_lens is None)."""
    binding = importlib.import_module(PKG + "._lib")
    B, H, Lq, Lk = pr.shape
    d = H * 128
    delta = torch.empty(B, H, Lq, device="cuda", dtype=torch.float32)
    outs = [torch.empty(B * L, d, device="cuda", dtype=torch.float32) for L in (Lq, Lk, Lk)]
    a = binding.AttnBwdArgs()
    for name, t in (("q", pr.q), ("k", pr.k), ("v", pr.v), ("o", pr.o), ("dout", pr.do), ("lse", pr.lse), ("delta", delta),
                    ("dq", outs[0]), ("dk", outs[1]), ("dv", outs[2]), ("k_lens", pr.kl), ("o32", pr.o32)):
        setattr(a, name, None if t is None else C.c_void_p(t.data_ptr()))
    a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
    a.q_rs = a.k_rs = a.o_rs = a.dq_rs = a.dk_rs = d
    a.q_bs = a.o_bs = a.dq_bs = Lq * d
    a.k_bs = a.dk_bs = Lk * d
    a.scale = 128 ** -0.5
    rc = binding.lib.omh_flash_attn_bwd_varlen_d128(C.byref(a), None if q_lens is None else C.c_void_p(q_lens.data_ptr()),
                                                    pr.window[0], pr.window[1],
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("idx", [1, 4])
def test_without_q_lens_is_the_band_entry(ops, idx):
    """q_lens = NULL through the new entry, and a q_lens that holds Lq everywhere, give omh_flash_attn_bwd_band_d128's bits."""
    pr = _problem(ops, idx, qlens=None)                               # the case's k_lens and window, every row live
    B, H, Lq, Lk = pr.shape
    band = pr.bwd(ops, q_lens=None)                                   # a bounded window, no q_lens: the band entry
    null = _entry_direct(ops, pr, None)
    full = pr.bwd(ops, q_lens=torch.full((B,), Lq, dtype=torch.int32, device="cuda"))
    for x, y, z in zip(band, null, full):
        assert torch.equal(x, y) and torch.equal(x, z)
    for got, ref in zip(band, pr.ref):
        assert rel_rms(got, ref) < 1.2e-2


def test_varlen_backward_phases_and_bf16(ops):
    """Phases 1 + 2 + 3 give phase 0's bits; bf16 out= is within 8e-3 of the fp32 result (case 2)."""
    pr = _problem(ops, 1)
    B, H, Lq, Lk = pr.shape
    d = H * 128
    f32 = pr.bwd(ops)
    ref0 = tuple(torch.empty(B * L, d, device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    pr.bwd(ops, out=ref0)
    for got, ref in zip(ref0, f32):
        assert rel_rms(got.float(), ref) < 8e-3
    delta = torch.full((B, H, Lq), float("nan"), device="cuda", dtype=torch.float32)
    pr.bwd(ops, phase=1, delta=delta)
    assert torch.isfinite(delta).all()                                # rows past q_lens: written, as zero
    ph = tuple(torch.full((B * L, d), float("nan"), device="cuda", dtype=torch.bfloat16) for L in (Lq, Lk, Lk))
    pr.bwd(ops, phase=3, delta=delta, out=ph)
    pr.bwd(ops, phase=2, delta=delta, out=ph)
    for a, b in zip(ph, ref0):
        assert torch.equal(a, b)
    # fp32 phases as well
    dq, _, _ = pr.bwd(ops, phase=2, delta=delta)
    _, dk, dv = pr.bwd(ops, phase=3, delta=delta)
    assert torch.equal(dq, f32[0]) and torch.equal(dk, f32[1]) and torch.equal(dv, f32[2])


def test_q_lens_needs_o32(ops):
    pr = _problem(ops, 0)
    B, H, Lq, Lk = pr.shape
    with pytest.raises(AssertionError):
        ops.flash_attn_bwd(pr.q, pr.k, pr.v, pr.o, pr.do, pr.lse, pr.kl, B, H, Lq, Lk, q_lens=pr.ql)
