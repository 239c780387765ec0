"""Chunk-causal attention, the part that needs no GPU: the rule as a dense mask (causal.chunk_causal_visible) against
loops, the argument checks of omh_flash_attn_fwd_chunk_d128 / omh_flash_attn_bwd_chunk_d128, the ValueErrors of the Python
layers, and the bookkeeping of causal.KVCache."""
import ctypes
import importlib

import pytest
import torch

from conftest import PKG


@pytest.fixture(scope="module")
def causal(omh):
    return importlib.import_module(PKG + ".causal")


def _loops(Lq, Lk, C, W, P, qlen, klen):
    qlen = Lq if qlen is None else min(max(qlen, 0), Lq)
    klen = Lk if klen is None else min(max(klen, 0), Lk)
    m = torch.zeros(Lq, Lk, dtype=torch.bool)
    for i in range(Lq):
        for j in range(Lk):
            ci, cj = (P + i) // C, j // C
            m[i, j] = i < qlen and j < klen and cj <= ci and (W < 0 or cj >= ci - W)
    return m


@pytest.mark.parametrize("Lq,Lk,C,W,P,qlen,klen", [
    (12, 12, 4, -1, 0, None, None),
    (12, 12, 5, 0, 0, None, None),
    (12, 12, 5, 1, 0, None, 11),            # klen inside a chunk
    (7, 19, 3, -1, 12, None, None),         # q_offset > 0
    (7, 19, 3, 1, 12, 5, 17),               # ... with a look-back, q_lens and klen inside a chunk
    (9, 20, 6, 0, 8, None, 13),             # rows whose own chunk starts past klen see nothing
    (5, 5, 1, 2, 0, None, None),
    (6, 9, 100, -1, 0, 4, 7),               # one chunk holds everything
])
def test_visible_against_loops(causal, Lq, Lk, C, W, P, qlen, klen):
    got = causal.chunk_causal_visible(Lq, Lk, C, W, P, qlen, klen)
    assert got.dtype == torch.bool and got.shape == (Lq, Lk) and got.device.type == "cpu"
    assert torch.equal(got, _loops(Lq, Lk, C, W, P, qlen, klen))
    # seen from the query: one interval of keys per row; seen from the key: one interval of rows per key
    ql = Lq if qlen is None else qlen
    kl = Lk if klen is None else klen
    for i in range(ql):
        I = (P + i) // C
        lo, hi = (0 if W < 0 else max(0, (I - W) * C)), min(kl, (I + 1) * C)
        assert got[i].nonzero().flatten().tolist() == list(range(lo, max(hi, lo)))
    for j in range(kl):
        J = j // C
        rows = [i for i in range(ql) if J * C <= P + i and (W < 0 or P + i < (J + W + 1) * C)]
        assert got[:, j].nonzero().flatten().tolist() == rows


def test_visible_special_cases(causal):
    L = 17
    i, j = torch.arange(L).view(L, 1), torch.arange(L).view(1, L)
    assert torch.equal(causal.chunk_causal_visible(L, L, 1), j <= i)                       # C = 1: token-causal
    assert torch.equal(causal.chunk_causal_visible(L, L, 1, 3), (j <= i) & (j >= i - 3))   # ... and the causal band
    for C in (L, L + 1, 1000):                                                           # C >= Lk, P = 0: all true up to klen
        vis = causal.chunk_causal_visible(9, L, C, -1, 0, None, 13)
        assert bool(vis[:, :13].all()) and not bool(vis[:, 13:].any())
    with pytest.raises(ValueError):
        causal.chunk_causal_visible(4, 4, 0)
    with pytest.raises(ValueError):
        causal.chunk_causal_visible(4, 4, 2, -1, -1)


def test_chunk_entries_validate_without_gpu(omh):
    """The two entries reject bad arguments before touching the device (fake, aligned pointers throughout)."""
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

    rule = binding.ChunkCausalArgs
    bad = -1                                                                     # OMH_E_BADARG
    fwd = lambda a, r: lib.omh_flash_attn_fwd_chunk_d128(by(a), None if r is None else by(r), None)
    bwd = lambda a, r: lib.omh_flash_attn_bwd_chunk_d128(by(a), None, None if r is None else by(r), None)
    assert lib.omh_flash_attn_fwd_chunk_d128(None, None, None) == bad
    assert lib.omh_flash_attn_bwd_chunk_d128(None, None, None, None) == bad
    assert lib.omh_flash_attn_fwd_chunk_d128(None, by(rule(64, -1, 0, 0)), None) == bad
    assert lib.omh_flash_attn_bwd_chunk_d128(None, None, by(rule(64, -1, 0, 0)), None) == bad
    for entry, args in ((fwd, fwd_args), (bwd, bwd_args)):
        assert entry(args(), None) == bad                                        # a null struct
        assert entry(args(), rule(0, -1, 0, 0)) == bad                           # chunk <= 0
        assert entry(args(), rule(-5, -1, 0, 0)) == bad
        assert entry(args(), rule(64, -1, -1, 0)) == bad                         # q_offset < 0
        assert entry(args(), rule(64, 1, 0, 7)) == bad                           # reserved != 0
        assert entry(args(), rule(64, -1, 2 ** 28, 0)) == -3                     # positions past the 32-bit arithmetic: OMH_E_SHAPE
    # a band beside the rule; (0, 0) is a zero-initialised struct and means "no band" here — it passes THIS check and is
    # stopped by the next one (q_lens' alignment, OMH_E_ALIGN), which tells the two apart without reaching a launch
    for wl, wr in ((16, 16), (-1, 0), (0, 5), (3, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr), rule(64, -1, 0, 0)) == bad
    for wl, wr in ((0, 0), (-1, -1)):
        assert fwd(fwd_args(window_left=wl, window_right=wr, q_lens=P + 2), rule(64, -1, 0, 0)) == -2
    # the backward needs the forward's fp32 output, as the varlen entry does; its q_lens is checked before any launch too
    assert bwd(bwd_args(o32=None), rule(64, -1, 0, 0)) == bad
    assert lib.omh_flash_attn_bwd_chunk_d128(by(bwd_args()), P + 2, by(rule(64, -1, 0, 0)), None) == -2
    assert bwd(bwd_args(phase=4, o_rs=256), rule(64, -1, 0, 0)) == bad
    assert lib.omh_abi_version() == 12


def test_python_refusals_without_gpu(omh):
    ops = importlib.import_module(PKG + ".ops")
    attn = importlib.import_module(PKG + ".wan.modules.attention")
    at = dict(H=2, Lq=256, Lk=256, device=torch.device("cpu"))
    assert ops.attn_mask((16, 16), chunk_causal=None, **at).kind == "band"
    cc = ops.attn_mask(chunk_causal=(1560, -3, 8), **at).rule
    assert (cc.chunk, cc.left_chunks, cc.q_offset, cc.reserved) == (1560, -1, 8, 0)
    with pytest.raises(ValueError):
        ops.attn_mask((16, -1), chunk_causal=(64, -1, 0), **at)
    with pytest.raises(ValueError):
        ops.attn_mask(chunk_causal=(64, -1, 0), block_mask=torch.ones(2, 2, dtype=torch.bool), **at)
    with pytest.raises(ValueError):
        ops.attn_mask(chunk_causal=(0, -1, 0), **at)
    with pytest.raises(ValueError):
        ops.attn_mask(chunk_causal=(64, -1, -1), **at)
    # the wrapper raises before it asks for a device
    q = torch.zeros(1, 256, 2, 128)
    mask = torch.ones(2, 2, dtype=torch.bool)
    for kw in (dict(causal=True), dict(window_size=(16, 16)), dict(window_size=(-1, 0)), dict(block_mask=mask)):
        with pytest.raises(ValueError):
            attn.flash_attention(q.cuda() if torch.cuda.is_available() else _FakeCuda(q), q, q, chunk_causal=(64, -1, 0), **kw)
    import inspect
    for fn in (attn.flash_attention, attn.attention, ops.flash_attn, ops.flash_attn_raw, ops.flash_attn_bwd, ops.flash_attn_func):
        assert "chunk_causal" in inspect.signature(fn).parameters


class _FakeCuda:
    """Stands in for a CUDA tensor in front of flash_attention's argument checks (which come before any device work)."""

    def __init__(self, t):
        self._t = t
        self.device = torch.device("cuda")
        self.shape, self.dtype, self.requires_grad = t.shape, t.dtype, False

    def size(self, i):
        return self._t.size(i)


def _tiny(wan_model_mod, **kw):
    return wan_model_mod.WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, text_len=8, freq_dim=64, **kw)


def test_set_causal_chunks_is_no_state_and_refuses(wan_model_mod):
    sparse = importlib.import_module(PKG + ".sparse")
    m = _tiny(wan_model_mod)
    before, config = {k: v.clone() for k, v in m.state_dict().items()}, dict(m.config)
    m.set_causal_chunks(3, 1)
    assert m._causal_chunks == (3, 1)
    assert m._causal_rule([(5, 7, 8), (3, 7, 8)]) == (3 * 56, 1, 0)             # C = frames x (h / p_h) x (w / p_w), q_offset 0
    m.set_causal_chunks(2)
    assert m._causal_rule([(5, 7, 8)]) == (112, -1, 0)
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before) and m.config == config
    with pytest.raises(ValueError):                                              # one C serves the call
        m._causal_rule([(5, 7, 8), (5, 8, 7)])
    with pytest.raises(ValueError):
        m.set_causal_chunks(0)
    m.set_causal_chunks(None)
    assert m._causal_chunks is None and m._causal_rule([(5, 7, 8), (5, 8, 7)]) is None
    with pytest.raises(ValueError):                                              # a windowed model
        _tiny(wan_model_mod, window_size=(70, 30)).set_causal_chunks(1)
    mask = torch.ones(3, 3, dtype=torch.bool)
    m.set_attention_block_mask(mask, layers=[1])
    with pytest.raises(ValueError):                                              # a layer with a block mask
        m.set_causal_chunks(1)
    m.set_attention_block_mask(None)
    m.set_attention_block_policy(sparse.DynamicBlockPolicy(0.9), layers=[0])
    with pytest.raises(ValueError):                                              # ... or a block policy
        m.set_causal_chunks(1)
    m.set_attention_block_policy(None)
    m.set_causal_chunks(1)
    m.set_attention_block_mask(mask)                                             # set afterwards: found at forward
    with pytest.raises(ValueError):
        m._causal_rule([(5, 7, 8)])


def test_kv_cache_bookkeeping(wan_model_mod, causal):
    m = _tiny(wan_model_mod)
    c = causal.KVCache(m, 2, 280, "cpu")
    assert len(c.k) == len(c.vt) == 2 and c.length == 0 and c.cap == 280 and c.pitch == 320
    assert c.k[0].shape == (2, 280, 256) and c.k[0].dtype == torch.bfloat16
    assert c.vt[1].shape == (2, 256, 320) and c.vt[1].dtype == torch.bfloat16 and float(c.vt[1].abs().sum()) == 0.0
    c.advance(112)
    c.advance(112)
    assert c.length == 224
    c.check_room(56)
    with pytest.raises(ValueError):                                              # running past cap
        c.check_room(57)
    with pytest.raises(ValueError):
        c.advance(64)
    assert c.length == 224
    c.truncate(112)
    assert c.length == 112
    with pytest.raises(ValueError):
        c.truncate(113)
    with pytest.raises(ValueError):
        c.truncate(-1)
    c.reset()
    assert c.length == 0
    with pytest.raises(ValueError):
        causal.KVCache(m, 0, 280, "cpu")
    ops = importlib.import_module(PKG + ".ops")
    if not torch.cuda.is_available():
        with pytest.raises(ops.OmhError):                                        # the "MI355X only" error comes first
            m.forward_chunk([torch.zeros(16, 1, 4, 4)], torch.tensor([1.]), [torch.zeros(3, 64)], c)


def test_library_exports_the_chunk_entries(omh):
    binding = importlib.import_module(PKG + "._lib")
    for name in ("omh_flash_attn_fwd_chunk_d128", "omh_flash_attn_bwd_chunk_d128"):
        assert name in binding.EXPORTED and hasattr(binding.lib, name)
    assert ctypes.sizeof(binding.ChunkCausalArgs) == 16
