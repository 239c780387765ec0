"""Block masks on the host: the tables of ``sparse.BlockMask``, ``block_mask_from_3d_window`` against the element rule,
the argument rules of the sparse C entries (rejected before the device is touched) and
``WanModel.set_attention_block_mask`` as far as it goes without a GPU."""
import ctypes
import importlib

import pytest
import torch

from conftest import PKG


@pytest.fixture(scope="module")
def sparse(omh):
    return importlib.import_module(PKG + ".sparse")


@pytest.mark.parametrize("shape,Lq,Lk", [((3, 5), 300, 520), ((2, 4, 4), 512, 400 + 100)])
def test_block_mask_tables_against_brute_force(sparse, shape, Lq, Lk):
    g = torch.Generator().manual_seed(sum(shape))
    mask = torch.rand(*shape, generator=g) < 0.5
    bm = sparse.BlockMask(mask, Lq, Lk)
    m3 = mask if mask.dim() == 3 else mask[None]
    H, nq, nk = m3.shape
    assert (bm.heads, bm.q_blocks, bm.k_blocks) == (H, nq, nk)
    assert bm.row_cnt.shape == (H, nq) and bm.row_idx.shape == (H, nq, nk)
    assert bm.col_cnt.shape == (H, nk) and bm.col_idx.shape == (H, nk, nq)
    for t in (bm.row_cnt, bm.row_idx, bm.col_cnt, bm.col_idx):
        assert t.dtype == torch.int32 and t.is_contiguous()
    pairs_rows, pairs_cols = set(), set()
    for h in range(H):
        for i in range(nq):
            want = [j for j in range(nk) if m3[h, i, j]]
            assert int(bm.row_cnt[h, i]) == len(want)
            assert bm.row_idx[h, i, :len(want)].tolist() == want                  # ascending, exactly the kept blocks
            pairs_rows.update((h, i, j) for j in want)
        for j in range(nk):
            want = [i for i in range(nq) if m3[h, i, j]]                          # the brute-force transpose
            assert int(bm.col_cnt[h, j]) == len(want)
            assert bm.col_idx[h, j, :len(want)].tolist() == want
            pairs_cols.update((h, i, j) for i in want)
    assert pairs_rows == pairs_cols                                              # both describe the same set
    assert bm.density == pytest.approx(len(pairs_rows) / (H * nq * nk))


def test_block_mask_validation(sparse):
    ok = torch.ones(3, 3, dtype=torch.bool)
    sparse.BlockMask(ok, 320, 320)
    with pytest.raises(ValueError):
        sparse.BlockMask(ok.float(), 320, 320)                                   # dtype
    with pytest.raises(ValueError):
        sparse.BlockMask(ok, 320, 400)                                           # 4 key blocks needed
    with pytest.raises(ValueError):
        sparse.BlockMask(ok[0], 320, 320)                                        # rank
    with pytest.raises(ValueError):
        sparse.BlockMask(ok, 0, 320)


def _element_rule(grid, window, seq_len, block):
    """Brute force: (allowed [n, n] element pairs, the block mask the definition gives)."""
    F, H, W = grid
    n = F * H * W
    idx = torch.arange(n)
    f, h, w = idx // (H * W), (idx // W) % H, idx % W
    ok = ((f[:, None] - f[None]).abs() <= window[0]) & ((h[:, None] - h[None]).abs() <= window[1]) & \
         ((w[:, None] - w[None]).abs() <= window[2])
    nb = (seq_len + block - 1) // block
    want = torch.zeros(nb, nb, dtype=torch.bool)
    for I in range(nb):
        for J in range(nb):
            a, b = slice(I * block, min((I + 1) * block, n)), slice(J * block, min((J + 1) * block, n))
            if I * block >= n or J * block >= n:
                want[I, J] = I == J and I * block >= n                            # wholly padding: itself only
            else:
                want[I, J] = bool(ok[a, b].any())
    return ok, want


@pytest.mark.parametrize("grid,window,seq_len", [((3, 6, 10), (1, 2, 3), 256), ((1, 30, 52), (0, 6, 52), None),
                                                 ((1, 30, 52), (0, 30, 52), None)])
def test_3d_window_mask_against_the_element_rule(sparse, grid, window, seq_len):
    n = grid[0] * grid[1] * grid[2]
    S = n if seq_len is None else seq_len
    got = sparse.block_mask_from_3d_window(grid, window, seq_len=seq_len, block=128)
    ok, want = _element_rule(grid, window, S, 128)
    assert got.dtype == torch.bool and got.shape == want.shape
    assert torch.equal(got, want)
    # the cover property: every element pair the window allows lies in a kept block
    dense = got.repeat_interleave(128, 0).repeat_interleave(128, 1)[:n, :n]
    assert bool(dense[ok].all())
    if window == (0, 30, 52):                                                    # the window spans the frame: all-true
        live = (n + 127) // 128
        assert bool(got[:live, :live].all())


def test_3d_window_mask_validation(sparse):
    with pytest.raises(ValueError):
        sparse.block_mask_from_3d_window((2, 4, 4), (1, 1, 1), seq_len=16)       # shorter than the grid
    with pytest.raises(ValueError):
        sparse.block_mask_from_3d_window((2, 4, 4), (1, -1, 1))


def test_sparse_entries_validate_without_gpu(omh):
    """The sparse entries reject bad arguments before touching the device (fake, aligned pointers throughout)."""
    binding = importlib.import_module(PKG + "._lib")
    lib, by = binding.lib, ctypes.byref
    P = 4096

    def fwd_args(**kw):
        a = binding.AttnArgs(P, P, P, P, None, 1, 2, 256, 384, 0, 256, 0, 256, 0, 0, 256, 384, 0.1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def bwd_args():
        a = binding.AttnBwdArgs()
        for name in ("q", "k", "v", "dout", "lse", "delta", "dq", "dk", "dv", "o32"):
            setattr(a, name, P)
        a.B, a.H, a.Lq, a.Lk = 1, 2, 256, 384
        for name in ("q_rs", "k_rs", "o_rs", "dq_rs", "dk_rs"):
            setattr(a, name, 256)
        return a

    def mask(heads=2, qb=2, kb=3, **kw):
        m = binding.BlockMaskArgs(heads, qb, kb, P, P, P, P)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    bad = -1                                                                     # OMH_E_BADARG
    # a NULL mask is the plain entry: its own validation answers
    assert lib.omh_flash_attn_fwd_sparse_d128(None, None, None) == lib.omh_flash_attn_fwd_d128(None, None) == bad
    assert lib.omh_flash_attn_bwd_sparse_d128(None, None, None, None) == bad
    empty = binding.AttnArgs()
    assert lib.omh_flash_attn_fwd_sparse_d128(by(empty), None, None) == lib.omh_flash_attn_fwd_d128(by(empty), None) == bad
    for entry, args in ((lambda a, m: lib.omh_flash_attn_fwd_sparse_d128(by(a), by(m), None), fwd_args),
                        (lambda a, m: lib.omh_flash_attn_bwd_sparse_d128(by(a), None, by(m), None), bwd_args)):
        assert entry(args(), mask(heads=3)) == bad                               # heads not in {1, H}
        assert entry(args(), mask(heads=0)) == bad
        assert entry(args(), mask(qb=3)) == bad                                  # block counts that do not match Lq / Lk
        assert entry(args(), mask(kb=2)) == bad
        for table in ("row_cnt", "row_idx", "col_cnt", "col_idx"):
            assert entry(args(), mask(**{table: None})) == bad                   # null tables
    # a band beside the mask; (0, 0) is a zero-initialised struct and means "no band" here — it passes THIS check and is
    # stopped by the next one (the tables' alignment, OMH_E_ALIGN), which tells the two apart without reaching a launch
    for wl, wr in ((16, 16), (-1, 0), (0, 5), (3, -1)):
        assert lib.omh_flash_attn_fwd_sparse_d128(by(fwd_args(window_left=wl, window_right=wr)), by(mask()), None) == bad
    unaligned = mask(row_cnt=P + 2)
    assert lib.omh_flash_attn_fwd_sparse_d128(by(fwd_args(window_left=0, window_right=0)), by(unaligned), None) == -2
    assert lib.omh_flash_attn_fwd_sparse_d128(by(fwd_args()), by(unaligned), None) == -2
    assert lib.omh_flash_attn_bwd_sparse_d128(by(bwd_args()), None, by(unaligned), None) == -2
    # the backward needs the forward's fp32 output, as the varlen entry does
    a = bwd_args()
    a.o32 = None
    assert lib.omh_flash_attn_bwd_sparse_d128(by(a), None, by(mask()), None) == bad
    assert lib.omh_abi_version() == 12


def test_python_refusals_without_gpu(omh, sparse):
    ops = importlib.import_module(PKG + ".ops")
    attn = importlib.import_module(PKG + ".wan.modules.attention")
    cpu = torch.device("cpu")
    with pytest.raises(ValueError):
        ops.attn_mask((16, 16), torch.ones(2, 2, dtype=torch.bool), H=2, Lq=256, Lk=256, device=cpu)
    with pytest.raises(ValueError):
        ops.attn_mask(block_mask=torch.ones(3, 2, 2, dtype=torch.bool), H=2, Lq=256, Lk=256, device=cpu)
    with pytest.raises(ValueError):
        ops.attn_mask(block_mask=sparse.BlockMask(torch.ones(2, 2, dtype=torch.bool), 256, 256), H=2, Lq=256, Lk=400, device=cpu)
    assert ops.attn_mask((16, 16), None, H=2, Lq=256, Lk=256, device=cpu).kind == "band"
    import inspect
    for fn in (attn.flash_attention, attn.attention):                            # a trailing keyword after the reference's own
        assert list(inspect.signature(fn).parameters)[-1] == "block_mask"


def _tiny(wan_model_mod, **kw):
    return wan_model_mod.WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, text_len=8, freq_dim=64, **kw)


def test_model_mask_is_no_state(wan_model_mod, sparse):
    m = _tiny(wan_model_mod)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    config = dict(m.config)
    names = [n for n, _ in m.named_buffers()] + [n for n, _ in m.named_parameters()]
    mask = torch.ones(2, 3, 3, dtype=torch.bool)
    m.set_attention_block_mask(mask, layers=[1])
    assert m.blocks[0].self_attn._block_mask is None and m.blocks[0].cross_attn._block_mask is None
    bm = m.blocks[1].self_attn._block_mask
    assert isinstance(bm, sparse.BlockMask) and (bm.heads, bm.q_blocks) == (2, 3)
    assert m.blocks[1].cross_attn._block_mask is None                            # cross-attention is never masked
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert m.config == config
    assert names == [n for n, _ in m.named_buffers()] + [n for n, _ in m.named_parameters()]
    m.set_attention_block_mask(sparse.BlockMask(mask[0], 384, 384))              # a BlockMask, all layers
    assert all(b.self_attn._block_mask is not None for b in m.blocks)
    m.set_attention_block_mask(None)
    assert all(b.self_attn._block_mask is None for b in m.blocks)


def test_model_mask_refusals(wan_model_mod, sparse):
    mask = torch.ones(3, 3, dtype=torch.bool)
    with pytest.raises(ValueError):
        _tiny(wan_model_mod, window_size=(70, 30)).set_attention_block_mask(mask)    # a windowed model
    m = _tiny(wan_model_mod)
    with pytest.raises(ValueError):
        m.set_attention_block_mask(torch.ones(3, 3, 3, dtype=torch.bool))        # 3 heads on a 2-head model
    with pytest.raises(ValueError):
        m.set_attention_block_mask(torch.ones(3, 4, dtype=torch.bool))           # not square
    with pytest.raises(ValueError):
        m.set_attention_block_mask(mask.float())
    with pytest.raises(ValueError):
        m.set_attention_block_mask(mask, layers=[2])
    # the wrong nb is found at forward; without a GPU the layer's own check is what can be reached
    m.set_attention_block_mask(mask)
    sa = m.blocks[0].self_attn
    def mask_for(S):
        fc = wan_model_mod._FwdCtx()
        fc.S = S
        return sa._call_mask(fc, torch.device("cpu")).rule
    assert mask_for(320) is sa._block_mask and mask_for(384) is sa._block_mask
    for S in (256, 385, 1560):
        with pytest.raises(ValueError):
            mask_for(S)
    ops = importlib.import_module(PKG + ".ops")
    if not torch.cuda.is_available():
        with pytest.raises(ops.OmhError):                                        # the existing "MI355X only" error comes first
            m([torch.zeros(16, 1, 4, 4)], torch.tensor([1.]), [torch.zeros(3, 64)], 4)
