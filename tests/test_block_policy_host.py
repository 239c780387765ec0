"""CPU: sparse.DynamicBlockPolicy, WanModel.set_attention_block_policy, the lazy BlockMask.density, the argument checks of
the three block-selection entries, and the selection rule's torch restatement (tests/dyn_mask_ref.py) in fp32 against fp64
on the structured operands the GPU tests use."""
import ctypes
import importlib

import pytest
import torch

import dyn_mask_ref as R
from conftest import PKG

CASES, UNDECIDED_CAP, case_operands = R.CASES, R.UNDECIDED_CAP, R.case_operands


@pytest.fixture(scope="module")
def sparse(omh):
    return importlib.import_module(PKG + ".sparse")


def test_policy_validation(sparse):
    P = sparse.DynamicBlockPolicy
    p = P(0.9)
    assert (p.mass, p.min_coherence, p.keep_diagonal, p.always) == (0.9, 0.0, True, None)
    assert P(1).mass == 1.0 and P(0.5, min_coherence=1).min_coherence == 1.0
    for bad in (0.0, -0.1, 1.0001, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError):
            P(bad)
    for bad in (-0.01, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError):
            P(0.5, min_coherence=bad)
    for bad in (torch.ones(3, 3), torch.ones(3, dtype=torch.bool), torch.ones(1, 2, 3, 3, dtype=torch.bool), [[True]],
                torch.zeros(0, 3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            P(0.5, always=bad)
    a = torch.zeros(2, 3, 3, dtype=torch.bool)
    a[1, 0, 2] = True
    p = P(0.5, always=a)
    p.check_blocks(3, 3, 2)
    for nq, nk, h in ((3, 4, 2), (4, 3, 2), (3, 3, 4)):
        with pytest.raises(ValueError):
            p.check_blocks(nq, nk, h)
    # always on a device: uint8, the diagonal of a square call OR-ed in, remembered per device and shape
    u = p.always_on(torch.device("cpu"), 3, 3, 2)
    assert u.dtype == torch.uint8 and u.shape == (2, 3, 3)
    assert torch.equal(u.bool(), a | torch.eye(3, dtype=torch.bool)[None]) and p.always_on(torch.device("cpu"), 3, 3, 2) is u
    assert torch.equal(P(0.5, always=a, keep_diagonal=False).always_on(torch.device("cpu"), 3, 3, 2).bool(), a)
    assert torch.equal(P(0.5).always_on(torch.device("cpu"), 2, 2, 4).bool(), torch.eye(2, dtype=torch.bool)[None])
    assert P(0.5).always_on(torch.device("cpu"), 2, 3, 4) is None                 # rectangular: no diagonal
    assert P(0.5, keep_diagonal=False).always_on(torch.device("cpu"), 2, 2, 4) is None
    ops = importlib.import_module(PKG + ".ops")
    with pytest.raises(ops.OmhError):                                            # no CPU fallback
        sparse.block_mask_from_qk(torch.zeros(1, 4, 2, 128, dtype=torch.bfloat16), torch.zeros(1, 4, 2, 128, dtype=torch.bfloat16), P(0.5))


def _tiny(wan_model_mod, **kw):
    return wan_model_mod.WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, text_len=8, freq_dim=64, **kw)


def test_model_policy_setter(wan_model_mod, sparse):
    pol = sparse.DynamicBlockPolicy(0.9)
    m = _tiny(wan_model_mod)
    before = list(m.state_dict())
    names = [n for n, _ in m.named_buffers()] + [n for n, _ in m.named_parameters()]
    config = dict(m.config)
    m.set_attention_block_policy(pol, layers=[1])
    assert m.blocks[0].self_attn._block_policy is None and m.blocks[1].self_attn._block_policy is pol
    assert all(b.cross_attn._block_policy is None for b in m.blocks)             # cross-attention never takes it
    m.set_attention_block_policy(pol)
    assert all(b.self_attn._block_policy is pol for b in m.blocks)
    assert list(m.state_dict()) == before and m.config == config                  # no state
    assert names == [n for n, _ in m.named_buffers()] + [n for n, _ in m.named_parameters()]
    # a static mask beside a policy is refused, both ways round
    with pytest.raises(ValueError):
        m.set_attention_block_mask(torch.ones(3, 3, dtype=torch.bool))
    m.set_attention_block_policy(None)
    assert all(b.self_attn._block_policy is None and b.self_attn.last_block_mask is None for b in m.blocks)
    m.set_attention_block_mask(torch.ones(3, 3, dtype=torch.bool), layers=[0])
    with pytest.raises(ValueError):
        m.set_attention_block_policy(pol)
    with pytest.raises(ValueError):
        m.set_attention_block_policy(pol, layers=[0])
    m.set_attention_block_policy(pol, layers=[1])                                # the other layer is free
    m.set_attention_block_mask(None)
    with pytest.raises(ValueError):
        m.set_attention_block_policy(pol, layers=[2])
    with pytest.raises(ValueError):
        m.set_attention_block_policy(torch.ones(3, 3, dtype=torch.bool))         # a mask is not a policy
    with pytest.raises(ValueError):
        _tiny(wan_model_mod, window_size=(70, 30)).set_attention_block_policy(pol)
    with pytest.raises(ValueError):                                              # always: square, 1 or num_heads heads
        m.set_attention_block_policy(sparse.DynamicBlockPolicy(0.5, always=torch.ones(3, 4, dtype=torch.bool)))
    with pytest.raises(ValueError):
        m.set_attention_block_policy(sparse.DynamicBlockPolicy(0.5, always=torch.ones(3, 3, 3, dtype=torch.bool)))
    # an always whose block count does not fit seq_len: ValueError where the call's seq_len is known
    fits3 = sparse.DynamicBlockPolicy(0.5, always=torch.ones(3, 3, dtype=torch.bool))
    m.set_attention_block_policy(fits3)
    fits3.check_blocks(3, 3, 2)
    with pytest.raises(ValueError):
        fits3.check_blocks(4, 4, 2)


def test_block_mask_from_bool_is_unchanged(sparse):
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(3, 5, 7, generator=g) < 0.4
    mask[1, 2] = False
    mask[:, :, 3] = False
    bm = sparse.BlockMask(mask, 5 * 128 - 3, 7 * 128)
    rc, ri = sparse._lists(mask)
    cc, ci = sparse._lists(mask.transpose(1, 2))
    assert torch.equal(bm.row_cnt, rc) and torch.equal(bm.row_idx, ri) and torch.equal(bm.col_cnt, cc) and torch.equal(bm.col_idx, ci)
    assert bm.density == float(mask.float().mean()) and isinstance(bm.density, float)
    assert bm.to("cpu") is bm
    # from_tables takes what it is given and checks only shapes and dtypes
    ft = sparse.BlockMask.from_tables(mask, rc, ri, cc, ci, 5 * 128 - 3, 7 * 128)
    assert (ft.heads, ft.q_blocks, ft.k_blocks, ft.Lq, ft.Lk) == (3, 5, 7, 5 * 128 - 3, 7 * 128)
    assert ft.row_idx is ri and ft.density == bm.density
    c = ft.c_struct()
    assert (c.heads, c.q_blocks, c.k_blocks, c.col_idx) == (3, 5, 7, ci.data_ptr())
    with pytest.raises(ValueError):
        sparse.BlockMask.from_tables(mask, rc, ri, cc, ci.long(), 5 * 128 - 3, 7 * 128)
    with pytest.raises(ValueError):
        sparse.BlockMask.from_tables(mask, rc, ri, cc, ci, 5 * 128 + 1, 7 * 128)
    with pytest.raises(ValueError):
        sparse.BlockMask.from_tables(mask.to(torch.uint8), rc, ri, cc, ci, 5 * 128, 7 * 128)


def test_selection_entries_validate_without_gpu(omh):
    """The three entries reject bad pointers and sizes before touching the device (fake, aligned pointers throughout)."""
    b = importlib.import_module(PKG + "._lib")
    lib, by = b.lib, ctypes.byref
    P = 4096
    bad, align, shape = -1, -2, -3

    def pool_op(**kw):
        ops = (b.BlockPoolOperand * 2)()
        for i in range(2):
            ops[i] = b.BlockPoolOperand(P, 256, 300, 0, None, P, P)
        for key, v in kw.items():
            setattr(ops[0], key, v)
        return ops
    assert lib.omh_block_pool_d128(None, 1, 1, 2, None) == bad
    for n_ops, B, H in ((0, 1, 2), (3, 1, 2), (1, 0, 2), (1, 1, 0)):
        assert lib.omh_block_pool_d128(pool_op(), n_ops, B, H, None) == bad
    for key in ("x", "mean", "coh"):
        assert lib.omh_block_pool_d128(pool_op(**{key: None}), 1, 1, 2, None) == bad
    assert lib.omh_block_pool_d128(pool_op(L=0), 1, 1, 2, None) == bad
    assert lib.omh_block_pool_d128(pool_op(ld=128), 1, 1, 2, None) == bad       # two heads need 256 columns
    assert lib.omh_block_pool_d128(pool_op(x=P + 8), 1, 1, 2, None) == align
    assert lib.omh_block_pool_d128(pool_op(ld=260), 1, 1, 2, None) == align
    assert lib.omh_block_pool_d128(pool_op(lens=P + 2), 1, 1, 2, None) == align
    second = pool_op()
    second[1].mean = None
    assert lib.omh_block_pool_d128(second, 2, 1, 2, None) == bad

    def sel(**kw):
        a = b.BlockSelectArgs(P, P, P, P, None, None, None, P, 1, 2, 300, 520, 1, 0.1, 0.9, 0.0)
        for key, v in kw.items():
            setattr(a, key, v)
        return a
    assert lib.omh_block_select(None, None) == bad
    for key in ("q_mean", "q_coh", "k_mean", "k_coh", "mask"):
        assert lib.omh_block_select(by(sel(**{key: None})), None) == bad
    for kw in (dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=-1), dict(mass=0.0), dict(mass=1.5), dict(mass=float("nan")),
               dict(min_coherence=-0.1), dict(min_coherence=1.1), dict(always=P, always_heads=3)):
        assert lib.omh_block_select(by(sel(**kw)), None) == bad, kw
    assert lib.omh_block_select(by(sel(Lk=1024 * 128 + 1)), None) == shape      # more than 1024 key blocks
    assert lib.omh_block_select(by(sel(k_mean=P + 4)), None) == align
    assert lib.omh_block_select(by(sel(k_lens=P + 1)), None) == align

    tab = [P, 2, 3, 5, P, P, P, P, None]
    assert lib.omh_block_mask_tables(None, 2, 3, 5, P, P, P, P, None) == bad
    for i in (4, 5, 6, 7):
        args = list(tab)
        args[i] = None
        assert lib.omh_block_mask_tables(*args) == bad
        args[i] = P + 2
        assert lib.omh_block_mask_tables(*args) == align
    for i in (1, 2, 3):
        args = list(tab)
        args[i] = 0
        assert lib.omh_block_mask_tables(*args) == bad
    assert lib.omh_abi_version() == 12


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_restatement_against_fp64(name):
    """The CPU check behind the GPU equality test, on the seeds it uses: with these operands at most 2 % of the live rows
    are undecided at delta = 1e-4, and the fp32 restatement of the rule picks the fp64 set on every decided row."""
    q, k, lens, masses = case_operands(name)
    B = q.shape[0]
    for mass in masses:
        keep64, p64, dec64, _, _ = R.select(q, k, mass, lens, lens, dtype=torch.float64)
        keep32, _, _, _, _ = R.select(q, k, mass, lens, lens, dtype=torch.float32)
        live = (R.live_counts(q.shape[1], lens, B) > 0)[:, None, :].expand_as(dec64)
        undecided, n_live = int((~dec64 & live).sum()), int(live.sum())
        print(f"{name} mass {mass}: {undecided} of {n_live} live rows undecided, density {float(keep64.float().mean()):.4f}")
        assert undecided <= UNDECIDED_CAP * n_live
        assert not ((keep64 != keep32).any(-1) & dec64).any()
        held = (p64 * keep32.to(torch.float64)).sum(-1)                          # undecided rows: the mass is still held
        assert bool((held[live] >= mass - R.DELTA).all())
        assert not keep64[~live].any()                                           # dead rows keep nothing by themselves
