"""The schedules of the long-sequence attention stream (csrc/gen_attn_w64.py, option W64_SCHED) on the host: schedule 1 is a
re-ordering of schedule 0 — the same instructions with the same operands, every register written and read by the same
arithmetic instructions in the same order — and schedule 0 is, line for line, what the generator emitted before the
schedules existed (digests under tests/golden/)."""
import collections
import hashlib
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "omnihuman-1-hack_amd", "csrc", "gen_attn_w64.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_w64_sched0_sha256.json")
VARIANTS = (2, 3, 4)


@pytest.fixture(scope="module")
def streams():
    spec = importlib.util.spec_from_file_location("gen_attn_w64_under_test", GEN)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return {(v, s): gen.generate(v, s).lines for v in VARIANTS for s in (0, 1)}, gen


def _norm(lines, v):
    """Drop assembler directives (the labels are the same in both schedules: they end in %=)."""
    return [ln for ln in lines if not ln.startswith(".p2align")]


def _sections(lines):
    """prologue (up to the loop label), the two loop bodies, the two `last` blocks, the epilogue."""
    idx = {name: next(i for i, ln in enumerate(lines) if re.match(rf"\.Lw64v\w+_{name}_%=:", ln))
           for name in ("loop", "last0", "last1", "epi")}
    body = lines[idx["loop"]:idx["last0"]]
    cut = [i for i, ln in enumerate(body) if ln.startswith("s_add_u32 s94, s94, 1")]
    assert len(cut) == 2
    return {"prologue": lines[:idx["loop"]], "body0": body[:cut[0] + 1], "body1": body[cut[0] + 1:],
            "last0": lines[idx["last0"]:idx["last1"]], "last1": lines[idx["last1"]:idx["epi"]], "epilogue": lines[idx["epi"]:]}


def _regs(tok):
    m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", tok)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    return [tok] if re.fullmatch(r"[va]\d+", tok) else []


def _arith(ln, gen):
    """(dst registers, source registers) of an arithmetic instruction, None for the others."""
    op, _, rest = ln.partition(" ")
    toks = [t.strip() for t in rest.split(",")]
    sums = {f"v{r}" for r in gen.L_A + gen.L_B}
    if op.startswith(("v_mfma", "v_exp_f32", "v_cvt_pk", "v_max")) or (op == "v_add_f32" and toks[0] in sums):
        return _regs(toks[0]), [r for t in toks[1:] for r in _regs(t)]
    return None


def _history(lines, gen):
    """register -> [(role, instruction)] over the arithmetic instructions, in program order."""
    h = collections.defaultdict(list)
    for ln in lines:
        a = _arith(ln, gen)
        if a:
            for r in a[1]:
                h[r].append(("r", ln))
            for r in a[0]:
                h[r].append(("w", ln))
    return h


@pytest.mark.parametrize("v", VARIANTS)
def test_schedule_1_reorders_schedule_0(streams, v):
    lines, gen = streams
    s0, s1 = _sections(_norm(lines[(v, 0)], v)), _sections(_norm(lines[(v, 1)], v))
    for name in s0:
        a, b = s0[name], s1[name]
        assert collections.Counter(a) == collections.Counter(b), f"V{v} {name}: not the same instructions"
        ha, hb = _history(a, gen), _history(b, gen)
        assert ha.keys() == hb.keys()
        for r in ha:
            assert ha[r] == hb[r], f"V{v} {name}: register {r} is written / read in another order"
        if not name.startswith("body"):
            assert a == b, f"V{v} {name}: only the loop body is re-ordered"
    assert s0["body0"] != s1["body0"] and s0["body1"] != s1["body1"]
    # behind the last MFMA of phase 2, in front of the rescale check / the tile counter: nothing that schedule 0 has not there
    for p in ("body0", "body1"):
        last = max(i for i, ln in enumerate(s1[p]) if ln.startswith("v_mfma"))
        last0 = max(i for i, ln in enumerate(s0[p]) if ln.startswith("v_mfma"))
        assert not collections.Counter(s1[p][last:]) - collections.Counter(s0[p][last0:])
    # the loop head of schedule 1 is aligned, schedule 0 carries no directive
    assert sum(ln.startswith(".p2align") for ln in lines[(v, 1)]) == 1 and not any(ln.startswith(".") and not ln.endswith(":")
                                                                                   for ln in lines[(v, 0)])


@pytest.mark.parametrize("v", VARIANTS)
def test_schedule_0_is_the_stream_as_it_was(streams, v):
    lines, _ = streams
    want = json.load(open(GOLDEN))
    assert hashlib.sha256("\n".join(lines[(v, 0)]).encode()).hexdigest() == want[f"V{v}"]
