"""What the instruction-stream generators (gen_*_w64.py) share: the line collector, register names, the LDS wait
tracker, the even spreader of the two attention generators and the two op-list interleavers of the GEMM generators.
Not a generator itself: build.py runs its explicit
list of them and only hashes this file into the build digest (every csrc/gen_*.py is).

An op list describes a stretch of a stream before its waits are known:
    ("m", text, [tags])   an instruction (an MFMA, as a rule) that needs the LDS reads with those tags landed
    ("r", tag, text)      an LDS read
    ("x", text)           anything else
"""


def vr(lo, n=1):   return f"v{lo}" if n == 1 else f"v[{lo}:{lo + n - 1}]"
def ar(lo, n=1):   return f"a{lo}" if n == 1 else f"a[{lo}:{lo + n - 1}]"


class Emit:
    """The lines of one stream.  ``prefix`` + ``tag`` name its labels; they end in %=, unique per asm statement."""

    def __init__(self, prefix, tag):
        self.lines, self.prefix, self.tag, self.cuts = [], prefix, tag, []

    def __call__(self, s):
        self.lines.append(s)

    def lab(self, name):
        return f".L{self.prefix}{self.tag}_{name}_%="

    def label(self, name):
        self.lines.append(f"{name}:")

    def cut(self):
        """A piece of the text ends here (pieces(): what two streams share is written into the .inc once)."""
        self.cuts.append(len(self.lines))

    def pieces(self):
        b = [0] + self.cuts + [len(self.lines)]
        return [self.lines[i:j] for i, j in zip(b, b[1:])]

    def text(self):
        return "\n".join('    "%s\\n\\t"' % ln for ln in self.lines)


def linearize(e, ops, pending):
    """Emit `ops` in order; before an instruction that needs ds_read results, emit the s_waitcnt lgkmcnt that makes
    exactly those reads complete (LDS returns in order; a tag may stand for several reads, the youngest counts; the
    counter has 4 bits, so more than 15 younger reads wait for a few of them too).  `pending` = tags of reads issued
    earlier and not yet waited for, oldest first.  Returns the pending list at the end."""
    pending = list(pending)
    for op in ops:
        if op[0] == "r":
            e(op[2])
            pending.append(op[1])
        elif op[0] == "m":
            need = [t for t in op[2] if t in pending]
            if need:
                last = max(len(pending) - 1 - pending[::-1].index(t) for t in need)
                allowed = min(15, len(pending) - last - 1)
                e(f"s_waitcnt lgkmcnt({allowed})")
                pending = pending[len(pending) - allowed:]
            e(op[1])
        else:
            e(op[1])
    return pending


def spread(items, gaps, start=0, end=None):
    """Distribute `items` (ordered) over gaps[start:end] as evenly as possible; returns a per-gap list of lists."""
    end = gaps if end is None else end
    n = end - start
    out = [[] for _ in range(gaps)]
    for i, it in enumerate(items):
        out[start + min(n - 1, (i * n) // len(items))].append(it)
    return out


def spread_after(mfmas, extras, start=0, end=None):
    """The op lists `extras` dealt evenly behind mfmas[start:end], in order."""
    end = len(mfmas) if end is None else end
    n = end - start
    slots = [[] for _ in mfmas]
    for k, ex in enumerate(extras):
        slots[start + min(n - 1, (k * n) // max(1, len(extras)))].extend(ex)
    ops = []
    for m, s in zip(mfmas, slots):
        ops.append(m)
        ops.extend(s)
    return ops


def with_dma_tail(ops, dm, start=12):
    """Insert the DMA op lists `dm` after every other MFMA from the (start+1)-th on."""
    out, idx, cnt = [], 0, 0
    for op in ops:
        out.append(op)
        if op[0] == "m":
            cnt += 1
            if cnt > start and idx < len(dm) and (cnt - start) % 2 == 1:
                out.extend(dm[idx]); idx += 1
    while idx < len(dm):
        out.extend(dm[idx]); idx += 1
    return out
