"""The instruction-stream generators (csrc/gen_*_w64.py) on the host: each tracked ``*_asm.inc`` is, byte for byte, what its
generator prints — whatever the environment holds.  The generators once built timing-only ablation streams under the
variables set below (removed; they read no variable now), so a generator that looked at one of them again would print
another text here."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnihuman-1-hack_amd", "csrc")
# the (generator, stream) pairs of build.py::_generate
PAIRS = (("gen_attn_w64.py", "attention_w64_asm.inc"), ("gen_gemm_w64.py", "gemm_w64_asm.inc"),
         ("gen_conv_w64.py", "conv_w64_asm.inc"), ("gen_gemm_tn_w64.py", "gemm_tn_w64_asm.inc"),
         ("gen_attn_bwd_w64.py", "attention_bwd2_asm.inc"))
# every variable a generator ever recognised, at a value that used to change its output
FORMER = {"OMH_ATTN_ABL": "3", "OMH_BWD_ABL": "nodma", "OMH_CW64_ABL": "dma", "OMH_GW64_P256": "1", "OMH_GW64_ABLATIONS": "1",
          "OMH_GW64_ABL_SET": "m16", "OMH_GW64_SCHED": "1", "OMH_GW64_RING": "3", "OMH_GW64_WIDE16": "1",
          "OMH_GTW64_READ_END": "16", "OMH_GTW64_DMA_START": "12"}


def test_pairs_are_the_build_list():
    src = open(os.path.join(ROOT, "omnihuman-1-hack_amd", "build.py")).read()
    for gen, inc in PAIRS:
        assert f'("{gen}", "{inc}")' in src
    assert src.count('_asm.inc")') == len(PAIRS)
    # every other csrc/gen_*.py is a helper module, hashed into the build digest and never run
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "gen_*.py"))) == \
        sorted([g for g, _ in PAIRS] + ["gen_w64_common.py"])


@pytest.mark.parametrize("gen,inc", PAIRS)
def test_committed_stream_is_what_the_generator_prints(gen, inc):
    env = dict(os.environ, **FORMER)
    # (cwd elsewhere: a generator finds gen_w64_common.py beside itself, not through the working directory)
    out = subprocess.run([sys.executable, os.path.join(CSRC, gen)], check=True, capture_output=True, text=True, env=env,
                         cwd=os.path.dirname(ROOT)).stdout
    assert out == open(os.path.join(CSRC, inc)).read()


def test_generators_do_not_read_the_environment():
    for f in glob.glob(os.path.join(CSRC, "gen_*.py")):
        src = open(f).read()
        assert "environ" not in src and "getenv" not in src, f
