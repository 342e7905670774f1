"""GPU: the opt-in of a kernel into more than 64 KB of LDS (allow_large_lds, csrc/common.h) when one process asks the same
kernel for more after it was granted less, and for less after more.  A process that has already run a width cannot show
that, so one fresh child process runs the existing checkers, with their own bars, in this order:

  EvolveGCN-H wide, (T, N, k) = (3, 70, 8), F = 50, 64, 50: the chain kernels keep U_Z, U_R, U_H in LDS with F padded to a
      multiple of 8 — 75 KB at F = 50 (the first grant), 97 KB at F = 64 (growth on the same kernel), 75 KB again.
  WD-GCN wide, (T, N) = (3, 70), (F0, H) = (16, 64), (64, 64), (16, 64), (8, 40): at H = 64 the forward's weight image
      grows with ⌈F0/16⌉ (133 KB -> 145 KB on the same instantiation); H = 40 runs the backward through the four-tile
      instantiation that H = 64 has opted in.

A mishandled opt-in is a refused launch (TMGCN_ERR_LAUNCH), reported as a RuntimeError in the child."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

# the seeds are ones at which the restatement's gap condition (test_gpu_evolvegcn_wide._checked_summarize) holds
_CHILD = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import _evolvegcn_ref as ref
import test_gpu_evolvegcn_wide as eg
import test_gpu_wdgcn_wide as wd
ref.summarize = eg._checked_summarize          # what the `gap` fixture does
for F, seed in ((50, 5058), (64, 6472), (50, 5058)):
    eg._check_evolve(3, 70, F, 8, seed, "scaled")
for F0, H in ((16, 64), (64, 64), (16, 64), (8, 40)):
    wd._check_kernel(3, 70, F0, H)
print("LDS OPT-IN SEQUENCE PASSED")
'''


def test_one_kernel_asks_for_more_lds_then_for_less():
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "tests": TESTS}], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0 and "LDS OPT-IN SEQUENCE PASSED" in r.stdout, out[-6000:]
