"""CPU: the WD-GCN entry points of include/tmgcn.h (tmgcn_wdgcn_*) validate their arguments before any device work —
from ctypes, and from a C program built in tmp_path with -fsanitize=address,undefined that calls each of them with
null, zero-size and mismatched arguments (the pattern of tests/sanitize/abi_invalid_args.c, which stays as it is)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tmgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_MARKS = ("ERROR: AddressSanitizer", "runtime error:", "SUMMARY: UndefinedBehaviorSanitizer")

DRIVER = r'''
#include <stdint.h>
#include <stdio.h>
#include "tmgcn.h"

static int failures = 0;
static void expect(const char* what, long long rc, int want_negative) {
  const int ok = want_negative ? (rc < 0) : (rc == 0);
  if (!ok) { ++failures; printf("FAIL %s rc=%lld\n", what, rc); }
  else if (want_negative && !tmgcn_last_error()[0]) { ++failures; printf("FAIL %s: no message\n", what); }
}
#define BAD(call) expect(#call, (long long)(call), 1)
#define NOP(call) expect(#call, (long long)(call), 0)

int main(void) {
  float* bogus = (float*)(uintptr_t)0x10;          /* never dereferenced: validation must fail first */
  void* ws = (void*)(uintptr_t)0x20;
  if (tmgcn_wdgcn_supported(2, 6) != 1 || tmgcn_wdgcn_supported(0, 6) || tmgcn_wdgcn_supported(2, 9) ||
      tmgcn_wdgcn_supported(9, 2)) { printf("FAIL supported\n"); ++failures; }
  if (tmgcn_wdgcn_param_count(2, 6) != 2 * 6 + 8 * 36 + 4 * 6 || tmgcn_wdgcn_param_count(2, 12) != -1) {
    printf("FAIL param_count\n"); ++failures;
  }
  if (tmgcn_wdgcn_bwd_workspace_bytes(-1, 2, 6) != -1 || tmgcn_wdgcn_bwd_workspace_bytes(100, 2, 12) != -1 ||
      tmgcn_wdgcn_bwd_workspace_bytes(0, 2, 6) != 0 || tmgcn_wdgcn_bwd_workspace_bytes(7301, 2, 6) <= 0) {
    printf("FAIL workspace_bytes\n"); ++failures;
  }
  /* forward */
  BAD(tmgcn_wdgcn_fwd_f32(0, 0, 0, 0, 0, 0, 10, 5, 2, 6, 0));                    /* nulls */
  BAD(tmgcn_wdgcn_fwd_f32(bogus, bogus, bogus, bogus, 0, 0, 10, 5, 2, 6, 0));    /* null Z */
  BAD(tmgcn_wdgcn_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 2, 9, 0)); /* H beyond the kernel */
  BAD(tmgcn_wdgcn_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 0, 6, 0)); /* F0 = 0 */
  BAD(tmgcn_wdgcn_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, -1, 5, 2, 6, 0)); /* negative N */
  BAD(tmgcn_wdgcn_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, -1, 2, 6, 0)); /* negative T_run */
  NOP(tmgcn_wdgcn_fwd_f32(0, 0, 0, 0, 0, 0, 0, 5, 2, 6, 0));                     /* no nodes */
  NOP(tmgcn_wdgcn_fwd_f32(0, 0, 0, 0, 0, 0, 10, 0, 2, 6, 0));                    /* no steps */
  /* backward */
  BAD(tmgcn_wdgcn_bwd_f32(0, 0, 0, 0, 0, 0, 0, 0, 10, 5, 2, 6, 0, 0, 0));        /* null dP */
  BAD(tmgcn_wdgcn_bwd_f32(bogus, bogus, bogus, bogus, bogus, 0, bogus, bogus, 10, 5, 2, 6, ws, 1 << 20, 0)); /* null C */
  BAD(tmgcn_wdgcn_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 2, 6, ws, 16, 0));  /* workspace short */
  BAD(tmgcn_wdgcn_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 2, 6, 0, 1 << 20, 0)); /* null ws */
  BAD(tmgcn_wdgcn_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 12, 6, ws, 1 << 20, 0)); /* F0 */
  BAD(tmgcn_wdgcn_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, -3, 5, 2, 6, ws, 1 << 20, 0)); /* N < 0 */
  printf("%d failures\n", failures);
  return failures != 0;
}
'''


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_wdgcn_entry_points_reject_bad_arguments_under_asan_ubsan(tmp_path):
    src = tmp_path / "wdgcn_invalid_args.c"
    src.write_text(DRIVER)
    exe = tmp_path / "wdgcn_invalid_args"
    lib_dir = os.path.join(ROOT, "tm-gcn_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + lib_dir, "-ltmgcn_hip", "-Wl,-rpath," + lib_dir])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "0 failures" in out and not any(m in out for m in BAD_MARKS), out[-3000:]


def test_wdgcn_validation_from_ctypes():
    lib = _lib.load()
    assert lib.tmgcn_wdgcn_supported(2, 8) == 1 and lib.tmgcn_wdgcn_supported(2, 12) == 0
    rc = lib.tmgcn_wdgcn_fwd_f32(None, None, None, None, None, None, 10, 5, 2, 12, None)
    assert rc == -1 and b"H=12" in lib.tmgcn_last_error()
    rc = lib.tmgcn_wdgcn_bwd_f32(*([C.c_void_p(16)] * 7), None, 10, 5, 2, 6, None, 0, None)
    assert rc == -1 and b"dP" in lib.tmgcn_last_error()
