"""CPU: the wide WD-GCN entry points of include/tmgcn.h (tmgcn_wdgcn_wide_*) validate their arguments before any device
work — from ctypes, and from a C program built in tmp_path with -fsanitize=address,undefined that calls each of them
with null, zero-size, short-workspace and out-of-domain arguments (the pattern of tests/test_wdgcn_abi.py)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tmgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_MARKS = ("ERROR: AddressSanitizer", "runtime error:", "SUMMARY: UndefinedBehaviorSanitizer")
NAMES = ("tmgcn_wdgcn_wide_supported", "tmgcn_wdgcn_wide_saved_bytes", "tmgcn_wdgcn_wide_fwd_f32",
         "tmgcn_wdgcn_wide_bwd_workspace_bytes", "tmgcn_wdgcn_wide_bwd_f32")

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
  if (tmgcn_wdgcn_wide_supported(2, 9) != 1 || tmgcn_wdgcn_wide_supported(64, 64) != 1 || tmgcn_wdgcn_wide_supported(9, 8) != 1 ||
      tmgcn_wdgcn_wide_supported(2, 6) || tmgcn_wdgcn_wide_supported(0, 9) || tmgcn_wdgcn_wide_supported(2, 65) ||
      tmgcn_wdgcn_wide_supported(65, 2)) { printf("FAIL supported\n"); ++failures; }
  if (tmgcn_wdgcn_wide_saved_bytes(100, 5, 2, 6) != -1 || tmgcn_wdgcn_wide_saved_bytes(100, 5, 2, 65) != -1 ||
      tmgcn_wdgcn_wide_saved_bytes(-1, 5, 16, 32) != -1 || tmgcn_wdgcn_wide_saved_bytes(0, 5, 16, 32) != 0 ||
      tmgcn_wdgcn_wide_saved_bytes(10, 5, 16, 32) != 6LL * 5 * 10 * 32 * 4) { printf("FAIL saved_bytes\n"); ++failures; }
  if (tmgcn_wdgcn_wide_bwd_workspace_bytes(-1, 5, 16, 32) != -1 || tmgcn_wdgcn_wide_bwd_workspace_bytes(100, 5, 2, 6) != -1 ||
      tmgcn_wdgcn_wide_bwd_workspace_bytes(100, 5, 65, 2) != -1 || tmgcn_wdgcn_wide_bwd_workspace_bytes(0, 5, 16, 32) != 0 ||
      tmgcn_wdgcn_wide_bwd_workspace_bytes(7301, 80, 16, 32) <= 0) { printf("FAIL workspace_bytes\n"); ++failures; }
  /* forward */
  BAD(tmgcn_wdgcn_wide_fwd_f32(0, 0, 0, 0, 0, 0, 10, 5, 16, 32, 0));                        /* nulls */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, 0, 0, 10, 5, 16, 32, 0));        /* null Z */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 2, 65, 0));     /* H beyond the kernel */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 65, 2, 0));     /* F0 beyond the kernel */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 2, 6, 0));      /* the narrow kernels' widths */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, 5, 0, 32, 0));     /* F0 = 0 */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, -1, 5, 16, 32, 0));    /* negative N */
  BAD(tmgcn_wdgcn_wide_fwd_f32(bogus, bogus, bogus, bogus, bogus, 0, 10, -1, 16, 32, 0));   /* negative T_run */
  NOP(tmgcn_wdgcn_wide_fwd_f32(0, 0, 0, 0, 0, 0, 0, 5, 16, 32, 0));                         /* no nodes */
  NOP(tmgcn_wdgcn_wide_fwd_f32(0, 0, 0, 0, 0, 0, 10, 0, 16, 32, 0));                        /* no steps */
  /* backward */
  BAD(tmgcn_wdgcn_wide_bwd_f32(0, 0, 0, 0, 0, 0, 0, 0, 10, 5, 16, 32, 0, 0, 0));            /* null dP */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, 0, bogus, bogus, 10, 5, 16, 32, ws, 1 << 30, 0)); /* null saved */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 16, 32, ws, 16, 0));  /* workspace short */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 16, 32, 0, 1 << 30, 0)); /* null ws */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 65, 32, ws, 1 << 30, 0)); /* F0 */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, 5, 2, 8, ws, 1 << 30, 0));   /* narrow */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, -3, 5, 16, 32, ws, 1 << 30, 0)); /* N < 0 */
  BAD(tmgcn_wdgcn_wide_bwd_f32(bogus, bogus, bogus, bogus, bogus, bogus, bogus, bogus, 10, -5, 16, 32, ws, 1 << 30, 0)); /* T_run < 0 */
  printf("%d failures\n", failures);
  return failures != 0;
}
'''


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_wdgcn_wide_entry_points_reject_bad_arguments_under_asan_ubsan(tmp_path):
    src = tmp_path / "wdgcn_wide_invalid_args.c"
    src.write_text(DRIVER)
    exe = tmp_path / "wdgcn_wide_invalid_args"
    lib_dir = os.path.join(ROOT, "tm-gcn_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + lib_dir, "-ltmgcn_hip", "-Wl,-rpath," + lib_dir])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "0 failures" in out and not any(m in out for m in BAD_MARKS), out[-3000:]


def test_wdgcn_wide_truth_table_and_sizes_from_ctypes():
    lib = _lib.load()
    for w in [(2, 9), (64, 64), (9, 8)]:
        assert lib.tmgcn_wdgcn_wide_supported(*w) == 1, w
    for w in [(2, 6), (0, 9), (2, 65), (65, 2)]:
        assert lib.tmgcn_wdgcn_wide_supported(*w) == 0, w
    # every width has exactly one kernel family
    for F0 in range(0, 67):
        for H in range(0, 67):
            assert lib.tmgcn_wdgcn_wide_supported(F0, H) + lib.tmgcn_wdgcn_supported(F0, H) == int(1 <= F0 <= 64 and 1 <= H <= 64)
    assert lib.tmgcn_wdgcn_wide_saved_bytes(100, 5, 2, 65) == -1 and lib.tmgcn_wdgcn_wide_saved_bytes(-1, 5, 16, 32) == -1
    assert lib.tmgcn_wdgcn_wide_saved_bytes(0, 5, 16, 32) == 0 and lib.tmgcn_wdgcn_wide_saved_bytes(7, 0, 16, 32) == 0
    assert lib.tmgcn_wdgcn_wide_bwd_workspace_bytes(100, 5, 2, 6) == -1 and lib.tmgcn_wdgcn_wide_bwd_workspace_bytes(-1, 5, 16, 32) == -1
    assert lib.tmgcn_wdgcn_wide_bwd_workspace_bytes(0, 5, 16, 32) == 0
    # the step gradients (5 per row and unit) and at least one slab of the packed parameters
    np_ = 16 * 32 + 8 * 32 * 32 + 4 * 32
    assert lib.tmgcn_wdgcn_wide_bwd_workspace_bytes(10, 5, 16, 32) >= (5 * 50 * 32 + np_) * 4


def test_wdgcn_wide_validation_from_ctypes():
    lib = _lib.load()
    rc = lib.tmgcn_wdgcn_wide_fwd_f32(None, None, None, None, None, None, 10, 5, 2, 65, None)
    assert rc == -1 and b"H=65" in lib.tmgcn_last_error()
    rc = lib.tmgcn_wdgcn_wide_fwd_f32(None, None, None, None, None, None, 10, 5, 2, 6, None)
    assert rc == -1 and b"H=6" in lib.tmgcn_last_error()
    rc = lib.tmgcn_wdgcn_wide_bwd_f32(*([C.c_void_p(16)] * 7), None, 10, 5, 16, 32, None, 0, None)
    assert rc == -1 and b"dP" in lib.tmgcn_last_error()
    rc = lib.tmgcn_wdgcn_wide_bwd_f32(*([C.c_void_p(16)] * 5), None, C.c_void_p(16), C.c_void_p(16), 10, 5, 16, 32,
                                      C.c_void_p(32), 1 << 30, None)
    assert rc == -1 and b"saved" in lib.tmgcn_last_error()
    rc = lib.tmgcn_wdgcn_wide_bwd_f32(*([C.c_void_p(16)] * 8), 10, 5, 16, 32, C.c_void_p(32), 16, None)
    assert rc != 0 and b"workspace" in lib.tmgcn_last_error()
    assert lib.tmgcn_wdgcn_wide_fwd_f32(None, None, None, None, None, None, 0, 5, 16, 32, None) == 0
    assert lib.tmgcn_wdgcn_wide_fwd_f32(None, None, None, None, None, None, 10, 0, 16, 32, None) == 0


def test_wdgcn_wide_symbols_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tmgcn.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n + "(" in header and n in _lib.SIGNATURES, n
