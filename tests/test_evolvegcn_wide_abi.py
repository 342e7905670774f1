"""CPU: the wide EvolveGCN-H entry points of include/tmgcn.h (tmgcn_egcn_wide_*) validate their arguments before any
device work — from ctypes, and from a C program built in tmp_path with -fsanitize=address,undefined that calls each of
them with null, zero-size and mismatched arguments (the pattern of tests/test_evolvegcn_abi.py) — and the narrow entry
points keep their domain and messages."""
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

int main(void) {
  float* f = (float*)(uintptr_t)0x10;              /* never dereferenced: validation must fail first */
  double* d = (double*)(uintptr_t)0x40;
  int32_t* i = (int32_t*)(uintptr_t)0x80;
  void* ws = (void*)(uintptr_t)0x20;
  if (tmgcn_egcn_wide_supported(2, 9) != 1 || tmgcn_egcn_wide_supported(9, 2) != 1 || tmgcn_egcn_wide_supported(64, 64) != 1 ||
      tmgcn_egcn_wide_supported(1, 64) != 1 || tmgcn_egcn_wide_supported(64, 1) != 1 || tmgcn_egcn_wide_supported(8, 8) ||
      tmgcn_egcn_wide_supported(6, 6) || tmgcn_egcn_wide_supported(0, 6) || tmgcn_egcn_wide_supported(65, 2) ||
      tmgcn_egcn_wide_supported(2, 65) || tmgcn_egcn_wide_supported(-1, 12)) {
    printf("FAIL wide_supported\n"); ++failures;
  }
  /* the narrow entry points keep their domain */
  if (tmgcn_egcn_supported(6, 6) != 1 || tmgcn_egcn_supported(6, 9) || tmgcn_egcn_supported(9, 2) ||
      tmgcn_egcn_param_count(2, 12) != -1 || tmgcn_egcn_param_count(6, 6) != 6 + 3 * (2 * 36 + 36) ||
      tmgcn_egcn_fwd_workspace_bytes(100, 5, 2, 12) != -1 || tmgcn_egcn_bwd_workspace_bytes(80, 9, 6) != -1) {
    printf("FAIL narrow domain\n"); ++failures;
  }
  if (tmgcn_egcn_wide_fwd_workspace_bytes(-1, 5, 2, 12) != -1 || tmgcn_egcn_wide_fwd_workspace_bytes(100, -1, 2, 12) != -1 ||
      tmgcn_egcn_wide_fwd_workspace_bytes(100, 5, 6, 6) != -1 || tmgcn_egcn_wide_fwd_workspace_bytes(100, 5, 2, 65) != -1 ||
      tmgcn_egcn_wide_fwd_workspace_bytes(7301, 80, 64, 64) <= 0 || tmgcn_egcn_wide_bwd_workspace_bytes(-1, 2, 12) != -1 ||
      tmgcn_egcn_wide_bwd_workspace_bytes(80, 6, 6) != -1 || tmgcn_egcn_wide_bwd_workspace_bytes(80, 65, 6) != -1 ||
      tmgcn_egcn_wide_bwd_workspace_bytes(80, 16, 32) <= 0) {
    printf("FAIL workspace_bytes\n"); ++failures;
  }
  /* forward */
#define FWD(H, idx, rp, Fp, N, T, F, k, w, wb) tmgcn_egcn_wide_fwd(H, d, d, rp, i, f, f, d, Fp, idx, d, d, d, d, f, 0, N, T, F, k, w, wb, 0)
  BAD(tmgcn_egcn_wide_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 100, 5, 2, 12, 0, 0, 0));   /* nulls */
  BAD(FWD(f, i, 0, 0, 100, 5, 2, 65, ws, 1 << 24));                       /* k beyond the kernels */
  BAD(FWD(f, i, 0, 0, 100, 5, 65, 2, ws, 1 << 24));                       /* F beyond the kernels */
  BAD(FWD(f, i, 0, 0, 100, 5, 6, 6, ws, 1 << 24));                        /* the narrow kernels' widths */
  BAD(FWD(f, i, 0, 0, 100, 5, 0, 12, ws, 1 << 24));                       /* F = 0 */
  BAD(FWD(f, i, 0, 0, 11, 5, 2, 12, ws, 1 << 24));                        /* N < k */
  BAD(FWD(f, i, 0, 0, -1, 5, 2, 12, ws, 1 << 24));                        /* negative N */
  BAD(FWD(f, i, 0, 0, 100, -1, 2, 12, ws, 1 << 24));                      /* negative T_run */
  BAD(FWD(f, i, 0, 0, 100, 70000, 2, 12, ws, 1 << 24));                   /* T_run > 65535 */
  BAD(FWD(f, 0, 0, 0, 100, 5, 2, 12, ws, 1 << 24));                       /* null idx */
  BAD(FWD(f, i, 0, 0, 100, 5, 2, 12, ws, 16));                            /* workspace short */
  BAD(FWD(f, i, 0, 0, 100, 5, 2, 12, 0, 1 << 24));                        /* null workspace */
  BAD(FWD(f, i, (const int64_t*)d, 0, 100, 5, 2, 12, ws, 1 << 24));       /* layer-2 rows, F_prev = 0 */
  BAD(FWD(f, i, (const int64_t*)d, -3, 100, 5, 2, 12, ws, 1 << 24));      /* layer-2 rows, F_prev < 0 */
  BAD(tmgcn_egcn_wide_fwd(f, d, d, (const int64_t*)d, i, f, 0, d, 12, i, d, d, d, d, f, 0, 100, 5, 2, 12, ws, 1 << 24, 0)); /* null X_prev */
  /* backward */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, d, f, d, 0, d, 0, 100, 5, 2, 12, ws, 1 << 24, 0)); /* null dP */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, 0, f, d, d, d, 0, 100, 5, 2, 12, ws, 1 << 24, 0)); /* null gates */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, 0, d, d, f, d, d, d, 0, 100, 5, 2, 12, ws, 1 << 24, 0)); /* null H_sel */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, d, f, d, d, d, 0, 100, 5, 2, 12, ws, 16, 0));      /* workspace short */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, d, f, d, d, d, 0, 100, 5, 65, 6, ws, 1 << 24, 0)); /* F */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, d, f, d, d, d, 0, 100, 5, 6, 6, ws, 1 << 24, 0));  /* narrow widths */
  BAD(tmgcn_egcn_wide_bwd(d, d, i, d, d, d, d, f, d, d, d, 0, 3, 5, 2, 12, ws, 1 << 24, 0));   /* N < k */
  printf("%d failures\n", failures);
  return failures != 0;
}
'''


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_egcn_wide_entry_points_reject_bad_arguments_under_asan_ubsan(tmp_path):
    src = tmp_path / "egcn_wide_invalid_args.c"
    src.write_text(DRIVER)
    exe = tmp_path / "egcn_wide_invalid_args"
    lib_dir = os.path.join(ROOT, "tm-gcn_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + lib_dir, "-ltmgcn_hip", "-Wl,-rpath," + lib_dir])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "0 failures" in out and not any(m in out for m in BAD_MARKS), out[-3000:]


def test_egcn_wide_domain_from_ctypes():
    lib = _lib.load()
    for F, k in ((2, 9), (9, 2), (64, 64), (1, 64), (64, 1)):
        assert lib.tmgcn_egcn_wide_supported(F, k) == 1, (F, k)
    for F, k in ((8, 8), (6, 6), (0, 6), (65, 2), (2, 65)):
        assert lib.tmgcn_egcn_wide_supported(F, k) == 0, (F, k)
    assert lib.tmgcn_egcn_wide_fwd_workspace_bytes(100, 5, 6, 6) == -1
    assert lib.tmgcn_egcn_wide_fwd_workspace_bytes(100, 5, 2, 65) == -1
    assert lib.tmgcn_egcn_wide_fwd_workspace_bytes(-1, 5, 2, 12) == -1
    assert lib.tmgcn_egcn_wide_fwd_workspace_bytes(100, -1, 2, 12) == -1
    assert lib.tmgcn_egcn_wide_bwd_workspace_bytes(5, 8, 8) == -1
    assert lib.tmgcn_egcn_wide_bwd_workspace_bytes(-1, 2, 12) == -1
    # 1024 nodes per selection block, 64 candidates (fp64 score + int32 node) each, and W_g·X of every step
    assert lib.tmgcn_egcn_wide_fwd_workspace_bytes(1025, 5, 16, 32) == 5 * 2 * 64 * 12 + 5 * 3 * 16 * 32 * 8
    assert lib.tmgcn_egcn_wide_bwd_workspace_bytes(5, 16, 32) == 5 * (4 * 16 * 32 + 32) * 8


def test_egcn_wide_validation_from_ctypes():
    lib = _lib.load()
    rc = lib.tmgcn_egcn_wide_fwd(*([None] * 8), 0, *([None] * 7), 100, 5, 2, 65, None, 0, None)
    assert rc == -1 and b"k=65" in lib.tmgcn_last_error()
    rc = lib.tmgcn_egcn_wide_fwd(*([C.c_void_p(16)] * 3), *([None] * 5), 0, *([C.c_void_p(16)] * 7), 11, 5, 2, 12,
                                 C.c_void_p(16), 1 << 24, None)
    assert rc == -1 and b"N >= k" in lib.tmgcn_last_error()
    rc = lib.tmgcn_egcn_wide_fwd(*([None] * 8), 0, *([None] * 7), 100, 5, 2, 12, None, 0, None)
    assert rc == -1 and b"null" in lib.tmgcn_last_error()
    rc = lib.tmgcn_egcn_wide_bwd(*([C.c_void_p(16)] * 9), None, C.c_void_p(16), None, 100, 5, 2, 12, C.c_void_p(16), 1 << 24,
                                 None)
    assert rc == -1 and b"null" in lib.tmgcn_last_error()
    for ws, nbytes in ((C.c_void_p(16), 16), (None, 1 << 24)):                   # short, null
        rc = lib.tmgcn_egcn_wide_fwd(*([C.c_void_p(16)] * 3), *([None] * 5), 0, *([C.c_void_p(16)] * 7), 100, 5, 2, 12, ws,
                                     nbytes, None)
        assert rc == -3 and b"workspace" in lib.tmgcn_last_error()               # TMGCN_ERR_WORKSPACE


def test_narrow_entry_points_keep_their_domain():
    lib = _lib.load()
    assert lib.tmgcn_egcn_supported(6, 9) == 0 and lib.tmgcn_egcn_supported(6, 8) == 1 and lib.tmgcn_egcn_supported(8, 8) == 1
    assert lib.tmgcn_egcn_param_count(2, 12) == -1 and lib.tmgcn_egcn_param_count(2, 6) == 2 + 3 * (8 + 12)
    rc = lib.tmgcn_egcn_fwd(*([None] * 8), 0, *([None] * 7), 100, 5, 2, 12, None, 0, None)
    assert rc == -1 and b"k=12" in lib.tmgcn_last_error() and b"1..8 x 1..8" in lib.tmgcn_last_error()
    rc = lib.tmgcn_egcn_bwd(*([C.c_void_p(16)] * 9), None, C.c_void_p(16), None, 100, 5, 12, 6, C.c_void_p(16), 1 << 20, None)
    assert rc == -1 and b"F=12" in lib.tmgcn_last_error()
    assert lib.tmgcn_abi_version() == 5
