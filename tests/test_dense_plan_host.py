"""The host's plan of the dense walks (ms_scan_best, ms_scan_affinity, ms_scan_score_histogram) under ASan + UBSan, in the CPU build
container only: motifscan_amd/csrc/ms_dense_plan.h (plain C++, no HIP call) driven by a program of its own
(tests/sanitize/dense_plan_asan.cpp) with a tiny geometry (8 window starts per segment, widest tiled motif 4, 16 entries per tile; with
and without partials) and the kernels' own geometries, on R in {0, 1, 3} with every combination of the region lengths {0, 1, seg - 1,
seg, seg + 1, 2 seg, 2 seg + 1}, P in {0, 1, 5}, every motif walked / none / only the middle one skipped, tiles that fill exactly and
one entry over, and motifs of tile_max_w and tile_max_w + 1 columns.  Every case is compared field by field with a brute-force
restatement and then walked over arrays of exactly the promised sizes.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "dense_plan_asan.bin")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")


def test_dense_plan_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "dense_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dense_plan_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    # geometries (tiny with and without partials, the two of the kernels) x region sets (R = 0, the 7 lengths for R = 1 and 7^3 for
    # R = 3) x motif sets (P = 0; P = 1: three widths, walked or not; P = 5: six width patterns x four walked patterns)
    assert int(out.stdout.split("(")[1].split()[0]) >= 4 * (1 + 7 + 7 ** 3) * (1 + 3 * 2 + 6 * 4)
