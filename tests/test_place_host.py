"""The host arithmetic of the variant scans' record placement under ASan + UBSan, in the CPU build container only: the chunk plan, the
record offsets and the layout of a carved block (motifscan_amd/csrc/ms_place.h: plain C++, no HIP call) driven by a program of its own
(tests/sanitize/place_asan.cpp) on V in {0, 1, tile - 1, tile, tile + 1}, P in {0, 1, 3}, chunk settings {0, 7, tile, tile + 1} and the
three-chunk case whose last chunk is one variant, with every array allocated at exactly the size the plan promises.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "place_asan.bin")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")


def test_placement_arithmetic_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "place_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "place_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert int(out.stdout.split("(")[1].split()[0]) >= 5 * 3 * 4 + 3
