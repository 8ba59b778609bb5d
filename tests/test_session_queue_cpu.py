"""The host-only bookkeeping of a session (atspeed_amd/csrc/session_queue.h: lane table, ticket table, submission queue) as a stand-alone
program under the address and undefined-behaviour sanitizers: tests/session_queue_check.cpp has its own main and covers submission order,
lane reuse, each ticket reported exactly once, a growing queue, retirement and admission at the same round boundary, an empty round, and the
replay of the 24 per-user round counts of golden case k6_dk12_new7_gamma3_s9 through 4 lanes (31 rounds against 36 in chunks of 4)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_session_queue_program_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile tests/session_queue_check.cpp")
    exe = str(tmp_path / "session_queue_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # the runtimes inside the program: no demand on what the loader puts first
                    "-I", os.path.join(ROOT, "atspeed_amd", "csrc"), os.path.join(ROOT, "tests", "session_queue_check.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("session_queue ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
