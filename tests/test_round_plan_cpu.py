"""The host-only arithmetic of a beam-SD round (atspeed_amd/csrc/round_plan.h: what a user does in a round, the rows a forward takes, where a
walk finds a block's logit rows, the transition, the worst round's capacity) as a stand-alone program under the address and
undefined-behaviour sanitizers.  tests/round_plan_check.cpp has its own main: without arguments it checks the header against literals of the
formulas it replaced in the engine; with a call's prompt lengths and accepted steps it replays the call as bssd_round does, and the forwards
it prints are compared with the independent Python restatement tests/round_ref.py (which tests/test_staged_verify_gpu.py holds against the
engine's own forward logs)."""
import json
import os
import shutil
import subprocess

import pytest

from tests.golden.cases import CASES
from tests.round_ref import expected_draft_log, expected_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile tests/round_plan_check.cpp")
    out = str(tmp_path_factory.mktemp("round_plan") / "round_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # the runtimes inside the program: no demand on what the loader puts first
                    "-I", os.path.join(ROOT, "atspeed_amd", "csrc"), os.path.join(ROOT, "tests", "round_plan_check.cpp"), "-o", out],
                   check=True)
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_round_plan_program_is_clean_under_the_sanitizers(exe):
    assert _run(exe).strip().endswith("round_plan ok")


def _golden_user():
    """the one user of golden case k6_dk12_new7_gamma3_s9: (gamma, new, K, DK), its prompt length and its recorded accepted steps"""
    case = [c for c in CASES if c["name"] == "k6_dk12_new7_gamma3_s9"][0]
    with open(os.path.join(ROOT, "tests", "golden", "bssd_golden.json")) as f:
        gold = [g for g in json.load(f) if g["name"] == case["name"]][0]
    return (case["gamma"], case["max_new_tokens"], case["K"], case["DK"]), [case["P"]], [[x["n_matches"] for x in gold["rounds"]]]


# the three-user lock-step batch recorded in profiles/scan_refactor_isa_and_speed.txt, section 3b: users 6, 15, 2 of
# tests/test_staged_verify_gpu.py (prompts of 18 + 5 * (u % 7) tokens) and the target forwards of its staged run
SCAN_3B = ((3, 7, 6, 12), [18 + 5 * (u % 7) for u in (6, 15, 2)], [[2, 2], [1, 3], [2, 1, 1]])
SCAN_3B_STAGED = [(99, 3), (36, 36), (24, 24), (18, 18), (36, 36), (24, 24), (12, 12), (18, 18), (12, 12)]


# one user whose rounds accept every block (tests/test_staged_verify_gpu.py::test_last_rounds, draft == target): its second round's draft
# step 0 re-ingests (dk + k tokens)
ALL_ACCEPTED = ((2, 7, 20, 40), [30], [[2, 2]])


@pytest.mark.parametrize("call", [_golden_user(), SCAN_3B, ALL_ACCEPTED], ids=["golden_k6_dk12_new7_gamma3_s9", "scan_refactor_3b", "all_accepted"])
def test_replay_equals_the_python_restatement(exe, call):
    (gamma, new, k, dk), lens, acc = call
    out = _run(exe, gamma, new, k, dk, *[f"{p}:{','.join(str(a) for a in steps)}" for p, steps in zip(lens, acc)])
    got = {}
    for line in out.splitlines():
        name, *pairs = line.split()
        got[name] = [tuple(int(x) for x in p.split(",")) for p in pairs]
    want_p, _, _, _ = expected_log(lens, acc, gamma, new, k, dk, False)
    want_s, _, _, _ = expected_log(lens, acc, gamma, new, k, dk, True)
    want_d, want_seq = expected_draft_log(lens, acc, gamma, new, k, dk)
    assert got["packed"] == want_p and got["staged"] == want_s and got["draft"] == want_d
    assert [got[f"user{u}"] for u in range(len(lens))] == want_seq
    for u, seq in enumerate(want_seq):                                    # every recorded round was replayed, and the call ended on time
        assert seq[-1][0] == len(acc[u]) and seq[-1][1] >= new
    if call is SCAN_3B:
        assert want_s == SCAN_3B_STAGED
    if call is ALL_ACCEPTED:
        assert want_d == [(30, 1), (40, 40), (60, 20), (40, 40)]
