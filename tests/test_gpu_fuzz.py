"""Short fixed-seed campaigns of the randomised differential checker (tests/fuzz_parity.py): random scheme / ring / chain /
level / batch / dispatcher switches / operation, every output word against the oracle.  The two base campaigns are time-bounded; the
fused ones are bounded by their case count (tests/test_fuzz_cases.py shows on the CPU what those seeds and counts cover), and one
campaign with an injected bit shows that the comparison and the exit path are live."""
import json
import os
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_parity as fp  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_cases_match_the_oracle(seed):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_parity.py"), "--seconds", "25", "--seed", str(seed)],
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    summary = json.loads(p.stdout.strip().splitlines()[-1])
    assert summary["cases"] >= 10


def _fuzz(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_parity.py")] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=600)


@pytest.mark.parametrize("seed,max_cases", fp.FUSED_CAMPAIGNS)
def test_random_fused_cases_match_the_oracle(seed, max_cases):
    """count-bounded: --seconds is a guard far above what the campaign takes"""
    t0 = time.time()
    p = _fuzz("--family", "fused", "--seed", seed, "--max-cases", max_cases, "--seconds", 300)
    print("fused campaign seed %d: %.1f s wall" % (seed, time.time() - t0))
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    summary = json.loads(p.stdout.strip().splitlines()[-1])
    assert summary["family"] == "fused" and summary["cases"] == max_cases and summary["skipped"] == 0
    assert sum(summary["passed_by_kind"].values()) == max_cases


def test_an_injected_bit_is_reported_and_the_printed_case_replays_it():
    p = _fuzz("--family", "fused", "--seed", fp.FUSED_INJECT_SEED, "--max-cases", 8, "--inject")
    assert p.returncode == 1, p.stdout[-3000:] + p.stderr[-3000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    assert report["result"].startswith("MISMATCH") and ": 1 words differ" in report["result"]
    case = report["case"]
    assert case["family"] == "fused" and case["logn"] == 10
    again = _fuzz("--case", json.dumps(case), "--inject")
    assert again.returncode == 0, again.stdout[-3000:] + again.stderr[-3000:]
    replay = json.loads(again.stdout.strip().splitlines()[-1])
    assert replay["result"] == report["result"] and replay["case"] == case
    clean = json.loads(_fuzz("--case", json.dumps(case)).stdout.strip().splitlines()[-1])
    assert clean["result"] == "ok"  # the words differ by the injected bit alone
