"""What the campaigns of tests/test_gpu_fuzz.py draw, checked without a GPU through `fuzz_parity.py --dry-run`: the very seeds and
--max-cases values that file runs (fuzz_parity.FUSED_CAMPAIGNS).  Together they must reach every fused kind, every entry of the fused
switch list, every ring, the ends of the level range and a batch past chunk * lanes; the base family must draw what it drew before
the fused family existed (tests/golden/fuzz_base_first50.json, recorded from that version); and the oracle side of the fused cases
must run on its own and give the shapes the header promises."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_parity as fp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_base_first50.json")


def _dry(capsys, *args):
    fp.main(["--dry-run"] + [str(a) for a in args])
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def campaigns():
    """the dry-run summary of every committed fused campaign, each with its cases"""
    import contextlib
    import io
    out = []
    for seed, max_cases in fp.FUSED_CAMPAIGNS:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fp.main(["--dry-run", "--list", "--family", "fused", "--seed", str(seed), "--max-cases", str(max_cases)])
        out.append(json.loads(buf.getvalue().strip().splitlines()[-1]))
    return out


def _total(campaigns, name):
    acc = {}
    for c in campaigns:
        for k, v in c[name].items():
            acc[k] = acc.get(k, 0) + v
    return acc


def test_every_campaign_draws_its_count_and_skips_nothing(campaigns):
    for (seed, max_cases), c in zip(fp.FUSED_CAMPAIGNS, campaigns):
        assert c["cases"] == max_cases == len(c["drawn"]) and c["skipped"] == 0, seed
        assert all(case["family"] == "fused" for case in c["drawn"])


def test_every_fused_kind_is_drawn_at_least_three_times(campaigns):
    kinds = _total(campaigns, "by_kind")
    assert set(kinds) == set(fp.FUSED_KINDS)
    assert len(fp.FUSED_KINDS) == 22  # the nineteen fused entry points and the CKKS forms of multiply_plain, add_plain and sub_plain
    short = {k: v for k, v in kinds.items() if v < 3}
    assert not short, short


def test_every_entry_of_the_fused_switch_list_meets_a_fused_kind(campaigns):
    met = {}
    for c in campaigns:
        for k, kinds in c["kinds_by_switch"].items():
            met.setdefault(k, set()).update(kinds)
    for entry in fp.FUSED_SWITCH_SETS:
        for k, v in entry.items():
            assert met.get("%s=%s" % (k, v)), "%s=%s is never drawn" % (k, v)
    assert any(not case["switches"] for c in campaigns for case in c["drawn"])  # and the default path


def test_the_switch_list_holds_the_base_list_and_the_twelve_newer_switches():
    assert all(s in fp.FUSED_SWITCH_SETS for s in fp.SWITCH_SETS)
    newer = {"ABC_HIP_NO_ROTATE_ADD_FUSION", "ABC_HIP_NO_ROTATE_MAC_FUSION", "ABC_HIP_NO_MULPLAIN_RESCALE_FUSION", "ABC_HIP_NO_TENSOR_SUM",
             "ABC_HIP_NO_PLAIN_MAC_SUM", "ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION", "ABC_HIP_NO_CONST_MAC_SUM", "ABC_HIP_MAIN_TWO_PER_CU",
             "ABC_HIP_PLAIN_SUM_RESCALE_TERMS", "ABC_HIP_CONST_SUM_RESCALE_FUSED", "ABC_HIP_LEAN_LIMIT", "ABC_HIP_PASS0_TARGET_LIMIT"}
    assert newer <= set(fp.FUSED_SWITCHES) and not newer & set(fp.ALL_SWITCHES)
    values = lambda name: sorted(s[name] for s in fp.FUSED_SWITCH_SETS if name in s)  # noqa: E731
    assert values("ABC_HIP_PLAIN_SUM_RESCALE_TERMS") == ["0", "1", "2", "4"] and values("ABC_HIP_CONST_SUM_RESCALE_FUSED") == ["0", "1"]
    with open(os.path.join(fp.ROOT, "abc_amd", "csrc", "abc_context.hip")) as f:
        src = f.read()
    assert all('"%s"' % name in src for name in fp.FUSED_SWITCHES)  # every name is one the library reads


def test_rings_levels_and_batches(campaigns):
    assert {"10", "11", "12", "13", "14"} <= set(_total(campaigns, "by_ring"))
    assert sum(c["level_is_one"] for c in campaigns) > 0 and sum(c["level_is_top"] for c in campaigns) > 0
    assert max(c["level_max"] for c in campaigns) >= 5
    assert sum(c["batch_over_chunk_lanes"] for c in campaigns) >= 1
    assert set(_total(campaigns, "by_batch")) == {"1", "2", "3", "5", "7"}
    for (seed, _), c in zip(fp.FUSED_CAMPAIGNS, campaigns):
        assert c["contexts_by_ring"].get("14", 0) <= 2, "campaign %d holds more than two N = 2^14 contexts" % seed


def test_a_round_shares_one_context_among_six_to_ten_operations(campaigns):
    for c in campaigns:
        runs, last = [], None
        for case in c["drawn"]:
            key = fp.fused_context_key(case)
            if key != last:
                runs.append(0)
                last = key
            runs[-1] += 1
        assert all(6 <= r <= 10 for r in runs[:-1]) and 1 <= runs[-1] <= 10  # --max-cases may cut the last round short


def test_a_case_replays_from_its_json(campaigns):
    for case in campaigns[0]["drawn"]:
        again = json.loads(json.dumps(case))
        assert again == case
        fp.validate_fused(again)
        for name in ("scheme", "logn", "bits", "style", "switches", "kind", "nl", "batch", "data_seed"):
            assert name in case


def test_legal_ranges_are_enforced():
    case = next(c for c in fp.fused_cases(1, 14, 400) if c["kind"] == "multiply_plain_sum_rescale")
    with pytest.raises(AssertionError):
        fp.validate_fused(dict(case, nl=1))
    poly = next(c for c in fp.fused_cases(1, 14, 2000) if c["kind"] == "poly_eval")
    with pytest.raises(AssertionError):
        fp.validate_fused(dict(poly, nl=fp._ceil_log2(poly["degree"]) + 1))
    with pytest.raises(AssertionError):
        fp.validate_fused(dict(poly, style=0))


@pytest.mark.parametrize("seed", [1, 2])
def test_the_base_family_draws_what_it_drew_before(capsys, seed):
    with open(GOLDEN) as f:
        want = json.load(f)[str(seed)]
    got = _dry(capsys, "--family", "base", "--seed", seed, "--max-cases", 50, "--list")
    assert got["cases"] == 50 and got["drawn"] == want
    assert _dry(capsys, "--seed", seed, "--max-cases", 50, "--list")["drawn"] == want  # base is the default family


def test_the_oracle_side_runs_clean_on_a_short_campaign(capsys):
    """--reference: no exception, the header's shapes and every word below its prime (run_fused_case asserts both) at N <= 2^11"""
    got = _dry(capsys, "--family", "fused", "--reference", "--seed", 5, "--max-cases", 160, "--list")
    small = [c for c in got["drawn"] if c["logn"] <= 11]
    assert got["referenced"] == len(small) >= 40 and got["skipped"] == 0
    assert len({c["kind"] for c in small}) >= 20


def test_the_comparator_reports_an_injected_bit():
    x = np.arange(64, dtype=np.uint64).reshape(2, 2, 1, 16)
    assert fp._verdict(x, x.copy(), 1, False) == "ok"
    assert fp._verdict(x, x.copy(), 1, True).startswith("MISMATCH nl=1: 1 words differ, first at (1, 0, 0, 0)")
    assert np.array_equal(x, np.arange(64, dtype=np.uint64).reshape(2, 2, 1, 16))  # the flip is made on a copy
    assert fp._verdict(x, x[:1], 1, False).startswith("MISMATCH")
