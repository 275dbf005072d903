"""CPU test of the closest-offer update rule the tree walks share (rays1bench_amd/csrc/r1_offer.h): a stand-alone
program (tools/check_offer_host.cpp) compiles the header for the host and compares the one unsigned 64-bit compare of {t bits, index}
with the rule written out on floats, (t < best) | (t == best & id < best_id).

Fixed grid, every combination: t in {the floats below, at and above 0.001, FLT_MIN, 1, FLT_MAX's predecessor, FLT_MAX, +inf, NaN of both
signs} x best in {0.001, FLT_MAX, t} x id in {0, 1, 0xFFFFFFFE} x best_id in {0, 1, 0xFFFFFFFE, 0xFFFFFFFF} = 360 cases.  Each is compared
three ways: as the old update predicate (t > 0.001) & (t < FLT_MAX) & better; under the function's precondition alone,
(t > 0.001) & better; and bare, wherever `best` is a number (336 of the 360: a NaN `best` exists only as "equal to a NaN t", which the
precondition excludes).  Then 10^6 seeded random cases with t > 0.001: a quarter exact ties in t, a quarter neighbours of t in either
direction, a quarter against FLT_MAX.

The `t < FLT_MAX` term is folded (form 2, the default): the compare alone would take a t of FLT_MAX against the "none" state (FLT_MAX,
0xFFFFFFFF) — the program counts those six grid cases — so the walk may hold (FLT_MAX, id) and r1_offer_settle_form puts "none" back
where it hands its state on.  10^6 random WALKS check that: one to six offers (FLT_MAX itself, its predecessor, +inf, values about 0.001,
negatives, NaNs, random numbers; indices 0..3) from "none" or from a query's t_max (FLT_MAX, its predecessor, small numbers), settled at
the end and at random places in between, against the written-out update with its `t < FLT_MAX`: the state handed on must be the same
bits and the same index.  Zero mismatches anywhere, for forms 0, 1 and 2."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_CASES = 1_000_000


def _compile(src_root, exe, *defines):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *defines,
                           os.path.join(src_root, "tools", "check_offer_host.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    c["returncode"] = out.returncode
    return c, out.stderr


@pytest.fixture(scope="module")
def counters(tmp_path_factory):
    exe = _compile(ROOT, str(tmp_path_factory.mktemp("offer") / "check_offer_host"))
    return _run(exe, "offer", str(RANDOM_CASES), "2028")[0]


def test_the_key_compare_is_the_rule(counters):
    c = counters
    assert c["form"] == 2                      # the header's default: the 64-bit compare with `t < FLT_MAX` folded
    assert c["grid_cases"] == 10 * 3 * 3 * 4   # every combination, none left out
    assert c["grid_raw_cases"] == 336          # all but t = best = NaN (both signs: 2 x 3 x 4)
    assert c["random_cases"] >= 10 ** 6 and c["sequences"] >= 10 ** 6
    assert c["mismatches"] == 0 and c["returncode"] == 0, c


def test_the_cases_reach_ties_updates_and_the_flt_max_state(counters):
    c = counters
    assert c["grid_updates"] > 0
    assert c["none_state_flt_max"] == 6        # 3 ids x both `best` values that are FLT_MAX: what the settle step is for
    assert c["random_ties"] > 200_000 and 0 < c["random_tie_wins"] < c["random_ties"]
    assert 300_000 < c["random_updates"] < 800_000
    assert c["sequences_that_held_flt_max"] > 10_000   # walks that held (FLT_MAX, id) on the way
    assert 100_000 < c["sequences_ending_none"] < 900_000


@pytest.mark.parametrize("form", [0, 1])
def test_the_other_forms_pass_too(tmp_path, form):
    """R1_OFFER_FORM 0 (the grid kernels' form) and 1 (the compare without the fold) are the same function; neither ever holds (FLT_MAX, id)."""
    c, _ = _run(_compile(ROOT, str(tmp_path / "form"), f"-DR1_OFFER_FORM={form}"), "offer", "100000", "3")
    assert c["form"] == form and c["mismatches"] == 0 and c["returncode"] == 0, c
    assert c["sequences_that_held_flt_max"] == 0


@pytest.mark.parametrize("what", ["compare", "settle"])
def test_the_program_reports_a_wrong_rule(tmp_path, what):
    """The comparison can fail: the same program over a header whose key compare admits equal keys, and over one that never settles."""
    src = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_offer.h")).read()
    good, bad = {"compare": ("return r1_offer_key(t, id) < r1_offer_key(best, best_id);", "return r1_offer_key(t, id) <= r1_offer_key(best, best_id);"),
                 "settle": ("return FORM == 2 ? (best < FLT_MAX ? best_id : 0xFFFFFFFFu) : best_id;", "return best_id;")}[what]
    assert src.count(good) == 1
    os.makedirs(tmp_path / "rays1bench_amd" / "csrc")
    os.makedirs(tmp_path / "tools")
    (tmp_path / "rays1bench_amd" / "csrc" / "r1_offer.h").write_text(src.replace(good, bad))
    (tmp_path / "tools" / "check_offer_host.cpp").write_text(open(os.path.join(ROOT, "tools", "check_offer_host.cpp")).read())
    c, err = _run(_compile(str(tmp_path), str(tmp_path / "wrong")), "offer", "100000", "1")
    assert c["returncode"] == 1 and "MISMATCH" in err and c["mismatches"] > 1000
