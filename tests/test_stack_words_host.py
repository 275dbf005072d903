"""CPU test of the packed attenuation stack's words (rays1bench_amd/csrc/r1_stack_words.h): a stand-alone program
(tools/check_stack_words.cpp) compiles the header the kernels use for the host and compares it with the forms it replaces.

  the quotient and the shift   r1_stack_word / r1_stack_shift against sp / 3 and 10 (sp % 3) for every sp in [0, 51], and the quotient for
                               every sp below 32768, as far as the header claims it
  the pushes                   20 000 paths of 1 .. 51 entries over words of arbitrary old contents: a word opened with the pad in its upper
                               slots and merged into afterwards holds the entries the plain merge holds, and the pad above the top entry
  the fold                     the padded word — every slot multiplies, the pad's row is {0, 1, 1, 1} — against the select form, bit for bit,
                               on 10^6 random albedos, radiances (finite and infinite bit patterns among them) and fills

Zero mismatches and the exact number of cases: nothing is skipped silently.  The same program under -fsanitize=address,undefined where the
compiler has the runtimes: a program of its own, never code loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(src_root, exe, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                           os.path.join(src_root, "tools", "check_stack_words.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    c["returncode"] = out.returncode
    return c, out.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(ROOT, str(tmp_path_factory.mktemp("stack") / "check_stack_words"))


def _all_cases(c):
    assert c["slots"] == 52 and c["quotients"] == 32768 and c["folds"] == 10 ** 6
    assert 20000 <= c["pushes"] <= 20000 * 51
    assert min(c["fill0"], c["fill1"], c["fill2"]) > 300000 and c["fill0"] + c["fill1"] + c["fill2"] == c["folds"]
    assert c["mismatches"] == 0 and c["returncode"] == 0, c


def test_the_header_is_the_division_the_plain_merge_and_the_select_form(exe):
    c, _ = _run(exe)
    _all_cases(c)


def test_the_same_program_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    c, err = _run(_compile(ROOT, str(tmp_path / "check_stack_words_san"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    _all_cases(c)
    assert "runtime error" not in err and "AddressSanitizer" not in err


@pytest.mark.parametrize("what", ["word", "shift", "open", "fold"])
def test_the_program_reports_a_wrong_header(tmp_path, what):
    """The comparison can fail: the same program over a header with a multiplier one too small, a shift of 8 bits per slot, a push that
    leaves the slots above it as they were, and a fold that skips the middle slot."""
    src = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_stack_words.h")).read()
    good, bad = {"word": ("return (sp * 0x5556u) >> 16;", "return (sp * 0x5555u) >> 16;"),
                 "shift": ("return sp * 10u - w * 30u;", "return sp * 8u - w * 24u;"),
                 "open": ("return (v & ~(0xFFFFFFFFu << sh)) | ((idx | 0xFFFFFC00u) << sh);", "return (v & ~(0x3FFu << sh)) | (idx << sh);"),
                 "fold": ("col[c] = s1[c] * col[c];", "col[c] = col[c];")}[what]
    assert src.count(good) == 1
    os.makedirs(tmp_path / "rays1bench_amd" / "csrc")
    os.makedirs(tmp_path / "tools")
    (tmp_path / "rays1bench_amd" / "csrc" / "r1_stack_words.h").write_text(src.replace(good, bad))
    (tmp_path / "tools" / "check_stack_words.cpp").write_text(open(os.path.join(ROOT, "tools", "check_stack_words.cpp")).read())
    c, err = _run(_compile(str(tmp_path), str(tmp_path / "wrong")))
    assert c["returncode"] == 1 and "MISMATCH" in err and c["mismatches"] > 0
