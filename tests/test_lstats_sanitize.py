"""host/lstats.c and host/netbuild.c under -fsanitize=address,undefined: a stand-alone program (tests/lstats_sanitize.c) runs the
planted-count cases on the CPU as a child process; nothing is loaded into Python.  What it writes is the reference's bytes."""
import os
import subprocess

import pytest

import lm_cases as lc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lstats_san") / "lstats_sanitize")
    host = os.path.join(ROOT, "htk_amd", "host")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "lstats_sanitize.c")] +
                          [os.path.join(host, f) for f in ("lstats.c", "netbuild.c", "slfout.c", "labio.c", "htktext.c")] + ["-o", out, "-lm"])
    return out


@pytest.mark.parametrize("case", ["toy", "rand12"])
def test_planted_cases_under_sanitizers(exe, case, tmp_path):
    d = lc.load_case(case)[0]
    r = subprocess.run([exe, d, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("lists.out", "lists.list", "lists.bigram", "mat_f001.bigram", "mat_f001.out"):
        assert (tmp_path / name).read_bytes() == open(os.path.join(d, name), "rb").read(), name
    if case == "toy":
        assert (tmp_path / "loop_t.slf").read_bytes() == open(os.path.join(d, "loop_t.slf"), "rb").read()
