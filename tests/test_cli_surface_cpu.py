"""The command line of the nine reads sub-commands and the dispatch in main(), byte for byte: every line of
tests/golden/cli/surface.json (tests/golden/make_cli_golden.py enumerates them) gives the exit status, the stdout and the stderr
recorded there.  Every line ends before a device context exists, so nothing here needs a GPU.  The fixture changes only in a
change that means to alter the command line."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

from ploidyfrost_amd import build

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
with open(os.path.join(ROOT, "tests", "golden", "cli", "surface.json")) as f:
    SURFACE = json.load(f)
SUBS = ["count", "build", "build-multi", "mask", "smudge", "qc", "trim", "run", "run-multi", "main"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def test_fixture_names_every_sub_command():
    assert sorted(SURFACE["cases"]) == sorted(SUBS) and sorted(SURFACE["usage"]) == sorted(SUBS[:-1])
    assert len(SURFACE["commit"]) == 40
    assert all(len(SURFACE["cases"][s]) >= 10 for s in SUBS)


@pytest.mark.parametrize("sub", SUBS)
def test_every_line_says_what_was_recorded(sub, tmp_path):
    cases = SURFACE["cases"][sub]
    usage = SURFACE["usage"].get(sub, "")
    valid_word, valid = SURFACE["markers"]["valid"], SURFACE["valid"].get(sub, [])
    env = dict(os.environ, LC_ALL="C", LANG="C")

    def run(case):
        argv = [w for a in case[0] for w in (valid if a == valid_word else [a])]
        r = subprocess.run([CLI] + argv, cwd=tmp_path, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        return r.returncode, r.stdout.decode("utf-8", "surrogateescape"), r.stderr.decode("utf-8", "surrogateescape")

    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(run, cases))
    wrong = []
    for case, g in zip(cases, got):
        # [argv, why]: the sub-command's own refusal; [argv, exit status, stdout, stderr]: every other line
        want = (1, "", "Error: %s: %s\n%s" % (sub, case[1], usage)) if len(case) == 2 else tuple(case[1:])
        if g != want:
            wrong.append((case[0], g, want))
    assert not wrong, "%d of %d lines differ; the first: %r\n gives    %r\n recorded %r" % ((len(wrong), len(cases)) + wrong[0])
    assert not os.listdir(tmp_path)
