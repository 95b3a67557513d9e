"""The threshold rule behind `--auto-cutoffs` without a GPU: pfh::cutoffs_from_rows (through the C facade and through the cutoffL /
cutoffU file forms) against a Python restatement of the reference's src/Main.cpp:200-277 (hist_cases.py), and the design of the
database on which the GPU tests check the switch end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import OUTPUT_SUFFIXES, ROOT

import hist_cases as hc

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

from ploidyfrost_amd import build, hostapi  # noqa: E402

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
REF = os.path.join(ROOT, "oracle", "_ref", "PloidyFrost")
QUANTILES = [0.5, 0.998, 0.999999]

ROW_SETS = {
    "abi": [900, 500, 200, 80, 60, 90, 150, 300, 420, 380, 260, 140, 70, 30, 12, 5, 2, 1],   # the histogram of test_abi_cpu.py
    "rise_at_1": [5, 9, 40, 30, 20, 10, 5, 1],
    "no_rise": [100, 90, 80, 80, 50, 20, 20, 3, 0, 0, 0],    # cutoffL answers from the row count
    "no_rise_fewer_zeros": [100, 90, 80, 80, 50, 20, 20, 3],
    "first_row_only": [1234, 0, 0, 0, 0, 0],
    "two_rows": [7, 3],
    "trailing_zeros": [900, 500, 200, 80, 60, 90, 150, 300, 420, 380, 260, 140, 70, 30, 12, 5, 2, 1, 0, 0, 0, 0],
    "past_2_32": [3 << 32, 1 << 31, 1 << 20, 5, 1 << 33, 1 << 32, 1 << 30, 77, 1],
    "valley": [300, 225, 169, 127, 95, 71, 53, 40, 30, 23, 17, 13, 351, 390, 374, 0, 0, 0, 313, 295, 296],
}


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def write_hist(path, rows, first=1):
    path.write_text("".join("%d\t%d\n" % (first + i, c) for i, c in enumerate(rows)))
    return path


@pytest.mark.parametrize("name", sorted(ROW_SETS))
def test_cutoffs_from_rows_is_the_reference_rule(name, tmp_path):
    rows = ROW_SETS[name]
    hist = write_hist(tmp_path / "hist.txt", rows)
    want_l = hc.ref_cutoff_l(rows)
    for q in QUANTILES:
        want_u = hc.ref_cutoff_u(rows, q)
        assert want_u is not None
        assert hostapi.cutoffs_from_rows(rows, q) == (want_l, want_u), (name, q)
        # the file forms call the same function: their text must not move
        assert run_cli("cutoffU", hist, repr(q)).stdout == "%d" % want_u
    assert run_cli("cutoffL", hist).stdout == "%d\n" % max(10, want_l)
    assert run_cli("cutoffU", hist).stdout == "%d\n" % hc.ref_cutoff_u(rows, 0.998)
    if os.path.exists(REF):
        for args in (["cutoffL", str(hist)], ["cutoffU", str(hist)]) + tuple(["cutoffU", str(hist), repr(q)] for q in QUANTILES):
            assert subprocess.run([REF] + args, stdout=subprocess.PIPE, text=True).stdout == run_cli(*args).stdout, args


def test_known_values():
    """worked out by hand: the restatement itself is held to the figures of test_abi_cpu.py"""
    assert (hc.ref_cutoff_l(ROW_SETS["abi"]), hc.ref_cutoff_u(ROW_SETS["abi"]), hc.ref_cutoff_u(ROW_SETS["abi"], 0.5)) == (5, 16, 8)
    assert hc.ref_cutoff_l(ROW_SETS["rise_at_1"]) == 0
    # a histogram that never rises: the loop runs off the end, the answer is 1.25 x (rows - 1) -- trailing zero rows move it
    assert hc.ref_cutoff_l(ROW_SETS["no_rise"]) == 13 and hc.ref_cutoff_l(ROW_SETS["no_rise_fewer_zeros"]) == 9
    # ... and they move nothing else
    a, b = ROW_SETS["abi"], ROW_SETS["trailing_zeros"]
    assert hc.ref_cutoff_l(a) == hc.ref_cutoff_l(b) and all(hc.ref_cutoff_u(a, q) == hc.ref_cutoff_u(b, q) for q in QUANTILES)
    assert hostapi.cutoffs_from_rows(b) == hostapi.cutoffs_from_rows(a)


def test_too_few_rows_is_the_reference_error(tmp_path):
    """cutoffH's `v.size() <= 2` (src/Main.cpp:262): v holds a leading 0 and one prefix sum per row, so a histogram of fewer than two
    rows is refused; cutoffL has no such test"""
    for rows in ([], [42]):
        assert hc.ref_cutoff_u(rows) is None
        with pytest.raises(ValueError, match="badly Formatted"):
            hostapi.cutoffs_from_rows(rows)
        hist = write_hist(tmp_path / ("hist%d.txt" % len(rows)), rows)
        r = run_cli("cutoffU", hist)
        assert r.returncode != 0 and "Error: Histogram File is badly Formatted." in r.stderr and r.stdout == ""
        assert run_cli("cutoffL", hist).stdout == "10\n"
        if os.path.exists(REF):
            ref = subprocess.run([REF, "cutoffU", str(hist)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert ref.returncode != 0 and ref.stdout == ""


@pytest.fixture(scope="module")
def oracle_lib():
    pyoracle.build()


def test_auto_cutoff_database_design(oracle_lib, tmp_path):
    """The database of the end-to-end GPU tests, proven here: its thresholds by the restated rule differ from the defaults, and the
    oracle's files at them differ from its files at 10 / 1000 without being empty."""
    meta, prefix, counts = hc.make_single(tmp_path)
    rows = np.bincount(counts)[1:]
    assert np.array_equal(rows, hc.db_rows(counts, dict(min_count=1, max_count=65535), 2)[:len(rows)])
    lower, upper = max(10, hc.ref_cutoff_l(rows)), hc.ref_cutoff_u(rows)
    assert (lower, upper) == hc.thresholds(counts)
    assert lower != 10 and upper != 1000 and lower <= upper
    outs = {}
    for name, (lo, up) in (("derived", (lower, upper)), ("default", (10, 1000))):
        d = tmp_path / name
        d.mkdir()
        pyoracle.Oracle(meta["gfa"], prefix).run(str(d), "g", z=int(meta["opts"]["-z"]), lower=lo, upper=up)
        outs[name] = {s: (d / ("g_%s.txt" % s)).read_bytes() for s in OUTPUT_SUFFIXES}
    assert any(outs["derived"][s] != outs["default"][s] for s in OUTPUT_SUFFIXES)
    assert any(outs["derived"][s] for s in OUTPUT_SUFFIXES if s.endswith("cov"))


def test_colored_databases_give_a_threshold_pair_per_colour(tmp_path):
    meta, prefixes, counts = hc.make_colored(tmp_path)
    pairs = [hc.thresholds(c) for c in counts]
    assert len(set(pairs)) == len(pairs) == meta["n_colors"]
    assert all(lo <= up and (lo, up) != (10, 1000) for lo, up in pairs)


def test_refusals_come_before_any_device_work(tmp_path):
    """--auto-cutoffs with another source of thresholds, or cut over several GPUs, is refused by name (no GPU is touched: this
    passes on a machine without one)"""
    meta, prefix, _ = hc.make_single(tmp_path)
    hist = write_hist(tmp_path / "h.txt", ROW_SETS["abi"])
    cfile = tmp_path / "c.txt"
    cfile.write_text("10\t1000\n")
    base = ["-g", meta["gfa"], "-d", prefix, "-o", "g", "--auto-cutoffs"]
    for extra, word in ((["-h", str(hist)], "-h"), (["-C", str(cfile)], "-C"), (["-l", "12"], "-l"), (["-u", "900"], "-u"),
                        (["--gpus", "2"], "--gpus 2")):
        r = subprocess.run([CLI] + base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp_path)
        assert r.returncode != 0, extra
        assert "--auto-cutoffs" in r.stderr and word in r.stderr.split("--auto-cutoffs", 1)[1], (extra, r.stderr)
        assert "CDBG" not in r.stdout and not os.path.exists(tmp_path / "PloidyFrost_output")
