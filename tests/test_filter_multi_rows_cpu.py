"""The multi row filter in front of the model (`--filter-multi`, the colored tables), the part that needs no GPU: the shared rule
(csrc/pf_filter_rows.hpp with FilterRule::multi -- the code the kernels of pf_call_model.hip run with a lane per row, exported as
pfh_filter_rows_multi) against the chain it stands for: `ploidyfrost filter-multi` (host/pf_filter.cpp, the definition) and then
the file readers of `ploidyfrost model`."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case
from filter_multi_cases import (CLI, EACH, HAND, HAND_COLOURS, HAND_SCI, HAND_WORDS, KEPT_COL4_MIX, ONE_COLOUR, POOLED, R_ERROR, SCI_WORDS, TABLES,
                                chain_values, kept_rows, read_tables, run_filter_multi, with_colour, write_tables)

from ploidyfrost_amd import build, hipapi, hostapi


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def compare_with_chain(prefix, words, kw, tmp_path, sources=("cov", "fre"), qs=(0.0, 0.05)):
    """the rule's array == the readers on what filter-multi wrote; where the chain stops with R's error, the rule stops with the same
    words.  Returns the number of values compared (0 when the chain stopped)."""
    texts = read_tables(prefix)
    filtered = str(tmp_path / "f")
    stopped = None
    try:
        run_filter_multi(prefix, words, filtered)
    except RuntimeError as e:
        stopped = str(e)
    n = 0
    for source in sources:
        for q in qs:
            if stopped is not None:
                with pytest.raises(RuntimeError) as e:
                    hostapi.filter_rows(source, texts, q, multi=True, **kw)
                assert R_ERROR in stopped and str(e.value) in stopped, (stopped, str(e.value))
                continue
            exp = chain_values(filtered, source, q)
            got = hostapi.filter_rows(source, texts, q, multi=True, **kw)
            assert got.dtype == np.float64 and len(got) == len(exp), (words, source, q, len(got), len(exp))
            assert np.array_equal(got, exp), (words, source, q)
            n += len(exp)
    return n


# ---- 1. the colored fixtures ----
@pytest.mark.parametrize("case", ["col3_dip", "col4_mix", "col100"])
@pytest.mark.parametrize("words,kw", [ONE_COLOUR, POOLED, EACH], ids=["one_colour", "pooled", "each_pooled"])
def test_rule_equals_filter_multi_and_the_readers_on_the_fixtures(case, words, kw, tmp_path):
    meta = load_case(case)
    assert compare_with_chain(os.path.join(meta["dir"], "expected", "g"), words, kw, tmp_path) > 0


@pytest.mark.parametrize("case", ["col3_dip", "col4_mix", "col100"])
def test_rule_equals_the_chain_colour_by_colour(case, tmp_path):
    meta = load_case(case)
    prefix = os.path.join(meta["dir"], "expected", "g")
    fitted = 0
    for c in range(meta["n_colors"]):
        words, kw = with_colour(*EACH, c)
        n = compare_with_chain(prefix, words, kw, tmp_path, qs=(0.0,))
        assert (n > 0) == (kept_rows(prefix, kw) > 0)
        fitted += n > 0
    assert fitted == (3 if case == "col4_mix" else meta["n_colors"])


def test_counts_the_fixtures_give():
    """what the GPU tests rely on: the option sets keep rows, and how many"""
    dip, mix, c100 = (os.path.join(load_case(c)["dir"], "expected", "g") for c in ("col3_dip", "col4_mix", "col100"))
    bi = ("bicov",)
    assert kept_rows(dip, ONE_COLOUR[1], bi) == 70 and len(read_tables(dip)[0].splitlines()) == 253
    assert kept_rows(mix, ONE_COLOUR[1], bi) == 180 and len(read_tables(mix)[0].splitlines()) == 453
    assert all(66 <= kept_rows(dip, dict(EACH[1], color=c)) <= 70 for c in range(3))
    assert tuple(kept_rows(mix, dict(EACH[1], color=c), bi) for c in range(4)) == KEPT_COL4_MIX
    assert tuple(kept_rows(mix, dict(EACH[1], color=c), ("tricov",)) for c in range(4)) == (1, 0, 0, 1)
    assert all(6 <= kept_rows(c100, dict(EACH[1], color=c)) <= 12 for c in range(100))
    assert kept_rows(dip, POOLED[1]) > 0 and kept_rows(mix, POOLED[1]) > 0


# ---- 2. hand-made colored tables ----
def test_rule_equals_the_chain_on_hand_made_tables(tmp_path):
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND)
    assert compare_with_chain(prefix, *HAND_WORDS, tmp_path) > 0
    for c in HAND_COLOURS:
        n = compare_with_chain(prefix, *with_colour(*HAND_WORDS, c), tmp_path)
        assert (n > 0) == (c != 2), c   # colour 2 keeps nothing and the others do: R's error for it alone
    assert compare_with_chain(prefix, "-v 0.25 -l 5 -u 1000 -S -I -n 2 -d 8 -s 1 -q 0.25",
                              dict(cramer=0.25, low=5, up=1000, simple=True, indel=True, num=2, distance=8, size=1, frequency=0.25), tmp_path) > 0


def test_hand_made_tables_by_hand():
    texts = [HAND[t].encode() for t in TABLES]
    kw = HAND_WORDS[1]
    # colour 70: bi row 3 (row 4 has Cramer's V == -v: dropped), tri row 2, penta row 2 (its 10 / 1050 is not above 0.05)
    got = hostapi.filter_rows("fre", texts, 0.0, multi=True, color=70, **kw)
    p = 0.2476190
    assert list(got) == [0.5, 0.5, 0.5, 0.25, 0.25, p, p, p, p, p]
    assert list(hostapi.filter_rows("cov", texts, 0.0, multi=True, color=70, **kw)) == [0.5, 0.5, 40 / 80, 20 / 80, 20 / 80]
    # the threshold is strict
    assert list(hostapi.filter_rows("fre", texts, 0.0, multi=True, color=70, **dict(kw, cramer=0.2499))) == [0.5, 0.4, 0.5, 0.6, 0.5, 0.25, 0.25, p, p, p, p, p]
    # colour 0 keeps the tetra row whose first four coverages sum to 1200 >= -u 1000; the single-sample rule drops such a row
    only = [b"", b"", TETRACOV_ROW2.encode(), b""]
    assert list(hostapi.filter_rows("fre", only, 0.0, multi=True, **kw)) == [0.25] * 5
    single = [b"", b"", b"300\t300\t300\t300\t1\t0\t14\t1\t30\t\n", b""]
    with pytest.raises(RuntimeError, match=R_ERROR):
        hostapi.filter_rows("fre", single, 0.0, low=5, up=1000)
    penta = [b"", b"", b"", HAND["pentacov"].splitlines(True)[1].encode()]
    assert list(hostapi.filter_rows("fre", penta, 0.0, multi=True, **kw)) == [p] * 5
    single = [b"", b"", b"", b"260\t260\t260\t260\t10\t1\t0\t16\t1\t30\t\n"]   # the same penta row in the single-sample layout (A + 5)
    with pytest.raises(RuntimeError, match=R_ERROR):
        hostapi.filter_rows("fre", single, 0.0, low=5, up=1000)
    assert list(hostapi.filter_rows("fre", single, 0.0, low=5, up=1041)) == [p] * 5   # (kept once -u is above the sum 1040)
    # all four tables empty
    with pytest.raises(RuntimeError, match=R_ERROR):
        hostapi.filter_rows("fre", [b"", b"", b"", b""], 0.0, multi=True, **kw)


TETRACOV_ROW2 = HAND["tetracov"].splitlines(True)[1]


def test_all_four_tables_empty_is_rs_error_on_both_sides(tmp_path):
    prefix = str(tmp_path / "in")
    write_tables(prefix, dict.fromkeys(TABLES, ""))
    with pytest.raises(RuntimeError, match=R_ERROR):
        run_filter_multi(prefix, HAND_WORDS[0], str(tmp_path / "f"))
    for source in ("cov", "fre"):
        with pytest.raises(RuntimeError, match=R_ERROR):
            hostapi.filter_rows(source, read_tables(prefix), 0.0, multi=True, **HAND_WORDS[1])


def test_a_kept_coverage_r_prints_in_scientific_notation_is_refused_for_cov_and_fine_for_fre(tmp_path):
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND_SCI)
    words, kw = with_colour(*SCI_WORDS, 1)
    assert compare_with_chain(prefix, words, kw, tmp_path, sources=("fre",)) > 0
    with pytest.raises(RuntimeError) as e:
        hostapi.filter_rows("cov", read_tables(prefix), 0.0, multi=True, **kw)
    assert "scientific notation" in str(e.value) and "row 10 of stream _bicov" in str(e.value)
    # under -u 1000 the row is dropped and both sources go through
    assert compare_with_chain(prefix, *with_colour(*HAND_WORDS, 1), tmp_path) > 0


def test_a_nan_cramer_cell_and_a_short_row_are_refused_with_the_filters_words(tmp_path):
    nan = dict(HAND, tricov=HAND["tricov"].replace("\t0.3\t11\t", "\t-nan\t11\t"))
    short = dict(HAND, bicov=HAND["bicov"] + "30\t30\t0\t1\t0\t19\t1\t\n")   # A + 5 fields
    for tables, words_in_both, named in ((nan, ("in line 2 of", "is not a finite decimal number", "refused (parity unpinned)"), "stream _tricov"),
                                         (short, ("Error in scan(", "line 10 did not have 9 elements"), "stream _bicov")):
        prefix = str(tmp_path / "in")
        write_tables(prefix, tables)
        with pytest.raises(RuntimeError) as chain:
            run_filter_multi(prefix, HAND_WORDS[0] + " -c 3", str(tmp_path / "f"))   # (a colour the refused row is not of)
        for source in ("cov", "fre"):
            with pytest.raises(RuntimeError) as e:
                hostapi.filter_rows(source, read_tables(prefix), 0.0, multi=True, color=3, **HAND_WORDS[1])
            for word in words_in_both:
                assert word in str(chain.value) and word in str(e.value), (word, str(chain.value), str(e.value))
            assert named in str(e.value)


def test_the_rule_under_address_and_ub_sanitizers_as_a_stand_alone_program(tmp_path):
    """the shared header is plain C++: a program with its own main runs it over the hand tables, every row in a heap buffer of
    exactly its length, under -fsanitize=address,undefined (host code only; nothing of this is loaded into Python or run on a GPU)"""
    exe = str(tmp_path / "rule")
    host = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", host,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_filter_multi_rule.cpp"), "-o", exe], check=True)
    tables = dict(HAND_SCI, pentacov=HAND_SCI["pentacov"] + "1\t2\t3\t\n-nan\t\n\n")
    prefix = str(tmp_path / "in")
    write_tables(prefix, tables)
    want = {"bicov": "5 10 0", "tricov": "2 6 0", "tetracov": "2 8 0", "pentacov": "3 10 5"}   # kept rows, frequencies written, first refusal
    for t, name in enumerate(TABLES):
        r = subprocess.run([exe, str(t), "-1", "0.25", "5", "1000", "%s_%s.txt" % (prefix, name)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr)
        assert r.stdout.strip() == want[name], (name, r.stdout)


# ---- 3. names ----
def test_entry_points_are_declared_and_exported():
    def declared(header):
        with open(os.path.join(ROOT, "include", header)) as f:
            return set(re.findall(r"\b(pfh?_[a-z0-9_]+)\s*\(", f.read()))

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        return set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    dev = {"pf_call_model_filter_multi", "pf_call_model_color_count", "pf_call_model_color_select"}
    host = {"pfh_set_filter_multi", "pfh_filter_rows_multi", "pfh_model_color_count", "pfh_model_color_at", "pfh_model_color_values", "pfh_model_color_fit",
            "pfh_model_color_ploidy"}
    assert dev <= declared("ploidyfrost_hip.h") and dev <= exported(hipapi.LIB_PATH) and dev <= set(hipapi.DECLARED_SYMBOLS)
    assert host <= declared("ploidyfrost_host.h") and host <= exported(hostapi.LIB_PATH) and host <= set(hostapi.DECLARED_SYMBOLS)
    for name in ("set_filter_multi", "model_colors", "model_values", "model_result"):
        assert hasattr(hostapi.ColoredRun, name)
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        assert "pf_filter_multi_opts" in f.read()
    with pytest.raises(RuntimeError, match="frequency should < 0.5"):
        hostapi.filter_rows("fre", [b"", b"", b"", b""], 0.0, multi=True, frequency=0.6)


# ---- 4. the command line says no before it reads anything ----
COLORED = ["-f", "graph.bfg_colors"]


@pytest.mark.parametrize("extra,word", [
    (["--model", "fre", "--filter-multi", "-v 0.25"], "-f"),
    (COLORED + ["--filter-multi", "-v 0.25"], "--model"),
    (COLORED + ["--model", "fre", "--model-each-color"], "--filter-multi"),
    (COLORED + ["--model", "fre", "--filter-multi", "-v 0.25 -c 2", "--model-each-color"], "-c 2"),
    (COLORED + ["--model", "fre", "--filter-multi", "-q 0.6"], "-q 0.6"),
    (COLORED + ["--model", "fre", "--filter-multi", "-i x"], "-i"),
    (COLORED + ["--model", "fre", "--filter-multi", "-o x"], "-o"),
    (COLORED + ["--model", "fre", "--filter-multi", "-v 0.25", "--gpus", "2"], "--gpus"),
    (COLORED + ["--model", "fre", "--filter-multi", "-v 0.25", "--filter", "-S"], "--filter"),
    (COLORED + ["--model", "cov"], "--filter-multi"),      # the refusal of --model with -f now says where to go
])
def test_refusals_name_the_option_and_write_nothing(extra, word, tmp_path):
    meta = load_case("col3_dip")
    r = subprocess.run([CLI, "-g", meta["gfa"], "-d", "dbs.txt", "-o", "g"] + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.startswith("Error:") and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert ("--filter-multi" in r.stderr or "--model-each-color" in r.stderr) and os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra,word", [
    (["--model-each-color"], "--filter-multi"),
    (["--filter-multi", "-v 0.25 -c 2", "--model-each-color"], "-c 2"),
    (["--filter-multi", "-v 0.25", "--filter", "-S"], "--filter"),
    (["--filter-multi", "-o x"], "-o"),
])
def test_model_from_files_refuses_by_name(extra, word, tmp_path):
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND)
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([CLI, "model", "-f", prefix, "-o", "one"] + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == before
