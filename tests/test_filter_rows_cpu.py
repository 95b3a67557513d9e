"""The row filter in front of the model, the part that needs no GPU: the shared rule (csrc/pf_filter_rows.hpp -- the code the kernels
of pf_call_model.hip run with a lane per row, exported as pfh_filter_rows) against the three-command chain it stands for:
`ploidyfrost filter` (host/pf_filter.cpp, the definition) and then the file readers of `ploidyfrost model`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_cases, load_case
from filter_cases import (DEFAULT_SET, HAND_SETS, HAND_TABLES, OPTION_SETS, R_ERROR, TABLES, chain_values, read_tables, run_filter,
                          write_tables)

from ploidyfrost_amd import build, hipapi, hostapi


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


# ---- 1. the scaled rounding ----
@pytest.fixture(scope="module")
def round7(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("round7") / "test_filter_round7")
    host = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", host, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_filter_round7.cpp"), os.path.join(host, "pf_filter.cpp"), "-o", exe], check=True)
    return exe


# every c / s with 0 <= c <= s <= 6000 (18 M cases in three parts of about equal size), and the doubles within 3 ulp of the
# 200 000 exact ties (n + 0.5) / 1e7
@pytest.mark.parametrize("args,cases", [
    (["fractions", "1", "3500"], 3500 * 3501 // 2 + 3500),
    (["fractions", "3501", "4950"], sum(s + 1 for s in range(3501, 4951))),
    (["fractions", "4951", "6000"], sum(s + 1 for s in range(4951, 6001))),
    (["ties", "200000"], 200000 * 7),
])
def test_scaled_rounding_is_the_long_double_path_and_the_value_is_what_the_chain_reads(round7, args, cases):
    r = subprocess.run([round7] + args, stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % cases, r.stdout


# ---- 2. every golden case ----
def compare_with_chain(prefix, words, kw, tmp_path, cov_refused=False):
    """both sources, model q of 0 and 0.05: the rule's array == the readers on what the filter wrote; where the chain stops, the
    rule stops with the same words"""
    texts = read_tables(prefix)
    filtered = str(tmp_path / "f")
    stopped = None
    try:
        run_filter(prefix, words, filtered)
    except RuntimeError as e:
        stopped = str(e)
    for source in ("cov", "fre"):
        for q in (0.0, 0.05):
            if stopped is not None:
                with pytest.raises(RuntimeError) as e:
                    hostapi.filter_rows(source, texts, q, **kw)
                assert R_ERROR in stopped and str(e.value) in stopped, (stopped, str(e.value))
                continue
            if source == "cov" and cov_refused:
                with pytest.raises(RuntimeError) as e:
                    hostapi.filter_rows(source, texts, q, **kw)
                assert "scientific notation" in str(e.value) and "three-command chain" in str(e.value) and "of stream _bicov" in str(e.value)
                continue
            refusal = None
            try:
                exp = chain_values(filtered, source, q)
            except RuntimeError as e:
                refusal = str(e)
            if refusal is not None:   # (a kept row that sums to 0: `model -f` stops)
                with pytest.raises(RuntimeError) as e:
                    hostapi.filter_rows(source, texts, q, **kw)
                assert "sums to 0" in refusal and "sums to 0" in str(e.value), (refusal, str(e.value))
                continue
            got = hostapi.filter_rows(source, texts, q, **kw)
            assert got.dtype == np.float64 and len(got) == len(exp), (source, q, len(got), len(exp))
            assert np.array_equal(got, exp), (source, q)
    return stopped


@pytest.mark.parametrize("case", golden_cases())
@pytest.mark.parametrize("words,kw,kept", OPTION_SETS + [DEFAULT_SET], ids=[s[0].replace(" ", "") or "defaults" for s in OPTION_SETS + [DEFAULT_SET]])
def test_rule_equals_the_host_filter_and_the_readers_on_every_golden_case(case, words, kw, kept, tmp_path):
    meta = load_case(case)
    stopped = compare_with_chain(os.path.join(meta["dir"], "expected", "g"), words, kw, tmp_path)
    if case in kept:
        rows = tuple(len(open(str(tmp_path / ("f_%s.txt" % t))).read().splitlines()) for t in TABLES[:3])
        assert rows == kept[case]
        assert (stopped is not None) == (sum(rows) == 0)


def test_a_kept_row_that_sums_to_zero_is_the_readers_error(tmp_path):
    """stranded20k has rows of zero coverage: -l 0 drops them (0 > 0 fails); with -l -1 they are kept, `model -f` stops at the first,
    and the frequencies 0 / 0 pass no test"""
    meta = load_case("stranded20k")
    prefix = os.path.join(meta["dir"], "expected", "g")
    assert any(ln.startswith("0\t0\t") for ln in open(prefix + "_bicov.txt"))
    compare_with_chain(prefix, "-l -1", dict(low=-1), tmp_path)
    with pytest.raises(RuntimeError, match="sums to 0"):
        hostapi.filter_rows("cov", read_tables(prefix), 0.0, low=-1)


# ---- 3. hand-made tables ----
@pytest.mark.parametrize("tables,words,kw,cov_refused", HAND_SETS, ids=[s[0] + s[1].replace(" ", "") for s in HAND_SETS])
def test_rule_equals_the_host_filter_on_hand_made_tables(tables, words, kw, cov_refused, tmp_path):
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND_TABLES[tables])
    assert compare_with_chain(prefix, words, kw, tmp_path, cov_refused) is None


def test_hand_made_tables_by_hand(tmp_path):
    texts = [HAND_TABLES["hand"][t].encode() for t in TABLES]
    # -l 5 -u 1000: bi rows 1-3, 9, 10; both tri rows; tetra row 1; penta rows 1 and 3.  Column by column, then the last token again.
    got = hostapi.filter_rows("fre", texts, 0.0, low=5, up=1000)
    bi_a = [0.5023965, 0.8363333, 0.5, 0.25, 0.07]
    bi_b = [0.4976035, 0.1636667, 0.5, 0.75, 0.93]
    tri = [0.3333333, 0.5, 0.3333333, 0.25, 0.3333333, 0.25]
    penta = [0.2, 0.2, 0.2, 0.2, 0.2, 0.9]   # row 3: 0.01, 0.02, 0.03 and 0.04 are not above 0.05
    assert list(got) == bi_a + bi_b + tri + [0.25] * 4 + penta + [0.9]
    # -q 0.25: a frequency equal to the bound goes (bi row 9 entirely; the tetra row; the penta 0.2s)
    got = hostapi.filter_rows("fre", texts, 0.0, low=5, up=1000, frequency=0.25)
    assert list(got) == [0.5023965, 0.5] + [0.4976035, 0.5] + [0.3333333, 0.5, 0.3333333, 0.3333333] + [0.3333333]
    # cov with the model's q = 0: the integer frequency test keeps every row whose integers do not sum to 10000 or more
    got = hostapi.filter_rows("cov", texts, 0.0, low=5, up=20000)
    assert list(got[:4]) == [60 / 119, 59 / 119, 100 / 119, 19 / 119] and 6000 / 11000 not in got
    # only the penta table keeps rows: nothing for cov (`model -f` never reads it), its frequencies for fre
    texts = [HAND_TABLES["only_penta"][t].encode() for t in TABLES]
    assert len(hostapi.filter_rows("cov", texts, 0.0, simple=True, up=1000)) == 0
    assert list(hostapi.filter_rows("fre", texts, 0.0, simple=True, up=1000)) == penta + [0.9]
    # the model's own test comes behind the filter's: the last token counts twice only when it passes
    assert list(hostapi.filter_rows("fre", texts, 0.3, simple=True, up=1000)) == []


@pytest.mark.parametrize("cell", ["nan", "-nan", "inf", "NA", "0x1p3"])
def test_a_cell_the_filter_refuses_is_refused_by_stream_and_line_kept_or_not(tmp_path, cell):
    tables = dict(HAND_TABLES["hand"])
    lines = tables["tricov"].splitlines()
    f = lines[1].split("\t")
    f[5] = cell   # VarId of a row -S would drop anyway: read_table reads every cell first
    lines[1] = "\t".join(f)
    tables["tricov"] = "\n".join(lines) + "\n"
    prefix = str(tmp_path / "in")
    write_tables(prefix, tables)
    with pytest.raises(RuntimeError) as chain:
        run_filter(prefix, "-S -l 5 -u 1000", str(tmp_path / "f"))
    for source in ("cov", "fre"):
        with pytest.raises(RuntimeError) as e:
            hostapi.filter_rows(source, read_tables(prefix), 0.0, simple=True, low=5, up=1000)
        for word in ("in line 2 of", "is not a finite decimal number", "refused (parity unpinned)"):
            assert word in str(chain.value) and word in str(e.value), (word, str(chain.value), str(e.value))
        assert "_tricov" in str(chain.value) and "stream _tricov" in str(e.value)


def test_a_row_without_its_fields_is_scans_error(tmp_path):
    tables = dict(HAND_TABLES["hand"])
    tables["tetracov"] = tables["tetracov"] + "20\t20\t20\t20\t1\t0\t9\t1\t\n"
    prefix = str(tmp_path / "in")
    write_tables(prefix, tables)
    with pytest.raises(RuntimeError) as chain:
        run_filter(prefix, "-l 5 -u 1000", str(tmp_path / "f"))
    with pytest.raises(RuntimeError) as e:
        hostapi.filter_rows("fre", read_tables(prefix), 0.0, low=5, up=1000)
    for word in ("Error in scan(", "line 3 did not have 9 elements"):
        assert word in str(chain.value) and word in str(e.value)
    assert "stream _tetracov" in str(e.value)


def test_entry_points_are_declared_and_exported():
    import re

    def declared(header):
        with open(os.path.join(ROOT, "include", header)) as f:
            return set(re.findall(r"\b(pfh?_[a-z0-9_]+)\s*\(", f.read()))

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        return set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    dev = {"pf_call_model_filter", "pf_call_model_take_text"}
    host = {"pfh_set_filter", "pfh_filter_rows"}
    assert dev <= declared("ploidyfrost_hip.h") and dev <= exported(hipapi.LIB_PATH) and dev <= set(hipapi.DECLARED_SYMBOLS)
    assert host <= declared("ploidyfrost_host.h") and host <= exported(hostapi.LIB_PATH) and host <= set(hostapi.DECLARED_SYMBOLS)
    assert hasattr(hostapi.Run, "set_filter") and hasattr(hostapi, "filter_rows")
    with pytest.raises(RuntimeError, match="frequency should < 0.5"):
        hostapi.filter_rows("fre", [b"", b"", b"", b""], 0.0, frequency=0.6)
