"""The rule of the heterozygous k-mer pairs (K-HETPAIR, `smudge`, `run --smudge`) without a GPU: the host's plain restatement
(pfh_hetpairs_host / pfh_smudge_report_text, csrc/pf_hetpair_rule.hpp) against the Python restatement of hetpair_cases.py on every small
case, the facts the rule is built on (self-neighbours, doubled neighbours, symmetry), the report of a small table as literal bytes, the
four labels worked by hand, the tie-break of the proposed ploidy, the refusals of the sub-commands by their words, the stand-alone
program tests/cpp/test_hetpair_rule.cpp under the sanitizers, and the declarations."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hetpair_cases as hp

from ploidyfrost_amd import build, hipapi, hostapi, synth

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def cases():
    return hp.small_cases()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def same(got, want):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    for f in ("pair_x", "pair_y", "cov_x", "cov_y"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["table"], want["table"]), np.argwhere(got["table"] != want["table"])[:8]


# ---- the rule ----

def test_the_facts_the_rule_is_built_on():
    k5 = hp.all_canonical(5)
    assert len(k5) == 512 and sum(x in hp.neighbours(x, 5) for x in k5) == 32
    assert hp.canon(hp.enc("ACTGT"), 5) == hp.enc("ACAGT") and hp.enc("ACAGT") in hp.neighbours(hp.enc("ACAGT"), 5)
    k4 = hp.all_canonical(4)
    doubled = sum(1 for x in k4 for y in set(hp.neighbours(x, 4)) if y != x and hp.neighbours(x, 4).count(y) > 1)
    assert doubled == 96 and hp.neighbours(hp.enc("AATT"), 4).count(hp.enc("AAAT")) == 2
    for k, keys in ((4, k4), (5, k5)):   # the relation is symmetric
        nb = {x: set(hp.neighbours(x, k)) for x in keys}
        assert all(x in nb[y] for x in keys for y in nb[x])


def test_host_rule_matches_the_python_rule_on_every_case(cases):
    for name, (km, ct, k, lo, hi) in cases.items():
        want = hp.hetpairs(km, ct, k, lo, hi)
        same(hostapi.hetpairs_host(km, ct, k, lo, hi), want)
        assert want["stats"]["kmers"] == len(km), name


def test_the_cases_hold_what_they_are_made_for(cases):
    r = {name: hp.hetpairs(*c)["stats"] for name, c in cases.items()}
    assert r["k5_all"] == {"kmers": 512, "in_range": 512, "one_partner": 0, "many_partners": 512, "pairs": 0}
    assert r["k5_every_second_out"]["in_range"] == 256
    assert r["k4_aatt"]["pairs"] == 1 and any(r["k4_subset%d" % j]["pairs"] for j in range(3))
    km, ct, k, lo, hi = cases["hap_k25"]
    h = hp.hetpairs(km, ct, k, lo, hi)
    assert len(km) == 3701 and h["stats"]["pairs"] == 29 * 25 == int(h["table"][20 - lo, 20 - lo])
    assert r["hap_k31"]["pairs"] == 29 * 31 and r["hap_k17"]["pairs"] == 29 * 17 and r["hap_k18"]["pairs"] == 29 * 18
    assert r["triallelic"]["pairs"] == 0 and r["triallelic"]["many_partners"] == 3 * 21
    assert r["two_close"]["pairs"] == 2 * 10 and r["two_close"]["one_partner"] == 4 * 10   # the windows over one substitution alone
    assert r["edges"]["pairs"] == 3 * 21 - 2   # lo and hi stay pairs, lo - 1 and hi + 1 do not
    assert r["w1"]["pairs"] == 21 and r["w4096"]["pairs"] == 21
    assert [r["n%d" % n]["kmers"] for n in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]
    assert [r["in_range%d" % n]["in_range"] for n in (15, 16, 17)] == [15, 16, 17]


def test_host_rule_refuses_its_arguments_by_name():
    km, ct = np.array([1], dtype=np.uint64), np.array([5], dtype=np.uint32)
    for k, lo, hi, word in ((25, 0, 10, "lower bound is below 1"), (25, 11, 10, "lower bound is above the upper bound"),
                            (25, 1, 4097, "above 4096"), (2, 1, 10, "k goes from 3 to 31"), (32, 1, 10, "k goes from 3 to 31")):
        with pytest.raises(ValueError, match=word):
            hostapi.hetpairs_host(km, ct, k, lo, hi)
    hostapi.hetpairs_host(km, ct, 25, 1, 4096)   # W = 4096 is the cap itself


# ---- the summary and the report ----

def test_the_four_labels_by_hand():
    for (a, b), want in (((20, 20), (2, 1, "AB")), ((20, 40), (3, 1, "AAB")), ((20, 60), (4, 1, "AAAB")), ((40, 40), (4, 2, "AABB"))):
        assert hp.smudge_of(a, b, 20) == want == hostapi.smudge_of(a, b, 20)
    for a in range(1, 60):   # the two restatements, and the clamps
        for b in range(a, 200, 7):
            for n in (1, 7, 20, 33):
                p, m, label = hostapi.smudge_of(a, b, n)
                assert (p, m, label) == hp.smudge_of(a, b, n) and 2 <= p <= 16 and 1 <= m <= p // 2 and len(label) == p


REPORT = b"""# ploidyfrost smudge 1
# k 21 lower 10 upper 70 n 20
>>totals
kmers\tin_range\tone_partner\tmany_partners\tpairs
100\t40\t30\t2\t12
>>table
cov_a\tcov_b\tpairs
19\t21\t3
20\t20\t4
20\t40\t3
40\t40\t2
>>total
cov_a+cov_b\tpairs
40\t7
60\t3
80\t2
>>smudges
label\tp\tm\tpairs
AB\t2\t1\t7
AAB\t3\t1\t3
AABB\t4\t2\t2
>>proposed
p\tlabel\tpairs
2\tAB\t7
"""


def small_table():
    t = np.zeros((61, 61), dtype=np.uint64)
    for a, b, c in ((19, 21, 3), (20, 20, 4), (20, 40, 3), (40, 40, 2)):
        t[a - 10, b - 10] = c
    return t, {"kmers": 100, "in_range": 40, "one_partner": 30, "many_partners": 2, "pairs": 12}


def test_report_of_a_small_table_as_literal_bytes():
    t, st = small_table()
    assert hostapi.smudge_report(t, st, 21, 10, 70, 20) == REPORT == hp.report(t, st, 21, 10, 70, 20)
    cut = REPORT[: REPORT.index(b">>smudges")].replace(b" n 20\n", b" n 0\n")
    assert hostapi.smudge_report(t, st, 21, 10, 70) == cut == hp.report(t, st, 21, 10, 70)
    empty = np.zeros((61, 61), dtype=np.uint64)
    assert hostapi.smudge_report(empty, st, 21, 10, 70, 20).endswith(b">>smudges\nlabel\tp\tm\tpairs\n>>proposed\np\tlabel\tpairs\n0\tnone\t0\n")
    assert hostapi.smudge_report(empty, st, 21, 10, 70, 20) == hp.report(empty, st, 21, 10, 70, 20)


def test_tie_break_of_the_proposed_ploidy():
    st = small_table()[1]
    for cells, want in (({(20, 20): 5, (20, 40): 5, (40, 40): 5}, b"2\tAB\t5\n"),        # ties go to the smaller p
                        ({(20, 60): 5, (40, 40): 5, (20, 20): 4}, b"4\tAAAB\t5\n"),       # ... then to the smaller m
                        ({(20, 60): 5, (40, 40): 6, (20, 20): 4}, b"4\tAABB\t6\n")):
        t = np.zeros((61, 61), dtype=np.uint64)
        for (a, b), c in cells.items():
            t[a - 10, b - 10] = c
        text = hostapi.smudge_report(t, st, 21, 10, 70, 20)
        assert text.endswith(b">>proposed\np\tlabel\tpairs\n" + want) and text == hp.report(t, st, 21, 10, 70, 20)


# ---- the sub-commands ----

def test_refusals_by_name(tmp_path):
    (km, ct), k = hp.haplotypes(25), 25
    synth.write_kmc1(str(tmp_path / "db"), km, ct, k)
    synth.write_kmc1(str(tmp_path / "dbb"), km, ct, k, both_strands=False)
    fq, fa = tmp_path / "in.fq", tmp_path / "in.fa"
    fq.write_bytes(b"@r\n" + hp.genome(60, 1).encode() + b"\n+\n" + b"I" * 60 + b"\n")
    fa.write_bytes(b">a\nACGT\n")
    before = sorted(os.listdir(tmp_path))
    d = ["smudge", "-d", tmp_path / "db"]
    kk = ["smudge", "-k", 25, "-i", fq]
    run1 = ["run", "-i", fq, "-o", "s"]
    cases = [
        (d + ["-k", 25, "-l", 10, "-u", 100, "-o", "out"], "-d does not go with -k"),
        (["smudge", "-l", 10, "-u", 100, "-o", "out"], "-d <KMCDatabase> or -k <k> with -i <reads.fq> is missing"),
        (d + ["-l", 10, "-u", 100, "--auto-cutoffs", "-o", "out"], "-l does not go with --auto-cutoffs"),
        (d + ["-u", 100, "--auto-cutoffs", "-o", "out"], "-u does not go with --auto-cutoffs"),
        (d + ["-o", "out"], "the bounds are missing"),
        (d + ["-l", 10, "-o", "out"], "the bounds are missing"),
        (d + ["-l", 0, "-u", 100, "-o", "out"], "the lower bound is below 1"),
        (d + ["-l", 11, "-u", 10, "-o", "out"], "-l 11 is above -u 10 (L > U)"),
        (d + ["-l", 10, "-u", 4106, "-o", "out"], "above 4096"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "-n", 0], "-n takes a haploid coverage of at least 1"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "-q", 0.9], "-q needs --auto-cutoffs"),
        (d + ["-l", 10, "-u", 100], "-o <out> is missing"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "-i", fq], "-i needs -k"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "-ci", 2], "-ci needs -k"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "--pairs", tmp_path / "db.kmc_suf"], "is a file of the database"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "--pairs", "out_smudge.tsv"], "is the report itself"),
        (["smudge", "-d", tmp_path / "dbb", "-l", 10, "-u", 100, "-o", "out"], "smudge needs canonical counts"),
        (["smudge", "-d", tmp_path / "none", "-l", 10, "-u", 100, "-o", "out"], "Open kmc database"),
        (kk + ["-l", 10, "-u", 100, "-o", "out", "-b"], "smudge needs canonical counts"),
        (kk + ["-l", 10, "-u", 100, "-o", "out", "--pairs", fq], "smudge: %s" % fq),             # an output that is an input
        (["smudge", "-k", 25, "-l", 10, "-u", 100, "-o", "out"], "-i <reads.fq> is missing"),
        (["smudge", "-k", 25, "-i", fa, "-l", 10, "-u", 100, "-o", "out"], "smudge: %s" % fa),    # what count refuses about its inputs
        (["smudge", "-k", 25, "-i", tmp_path / "none.fq", "-l", 10, "-u", 100, "-o", "out"], "none.fq"),
        (["smudge", "-k", 40, "-i", fq, "-l", 10, "-u", 100, "-o", "out"], "-k goes from 3 to 31"),
        (["smudge", "-k", 25, "-ci", 0, "-i", fq, "-l", 10, "-u", 100, "-o", "out"], "-ci is below 1"),
        (d + ["-l", 10, "-u", 100, "-o", "out", "--smudge"], "unknown option --smudge"),
        (run1 + ["--smudge-n", 20], "--smudge-n needs --smudge"),
        (run1 + ["--smudge-pairs", "p.tsv"], "--smudge-pairs needs --smudge"),
        (run1 + ["--smudge", "--smudge-n", 0], "--smudge-n takes a haploid coverage of at least 1"),
        (run1 + ["--smudge", "--smudge-pairs"], "--smudge-pairs needs a value"),
        (run1 + ["--smudge", "--smudge-pairs", fq], "run: %s" % fq),
        (run1 + ["--smudge", "--gfa-out", "g", "--smudge-pairs", "g.gfa"], "two outputs have the same path"),
    ]
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    for sub in ("run-multi", "mask", "count", "build"):
        assert "unknown option --smudge" in run_cli(sub, "--smudge", cwd=tmp_path).stderr
    usage = run_cli().stdout + run_cli().stderr
    assert "Usage: PloidyFrost smudge -d <KMCDatabase> (-l L -u U | --auto-cutoffs [-q Q]) -o <out> [-n N] [--pairs <file>] [-v]" in usage
    assert "--smudge [--smudge-n N] [--smudge-pairs FILE]" in run_cli("run").stderr


def test_python_refusals(tmp_path):
    (km, ct), k = hp.haplotypes(25), 25
    synth.write_kmc1(str(tmp_path / "dbb"), km, ct, k, both_strands=False)
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\n" + hp.genome(60, 1).encode() + b"\n+\n" + b"I" * 60 + b"\n")
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(RuntimeError, match="smudge needs canonical counts"):
        hostapi.smudge(str(tmp_path / "o"), db=str(tmp_path / "dbb"), lower=10, upper=100)
    with pytest.raises(RuntimeError, match="above 4096"):
        hostapi.smudge(str(tmp_path / "o"), db=str(tmp_path / "dbb"), lower=10, upper=5000)
    with pytest.raises(RuntimeError, match="either a database or inputs to count are given"):
        hostapi.smudge(str(tmp_path / "o"), inputs=[], lower=10, upper=100)
    with pytest.raises(ValueError, match="either db or inputs"):
        hostapi.smudge(str(tmp_path / "o"), lower=10, upper=100)
    with pytest.raises(ValueError, match="either lower=L and upper=U or auto=True"):
        hostapi.smudge(str(tmp_path / "o"), db=str(tmp_path / "dbb"), lower=10)
    with pytest.raises(RuntimeError, match="run: --smudge-n needs --smudge"):
        hostapi.run_reads(fq, "s", smudge_n=20)
    with pytest.raises(ValueError, match="either inputs or pairs"):   # refused in Python: the switch is not left on for the next call
        hostapi.run_reads(fq, "s", pairs=[(fq, fq)], smudge=True)
    with pytest.raises(RuntimeError, match="none.fq"):   # (with the switch on, run-multi would refuse --smudge first)
        hostapi.run_multi_reads([("a", tmp_path / "none.fq")], "s")
    with pytest.raises(RuntimeError, match="--smudge is not built into run-multi"):
        hostapi.load_library().pfh_reads_smudge(1, -1, None)
        hostapi.run_multi_reads([("a", fq)], "s")
    assert sorted(os.listdir(tmp_path)) == before


# ---- the stand-alone program and the declarations ----

def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_hetpair_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined over exact-size buffers
    (host code only: nothing of it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_hetpair_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_hetpair_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    for s in ("pf_hetpairs", "pf_hetpair_table"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_hetpairs_host", "pfh_smudge_report_text", "pfh_smudge_of", "pfh_smudge", "pfh_reads_smudge", "pfh_reads_smudge_result"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_HETPAIR == hipapi.K_QC + 1
    hip = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "ploidyfrost_host.h")).read()
    assert re.search(r"PF_K_QC,[^\n]*PF_K_HETPAIR,[^\n]*\n\s*PF_K_COUNT_", hip)
    assert re.search(r"int pf_hetpairs\(pf_ctx \*, const uint64_t \*kmers, const uint32_t \*counts, uint64_t n, uint32_t k, uint32_t lo, uint32_t hi,", hip)
    assert "typedef struct pf_hetpair_stats" in hip and "int pf_hetpair_table(" in hip
    for s in ("int pfh_hetpairs_host(", "int pfh_smudge_report_text(", "int pfh_smudge(", "void pfh_reads_smudge("):
        assert s in host
    assert hipapi.HETPAIR_STATS.names == hostapi.HETPAIR_STATS_FIELDS
