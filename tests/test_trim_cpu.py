"""The rule of `ploidyfrost trim` (K-TRIM) without a GPU: the Python restatement of trim_cases.py on the figures worked out by hand,
the host's plain restatement (pfh_trim_read / pfh_trim_fastq_chunk, csrc/pf_trim_rule.hpp) against it on hand, edge and generated
reads in every step order, chunks (CRLF, no last newline, a record cut in each of its lines), the refusals of the steps and of the
sub-command by their texts, the stand-alone program tests/cpp/test_trim_rule.cpp under the sanitizers, and the declarations."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import trim_cases as tc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def generated():
    return tc.make_reads(2000, seed=7)


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


# ---- the Python restatement itself, on the figures worked out by hand ----

def test_python_rule_by_hand():
    for q, first, second in tc.HAND:
        assert tc.trim_read(q, tc.HAND_STEPS[0]) == first, q
        assert tc.trim_read(q, tc.HAND_STEPS[1]) == second, q
    assert tc.trim_read([], ["MINLEN:0"]) is None                       # e == b after the last step
    assert tc.trim_read([40] * 5, ["SLIDINGWINDOW:6:0"]) is None        # fewer bases than the window
    assert tc.trim_read([40, 40, 2, 2, 40], ["SLIDINGWINDOW:2:20"]) == (0, 3)   # window 1 (40 + 2 = 42 >= 40) is good, window 2 is the first bad one
    assert tc.trimlog(tc.trim_fastq(b"@a b\nACGT\n+\nI##I\n@c\nAC\n+\n##\n", ["TRAILING:10", "LEADING:10"])) == b"a b 4 0 4 0\nc 0 0 0 0\n"


def test_generated_reads_cover_the_four_outcomes(generated):
    dropped, whole, lead, trail = tc.outcome_shares(generated)
    assert dropped >= 0.10 and whole >= 0.10 and lead >= 0.10 and trail >= 0.10, (dropped, whole, lead, trail)
    assert {len(r[1]) for r in generated} == set(tc.GEN_LENGTHS)


# ---- pfh_trim_read against it ----

def test_host_rule_on_hand_cases():
    for q, first, second in tc.HAND:
        assert hostapi.trim_read(tc.qline(q), tc.HAND_STEPS[0]) == first, q
        assert hostapi.trim_read(tc.qline(q), tc.HAND_STEPS[1]) == second, q
        assert hostapi.trim_read(tc.qline(q, 64), tc.HAND_STEPS[0], phred=64) == first, q


@pytest.mark.parametrize("steps", tc.EDGE_STEPS, ids=lambda s: "_".join(s))
def test_host_rule_on_edge_reads(steps):
    n_kept = 0
    for n in tc.EDGE_LENGTHS:
        for name, q in tc.edge_quals(n):
            want = tc.trim_read(q, steps)
            assert hostapi.trim_read(tc.qline(q), steps) == want, (n, name)
            assert hostapi.trim_read(tc.qline(q, 64), steps, phred=64) == want, (n, name)
            n_kept += want is not None
    assert n_kept


@pytest.mark.parametrize("steps", tc.ORDERS, ids=lambda s: "_".join(s))
def test_host_rule_on_generated_reads(generated, steps):
    for _, _, qual in generated:
        assert hostapi.trim_read(qual, steps) == tc.trim_read(tc.quals(qual), steps)


# ---- chunks ----

def same_chunk(got, want):
    assert got["clause"] == "none"
    for key in ("out", "bytes_used", "n_records", "begin", "len", "stats"):
        assert got[key] == want[key], key


def test_host_chunk_line_ends(generated):
    recs = generated[:200] + tc.edge_records()[:60]
    plain = tc.trim_fastq(tc.fastq(recs), tc.WORKFLOW)
    for crlf in (False, True):
        for last_newline in (True, False):
            text = tc.fastq(recs, crlf=crlf, last_newline=last_newline)
            got = hostapi.trim_fastq_chunk(text, tc.WORKFLOW)
            same_chunk(got, tc.trim_fastq(text, tc.WORKFLOW))
            assert got["out"] == plain["out"] and got["bytes_used"] == len(text)   # CRLF comes out with '\n', the last line gets one
    assert hostapi.trim_fastq_chunk(b"", tc.WORKFLOW)["n_records"] == 0


def test_host_chunk_cut_inside_every_line(generated):
    recs = generated[:5]
    text, head = tc.fastq(recs), tc.fastq(recs[:4])
    whole = hostapi.trim_fastq_chunk(text, tc.WORKFLOW)
    for cut in range(len(head), len(text)):   # inside each of the last record's four lines, and right behind their ends
        first = hostapi.trim_fastq_chunk(text[:cut], tc.WORKFLOW, final=False)
        same_chunk(first, tc.trim_fastq(text[:cut], tc.WORKFLOW, final=False))
        assert first["bytes_used"] == len(head) and first["n_records"] == 4, cut
        second = hostapi.trim_fastq_chunk(text[first["bytes_used"]:], tc.WORKFLOW, final=True)
        assert first["out"] + second["out"] == whole["out"], cut
    assert hostapi.trim_fastq_chunk(text, tc.WORKFLOW, final=False)["bytes_used"] == len(text)


def test_host_chunk_format_clause_writes_nothing():
    got = hostapi.trim_fastq_chunk(b"@a\nAC\n+\nII\n@b\nAC\n+\nIII\n", tc.WORKFLOW)
    assert (got["clause"], got["bad_record"], got["out"], got["n_records"]) == ("quality", 1, b"", 0)


# ---- the refusals of the steps ----

@pytest.mark.parametrize("word,name,text", [
    ("ILLUMINACLIP:TruSeq3-PE.fa:2:30:10", "unknown", "unknown step"),
    ("CROP:100", "unknown", "unknown step"),
    ("leading:10", "unknown", "unknown step"),
    ("LEADING", "field", "a field of the step is missing or is not a number"),
    ("LEADING:ten", "field", "a field of the step is missing or is not a number"),
    ("SLIDINGWINDOW:3", "field", "a field of the step is missing or is not a number"),
    ("SLIDINGWINDOW:3:20:1", "field", "a field of the step is missing or is not a number"),
    ("LEADING:94", "range", "a value of the step is out of range"),
    ("SLIDINGWINDOW:0:20", "range", "a value of the step is out of range"),
    ("SLIDINGWINDOW:65:20", "range", "a value of the step is out of range"),
    ("MINLEN:4294967296", "range", "a value of the step is out of range"),
])
def test_step_refusals_by_name(word, name, text):
    with pytest.raises(ValueError) as e:
        hostapi.trim_parse_steps(["LEADING:10", word])
    assert e.value.refusal == name and text in str(e.value) and word in str(e.value)


def test_step_count_and_phred_refusals():
    with pytest.raises(ValueError, match="more than 8 steps"):
        hostapi.trim_read(b"IIII", ["MINLEN:1"] * 9)
    with pytest.raises(ValueError, match="no step is given"):
        hostapi.trim_read(b"IIII", [])
    with pytest.raises(ValueError, match="the quality offset is 33 or 64, not 50"):
        hostapi.trim_read(b"IIII", ["MINLEN:1"], phred=50)
    assert hostapi.trim_read(b"IIII", ["MINLEN:1"] * 8) == (0, 4)
    assert [tuple(s) for s in hostapi.trim_parse_steps("LEADING:10 SLIDINGWINDOW:3:20 MINLEN:4294967295")] == [(1, 10, 0), (3, 3, 20), (4, 4294967295, 0)]
    assert [tuple(s) for s in hipapi.trim_steps(tc.WORKFLOW)] == [tuple(s) for s in hostapi.trim_parse_steps(tc.WORKFLOW)]


# ---- the sub-command's refusals: by name, before any device work (this passes on a machine without a GPU) ----

def test_cli_refusals(tmp_path):
    fq, fq2 = tmp_path / "in.fq", tmp_path / "in2.fq"
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    fq2.write_bytes(tc.fastq(tc.make_reads(3, 2)))
    fa, gz = tmp_path / "in.fa", tmp_path / "in.fq.gz"
    fa.write_bytes(b">s\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    out, log = tmp_path / "out.fq", tmp_path / "log.txt"
    o = [tmp_path / n for n in ("p1.fq", "u1.fq", "p2.fq", "u2.fq")]
    single = ["trim", "-i", fq, "-o", out]
    pair_in = ["trim", "-1", fq, "-2", fq2]
    pair = pair_in + ["-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3]]
    steps = tc.WORKFLOW
    cases = [
        (single, "no step is given"),
        (single + ["ILLUMINACLIP:a.fa:2:30:10"], "ILLUMINACLIP:a.fa:2:30:10: unknown step"),
        (single + ["LEADING:10", "HEADCROP:5"], "HEADCROP:5: unknown step"),
        (single + ["LEADING:x"], "LEADING:x: a field of the step is missing or is not a number"),
        (single + ["SLIDINGWINDOW:3"], "SLIDINGWINDOW:3: a field of the step is missing or is not a number"),
        (single + ["TRAILING:94"], "TRAILING:94: a value of the step is out of range"),
        (single + ["MINLEN:1"] * 9, "more than 8 steps"),
        (["trim", "-o", out] + steps, "-i <reads.fq> is missing"),
        (["trim", "-i", fq] + steps, "-o <trimmed.fq> is missing"),
        (single + ["-1", fq2] + steps, "-i does not go with -1 / -2"),
        (pair_in + ["-o", out] + steps, "-o does not go with -1 / -2"),
        (single + ["-o1", o[0]] + steps, "-o1 -u1 -o2 -u2 do not go with -i"),
        (["trim", "-1", fq, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3]] + steps, "-2 <r2.fq> is missing"),
        (pair_in + ["-o1", o[0], "-u1", o[1], "-o2", o[2]] + steps, "-u2 <out.fq> is missing"),
        (single + steps + ["--phred", "50"], "--phred takes 33 or 64, not '50'"),
        (single + steps + ["--chunk-bytes", "0"], "--chunk-bytes takes a positive number"),
        (single + steps + ["--frobnicate"], "unknown option --frobnicate"),
        (single + steps + ["--trimlog"], "--trimlog needs a value"),
        (["trim", "-i", fq, "-o", fq] + steps, "the output path is an input path"),
        (single + steps + ["--trimlog", fq], "the output path is an input path"),
        (single + steps + ["--trimlog", out], "two outputs have the same path"),
        (pair_in + ["-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[0]] + steps, "two outputs have the same path"),
        (pair_in + ["-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", fq2] + steps, "the output path is an input path"),
        (["trim", "-i", fq, "-i", fa, "-o", out] + steps, "%s: record 1: the input is FASTA (first byte '>'): only FASTQ is trimmed" % fa),
        (["trim", "-i", gz, "-o", out] + steps, "%s: record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is trimmed" % gz),
        (["trim", "-i", tmp_path / "none.fq", "-o", out] + steps, "cannot read %s" % (tmp_path / "none.fq")),
        (["trim", "-1", fq, "-2", gz, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "--trimlog", log] + steps, "%s: record 1: the input is gzip-compressed" % gz),
    ]
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["in.fa", "in.fq", "in.fq.gz", "in2.fq"], args   # no output, no temporary file
    usage = run_cli().stdout + run_cli().stderr
    assert "trim -i <reads.fq>" in usage and "trim -1 <r1.fq> -2 <r2.fq>" in usage


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_trim_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_trim_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_trim_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- names ----

def declaration(header, name):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = f.read()
    at = text.index(name + "(")
    return " ".join(text[at: text.index(";", at)].split())


def test_entry_points_are_declared():
    for s in ("pf_trim_fastq", "pf_trim_fastq_pair"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_trim_fastq", "pfh_trim_fastq_pair", "pfh_trim_read", "pfh_trim_parse_step", "pfh_trim_fastq_chunk"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_TRIM == hipapi.K_COUNT + 1
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_TRIM" in text.split("PF_K_COUNT,")[1].split("PF_K_COUNT_")[0]
    assert "typedef struct pf_trim_step" in text and "typedef struct pf_trim_stats" in text
    assert declaration("ploidyfrost_hip.h", "int pf_trim_fastq") == (
        "int pf_trim_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, "
        "char *out, uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t *n_records, pf_trim_stats *stats, "
        "uint64_t *bad_record)")
    assert declaration("ploidyfrost_hip.h", "int pf_trim_fastq_pair") == (
        "int pf_trim_fastq_pair(pf_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, "
        "uint32_t n_steps, uint32_t phred, char *out[4], uint64_t out_bytes[4], uint64_t bytes_used[2], uint32_t *rec_begin[2], uint32_t *rec_len[2], "
        "uint64_t *n_records, pf_trim_stats stats[2], uint64_t *bad_record)")
    assert declaration("ploidyfrost_host.h", "int pfh_trim_read").startswith("int pfh_trim_read(const char *qual, uint64_t n, const pf_trim_step *steps")
    assert hostapi.TRIM_STATS_FIELDS == tc.STATS == hipapi.TRIM_STATS.names
    assert hipapi.TRIM_STEP == hostapi.TRIM_STEP and hipapi.TRIM_STEP.itemsize == 12 and hipapi.TRIM_STATS.itemsize == 72
