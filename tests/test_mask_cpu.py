"""The rule of `ploidyfrost mask` (K-MASK) without a GPU: the host's plain restatement (pfh_mask_read, csrc/pf_mask_rule.hpp) against
the Python restatement of mask_cases.py on hand cases and on seeded reads of a golden case, the FASTQ index with each format clause by
its name, the stand-alone program tests/cpp/test_mask_rule.cpp under the sanitizers, the declarations, and the refusals of the
sub-command that come before any device work."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case

import mask_cases as mc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def dip():
    return mc.Database(load_case("dip20k")["db"])


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


# ---- the Python restatement itself, on figures worked out by hand ----

def test_python_rule_by_hand():
    k = 3
    kmers = np.array([0b000110, 0b110001], dtype=np.uint64)   # ACG (the canonical form of CGT too) and TAC (GTA's other strand: never the canonical form)
    counts = np.array([7, 9], dtype=np.uint32)
    # ACGTA: windows ACG (7), CGT -> ACG (7), GTA = 0b101100 < TAC: absent -> 0
    c = mc.counters(b"ACGTA", kmers, counts, k, True)
    assert list(c) == [7, 7, 0]
    assert mc.mask_with_counters(b"ACGTA", k, c, 1, mc.NO_UPPER) == (b"ACNNN", 3, 1, 3)
    assert mc.mask_with_counters(b"ACGTA", k, c, 0, mc.NO_UPPER) == (b"ACGTA", 3, 0, 0)       # low = 0: nothing is bad
    assert mc.mask_with_counters(b"ACGTA", k, c, 0, 6) == (b"NNNNA", 3, 2, 4)                  # up below a present count
    # the window as it reads for a database that is not both_strands: CGT itself is absent
    assert list(mc.counters(b"ACGTA", kmers, counts, k, False)) == [7, 0, 0]
    # lower case is read as upper case and kept; a byte outside ACGTacgt gives its windows 0
    assert list(mc.counters(b"acgNACG", kmers, counts, k, True)) == [7, 0, 0, 0, 7]
    assert mc.mask_with_counters(b"acgNACG", k, mc.counters(b"acgNACG", kmers, counts, k, True), 1, mc.NO_UPPER) == (b"aNNNNNG", 5, 3, 4)   # the input N does not count
    assert mc.parse_fastq(b"@a\r\nACGT\r\n+\r\n@III\r\n@b\nAC\n+\n+I") == [(4, 4), (22, 2)]


# ---- pfh_mask_read against it ----

HAND = [(b"", 25), (b"A", 25), (b"ACGT" * 6, 25), (b"ACGT" * 6 + b"A", 25), (b"N" * 40, 25), (b"acgt" * 20, 25), (b"ACGT" * 40, 31), (b"ACGTN" * 30, 3)]


@pytest.mark.parametrize("low,up", [(0, mc.NO_UPPER), (1, mc.NO_UPPER), (5, 9), (10, 10)])
def test_host_rule_on_hand_cases(low, up):
    rng = np.random.default_rng(low)
    for seq, k in HAND:
        windows = max(len(seq) - k + 1, 0)
        for pattern in ("zero", "big", "random", "first", "last", "k_apart", "k1_apart"):
            c = np.full(windows, 7, dtype=np.uint32)
            if pattern == "zero":
                c[:] = 0
            elif pattern == "big":
                c[:] = 0xFFFFFFFF
            elif pattern == "random":
                c = rng.integers(0, 14, size=windows, dtype=np.uint32)
            elif pattern == "first" and windows:
                c[0] = 0
            elif pattern == "last" and windows:
                c[-1] = 0
            elif pattern in ("k_apart", "k1_apart") and windows > k + 1:
                c[0] = 0
                c[k + (pattern == "k1_apart")] = 0
            want = mc.mask_with_counters(seq, k, c, low, up)
            got = hostapi.mask_read(seq, k, c, low, up)
            assert got == (want[0], want[3]), (seq, k, pattern)


def test_one_unmasked_base_between_two_windows_k_plus_1_apart():
    k, seq = 5, b"ACGTACGTACGTACGT"
    c = np.full(len(seq) - k + 1, 9, dtype=np.uint32)
    c[1] = c[1 + k + 1] = 0
    assert hostapi.mask_read(seq, k, c, 1)[0] == b"ANNNNNGNNNNNACGT"
    c[:] = 9
    c[1] = c[1 + k] = 0
    assert hostapi.mask_read(seq, k, c, 1)[0] == b"ANNNNNNNNNNTACGT"


def test_host_rule_on_seeded_reads(dip):
    reads = mc.make_reads("dip20k", 3000, seed=11, k=dip.k)
    changed_reads = 0
    for low, up in ((10, mc.NO_UPPER), (15, 30)):
        for r in reads:
            c = mc.counters(r, dip.kmers, dip.counts, dip.k, dip.both_strands)
            want = mc.mask_with_counters(r, dip.k, c, low, up)
            assert hostapi.mask_read(r, dip.k, c, low, up) == (want[0], want[3])
            changed_reads += want[3] > 0
    assert 0 < changed_reads < 2 * len(reads)   # the maker damages some reads and leaves others whole


def test_reads_cut_from_the_graph_are_clean(dip):
    """the premise of the GPU cases: every window of an undamaged read is in the case's database"""
    for case in ("dip20k", "k31_z16", "stranded20k"):
        db = dip if case == "dip20k" else mc.Database(load_case(case)["db"])
        for r in mc.make_reads(case, 200, seed=3, sub_rate=0, n_rate=0, lower_rate=0.5, k=db.k):
            if len(r) >= db.k:
                assert mc.counters(r, db.kmers, db.counts, db.k, db.both_strands).min() > 0, case
        assert mc.counters(mc.clean_read(case, 150), db.kmers, db.counts, db.k, db.both_strands).min() > 0
    genome, sdb = mc.synthetic(1, 2500, 25, weak=(1023,))
    c = mc.counters(genome, sdb.kmers, sdb.counts, 25, True)
    assert c[1023] == 2 and (np.delete(c, 1023) == 20).all()


# ---- the FASTQ index and its clauses ----

def test_index_matches_the_python_parser():
    reads = mc.make_reads("dip20k", 257, seed=5)
    for crlf in (False, True):
        for last_newline in (True, False):
            text = mc.fastq(reads, crlf=crlf, last_newline=last_newline, quals={3: b"@" + b"I" * (len(reads[3]) - 1), 4: b"+" * len(reads[4])})
            ix = hostapi.mask_index_fastq(text, final=True)
            assert ix["clause"] == "none" and ix["n_records"] == len(reads) and ix["bytes_used"] == len(text)
            assert list(zip(ix["read_off"].tolist(), ix["read_len"].tolist())) == mc.parse_fastq(text)
    assert hostapi.mask_index_fastq(b"", final=True)["n_records"] == 0


def test_chunk_ends():
    a, b = mc.fastq([b"ACGTACGT"], name=b"a"), mc.fastq([b"GGCC"], name=b"b")
    for cut in range(len(b)):   # inside every line of the second record, and right behind its lines' ends
        ix = hostapi.mask_index_fastq(a + b[:cut], final=False)
        assert (ix["clause"], ix["n_records"], ix["bytes_used"]) == ("none", 1, len(a)), cut
    assert hostapi.mask_index_fastq(a + b, final=False)["bytes_used"] == len(a + b)
    assert hostapi.mask_index_fastq(a[:-1], final=False)["bytes_used"] == 0       # no whole record
    assert hostapi.mask_index_fastq(a[:-1], final=True)["bytes_used"] == len(a) - 1


@pytest.mark.parametrize("name,text,record", [
    ("header", b"@a\nAC\n+\nII\nb\nAC\n+\nII\n", 1),
    ("plus", b"@a\nAC\n-\nII\n", 0),
    ("quality", b"@a\nAC\n+\nII\n@b\nAC\n+\nIII\n", 1),
    ("quality", b"@a\nAC\r\n+\nII\r\r\n", 0),          # only the \r directly before the \n belongs to the line end
    ("line_count", b"@a\nAC\n+\nII\n@b\nAC\n", 1),
    ("header", b">s\nACGT\n>t\nAC\n", 0),              # FASTA reaches the index as a record without '@'; the file check names it
])
def test_format_clauses_by_name(name, text, record):
    ix = hostapi.mask_index_fastq(text, final=True)
    assert ix["clause"] == name and ix["bad_record"] == record
    assert ix["message"] and ix["message"] != hostapi.mask_index_fastq(b"", True)["message"]


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_mask_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_mask_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_mask_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- names ----

def test_entry_points_are_declared():
    assert "pf_mask_reads" in hipapi.DECLARED_SYMBOLS and "pf_mask_fastq" in hipapi.DECLARED_SYMBOLS
    assert hipapi.K_MASK == hipapi.K_HIST + 1 and hipapi.KERNELS[-1] == "k_call_model"
    for s in ("pfh_mask_fastq", "pfh_mask_read", "pfh_mask_index_fastq"):
        assert s in hostapi.DECLARED_SYMBOLS
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_MASK" in text.split("PF_K_HIST,")[1].split("PF_K_COUNT_")[0]
    assert hostapi.MASK_STATS_FIELDS == mc.STATS == hipapi.MASK_STATS.names


# ---- the sub-command's refusals: by name, before any device work (this passes on a machine without a GPU) ----

def test_cli_refusals(tmp_path):
    db = load_case("dip20k")["db"]
    fq = tmp_path / "in.fq"
    fq.write_bytes(mc.fastq([b"ACGT" * 10]))
    out = tmp_path / "out.fq"
    base = ["mask", "-d", db, "-i", fq, "-o", out]
    cases = [
        (base + ["-l", "5", "--auto-cutoffs"], "-l does not go with --auto-cutoffs"),
        (base, "the lower threshold is missing"),
        (["mask", "-i", fq, "-o", out, "-l", "5"], "-d <KMCDatabase> is missing"),
        (["mask", "-d", db, "-o", out, "-l", "5"], "-i <reads.fq> is missing"),
        (["mask", "-d", db, "-i", fq, "-l", "5"], "-o <out.fq> is missing"),
        (base + ["-l", "9", "-u", "8"], "L > U"),
        (base + ["-l", "x"], "-l takes a number"),
        (base + ["-l", "5", "--chunk-bytes", "0"], "--chunk-bytes takes a positive number"),
        (["mask", "-d", db, "-i", fq, "-o", fq, "-l", "5"], "the output path is an input path"),
    ]
    fa, gz = tmp_path / "in.fa", tmp_path / "in.fq.gz"
    fa.write_bytes(b">s\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    cases += [(["mask", "-d", db, "-i", fq, "-i", fa, "-o", out, "-l", "5"], "%s: record 1: the input is FASTA" % fa),
              (["mask", "-d", db, "-i", gz, "-o", out, "-l", "5"], "%s: record 1: the input is gzip-compressed" % gz)]
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["in.fa", "in.fq", "in.fq.gz"], args   # no output, no temporary file
    assert "mask -d <KMCDatabase>" in run_cli().stdout + run_cli().stderr
