"""The rule of duplicate removal (K-DEDUP, `--dedup`) without a GPU: the Python restatement of dedup_cases.py on hand cases, the host's
plain restatement (pfh_dedup_key / pfh_dedup_units / pfh_trim_fastq[_pair]_chunk_dedup, csrc/pf_dedup_rule.hpp) against it on hand, edge
and generated reads and on chunks, the refusals of the options by their texts, the stand-alone program tests/cpp/test_dedup_rule.cpp
under the sanitizers, and the declarations."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import dedup_cases as dc
import trim_cases as tc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
STEPS = ["LEADING:10", "TRAILING:10", "MINLEN:30"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


# ---- the key ----

def test_hand_cases_of_the_key():
    """the properties of the key, asked of the host rule and of the Python restatement alike"""
    def k(seq1, seq2=None, bases=0):
        got = hostapi.dedup_key(seq1, seq2, bases)
        assert got == dc.key_of(seq1, seq2, bases)
        return got
    assert dc.code(ord("A")) == dc.code(ord("a")) == 0 and dc.code(ord("t")) == 3 and dc.code(ord("N")) == dc.code(0) == dc.code(ord("\r")) == 4
    s = b"ACGTTGCAACGTTGCAAC"
    assert k(s) == k(s.lower()) == k(s, None, 0) == k(s, None, 4096)
    assert k(s) != k(s[:-1]) and k(s) != k(s[:-1] + b"G") and k(s, None, 16) == k(s[:16]) == k(s[:16] + b"TTTT", None, 16)
    assert k(b"ACNT" * 5) == k(b"AC.T" * 5) != k(b"ACGT" * 5)
    assert k(s, s[::-1]) != k(s[::-1], s) and k(s, b"") != k(s) and k(b"", b"") != k(b"")
    assert k(b"") == k(b"", None, 16) and all(h != 0 for h in k(b""))
    assert k(b"A" * 16) != k(b"A" * 17) != k(b"A" * 32)   # words of 0: the length alone


def test_host_key_equals_the_restatement():
    recs = dc.edge_records()
    assert {len(r[1]) for r in recs} >= set(dc.EDGE_LENGTHS)
    for bases in (0, 16, 100, 4096):
        for _, seq, _ in recs:
            assert hostapi.dedup_key(seq, bases=bases) == dc.key_of(seq, None, bases)
        for (_, a, _), (_, b, _) in zip(recs[::3], recs[1::3]):
            assert hostapi.dedup_key(a, b, bases=bases) == dc.key_of(a, b, bases)
    long = dc.rand_seq(__import__("random").Random(1), 70000)   # beyond 2^16 words of one read
    assert hostapi.dedup_key(long) == dc.key_of(long) != dc.key_of(long[:-1])


def test_key_refusals():
    for bases in (1, 15, 4097):
        with pytest.raises(RuntimeError, match=r"pfh_dedup_key: bases is 0 \(the whole read\) or 16 \.\. 4096, not %d" % bases):
            hostapi.dedup_key(b"ACGT", bases=bases)


# ---- the decision ----

def test_hand_cases_of_the_decision():
    keys = np.array([[1, 2], [3, 4], [1, 2], [1, 3], [0, 2], [1, 2], [3, 4]], dtype=np.uint64)
    keep, st = hostapi.dedup_units(keys)
    assert list(keep) == [1, 1, 0, 1, 0, 0, 0]   # (a zero word counts as 1: [0, 2] is [1, 2])
    assert st == dict(units=7, unique=3, duplicates=4, max_copies=4, levels=[1, 1, 0, 1, 0, 0, 0, 0, 0, 0], slots=0, growths=0)
    d = dc.Dedup()
    assert list(d.keys(keys)) == list(keep) and d.stats() == {f: st[f] for f in dc.STATS}
    # a unit that takes no part stays and shadows nothing
    keep, st = hostapi.dedup_units(keys, [0, 1, 1, 1, 1, 1, 1])
    assert list(keep) == [1, 1, 1, 1, 0, 0, 0] and st["units"] == 6 and st["unique"] == 3 and st["max_copies"] == 3
    keep, st = hostapi.dedup_units(np.zeros((0, 2), dtype=np.uint64))
    assert len(keep) == 0 and st["units"] == 0 and st["max_copies"] == 0 and st["levels"] == [0] * 10


def test_levels_of_the_decision():
    keys = np.array([[7 + c, 9] for c in range(1, 13) for _ in range(c)], dtype=np.uint64)   # key c has c copies, c = 1 .. 12
    rng = np.random.default_rng(4)
    keys = keys[rng.permutation(len(keys))]
    keep, st = hostapi.dedup_units(keys)
    d = dc.Dedup()
    assert list(keep) == list(d.keys(keys)) and int(keep.sum()) == 12
    assert st["levels"] == [1] * 9 + [3] and st["max_copies"] == 12 and st["duplicates"] == len(keys) - 12 and d.stats()["levels"] == st["levels"]


# ---- chunks: the restatement composed with the trimming ----

def same_chunk(h, p, paired):
    assert h["clause"] == 0 and h["n_records"] == p["n_records"]
    if paired:
        assert h["outs"] == p["out"] and list(h["bytes_used"]) == list(p["bytes_used"])
        for f in range(2):
            assert list(h["begin"][f]) == p["begin"][f] and list(h["len"][f]) == p["len"][f] and h["stats"][f] == p["stats"][f]
    else:
        assert h["out"] == p["out"] and h["bytes_used"] == p["bytes_used"]
        assert list(h["begin"]) == p["begin"] and list(h["len"]) == p["len"] and h["stats"] == p["stats"]


@pytest.mark.parametrize("bases", [0, 16, 100])
@pytest.mark.parametrize("steps", [STEPS, []])
def test_chunks_against_the_restatement(bases, steps):
    recs = dc.dup_reads(600, 11, copies_of_one=12) + dc.edge_records()
    text = tc.fastq(recs)
    # one chunk, and the same text cut at record boundaries with the keys carried
    d = dc.Dedup(bases)
    whole = hostapi.trim_fastq_chunk_dedup(text, steps, bases=bases)
    same_chunk(whole, d.trim_fastq(text, steps), False)
    assert d.stats()["duplicates"] > 100 and d.stats()["max_copies"] >= 13
    cuts = [0, len(tc.fastq(recs[:1])), len(tc.fastq(recs[:250])), len(tc.fastq(recs[:251])), len(text)]
    d2, seen, out, lens = dc.Dedup(bases), np.zeros((0, 2), dtype=np.uint64), b"", []
    for a, b in zip(cuts, cuts[1:]):
        h = hostapi.trim_fastq_chunk_dedup(text[a:b], steps, bases=bases, seen_keys=seen)
        same_chunk(h, d2.trim_fastq(text[a:b], steps), False)
        seen = np.concatenate([seen, h["keys"][h["keys"].any(axis=1)]])
        out += h["out"]
        lens += list(h["len"])
    assert out == whole["out"] and lens == list(whole["len"]) and d2.stats() == d.stats()


def test_pair_chunks_against_the_restatement():
    recs = dc.dup_reads(500, 12)
    m = dc.mates(recs, 3)
    m[7] = (m[7][0], m[7][1], b"#" * len(m[7][1]))   # a pair of which file 2 is dropped: no unit
    t1, t2 = tc.fastq(recs, crlf=True), tc.fastq(m)
    d = dc.Dedup()
    h = hostapi.trim_fastq_chunk_dedup(t1, STEPS, text2=t2)
    p = d.trim_pair(t1, t2, STEPS)
    same_chunk(h, p, True)
    assert p["stats"][0]["only1"] >= 1 and d.stats()["duplicates"] > 50 and not h["keys"][7].any()
    # a refused chunk leaves nothing
    bad = hostapi.trim_fastq_chunk_dedup(t1.replace(b"+", b"-", 1), STEPS, text2=t2)
    assert bad["clause"] != 0 and bad["n_records"] == 0 and bad["outs"] == [b""] * 4


# ---- refusals by their texts ----

@pytest.mark.parametrize("args,text", [
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup-bases", "32"], "trim: --dedup-bases needs --dedup"),
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup-initial-slots", "64"], "trim: --dedup-initial-slots needs --dedup"),
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup", "--dedup-bases", "15"], "trim: --dedup-bases takes 16 to 4096, not '15'"),
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup", "--dedup-bases", "4097"], "trim: --dedup-bases takes 16 to 4096, not '4097'"),
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup", "--dedup-bases"], "trim: --dedup-bases needs a value"),
    (["trim", "-i", "in.fq", "-o", "o.fq", "--dedup", "--fasta"], "trim: --fasta does not go with --dedup"),
    (["trim", "-1", "in.fq", "-2", "in.fq", "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d", "--dedup"], "trim: the two inputs of a pair are the same file"),
    (["run", "-i", "in.fq", "-o", "s", "--dedup", "--fasta"], "run: --fasta does not go with --dedup"),
    (["run", "-i", "in.fq", "-o", "s", "--dedup-bases", "20"], "run: --dedup-bases needs --dedup"),
    (["run", "-i", "in.fq", "-o", "s", "--dedup", "--dedup-bases", "x"], "run: --dedup-bases takes 16 to 4096, not 'x'"),
    (["run-multi", "--sample", "A", "-i", "in.fq", "-o", "s", "--dedup-initial-slots", "64"], "run-multi: --dedup-initial-slots needs --dedup"),
    (["run-multi", "--sample", "A", "-i", "in.fq", "-o", "s", "--dedup", "--fasta"], "run-multi: --fasta does not go with --dedup"),
    (["mask", "-i", "in.fq", "-o", "o.fq", "-d", "db", "--dedup"], "unknown option --dedup"),
    (["count", "-i", "in.fq", "-o", "db", "--dedup"], "unknown option --dedup"),
    (["build", "-r", "in.fq", "-o", "g", "--dedup"], "unknown option --dedup"),
    (["build-multi", "-r", "in.fq", "-o", "g", "--dedup"], "unknown option --dedup"),
    (["qc", "-i", "in.fq", "-o", "r.tsv", "--dedup"], "unknown option --dedup"),
    (["smudge", "-d", "db", "-o", "r.tsv", "--dedup"], "unknown option --dedup"),
])
def test_cli_refusals(tmp_path, args, text):
    (tmp_path / "in.fq").write_bytes(tc.fastq(tc.make_reads(4, 1)))
    r = run_cli(*args, cwd=tmp_path)
    assert r.returncode != 0 and text in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.fq"]


def test_python_refusals(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(tc.fastq(tc.make_reads(4, 1)))
    with pytest.raises(RuntimeError, match="--dedup-bases needs --dedup"):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", tc.WORKFLOW, dedup_bases=32)
    with pytest.raises(RuntimeError, match="--dedup-initial-slots needs --dedup"):
        hostapi.trim_fastq_pair(fq, fq, [tmp_path / n for n in "abcd"], tc.WORKFLOW, dedup_initial_slots=64)
    with pytest.raises(RuntimeError, match="trim: --dedup-bases takes 16 to 4096, not 8"):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [], dedup=True, dedup_bases=8)
    with pytest.raises(RuntimeError, match="run: --fasta does not go with --dedup"):
        hostapi.run_reads([fq], "s", fasta=True, dedup=True)
    with pytest.raises(RuntimeError, match="--dedup-bases needs --dedup"):
        hostapi.run_reads([fq], "s", dedup_bases=32)
    with pytest.raises(RuntimeError, match="run-multi: sample A: --dedup-bases takes 16 to 4096, not 5000"):
        hostapi.run_multi_reads([("A", fq)], "s", dedup=True, dedup_bases=5000)
    with pytest.raises(RuntimeError, match="no step is given"):   # without the switch: as before
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [])
    assert sorted(os.listdir(tmp_path)) == ["in.fq"]


def test_the_pinned_usage_texts_do_not_name_the_options():
    surface = open(os.path.join(ROOT, "tests", "golden", "cli", "surface.json")).read()
    assert "--dedup" not in surface


# ---- the stand-alone program and the declarations ----

def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_dedup_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_dedup_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_dedup_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    for s in ("pf_dedup_begin", "pf_dedup_stats_get", "pf_dedup_end", "pf_dedup_keys"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_reads_dedup", "pfh_reads_dedup_report", "pfh_dedup_key", "pfh_dedup_units", "pfh_trim_fastq_chunk_dedup", "pfh_trim_fastq_pair_chunk_dedup"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_DEDUP == hipapi.K_HETPAIR + 1
    hip = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "ploidyfrost_host.h")).read()
    assert re.search(r"PF_K_HETPAIR,[^\n]*PF_K_DEDUP,[^\n]*\n\s*PF_K_COUNT_", hip)   # appended: the values of old stay
    assert "typedef struct pf_dedup_stats { uint64_t units, unique, duplicates, max_copies, levels[10], slots, growths; } pf_dedup_stats;" in hip
    for s in ("int pf_dedup_begin(pf_ctx *, uint32_t bases", "int pf_dedup_stats_get(pf_ctx *, pf_dedup_stats *);", "int pf_dedup_end(pf_ctx *);",
              "int pf_dedup_keys(pf_ctx *, const uint64_t *keys"):
        assert s in hip
    for s in ("void pfh_reads_dedup(int on, uint32_t bases, uint64_t initial_slots);", "void pfh_reads_dedup_report(pf_dedup_stats *stats);", "int pfh_dedup_key(",
              "int pfh_dedup_units("):
        assert s in host
    assert hipapi.DEDUP_STATS.names == hostapi.DEDUP_STATS_FIELDS
    mk = open(os.path.join(ROOT, "ploidyfrost_amd", "csrc", "Makefile")).read()
    assert mk.count("pf_qc.hip") == mk.count("pf_dedup.hip") and "pf_dedup_rule.hpp" in mk
