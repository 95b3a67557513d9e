"""The rule of the read quality report (K-QC, `qc`, `--report`) without a GPU: the Python restatement of qc_cases.py on the hand-worked
records, the host's plain restatement (pfh_qc_fastq_chunk / pfh_qc_report_text, csrc/pf_qc_rule.hpp) against it on generated and edge
reads and on chunks (CRLF, no last newline, a text cut at every byte of its last record, steps that drop everything, a clip open), the
report of a small case as literal bytes, the hint, the refusals of the sub-commands by their words, the stand-alone program
tests/cpp/test_qc_rule.cpp under the sanitizers, and the declarations."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import clip_cases as cc
import qc_cases as qc
import trim_cases as tc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
DROP_ALL = ["MINLEN:100000"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 16], seed=3, sides=[0, 1, 2])


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def host_adapters(adapters):
    return hostapi.clip_parse_adapters(cc.adapters_fa(adapters))


def both(text, side=1, phred=33, final=True, steps=None, adapters=None):
    """(Python tables and clip, host tables and clip) of one chunk; the counts of records and bytes must agree as well"""
    pt, pc = qc.new_tables(), qc.new_clip()
    n, used = qc.add_chunk(pt, pc, text, side, phred, final, steps, adapters)
    h = hostapi.qc_fastq_chunk(text, side=side, phred=phred, final=final, steps=steps, adapters=None if adapters is None else host_adapters(adapters))
    assert h["clause"] == "none" and (h["n_records"], h["bytes_used"]) == (n, used)
    return pt, pc, h["tables"], h["clip"]


def same(pt, pc, ht, hc):
    assert np.array_equal(pt, ht), np.argwhere(pt != ht)[:8]
    assert np.array_equal(pc, hc)


# ---- the rule ----

def test_python_rule_by_hand():
    t, c = qc.new_tables(), qc.new_clip()
    assert qc.add_chunk(t, c, qc.HAND_TEXT, steps=qc.HAND_STEPS) == (3, len(qc.HAND_TEXT))
    assert t[0][qc.RAW].tolist() == qc.hand_raw()
    assert t[0][qc.KEPT].tolist() == qc.hand_kept()
    assert not t[1].any() and not c.any()


def test_host_rule_by_hand():
    h = hostapi.qc_fastq_chunk(qc.HAND_TEXT, steps=qc.HAND_STEPS)
    assert h["tables"][0][qc.RAW].tolist() == qc.hand_raw() and h["tables"][0][qc.KEPT].tolist() == qc.hand_kept()


def test_report_text_as_literal_bytes():
    h = hostapi.qc_fastq_chunk(qc.HAND_TEXT, steps=qc.HAND_STEPS)
    assert hostapi.qc_report_text(h["tables"]) == qc.HAND_REPORT
    assert qc.report_text(h["tables"]) == qc.HAND_REPORT


@pytest.mark.parametrize("phred", [33, 64])
def test_host_rule_on_edge_reads(phred):
    text = tc.fastq(qc.edge_records(phred=phred))
    for side in (1, 2):
        for steps in (None, tc.WORKFLOW, ["LEADING:3"]):
            same(*both(text, side, phred, steps=steps))


def test_host_rule_on_generated_reads():
    recs = qc.make_reads(400, 5)
    pt, pc, ht, hc = both(tc.fastq(recs), steps=tc.WORKFLOW)
    same(pt, pc, ht, hc)
    assert 0 < pt[0][qc.KEPT][qc.W_READS] < pt[0][qc.RAW][qc.W_READS] == 400
    assert hostapi.qc_report_text(ht) == qc.report_text(pt)


def test_host_rule_on_line_ends_and_cuts():
    recs = qc.make_reads(6, 2)
    same(*both(tc.fastq(recs, crlf=True), steps=tc.WORKFLOW))
    same(*both(tc.fastq(recs, last_newline=False), steps=tc.WORKFLOW))
    text = tc.fastq(recs)
    last = len(tc.fastq(recs[:-1]))
    for cut in range(last, len(text)):   # not final: the cut record is carried, whichever byte it is cut at
        pt, pc, ht, hc = both(text[:cut], final=False, steps=tc.WORKFLOW)
        same(pt, pc, ht, hc)
        assert pt[0][qc.RAW][qc.W_READS] == 5
    # the chunks of a file add up to the file
    whole = both(text, steps=tc.WORKFLOW)[2]
    h = hostapi.qc_fastq_chunk(text[:last], final=False, steps=tc.WORKFLOW)
    h = hostapi.qc_fastq_chunk(text[last:], tables=h["tables"], clip=h["clip"], steps=tc.WORKFLOW)
    assert np.array_equal(h["tables"], whole)


def test_steps_that_drop_every_read():
    pt, pc, ht, hc = both(tc.fastq(qc.make_reads(50, 3)), steps=DROP_ALL)
    same(pt, pc, ht, hc)
    kept = ht[0][qc.KEPT].copy()
    assert kept[qc.W_SEEN] == 1
    kept[qc.W_SEEN] = 0
    assert not kept.any()
    assert b"1\tkept\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n" in hostapi.qc_report_text(ht)


def test_a_clip_open(adapters):
    text = tc.fastq(cc.make_reads(200, adapters, seed=9))
    for side in (1, 2):
        for steps in ([], ["LEADING:3", "TRAILING:3", "MINLEN:20"]):   # (the generator's qualities are noise: the workflow's window would drop all)
            pt, pc, ht, hc = both(text, side, steps=steps, adapters=adapters)
            same(pt, pc, ht, hc)
            assert pc[side - 1].sum() > 20 and not pc[2 - side].any()
            # kept sees the clipped interval: fewer bases than the same steps without the clip
            assert ht[side - 1][qc.KEPT][qc.W_POS_BASE:qc.W_POS_QSUM].sum() < both(text, side, steps=steps or ["MINLEN:1"])[2][side - 1][qc.KEPT][qc.W_POS_BASE:qc.W_POS_QSUM].sum()
    assert hostapi.qc_report_text(ht, hc) == qc.report_text(pt, pc)
    assert b">>clip\nside\tclip_end\treads\n2\t" in hostapi.qc_report_text(ht, hc)


def test_phred_hint():
    for byte, want in ((58, 33), (59, 0), (63, 0), (64, 64)):
        assert hostapi.qc_phred_hint(byte, 1) == qc.phred_hint(byte, 1) == want
    assert hostapi.qc_phred_hint(33, 0) == hostapi.qc_phred_hint(64, 0) == 0
    for byte, want in ((58, 33), (59, 0), (63, 0), (64, 64)):   # through the tables and the report's second line
        t = hostapi.qc_fastq_chunk(b"@r\nAC\n+\n" + bytes([byte, 100]) + b"\n")["tables"]
        assert hostapi.qc_report_text(t).split(b"\n")[1] == b"# phred 33 hint %d" % want
    assert hostapi.qc_report_text(qc.new_tables()).split(b"\n")[1] == b"# phred 33 hint 0"
    assert hostapi.qc_report_text(hostapi.qc_fastq_chunk(b"@r\n\n+\n\n")["tables"]).split(b"\n")[1] == b"# phred 33 hint 0"   # a read without a byte


def test_format_refusal_of_the_chunk():
    h = hostapi.qc_fastq_chunk(b"@r\nACGT\n+\nII\n")
    assert h["clause"] == "quality" and h["bad_record"] == 0 and not h["tables"].any()
    with pytest.raises(ValueError, match="the quality offset is 33 or 64, not 50"):
        hostapi.qc_fastq_chunk(qc.HAND_TEXT, phred=50)


# ---- the sub-commands ----

def test_refusals_by_name(tmp_path):
    fq, fq2, fa, gz = (tmp_path / n for n in ("in.fq", "in2.fq", "in.fa", "in.fq.gz"))
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    fq2.write_bytes(tc.fastq(tc.make_reads(3, 2)))
    fa.write_bytes(b">a\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00" + bytes(20))
    before = sorted(os.listdir(tmp_path))
    rep = tmp_path / "rep.tsv"
    o = [tmp_path / n for n in ("p1.fq", "u1.fq", "p2.fq", "u2.fq")]
    single = ["trim", "-i", fq, "-o", tmp_path / "out.fq", "LEADING:3"]
    pair = ["trim", "-1", fq, "-2", fq2, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "LEADING:3"]
    run1 = ["run", "-i", fq, "-o", "s", "LEADING:3"]
    cases = [
        (single + ["--report"], "--report needs a value"),
        (pair + ["--report"], "--report needs a value"),
        (run1 + ["--report"], "--report needs a value"),
        (single + ["--report", fq], "trim: %s" % fq),                                        # the report is an input
        (single + ["--report", tmp_path / "out.fq"], "two outputs have the same path"),
        (pair + ["--report", o[2]], "two outputs have the same path"),
        (pair + ["--report", fq2], "trim: %s" % fq2),
        (run1 + ["--report", fq], "run: %s" % fq),
        (run1 + ["--gfa-out", "g", "--report", "g.gfa"], "two outputs have the same path"),
        (["run", "-i", fq, "-o", "s", "--report", rep], "--report needs a step or --adapters in run: ploidyfrost qc reports on files as they are"),
        (["run", "-i", fa, "-o", "s", "--fasta", "--report", rep], "--fasta does not go with --report"),
        (single + ["--fasta", "--report", rep], "--fasta does not go with trim"),
        (["qc", "-i", fa, "-o", rep, "--fasta"], "--fasta does not go with qc"),
        (["qc", "-o", rep], "-i <reads.fq> is missing"),
        (["qc", "-i", fq], "-o <report.tsv> is missing"),
        (["qc", "-i", fq, "-1", fq2, "-o", rep], "-i does not go with -1 / -2"),
        (["qc", "-i", fq, "-2", fq2, "-o", rep], "-i does not go with -1 / -2"),
        (["qc", "-i", fq, "-o", rep, "--phred", "50"], "--phred takes 33 or 64, not '50'"),
        (["qc", "-i", fq, "-o", fq], "qc: %s" % fq),
        (["qc", "-i", fa, "-o", rep], "qc: %s" % fa),                                        # FASTA by its first byte
        (["qc", "-i", gz, "-o", rep], "qc: %s" % gz),                                        # gzip without --gz
        (["qc", "-i", tmp_path / "none.fq", "-o", rep], "none.fq"),
        (["qc", "-i", fq, "-o", rep, "--report", rep], "unknown option --report"),
    ]
    for sub in ("mask", "count", "build", "build-multi", "run-multi"):
        cases.append(([sub, "--report", rep], "--report"))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    for sub in ("mask", "count", "build", "build-multi", "run-multi"):
        assert "unknown option --report" in run_cli(sub, "--report", rep, cwd=tmp_path).stderr
    usage = run_cli().stdout + run_cli().stderr
    assert "Usage: PloidyFrost qc (-i <a.fq> [-i <b.fq> ...] | -1 <r1.fq> [-1 ...] -2 <r2.fq> [-2 ...]) -o <report.tsv>" in usage and "[--report <report.tsv>]" in usage
    assert "--report report.tsv" in run_cli("trim").stderr and "--report report.tsv" in run_cli("run").stderr
    assert "unknown step (LEADING:t, TRAILING:t, SLIDINGWINDOW:w:t and MINLEN:l are known)" in run_cli(*(single + ["CROP:5", "--report", rep])).stderr


def test_python_refusals(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    with pytest.raises(RuntimeError, match="run: --report needs a step or --adapters in run"):
        hostapi.run_reads(fq, "s", report=tmp_path / "r.tsv")
    with pytest.raises(RuntimeError, match="qc: the quality offset is 33 or 64, not 50"):
        hostapi.qc_fastq(fq, tmp_path / "r.tsv", phred=50)
    with pytest.raises(RuntimeError, match="qc: no input"):
        hostapi.qc_fastq([], tmp_path / "r.tsv")
    with pytest.raises(RuntimeError, match=re.escape("trim: %s" % fq)):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", ["LEADING:3"], report=fq)
    with pytest.raises(RuntimeError, match="no step is given"):   # the switch went with the refused call
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [])
    with pytest.raises(RuntimeError, match="--report is not built into run-multi"):
        L = hostapi.load_library()
        L.pfh_reads_report(os.fsencode(str(tmp_path / "r.tsv")))
        hostapi.run_multi_reads([("a", fq)], "s")
    assert sorted(os.listdir(tmp_path)) == ["in.fq"]


# ---- the stand-alone program and the declarations ----

def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_qc_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of it
    is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_qc_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_qc_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    for s in ("pf_qc_begin", "pf_qc_get", "pf_qc_clip_get", "pf_qc_fastq", "pf_qc_end"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_reads_report", "pfh_qc_fastq", "pfh_qc_fastq_chunk", "pfh_qc_report_text", "pfh_qc_phred_hint"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_QC == hipapi.K_PALIN + 1
    assert (hipapi.QC_TABLE_WORDS, hipapi.QC_CLIP_WORDS) == (qc.TABLE_WORDS, qc.CLIP_WORDS) == (hostapi.QC_TABLE_WORDS, hostapi.QC_CLIP_WORDS)
    hdr = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    assert re.search(r"PF_K_CLIP,[^\n]*PF_K_PALIN,[^\n]*PF_K_QC,[^\n]*\n\s*PF_K_COUNT_", hdr)
    assert "#define PF_QC_TABLE_WORDS 9515u" in hdr and "#define PF_QC_CLIP_WORDS 1025u" in hdr
