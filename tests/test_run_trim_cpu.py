"""`ploidyfrost run STEP...` / `run-multi STEP...` without a GPU: the hand-on rule (csrc/pf_trimrun_rule.hpp) -- the stand-alone program
tests/cpp/test_trimrun_rule.cpp under the sanitizers, the host's restatement (hostapi.trim_table_chunk) against trim_cases --, the
conditions the GPU tests' generated inputs must meet, the declarations, and every refusal of the two sub-commands that comes before a
device context exists, by its text and with nothing left behind."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import trim_cases as tc
import trimrun_cases as trc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
WORKFLOW = tc.WORKFLOW


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_trimrun_rule.cpp: the shared headers alone, plain g++ with -fsanitize=address,undefined (host code only: nothing
    of it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_trimrun_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_trimrun_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def same(got, want):
    assert got["clause"] == "none"
    for f in ("read_off", "read_len", "bytes_used", "n_records", "stats"):
        assert got[f] == want[f], f
    assert got["n_reads"] == len(want["read_off"][0] if isinstance(want["bytes_used"], list) else want["read_off"])


def test_table_of_the_edge_records():
    recs = tc.edge_records()
    text = tc.fastq(recs)
    for steps in (WORKFLOW, tc.ORDERS[1], tc.ORDERS[3]):
        want = trc.table(text, steps)
        assert 0 < len(want["read_off"]) < len(recs)
        same(hostapi.trim_table_chunk(text, steps), want)
    t64 = tc.fastq(tc.edge_records(phred=64))
    want = trc.table(t64, WORKFLOW, phred=64)
    assert want["read_off"] == trc.table(text, WORKFLOW)["read_off"] and want["read_off"] != trc.table(t64, WORKFLOW)["read_off"]
    same(hostapi.trim_table_chunk(t64, WORKFLOW, phred=64), want)


def test_table_crlf_no_last_newline_and_a_chunk_that_ends_inside_a_record():
    recs = tc.make_reads(120, 7)
    for text, final in ((tc.fastq(recs, crlf=True), True), (tc.fastq(recs, last_newline=False), True),
                        (tc.fastq(recs, crlf=True, last_newline=False), True), (tc.fastq(recs)[:-200], False)):
        want = trc.table(text, WORKFLOW, final=final)
        assert len(want["read_off"]) > 10 and (final or want["bytes_used"] < len(text))
        same(hostapi.trim_table_chunk(text, WORKFLOW, final=final), want)


def test_table_of_a_pair():
    t1, t2 = tc.fastq(tc.make_reads(400, 1)), tc.fastq(tc.make_reads(400, 2))
    same(hostapi.trim_table_chunk(t1, WORKFLOW, text2=t2), trc.table_pair(t1, t2, WORKFLOW))
    # not final, different whole-record counts: the smaller count from each
    a, b = t1[:len(t1) // 2 + 3], t2[:len(t2) // 3 + 1]
    want = trc.table_pair(a, b, WORKFLOW, final=False)
    assert 0 < want["n_records"] < 200 and want["bytes_used"][0] < len(a) - 1000
    same(hostapi.trim_table_chunk(a, WORKFLOW, final=False, text2=b), want)
    # final, different counts: refused, 2 * record + the file that ends first
    three = tc.fastq(tc.make_reads(3, 1))
    got = hostapi.trim_table_chunk(t1, WORKFLOW, text2=three + b"@x\nAC\n+\nII\n")
    assert got["clause"] == "pair_count" and "different numbers of records" in got["message"] and got["bad_record"] == 2 * 4 + 1 and got["n_reads"] == 0
    bad = hostapi.trim_table_chunk(t1, WORKFLOW, text2=three.replace(b"@r1/", b"#r1/"))
    assert bad["clause"] == "header" and bad["bad_record"] == 2 * 1 + 1
    with pytest.raises(ValueError, match="no step is given"):
        hostapi.trim_table_chunk(t1, [])


def test_by_hand_three_records_k3():
    """LEADING:10 TRAILING:10 on three records: [2, 7) of AAACGTACC, a dropped record, [0, 4) of GGTTA.  The table starts behind the
    header lines; with k = 3 the two reads hold 3 + 2 windows, none of which touches a trimmed-off base."""
    q = lambda *x: tc.qline(list(x))
    text = tc.fastq([(b"a", b"AAACGTACC", q(2, 2, 30, 30, 30, 30, 30, 2, 2)), (b"b", b"ACGT", q(2, 2, 2, 2)), (b"c", b"GGTTA", q(30, 30, 30, 30, 2))])
    got = hostapi.trim_table_chunk(text, ["LEADING:10", "TRAILING:10"])
    assert got["read_off"] == [3 + 2, text.index(b"GGTTA")] and got["read_len"] == [5, 4] and got["n_records"] == 3 and got["bytes_used"] == len(text)
    assert [text[o:o + n] for o, n in zip(got["read_off"], got["read_len"])] == [b"ACGTA", b"GGTT"]
    assert got["stats"] == dict(reads=3, kept=2, dropped=1, bases=18, bases_kept=9, both=0, only1=0, only2=0, neither=0)
    assert sum(max(n - 3 + 1, 0) for n in got["read_len"]) == 5
    # as a pair with itself shifted by one record: a record goes on only when its partner is kept
    other = tc.fastq([(b"b", b"ACGT", q(2, 2, 2, 2)), (b"a", b"AAACGTACC", q(2, 2, 30, 30, 30, 30, 30, 2, 2)), (b"c", b"GGTTA", q(30, 30, 30, 30, 2))])
    pair = hostapi.trim_table_chunk(text, ["LEADING:10", "TRAILING:10"], text2=other)
    assert pair["n_reads"] == 1 and pair["read_len"] == [[4], [4]] and pair["stats"][0]["both"] == 1
    assert (pair["stats"][0]["only1"], pair["stats"][0]["only2"], pair["stats"][0]["neither"]) == (1, 1, 0)


def test_generated_inputs_are_not_vacuous():
    """what the GPU tests rely on: the pair shows all four outcomes, the reads all four shapes of an interval"""
    t1, t2 = tc.fastq(tc.make_reads(400, 1)), tc.fastq(tc.make_reads(400, 2))
    assert all(x >= 1 for x in trc.pair_outcomes(t1, t2, WORKFLOW))
    for recs in (tc.make_reads(400, 1), trc.genome_reads(500, 21)):
        dropped, whole, lead, trail = tc.outcome_shares(recs)
        assert dropped > 0 and whole > 0 and lead > 0 and trail > 0
    g1, g2 = tc.fastq(trc.genome_reads(300, 31, genome_seed=3)), tc.fastq(trc.genome_reads(300, 32, genome_seed=3))
    assert all(x >= 1 for x in trc.pair_outcomes(g1, g2, WORKFLOW))


def test_entry_points_are_declared():
    new_dev = ("pf_trim_table_fastq", "pf_trim_table_fastq_pair", "pf_count_fastq_trimmed", "pf_count_fastq_pair_trimmed",
               "pf_maskcount_fastq_trimmed", "pf_maskcount_fastq_pair_trimmed")
    for s in new_dev:
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_run_fastq_trimmed", "pfh_run_multi_fastq_trimmed", "pfh_trim_table_chunk", "pfh_trim_table_chunk_pair"):
        assert s in hostapi.DECLARED_SYMBOLS
    L, H = hipapi.load_library(), hostapi.load_library()
    for s in new_dev:
        getattr(L, s)
    getattr(H, "pfh_run_fastq_trimmed")
    assert hipapi.K_TRIMCOUNT == hipapi.K_COLORSET + 1
    assert L.pf_kernel_name(hipapi.K_TRIMCOUNT) == b"k_trimcount"
    # the old ids are unchanged
    names = {hipapi.K_DENSITY: b"k_density", hipapi.K_HIST: b"k_hist", hipapi.K_MASK: b"k_mask", hipapi.K_COUNT: b"k_count", hipapi.K_TRIM: b"k_trim",
             hipapi.K_UNITIG: b"k_unitig", hipapi.K_MASKCOUNT: b"k_maskcount", hipapi.K_UNION: b"k_union", hipapi.K_COLORSET: b"k_colorset"}
    for k, name in names.items():
        assert L.pf_kernel_name(k) == name
    for i, name in enumerate(hipapi.KERNELS):
        assert L.pf_kernel_name(i) == name.encode()
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_TRIMCOUNT" in text.split("PF_K_COLORSET,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    for who in (hostapi.run_reads, hostapi.run_multi_reads):
        assert {"steps", "phred", "pairs"} <= set(who.__code__.co_varnames)


# ---- the refusals that come before a device context exists (these pass on a machine without a GPU) ----

@pytest.fixture()
def files(tmp_path):
    a, b = tmp_path / "a.fq", tmp_path / "b.fq"
    a.write_bytes(tc.fastq(tc.make_reads(20, 1)))
    b.write_bytes(tc.fastq(tc.make_reads(20, 2)))
    os.link(a, tmp_path / "a_again.fq")                 # one file under two names
    (tmp_path / "in.fa").write_bytes(b">s\nACGT\n")
    (tmp_path / "in.fq.gz").write_bytes(b"\x1f\x8b\x08\x00rest")
    (tmp_path / "same.gfa").write_bytes(tc.fastq(tc.make_reads(3, 3)))
    return tmp_path


def refused(tmp_path, cases):
    before = sorted(os.listdir(tmp_path))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args, r.stdout, r.stderr)
        assert "no device context" not in r.stderr, args
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file, no output directory


def test_run_refusals(files):
    step = ["MINLEN:5"]
    pair = ["run", "-1", "a.fq", "-2", "b.fq", "-o", "r"]
    single = ["run", "-i", "a.fq", "-o", "r"]
    refused(files, [
        (["run", "-1", "a.fq", "-o", "r"] + step, "-1 a.fq has no -2 behind it"),
        (["run", "-1", "a.fq", "-1", "b.fq", "-2", "b.fq", "-o", "r"] + step, "-1 a.fq has no -2 behind it"),
        (["run", "-2", "b.fq", "-o", "r"] + step, "-2 b.fq has no -1 in front of it"),
        (pair, "-1 / -2 need a step"),
        (pair, "two files without trimming go with -i"),
        (["run", "-i", "a.fq"] + pair[1:] + step, "-i does not go with -1 / -2"),
        (single + ["--phred", "64"], "--phred needs a step"),
        (single + ["--phred", "50"] + step, "--phred takes 33 or 64, not '50'"),
        (single + ["--phred"], "--phred needs a value"),
        (single + step + ["--trimlog", "log.txt"], "--trimlog is not built into run: `trim` writes"),
        (pair + step + ["-o1", "x.fq"], "-o1 is not built into run"),
        (pair + step + ["-u1", "x.fq"], "-u1 is not built into run"),
        (pair + step + ["-o2", "x.fq"], "-o2 is not built into run"),
        (pair + step + ["-u2", "x.fq"], "-u2 is not built into run"),
        (["run", "-1", "a.fq", "-2", "a.fq", "-o", "r"] + step, "a.fq is given twice"),
        (["run", "-i", "a.fq", "-i", "b.fq", "-i", "a.fq", "-o", "r"] + step, "a.fq is given twice"),
        (["run", "-1", "a.fq", "-2", "a_again.fq", "-o", "r"] + step, "a_again.fq and a.fq are one file"),
        # the steps: `trim`'s parser, refusals and texts
        (single + ["CROP:5"], "CROP:5: unknown step (LEADING:t, TRAILING:t, SLIDINGWINDOW:w:t and MINLEN:l are known)"),
        (single + ["leading:5"], "leading:5: unknown step"),
        (single + ["LEADING"], "LEADING: a field of the step is missing or is not a number"),
        (single + ["LEADING:94"], "LEADING:94: a value of the step is out of range"),
        (single + ["SLIDINGWINDOW:0:20"], "SLIDINGWINDOW:0:20: a value of the step is out of range"),
        (single + ["MINLEN:1"] * 9, "more than 8 steps"),
        # everything `run` refuses today, on the -1 / -2 files as well
        (["run", "-1", "a.fq", "-2", "in.fa", "-o", "r"] + step, "in.fa: record 1: the input is FASTA"),
        (["run", "-1", "in.fq.gz", "-2", "b.fq", "-o", "r"] + step, "in.fq.gz: record 1: the input is gzip-compressed"),
        (["run", "-1", "a.fq", "-2", "same.gfa", "-o", "r", "--gfa-out", "same"] + step, "same.gfa: the output path is an input path"),
        (["run", "-1", "a.fq", "-2", "missing.fq", "-o", "r"] + step, "cannot read missing.fq"),
        (pair[:5] + step, "-o <sample> is missing"),
        (pair + step + ["-k", "32"], "-k goes from 3 to 31"),
        (pair + step + ["-l", "5"], "-l does not go with run"),
    ])


def test_run_multi_refusals(files):
    step = ["MINLEN:5"]
    ok = ["run-multi", "--sample", "s", "-1", "a.fq", "-2", "b.fq", "-o", "r"]
    refused(files, [
        (ok, "-1 / -2 need a step"),
        (["run-multi", "-1", "a.fq", "-2", "b.fq", "-o", "r"] + step, "-1 stands before any --sample NAME"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "--sample", "t", "-i", "b.fq", "-o", "r"] + step, "-1 a.fq has no -2 behind it"),
        (["run-multi", "--sample", "s", "-2", "b.fq", "-o", "r"] + step, "-2 b.fq has no -1 in front of it"),
        (["run-multi", "--sample", "s", "-i", "a.fq", "-1", "a.fq", "-2", "b.fq", "-o", "r"] + step, "sample s: -i does not go with -1 / -2"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "b.fq", "-i", "a.fq", "-o", "r"] + step, "sample s: -i does not go with -1 / -2"),
        (["run-multi", "--sample", "s", "-i", "a.fq", "-o", "r", "--phred", "64"], "--phred needs a step"),
        (ok + step + ["--phred", "12"], "--phred takes 33 or 64, not '12'"),
        (ok + step + ["--trimlog", "x"], "--trimlog is not built into run-multi"),
        (ok + step + ["-u2", "x"], "-u2 is not built into run-multi"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "a.fq", "-o", "r"] + step, "sample s: a.fq is given twice"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "a_again.fq", "-o", "r"] + step, "a_again.fq and a.fq are one file"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "b.fq", "--sample", "t", "-i", "a_again.fq", "-o", "r"] + step, "the same file is given in two samples"),
        (ok + ["ILLUMINACLIP:x.fa:2:30:10"], "ILLUMINACLIP:x.fa:2:30:10: unknown step"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "in.fa", "-o", "r"] + step, "in.fa: record 1: the input is FASTA"),
        (["run-multi", "--sample", "s", "-1", "a.fq", "-2", "b.fq", "--sample", "s", "-i", "a.fq", "-o", "r"] + step, "sample s is given twice"),
        (ok[:-2] + step, "-o <out> is missing"),
    ])


def test_without_a_step_nothing_is_new(files):
    """`run -i x.fq -o r` and `run-multi --sample s -i x.fq -o r` with no step pass every refusal and reach the device context (or, on a
    machine with a GPU, run): no new refusal stands in their way.  A file given twice is still taken without steps, as before."""
    for args in (["run", "-i", "a.fq", "-o", "r"], ["run", "-i", "a.fq", "-i", "a.fq", "-o", "r"], ["run-multi", "--sample", "s", "-i", "a.fq", "-o", "r"],
                 ["run", "-i", "a.fq", "-o", "r", "MINLEN:5"], ["run", "-1", "a.fq", "-2", "b.fq", "-o", "r", "LEADING:3", "--phred", "64"],
                 ["run-multi", "--sample", "s", "-1", "a.fq", "-2", "b.fq", "--sample", "t", "-i", "same.gfa", "-o", "r", "MINLEN:5"]):
        r = run_cli(*args, cwd=files)
        assert r.returncode == 0 or "no device context" in r.stderr, (args, r.stderr)
    for sub in ("run", "run-multi"):
        assert "STEP..." in run_cli(sub, cwd=files).stderr


def test_api_refusals(files, monkeypatch):
    monkeypatch.chdir(files)
    with pytest.raises(RuntimeError, match="run: -1 / -2 need a step|run: the files of a pair are trimmed together"):
        hostapi.run_reads(None, "r", pairs=[("a.fq", "b.fq")])
    with pytest.raises(RuntimeError, match="run: a.fq is given twice"):
        hostapi.run_reads(None, "r", pairs=[("a.fq", "a.fq")], steps=WORKFLOW)
    with pytest.raises(RuntimeError, match="run: the quality offset is 33 or 64, not 50"):
        hostapi.run_reads("a.fq", "r", steps=WORKFLOW, phred=50)
    with pytest.raises(ValueError, match="unknown step"):
        hostapi.run_reads("a.fq", "r", steps=["CROP:4"])
    with pytest.raises(RuntimeError, match="run-multi: sample s: a.fq is given twice"):
        hostapi.run_multi_reads([("s", ["a.fq", "a.fq"])], "r", steps=WORKFLOW, pairs=["s"])
    with pytest.raises(RuntimeError, match="run-multi: sample s: in.fa: the first file of a pair without its second"):
        hostapi.run_multi_reads([("s", ["a.fq", "b.fq", "in.fa"])], "r", steps=WORKFLOW, pairs=["s"])
