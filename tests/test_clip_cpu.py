"""The rule of adapter clipping (K-CLIP, `--adapters`) without a GPU: the Python restatement of clip_cases.py on the hand-worked reads,
the host's plain restatement (pfh_clip_read / pfh_clip_parse_adapters / pfh_trim_fastq_chunk_clip, csrc/pf_clip_rule.hpp) against it on
hand, edge and generated reads, chunks (CRLF, no last newline, a record cut in each of its lines), the refusals of the file, the
values and the sub-commands by their texts, the stand-alone program tests/cpp/test_clip_rule.cpp under the sanitizers, and the
declarations."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

import clip_cases as cc
import trim_cases as tc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 16, 128], seed=3, sides=[0, 1, 2, 0])


@pytest.fixture(scope="module")
def generated(adapters):
    return cc.make_reads(300, adapters, seed=9)


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


# ---- the rule ----

def test_python_rule_by_hand():
    for seq, qual, ads, side, seed, score, phred, end in cc.hand_cases():
        assert cc.clip_read(seq, qual, ads, side, seed, score, phred)[0] == end, (seq, ads, side, seed, score, phred)
    assert 17 * cc.MATCH == 1023502 and 16 * cc.MATCH == 963296


def test_host_rule_on_hand_cases():
    for seq, qual, ads, side, seed, score, phred, end in cc.hand_cases():
        assert hostapi.clip_read(seq, qual, ads, side, seed, score, phred, scored=True) == cc.clip_read(seq, qual, ads, side, seed, score, phred)
        assert hostapi.clip_read(seq, qual, ads, side, seed, score, phred) == end


def test_host_rule_on_edge_reads():
    """every read length x adapter length x edge offset: the first offset, -1, 0, 1, n - 16 (a candidate) and n - 15 (none)"""
    n_clipped = n_untouched = 0
    for seq, qual, ads in cc.edge_reads():
        want = cc.clip_read(seq, qual, ads)
        assert hostapi.clip_read(seq, qual, ads, scored=True) == want, (len(seq), len(ads[0][0]))
        n_clipped += want[0] != len(seq)
        n_untouched += want[0] == len(seq)
    assert n_clipped > 50 and n_untouched > 50
    # n - 16 is the last candidate: 16 matches hold the seed but not T = 10; with T = 9 they pass; n - 15 is none
    ad = cc.make_adapters([33], 21)[0][0]
    for n in (100, 257):
        seq = cc.plant(__import__("random").Random(n), n, ad, n - 16)
        assert hostapi.clip_read(seq, b"I" * n, [(ad, 0)], score=9) == n - 16 and hostapi.clip_read(seq, b"I" * n, [(ad, 0)], score=10) == n
        seq = seq[:-1]
        assert hostapi.clip_read(seq, b"I" * (n - 1), [(ad, 0)], score=1, scored=True) == cc.clip_read(seq, b"I" * (n - 1), [(ad, 0)], score=1)


@pytest.mark.parametrize("seed,score,phred", [(2, 10, 33), (0, 7, 33), (8, 1, 64), (3, 30, 33)])
def test_host_rule_on_generated_reads(generated, adapters, seed, score, phred):
    outcomes = set()
    for side in (1, 2):
        for _, seq, qual in generated:
            want = cc.clip_read(seq, qual, adapters, side, seed, score, phred)
            assert hostapi.clip_read(seq, qual, adapters, side, seed, score, phred, scored=True) == want
            outcomes.add("untouched" if want[0] == len(seq) else "dropped" if want[0] == 0 else "clipped")
    if (seed, score) == (2, 10):
        assert outcomes == {"untouched", "dropped", "clipped"}


# ---- chunks ----

def _chunk(text, steps, adapters, final=True, side=1):
    got = hostapi.trim_fastq_chunk_clip(text, steps, adapters, side=side, final=final)
    want = cc.trim_fastq(text, steps, adapters, side=side, final=final)
    assert got["clause"] == "none"
    for key in ("out", "bytes_used", "n_records", "begin", "len"):
        assert got[key] == want[key], key
    assert {k: v[side - 1] for k, v in got["clip"].items()} == want["clip"] and all(v[2 - side] == 0 for v in got["clip"].values())
    return got


@pytest.mark.parametrize("steps", [[], tc.WORKFLOW, ["MINLEN:40"]], ids=["none", "workflow", "minlen"])
def test_host_chunk_against_python(generated, adapters, steps):
    recs = generated[:120]
    plain = _chunk(tc.fastq(recs), steps, adapters)
    assert _chunk(tc.fastq(recs, crlf=True), steps, adapters)["out"] == plain["out"]
    assert _chunk(tc.fastq(recs, last_newline=False), steps, adapters)["out"] == plain["out"]
    _chunk(tc.fastq(recs), steps, adapters, side=2)
    # the clipped interval is what the steps see: the same as trimming the text clipped beforehand
    clipped, _ = cc.clip_fastq(tc.fastq(recs), adapters)
    if steps:
        assert hostapi.trim_fastq_chunk(clipped, steps)["out"] == plain["out"]


def test_host_chunk_cut_inside_every_line(generated, adapters):
    recs = generated[:5]
    text, head = tc.fastq(recs), tc.fastq(recs[:4])
    whole = _chunk(head, [], adapters)
    for cut in range(len(head), len(text)):   # the fifth record cut at every byte: four whole records are taken
        got = _chunk(text[:cut], [], adapters, final=False)
        assert (got["out"], got["bytes_used"], got["n_records"]) == (whole["out"], len(head), 4), cut


def test_host_chunk_format_clause_writes_nothing(adapters):
    got = hostapi.trim_fastq_chunk_clip(b"@a\nAC\n+\nII\n@b\nAC\n+\nIII\n", [], adapters)
    assert (got["clause"], got["bad_record"], got["out"], got["n_records"]) == ("quality", 1, b"", 0)
    assert all(v == [0, 0] for v in got["clip"].values())


# ---- the adapter file ----

def test_parser_against_python(adapters):
    for kw in (dict(), dict(crlf=True), dict(wrap=7), dict(prefix_entries=3), dict(prefix_entries=2, crlf=True, wrap=20)):
        text = cc.adapters_fa(adapters, **kw)
        for t in (text, text.rstrip(b"\r\n"), text.lower().replace(b">a", b">A").replace(b">prefix", b">Prefix")):
            want = cc.parse_adapters(t)
            got = hostapi.clip_parse_adapters(t)
            assert [s for s, _ in want[0]] == [got["bases"][got["off"][i]:got["off"][i + 1]] for i in range(got["n"])]
            assert [sd for _, sd in want[0]] == got["side"].tolist() == [0, 1, 2, 0]
            assert got["skipped"] == want[2] == kw.get("prefix_entries", 0)


def test_parser_on_a_file_cut_at_every_byte(adapters):
    text = cc.adapters_fa(adapters[:3], prefix_entries=1, wrap=25)
    for cut in range(len(text) + 1):
        want = cc.parse_adapters(text[:cut])
        try:
            got = hostapi.clip_parse_adapters(text[:cut])
        except ValueError as e:
            assert (e.refusal, e.bad_record) == want, cut
            continue
        assert len(want) == 3 and [s for s, _ in want[0]] == [got["bases"][got["off"][i]:got["off"][i + 1]] for i in range(got["n"])], cut


A16, A129 = b"ACGT" * 4, b"ACGT" * 32 + b"A"


@pytest.mark.parametrize("text,name,record,word", [
    (b"", "not_fasta", 0, "the adapter file is empty or is not FASTA"),
    (b"\n\n", "not_fasta", 0, "the adapter file is empty or is not FASTA"),
    (b"@r\n" + A16 + b"\n+\n" + b"I" * 16 + b"\n", "not_fasta", 0, "is not FASTA"),
    (b">a\n" + A16 + b"\n>b\n" + A16[:8] + b"N" + A16[9:] + b"\n", "byte", 2, "record 2: an adapter holds a byte outside ACGTacgt"),
    (b">a\n" + A16[:15] + b"\n", "length", 1, "record 1: an adapter holds 16 to 128 bases"),
    (b">a\n" + A16 + b"\n>b\n" + A129 + b"\n", "length", 2, "record 2: an adapter holds 16 to 128 bases"),
    (b">a\n" + A16 + b"\n>b\n>c\n" + A16 + b"\n", "length", 2, "record 2: an adapter holds 16 to 128 bases"),
    (b"".join(b">a%d\n" % i + A16 + b"\n" for i in range(65)), "too_many", 65, "more than 64 usable adapters"),
    (b">PrefixPE/1\n" + A16 + b"\n>PrefixPE/2\n" + A16 + b"\n", "no_adapter", 0, "no usable adapter"),
])
def test_file_refusals_by_name(text, name, record, word):
    assert cc.parse_adapters(text) == (name, record)
    with pytest.raises(ValueError) as e:
        hostapi.clip_parse_adapters(text)
    assert (e.value.refusal, e.value.bad_record) == (name, record) and word in str(e.value)


def test_value_refusals_by_name(adapters):
    seq = b"ACGT" * 10
    for kw, word in ((dict(seed=9), "the adapter seed is 0 to 8 mismatches"), (dict(score=0), "the adapter score is 1 to 1000"),
                     (dict(score=1001), "the adapter score is 1 to 1000"), (dict(side=3), "the side of a file is 1 or 2"),
                     (dict(side=0), "the side of a file is 1 or 2"), (dict(phred=50), "the quality offset is 33 or 64, not 50")):
        with pytest.raises(ValueError, match=word):
            hostapi.clip_read(seq, b"I" * 40, adapters, **kw)
    for ads, word in (([], "no usable adapter"), ([(A16[:15], 0)], "an adapter holds 16 to 128 bases"), ([(A129, 0)], "an adapter holds 16 to 128 bases"),
                      ([(A16, 0)] * 65, "more than 64 usable adapters"), ([(A16[:15] + b"N", 0)], "an adapter holds a byte outside ACGTacgt"),
                      ([(A16, 3)], "the side of an adapter is 0")):
        with pytest.raises(ValueError, match=word):
            hostapi.clip_read(seq, b"I" * 40, ads)
    assert hostapi.clip_read(seq, b"I" * 40, [(A16, 0)] * 64, score=9) == 0   # 64 adapters are taken (the read starts with them: 16 matches reach T = 9)


# ---- the sub-commands' refusals: by name, before any device work (this passes on a machine without a GPU) ----

def test_cli_refusals(tmp_path, adapters):
    fq, fq2, fa = tmp_path / "in.fq", tmp_path / "in2.fq", tmp_path / "in.fa"
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    fq2.write_bytes(tc.fastq(tc.make_reads(3, 2)))
    fq3 = tmp_path / "in3.fq"
    fq3.write_bytes(tc.fastq(tc.make_reads(3, 3)))
    fa.write_bytes(b">s\nACGT\n")
    ad, short, empty, prefix = tmp_path / "ad.fa", tmp_path / "short.fa", tmp_path / "empty.fa", tmp_path / "prefix.fa"
    ad.write_bytes(cc.adapters_fa(adapters))
    short.write_bytes(b">a\n" + A16 + b"\n>b\nACGT\n")
    empty.write_bytes(b"")
    prefix.write_bytes(b">PrefixPE/1\n" + A16 + b"\n")
    before = sorted(os.listdir(tmp_path))
    out = tmp_path / "out.fq"
    o = [tmp_path / n for n in ("p1.fq", "u1.fq", "p2.fq", "u2.fq")]
    single = ["trim", "-i", fq, "-o", out]
    pair = ["trim", "-1", fq, "-2", fq2, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3]]
    run1 = ["run", "-i", fq, "-o", "s"]
    runp = ["run", "-1", fq, "-2", fq2, "-o", "s"]
    multi = ["run-multi", "--sample", "a", "-1", fq, "-2", fq2, "--sample", "b", "-i", fq3, "-o", "s"]
    cases = []
    for cmd in (single, pair, run1, runp, multi):
        cases += [
            (cmd + ["--adapter-seed", "2"], "--adapter-seed needs --adapters"),
            (cmd + ["--adapter-score", "10"], "--adapter-score needs --adapters"),
            (cmd + ["--adapters"], "--adapters needs a value"),
            (cmd + ["--adapters", ad, "--adapter-seed", "9"], "--adapter-seed takes 0 to 8, not '9'"),
            (cmd + ["--adapters", ad, "--adapter-seed", "x"], "--adapter-seed takes 0 to 8, not 'x'"),
            (cmd + ["--adapters", ad, "--adapter-score", "0"], "--adapter-score takes 1 to 1000, not '0'"),
            (cmd + ["--adapters", ad, "--adapter-score", "1001"], "--adapter-score takes 1 to 1000, not '1001'"),
            (cmd + ["--adapters", short], "adapters %s: record 2: an adapter holds 16 to 128 bases" % short),
            (cmd + ["--adapters", empty], "adapters %s: the adapter file is empty or is not FASTA" % empty),
            (cmd + ["--adapters", fq], "adapters %s: the adapter file is empty or is not FASTA" % fq),
            (cmd + ["--adapters", prefix], "adapters %s: no usable adapter" % prefix),
            (cmd + ["--adapters", tmp_path / "none.fa"], "adapters %s: cannot be opened" % (tmp_path / "none.fa")),
            # the word itself stays refused, with the same text
            (cmd + ["--adapters", ad, "ILLUMINACLIP:a.fa:2:30:10"], "ILLUMINACLIP:a.fa:2:30:10: unknown step (LEADING:t, TRAILING:t, SLIDINGWINDOW:w:t and MINLEN:l are known)"),
            (cmd + ["--adapters", ad, "CROP:5"], "CROP:5: unknown step (LEADING:t, TRAILING:t, SLIDINGWINDOW:w:t and MINLEN:l are known)"),
        ]
    cases += [
        (single + ["--adapters", ad, "--fasta"], "--fasta does not go with trim"),
        (["run", "-i", fa, "-o", "s", "--fasta", "--adapters", ad], "--fasta does not go with --adapters"),
        (single, "no step is given"),
        (runp, "-1 / -2 need a step"),
    ]
    for sub in ("mask", "count", "build", "build-multi"):
        cases.append(([sub, "--adapters", ad], "--adapters"))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    usage = run_cli().stdout + run_cli().stderr
    assert "--adapters <adapters.fa> [--adapter-seed 0..8] [--adapter-score 1..1000]" in usage
    assert "--adapters adapters.fa" in run_cli("trim").stderr


def test_python_refusals(tmp_path, adapters):
    fq = tmp_path / "in.fq"
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    short = tmp_path / "short.fa"
    short.write_bytes(b">a\nACGT\n")
    with pytest.raises(RuntimeError, match="trim: adapters %s: record 1: an adapter holds 16 to 128 bases" % re.escape(str(short))):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [], adapters=short)
    with pytest.raises(RuntimeError, match="run: adapters %s: record 1: an adapter holds 16 to 128 bases" % re.escape(str(short))):
        hostapi.run_reads(fq, "s", adapters=short)
    ad = tmp_path / "ad.fa"
    ad.write_bytes(cc.adapters_fa(adapters))
    with pytest.raises(RuntimeError, match="trim: the adapter seed is 0 to 8 mismatches"):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [], adapters=ad, adapter_seed=9)
    with pytest.raises(RuntimeError, match="the adapter score is 1 to 1000"):
        hostapi.run_multi_reads([("a", fq)], "s", adapters=ad, adapter_score=0)
    # an empty list of steps beside adapters is "adapters alone" in all four calls (the file's refusal is reached, not `no step`)
    for call in (lambda: hostapi.run_reads(fq, "s", steps=[], adapters=short), lambda: hostapi.run_multi_reads([("a", fq)], "s", steps=[], adapters=short),
                 lambda: hostapi.trim_fastq(fq, tmp_path / "o.fq", [], adapters=short),
                 lambda: hostapi.trim_fastq_pair(fq, fq, [tmp_path / n for n in "abcd"], [], adapters=short)):
        with pytest.raises(RuntimeError, match="record 1: an adapter holds 16 to 128 bases"):
            call()
    # the switch is taken by the call it was set for, also when that call refuses its arguments at once
    L = hostapi.load_library()
    L.pfh_reads_adapters(os.fsencode(str(ad)), 2, 10)
    assert L.pfh_trim_fastq(None, 1, None, None, 0, 33, None, 0, 0, None) != 0 and b"inputs and output are needed" in L.pfh_last_error(None)
    with pytest.raises(RuntimeError, match="no step is given"):
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [])
    with pytest.raises(RuntimeError, match="no step is given"):   # without adapters: as before
        hostapi.trim_fastq(fq, tmp_path / "o.fq", [])
    assert sorted(os.listdir(tmp_path)) == ["ad.fa", "in.fq", "short.fa"]


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_clip_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_clip_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_clip_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    for s in ("pf_clip_begin", "pf_clip_stats_get", "pf_clip_end"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_clip_parse_adapters", "pfh_clip_read", "pfh_trim_fastq_chunk_clip", "pfh_reads_adapters", "pfh_reads_adapters_report"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_CLIP == hipapi.K_DEFLATE + 1
    hdr = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    assert re.search(r"PF_K_CLIP,[^\n]*\n\s*PF_K_COUNT_", hdr)
