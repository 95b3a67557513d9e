"""Palindrome adapter clipping (K-PALIN, `--adapter-pairs`) without a GPU: the Python restatement of clip_pair_cases.py on the
hand-worked pairs, the host's plain restatement (pfh_clip_pair / pfh_clip_parse_adapter_pairs / pfh_trim_fastq_pair_chunk_clip,
csrc/pf_clip_rule.hpp) against it on hand, edge and generated pairs and chunks, the refusals of the file, the values and the
sub-commands by their texts, the stand-alone program tests/cpp/test_clip_pair_rule.cpp under the sanitizers, and the declarations."""
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

import clip_cases as cc
import clip_pair_cases as pc
import trim_cases as tc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
STEPS = ["LEADING:5", "TRAILING:5", "MINLEN:20"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


@pytest.fixture(scope="module")
def prefix_pairs():
    return pc.make_prefix_pairs([34], seed=41)


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 20], seed=3, sides=[0, 1, 2])


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def host_pair(s1, q1, s2, q2, ads, pairs, **opt):
    return hostapi.clip_pair(s1, q1, s2, q2, (ads, pairs), stats=True, **opt)


def same_as_python(s1, q1, s2, q2, ads, pairs, **opt):
    """the host rule and the Python rule agree on the ends, the counters and the candidates scored; returns the ends"""
    ends, clip, ps = host_pair(s1, q1, s2, q2, ads, pairs, **opt)
    want, simple, I, too_long, scored = pc.clip_pair(s1, q1, s2, q2, ads, pairs, **opt)
    assert ends == want, (len(s1), len(s2), opt)
    assert ps["candidates_scored"] == scored and ps["pairs_too_long"] == int(too_long)
    assert ps["pairs_clipped"] == int(I is not None and I != 0) and ps["pairs_dropped"] == int(I == 0)
    assert ps["bases_clipped"] == [simple[0] - want[0], simple[1] - want[1]]
    n = [len(s1), len(s2)]
    assert clip["bases_clipped"] == [n[f] - want[f] for f in range(2)]
    assert clip["reads_clipped"] == [int(want[f] not in (0, n[f])) for f in range(2)]
    assert clip["reads_dropped"] == [int(want[f] == 0 and n[f] != 0) for f in range(2)]
    return ends


# ---- the rule ----

def test_python_rule_by_hand():
    for s1, q1, s2, q2, ads, pairs, opt, ends in pc.hand_cases():
        assert pc.clip_pair(s1, q1, s2, q2, ads, pairs, **opt)[0] == ends, opt
    assert 50 * pc.MATCH == 3010300 and 49 * pc.MATCH == 2950094 < 30 * pc.UNIT <= 50 * pc.MATCH


def test_host_rule_on_hand_cases():
    for s1, q1, s2, q2, ads, pairs, opt, ends in pc.hand_cases():
        assert same_as_python(s1, q1, s2, q2, ads, pairs, **opt) == ends, opt


def test_tandem_repeat_insert_passes_below_the_true_insert(prefix_pairs):
    """the known property: (AT)n is its own reverse complement at every even shift, so a smaller I passes; the smallest wins"""
    rng = random.Random(2)
    r1, r2 = pc.read_through(rng, 100, 100, 60, *prefix_pairs[0], insert=b"AT" * 30)
    ends = same_as_python(r1, b"I" * 100, r2, b"I" * 100, [], prefix_pairs, keep_both=True)
    assert ends[0] == ends[1] and ends[0] < 60 and ends[0] % 2 == 0


def test_host_rule_on_the_edge_grid():
    """read lengths 0 .. 1025 (equal and unequal) x prefix lengths 16 .. 128 x planted I in {0, 1, n - A}"""
    seen = set()
    for s1, q1, s2, q2, pairs in pc.edge_pairs():
        for opt in (dict(), dict(keep_both=True, pair_min=1, seed=0)):
            ends = same_as_python(s1, q1, s2, q2, [], pairs, **opt)
            seen.add("too_long" if max(len(s1), len(s2)) > 1024 else "dropped" if ends == [0, 0] else "untouched" if ends == [len(s1), len(s2)] else "clipped")
    assert seen == {"too_long", "dropped", "untouched", "clipped"}


def test_host_rule_finds_every_planted_insert(prefix_pairs):
    """reads of 50 and 151 bases at q 40: every planted I from 0 to n - 8 is found exactly, n - 7 is not"""
    rng = random.Random(6)
    for n in (50, 151):
        for I in range(0, n - 7 + 1):
            r1, r2 = pc.read_through(rng, n, n, I, *prefix_pairs[0])
            got = hostapi.clip_pair(r1, b"I" * n, r2, b"I" * n, ([], prefix_pairs), keep_both=True)
            assert got == ([I, I] if I <= n - 8 else [n, n]), (n, I)


def test_host_chunks_on_300_seeded_pairs(prefix_pairs, adapters):
    f1, f2 = pc.make_pairs(300, prefix_pairs, seed=5, adapters=adapters)
    t1, t2 = tc.fastq(f1), tc.fastq(f2)
    for ads, opt in ((adapters, dict()), ([], dict(keep_both=True)), (adapters, dict(keep_both=True, seed=1, pair_score=20, pair_min=4))):
        got = hostapi.trim_fastq_pair_chunk_clip(t1, t2, STEPS, (ads, prefix_pairs), **opt)
        assert got["clause"] == "none" and got["n_records"] == 300 and got["bytes_used"] == [len(t1), len(t2)]
        ends = [pc.clip_pair(a[1], a[2], b[1], b[2], ads, prefix_pairs, **opt) for a, b in zip(f1, f2)]
        assert got["clip_end"] == [[e[0][f] for e in ends] for f in range(2)]
        assert got["pairs"]["pairs_clipped"] == sum(e[2] not in (None, 0) for e in ends) > 60
        assert got["pairs"]["candidates_scored"] == sum(e[4] for e in ends)
        out = [bytearray() for _ in range(4)]
        for r, (a, b) in enumerate(zip(f1, f2)):
            iv = []
            for f, rec in enumerate((a, b)):
                e = ends[r][0][f]
                x = tc.trim_read(tc.quals(rec[2][:e], 33), STEPS) if e else None
                iv.append(x if x and x[1] > x[0] else None)
                assert (got["begin"][f][r], got["len"][f][r]) == ((x[0], x[1] - x[0]) if iv[f] else (0, 0))
            for f, rec in enumerate((a, b)):
                if iv[f]:
                    out[2 * f + (0 if iv[1 - f] else 1)] += tc.record_bytes((b"@" + rec[0], rec[1], b"+", rec[2]), *iv[f])
        assert got["out"] == [bytes(o) for o in out]
        assert got["stats"][0]["both"] == got["stats"][1]["both"] == got["out"][0].count(b"\n") // 4


def test_host_chunk_where_file_2_holds_fewer_whole_records(prefix_pairs):
    f1, f2 = pc.make_pairs(12, prefix_pairs, seed=8, lengths=(40, 80))
    t1, t2 = tc.fastq(f1), tc.fastq(f2)
    cut = t2[: len(t2) - 25]
    got = hostapi.trim_fastq_pair_chunk_clip(t1, cut, [], ([], prefix_pairs), final=False)
    whole = hostapi.trim_fastq_pair_chunk_clip(t1, t2, [], ([], prefix_pairs))
    assert got["n_records"] == 11 and got["bytes_used"] == [len(tc.fastq(f1[:11])), len(tc.fastq(f2[:11]))]
    assert got["clip_end"] == [x[:11] for x in whole["clip_end"]]
    assert hostapi.trim_fastq_pair_chunk_clip(t1, tc.fastq(f2[:11]), [], ([], prefix_pairs))["clause"] == "pair_count"


def test_remnants_of_1_to_15_bases_need_pair_mode(prefix_pairs):
    """inserts that leave 1 .. 15 adapter bases: simple mode (the prefixes' reverse complements as its adapters, what reads through)
    leaves every such read untouched, pair mode clips them"""
    P1, P2 = prefix_pairs[0]
    simple = [(pc.revcomp(P2), 1), (pc.revcomp(P1), 2)]
    rng = random.Random(12)
    for left in range(1, 16):
        r1, r2 = pc.read_through(rng, 100, 100, 100 - left, P1, P2)
        q = b"I" * 100
        assert hostapi.clip_read(r1, q, simple, side=1) == 100 and hostapi.clip_read(r2, q, simple, side=2) == 100
        got = hostapi.clip_pair(r1, q, r2, q, (simple, prefix_pairs), pair_min=1, keep_both=True)
        assert got == [100 - left] * 2
        assert hostapi.clip_pair(r1, q, r2, q, (simple, prefix_pairs), keep_both=True) == ([100 - left] * 2 if left >= 8 else [100, 100])
    r1, r2 = pc.read_through(rng, 100, 100, 60, P1, P2)   # 40 adapter bases: both modes see them
    assert hostapi.clip_read(r1, q, simple, side=1) == 60 and hostapi.clip_pair(r1, q, r2, q, (simple, prefix_pairs)) == [60, 0]


# ---- the adapter file ----

def refusal_files():
    b34, b20 = b"ACGT" * 8 + b"AC", b"TTGCA" * 4
    pe = lambda x, s, seq: b">Prefix" + x + b"/%d\n" % s + seq + b"\n"
    nine = b"".join(pe(b"P%d" % q, 1, b34) + pe(b"P%d" % q, 2, b34) for q in range(9))
    return [
        (pe(b"PE", 1, b34), "pair_partner", 1, "a Prefix entry needs its partner"),
        (b">a\n" + b20 + b"\n" + pe(b"PE", 2, b34) + b">b\n" + b20 + b"\n", "pair_partner", 2, "a Prefix entry needs its partner"),
        (b">PrefixPE\n" + b34 + b"\n", "pair_partner", 1, "a Prefix entry needs its partner"),
        (pe(b"PE", 1, b34) + pe(b"PE", 1, b34), "pair_partner", 2, "a Prefix entry needs its partner"),
        (pe(b"PE", 1, b34) + pe(b"PE", 2, b34) + pe(b"PE", 1, b34), "pair_partner", 3, "a Prefix entry needs its partner"),
        (pe(b"PE", 1, b34) + pe(b"PE", 2, b20), "pair_lengths", 2, "the two entries of a prefix pair hold the same number of bases"),
        (pe(b"PE", 1, b34[:15]) + pe(b"PE", 2, b34[:15]), "length", 1, "an adapter holds 16 to 128 bases"),
        (pe(b"PE", 1, b34) + pe(b"PE", 2, b34 * 4), "length", 2, "an adapter holds 16 to 128 bases"),
        (pe(b"PE", 1, b34) + pe(b"PE", 2, b34[:33] + b"N"), "byte", 2, "an adapter holds a byte outside ACGTacgt"),
        (nine, "too_many_pairs", 18, "more than 8 prefix pairs"),
        (b">a\n" + b20 + b"\n", "no_pair", 0, "no prefix pair"),
        (b"", "not_fasta", 0, "the adapter file is empty or is not FASTA"),
    ]


def test_adapter_file_refusals_by_text_and_record(tmp_path):
    for text, name, record, word in refusal_files():
        assert pc.parse_adapter_pairs(text) == (name, record)
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            hostapi.clip_parse_adapters(text, pairs=True)
        assert e.value.refusal == name and e.value.bad_record == record and (("record %d:" % record) in str(e.value)) == (record != 0)
    assert hostapi.CLIP_REFUSALS[:9] == ("none", "not_fasta", "byte", "length", "too_many", "no_adapter", "seed", "score", "side")
    fq, fq2 = tmp_path / "in.fq", tmp_path / "in2.fq"
    fq.write_bytes(tc.fastq(tc.make_reads(3, 1)))
    fq2.write_bytes(tc.fastq(tc.make_reads(3, 2)))
    bad = tmp_path / "bad.fa"
    bad.write_bytes(refusal_files()[5][0])
    outs = [tmp_path / n for n in "abcd"]
    with pytest.raises(RuntimeError, match="trim: adapters %s: record 2: the two entries of a prefix pair hold the same number of bases" % re.escape(str(bad))):
        hostapi.trim_fastq_pair(fq, fq2, outs, [], adapters=bad, adapter_pairs=True)
    with pytest.raises(RuntimeError, match="run: adapters %s: record 2: the two entries" % re.escape(str(bad))):
        hostapi.run_reads(None, "s", pairs=[(fq, fq2)], adapters=bad, adapter_pairs=True)
    with pytest.raises(RuntimeError, match="--adapter-pairs needs -1 / -2"):
        hostapi.run_reads(fq, "s", adapters=bad, adapter_pairs=True)
    with pytest.raises(RuntimeError, match="--adapter-pairs needs -1 / -2"):
        hostapi.run_multi_reads([("a", fq)], "s", adapters=bad, adapter_pairs=True)
    with pytest.raises(RuntimeError, match="the adapter pair score is 1 to 1000"):
        hostapi.trim_fastq_pair(fq, fq2, outs, [], adapters=bad, adapter_pairs=True, adapter_pair_score=0)
    with pytest.raises(RuntimeError, match="the fewest adapter bases of a pair are 1 to 16"):
        hostapi.trim_fastq_pair(fq, fq2, outs, [], adapters=bad, adapter_pairs=True, adapter_pair_min=17)
    with pytest.raises(ValueError, match="need adapter_pairs"):
        hostapi.trim_fastq_pair(fq, fq2, outs, [], adapters=bad, adapter_keep_both=True)
    with pytest.raises(ValueError, match="need adapters"):
        hostapi.trim_fastq_pair(fq, fq2, outs, [], adapter_pairs=True)
    assert sorted(os.listdir(tmp_path)) == ["bad.fa", "in.fq", "in2.fq"]


def test_parser_against_the_python_parser(prefix_pairs, adapters):
    many = pc.make_prefix_pairs([16, 33, 128, 64, 65, 34, 17, 100], seed=2)
    for ads, pairs in ((adapters, prefix_pairs), ([], many), (adapters, many)):
        text = pc.adapters_fa(ads, pairs)
        got = hostapi.clip_parse_adapters(text, pairs=True)
        want_ads, want_pairs = pc.parse_adapter_pairs(text)
        assert want_pairs == pairs and [a for a, _ in want_ads] == [a for a, _ in ads]
        assert got["n"] == len(ads) and got["n_pairs"] == len(pairs) and got["skipped"] == 0
        off = got["prefix_off"].tolist()
        assert [(got["prefix_bases"][off[2 * q]:off[2 * q + 1]], got["prefix_bases"][off[2 * q + 1]:off[2 * q + 2]]) for q in range(len(pairs))] == pairs
        if ads:   # without the switch the same file is what it was: the Prefix entries skipped and counted
            plain = hostapi.clip_parse_adapters(text)
            assert plain["skipped"] == 2 * len(pairs) and plain["n"] == len(ads) and "n_pairs" not in plain
    # /2 in front of /1, lower case, wrapped lines, CRLF
    P1, P2 = prefix_pairs[0]
    text = b">PrefixX/2\r\n" + P2[:10].lower() + b"\r\n" + P2[10:] + b"\r\n>PrefixX/1 words\r\n" + P1 + b"\r\n"
    got = hostapi.clip_parse_adapters(text, pairs=True)
    assert got["prefix_bases"] == P1 + P2 and got["n"] == 0 and pc.parse_adapter_pairs(text) == ([], [(P1, P2)])


def test_values_refused_by_name(prefix_pairs):
    s, q = b"ACGT" * 10, b"I" * 40
    for opt, word in ((dict(pair_score=0), "the adapter pair score is 1 to 1000"), (dict(pair_score=1001), "the adapter pair score is 1 to 1000"),
                      (dict(pair_min=0), "the fewest adapter bases of a pair are 1 to 16"), (dict(pair_min=17), "the fewest adapter bases"),
                      (dict(seed=9), "the adapter seed is 0 to 8"), (dict(phred=50), "33 or 64")):
        with pytest.raises(ValueError, match=word):
            hostapi.clip_pair(s, q, s, q, ([], prefix_pairs), **opt)
    for pairs, word in (([], "no prefix pair"), (prefix_pairs * 9, "more than 8 prefix pairs"), ([(b"ACGT" * 4, b"ACGT" * 5)], "the same number of bases"),
                        ([(b"ACGT" * 3, b"ACGT" * 3)], "16 to 128 bases"), ([(b"ACGN" * 4, b"ACGT" * 4)], "a byte outside ACGTacgt")):
        with pytest.raises(ValueError, match=word):
            hostapi.clip_pair(s, q, s, q, ([], pairs))
    assert hostapi.clip_pair(s, q, s, q, ([], prefix_pairs * 8)) == [40, 40]


# ---- the sub-commands' refusals: by name, before any device work (this passes on a machine without a GPU) ----

def test_cli_refusals(tmp_path, prefix_pairs, adapters):
    fq, fq2, fq3, fq4 = tmp_path / "in.fq", tmp_path / "in2.fq", tmp_path / "in3.fq", tmp_path / "in4.fq"
    for k, f in enumerate((fq, fq2, fq3, fq4)):
        f.write_bytes(tc.fastq(tc.make_reads(3, k + 1)))
    ad, lone, simple = tmp_path / "ad.fa", tmp_path / "lone.fa", tmp_path / "simple.fa"
    ad.write_bytes(pc.adapters_fa(adapters, prefix_pairs))
    lone.write_bytes(b">PrefixPE/1\n" + b"ACGT" * 5 + b"\n>a\n" + b"ACGT" * 5 + b"\n")
    simple.write_bytes(cc.adapters_fa(adapters))
    before = sorted(os.listdir(tmp_path))
    o = [tmp_path / n for n in ("p1.fq", "u1.fq", "p2.fq", "u2.fq")]
    single = ["trim", "-i", fq, "-o", tmp_path / "out.fq"]
    pair = ["trim", "-1", fq, "-2", fq2, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3]]
    run1 = ["run", "-i", fq, "-o", "s"]
    runp = ["run", "-1", fq, "-2", fq2, "-o", "s"]
    multi = ["run-multi", "--sample", "a", "-1", fq, "-2", fq2, "--sample", "b", "-1", fq3, "-2", fq4, "-o", "s"]
    mixed = ["run-multi", "--sample", "a", "-1", fq, "-2", fq2, "--sample", "b", "-i", fq3, "-o", "s"]
    cases = []
    for cmd in (single, pair, run1, runp, multi):
        cases += [
            (cmd + ["--adapter-pairs"], "--adapter-pairs needs --adapters"),
            (cmd + ["--adapter-pair-score", "30"], "--adapter-pair-score needs --adapters"),
            (cmd + ["--adapter-pair-min", "8"], "--adapter-pair-min needs --adapters"),
            (cmd + ["--adapter-keep-both"], "--adapter-keep-both needs --adapters"),
            (cmd + ["--adapters", ad, "--adapter-pair-score", "30"], "--adapter-pair-score needs --adapter-pairs"),
            (cmd + ["--adapters", ad, "--adapter-pair-min", "8"], "--adapter-pair-min needs --adapter-pairs"),
            (cmd + ["--adapters", ad, "--adapter-keep-both"], "--adapter-keep-both needs --adapter-pairs"),
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-score"], "--adapter-pair-score needs a value"),
        ]
    for cmd in (pair, runp, multi):
        cases += [
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-score", "0"], "--adapter-pair-score takes 1 to 1000, not '0'"),
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-score", "1001"], "--adapter-pair-score takes 1 to 1000, not '1001'"),
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-min", "0"], "--adapter-pair-min takes 1 to 16, not '0'"),
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-min", "17"], "--adapter-pair-min takes 1 to 16, not '17'"),
            (cmd + ["--adapters", ad, "--adapter-pairs", "--adapter-pair-min", "x"], "--adapter-pair-min takes 1 to 16, not 'x'"),
            (cmd + ["--adapters", lone, "--adapter-pairs"], "adapters %s: record 1: a Prefix entry needs its partner" % lone),
            (cmd + ["--adapters", simple, "--adapter-pairs"], "adapters %s: no prefix pair" % simple),
            (cmd + ["--adapters", simple, "--adapter-pairs", "--adapter-seed", "9"], "--adapter-seed takes 0 to 8"),
        ]
    for cmd in (single, run1, mixed):
        cases.append((cmd + ["--adapters", ad, "--adapter-pairs"], "--adapter-pairs needs -1 / -2"))
    for sub in ("mask", "count", "build", "build-multi"):
        for opt in ("--adapter-pairs", "--adapter-pair-score", "--adapter-pair-min", "--adapter-keep-both"):
            cases.append(([sub, opt], opt))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    usage = run_cli().stdout + run_cli().stderr
    assert "--adapter-pairs [--adapter-pair-score 1..1000] [--adapter-pair-min 1..16] [--adapter-keep-both]" in usage
    assert "--adapter-pairs" in run_cli("trim").stderr


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_clip_pair_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing
    of it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_clip_pair_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_clip_pair_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    for s in ("pf_clip_begin_pairs", "pf_clip_pair_stats_get"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_reads_adapter_pairs", "pfh_reads_adapters_pair_report", "pfh_clip_parse_adapter_pairs", "pfh_clip_pair", "pfh_trim_fastq_pair_chunk_clip"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_PALIN == hipapi.K_CLIP + 1
    hdr = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    assert re.search(r"PF_K_CLIP,.*PF_K_PALIN,[^\n]*\n\s*PF_K_COUNT_", hdr)
    assert hostapi.CLIP_REFUSALS[9:] == ("pair_partner", "pair_lengths", "too_many_pairs", "no_pair", "pair_score", "pair_min")
