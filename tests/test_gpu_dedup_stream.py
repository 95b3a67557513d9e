"""`--dedup` on the commands: `trim --dedup`, both forms, against the text built in Python from the rule (dedup_cases.py composed with
trim_cases.py: outputs, trim log, `dedup:` line, `trim:` line), and `run --dedup` / `run-multi --dedup` against the chains they replace
(`trim --dedup` per unit, then `run -i` / `run-multi` on its outputs).  Every comparison is exact: bytes of files and lines of stderr."""
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import clip_cases as cc
import clip_pair_cases as pc
import dedup_cases as dc
import trim_cases as tc

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS = ["LEADING:10", "TRAILING:10", "MINLEN:30"]
WORKFLOW = tc.WORKFLOW
MODEL = ["--model", "fre"]
DEPTH = 64


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def read(p):
    with open(p, "rb") as f:
        return f.read()


def lines_with(text, *words):
    return [l for l in text.splitlines() if l.startswith(words)]


# ---- trim --dedup against the rule ----

@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """3 000 records of 100 bases, a fifth of them copies of an earlier one, three in ten with a degraded tail; their mates"""
    root = tmp_path_factory.mktemp("dedupreads")
    r1 = dc.dup_reads(3000, 81, copies_of_one=11)
    r2 = dc.mates(r1, 4)
    for i in range(0, len(r2), 41):
        r2[i] = (r2[i][0], r2[i][1], b"#" * len(r2[i][1]))   # file 2 dropped: the pair is no unit
    t1, t2 = tc.fastq(r1), tc.fastq(r2)
    (root / "r1.fq").write_bytes(t1)
    (root / "r2.fq").write_bytes(t2)
    return dict(root=root, r1=root / "r1.fq", r2=root / "r2.fq", t1=t1, t2=t2)


@pytest.mark.parametrize("name,steps,extra", [
    ("plain", STEPS, []), ("chunks", STEPS, ["--chunk-bytes", 4096]), ("small_table", STEPS, ["--dedup-initial-slots", 64, "--chunk-bytes", 65536]),
    ("no_step", [], []), ("bases", STEPS, ["--dedup-bases", 16])])
def test_trim_single_writes_the_rule(reads, tmp_path, name, steps, extra):
    bases = 16 if name == "bases" else 0
    d = dc.Dedup(bases)
    want = d.trim_fastq(reads["t1"] + reads["t2"], steps)   # one table over all inputs of the command
    r = cli("trim", "-i", reads["r1"], "-i", reads["r2"], "-o", tmp_path / "o.fq", "--trimlog", tmp_path / "log", "--dedup", *extra, *steps, cwd=tmp_path)
    assert read(tmp_path / "o.fq") == want["out"] and read(tmp_path / "log") == tc.trimlog(want)
    assert lines_with(r.stderr, "dedup: ", "trim: ") == [d.line(), dc.trim_line(want["stats"], False)]
    assert d.stats()["duplicates"] > 500 and d.stats()["max_copies"] >= 12
    assert sorted(os.listdir(tmp_path)) == ["log", "o.fq"]


@pytest.mark.parametrize("name,steps,extra", [("plain", STEPS, []), ("chunks_small_table", WORKFLOW, ["--chunk-bytes", 4096, "--dedup-initial-slots", 64]),
                                              ("no_step", [], [])])
def test_trim_pair_writes_the_rule(reads, tmp_path, name, steps, extra):
    d = dc.Dedup()
    want = d.trim_pair(reads["t1"], reads["t2"], steps)
    outs = [tmp_path / n for n in ("o1.fq", "u1.fq", "o2.fq", "u2.fq")]
    r = cli("trim", "-1", reads["r1"], "-2", reads["r2"], "-o1", outs[0], "-u1", outs[1], "-o2", outs[2], "-u2", outs[3], "--trimlog", tmp_path / "log",
            "--dedup", *extra, *steps, cwd=tmp_path)
    assert [read(o) for o in outs] == want["out"] and read(tmp_path / "log") == tc.trimlog(want)
    assert lines_with(r.stderr, "dedup: ", "trim: ") == [d.line(), dc.trim_line(want["stats"], True)]
    assert (want["stats"][0]["only1"] > 0 or not steps) and d.stats()["duplicates"] > 300   # (without a step K-TRIM drops nothing: no pair is split)
    # the Python interface gives the same statistics
    api = hostapi.trim_fastq_pair(reads["r1"], reads["r2"], [tmp_path / ("api%d" % i) for i in range(4)], steps, dedup=True,
                                  chunk_bytes=4096 if "--chunk-bytes" in extra else 0, dedup_initial_slots=64 if "--dedup-initial-slots" in extra else 0)
    assert {f: api[0]["dedup"][f] for f in dc.STATS} == d.stats() and [{f: a[f] for f in tc.STATS} for a in api] == want["stats"]
    assert [read(tmp_path / ("api%d" % i)) for i in range(4)] == want["out"]


def test_trim_gz_in_and_out(reads, tmp_path):
    d = dc.Dedup()
    want = d.trim_fastq(reads["t1"], STEPS)
    cli("trim", "-i", reads["r1"], "-o", tmp_path / "plain.gz", "--gz-out", "MINLEN:1", cwd=tmp_path)   # the input as blocked gzip
    r = cli("trim", "-i", tmp_path / "plain.gz", "-o", tmp_path / "o.fq.gz", "--gz", "--gz-out", "--dedup", *STEPS, cwd=tmp_path)
    assert gzip.decompress(read(tmp_path / "o.fq.gz")) == want["out"]
    assert lines_with(r.stderr, "dedup: ", "trim: ") == [d.line(), dc.trim_line(want["stats"], False)]


def test_trim_with_adapters_and_palindrome_mode(tmp_path):
    """--adapters with --adapter-pairs --adapter-keep-both on reads that hold the adapter of file 1: half of the fragments read through
    into it at base 55, and so do all their copies.  The same command without --dedup decides the intervals; --dedup drops the later
    copies among the pairs it keeps whole.  The key is of the raw reads: a copy is dropped although the clip shortened both, and a twin
    that differs behind the adapter alone -- the same bytes once clipped -- stays."""
    ads = cc.make_adapters([34, 30], seed=3, sides=[1, 2])
    ad1, GOOD = bytes(ads[0][0]), tc.qline([36] * 100)
    planted = lambda seq: seq[:55] + ad1 + seq[89:] if seq[0] in b"AC" else seq
    r1 = [(name, planted(seq), qual) for name, seq, qual in dc.dup_reads(1500, 83)]
    twins = [i for i, r in enumerate(r1) if r[1][55:89] == ad1 and r[0].endswith(b"new")][:40]
    for n, i in enumerate(twins):   # the same insert and adapter, other bases behind it, right behind the original
        r1.insert(i + n + 1, (b"twin%d" % i, r1[i + n][1][:89] + bytes(b"ACGT"[(c + 1) & 3] for c in r1[i + n][1][89:]), GOOD))
    twin_at = [i for i, r in enumerate(r1) if r[0].startswith(b"twin")]
    r2 = dc.mates([(n, s[:55], q) for n, s, q in r1], 4)   # (the mate is a function of the insert: copies and twins share it)
    t1, t2 = tc.fastq(r1), tc.fastq(r2)
    (tmp_path / "r1.fq").write_bytes(t1)
    (tmp_path / "r2.fq").write_bytes(t2)
    fa = tmp_path / "ad.fa"
    fa.write_bytes(pc.adapters_fa(ads, pc.make_prefix_pairs([34], seed=23)))
    common = ["--adapters", fa, "--adapter-pairs", "--adapter-keep-both", *STEPS]
    names = ("o1.fq", "u1.fq", "o2.fq", "u2.fq")

    def run(tag, *more):
        o = tmp_path / tag
        o.mkdir()
        r = cli("trim", "-1", tmp_path / "r1.fq", "-2", tmp_path / "r2.fq", "-o1", o / names[0], "-u1", o / names[1], "-o2", o / names[2], "-u2", o / names[3],
                "--trimlog", o / "log", *more, *common, cwd=o)
        return o, r

    plain, rp = run("plain")
    mine, rm = run("dedup", "--dedup")
    # what the rule makes of the plain command's log: a pair kept whole takes part with the key of its raw reads
    recs = [tc.parse_records(t1)[0], tc.parse_records(t2)[0]]
    log = read(plain / "log").decode().splitlines()
    d, want_log, dups, whole = dc.Dedup(), [], set(), []
    for i in range(len(recs[0])):
        kept = [not log[2 * i + f].endswith(" 0 0 0 0") for f in range(2)]
        if all(kept):
            whole.append(i)
            if not d.unit(dc.key_of(recs[0][i][1], recs[1][i][1])):
                dups.add(i)
        for f in range(2):
            want_log.append(log[2 * i + f].rsplit(" ", 4)[0] + " 0 0 0 0" if i in dups else log[2 * i + f])
    got_log = read(mine / "log").decode().splitlines()
    assert got_log == want_log and len(dups) > 150
    # the clip did its work: every read that holds the adapter is logged with 55 bases, its dropped copies among them were 55 as well
    holds = [i for i, r in enumerate(r1) if r[1][55:89] == ad1 and r[2] == GOOD]
    assert len(holds) > 400 and all(log[2 * i].rsplit(" ", 4)[1:] == ["55", "0", "55", "0"] for i in holds)
    assert sum(1 for i in holds if i in dups) > 50
    # a twin is the bytes of its original once clipped, and stays: its raw read is another
    for i in twin_at:
        assert i not in dups and not got_log[2 * i].endswith(" 0 0 0 0") and r1[i][1][:89] == r1[i - 1][1][:89] and r1[i][1] != r1[i - 1][1]
    for n in ("u1.fq", "u2.fq"):
        assert read(mine / n) == read(plain / n)
    for n in ("o1.fq", "o2.fq"):
        written = tc.parse_records(read(plain / n))[0]
        assert len(written) == len(whole)
        assert read(mine / n) == b"".join(tc.record_bytes(r, 0, len(r[1])) for r, i in zip(written, whole) if i not in dups)
    assert lines_with(rm.stderr, "clip: ") == lines_with(rp.stderr, "clip: ")
    assert [l.split(" ")[0] for l in rm.stderr.splitlines() if l.startswith(("clip:", "dedup:", "trim:"))] == ["clip:", "dedup:", "trim:"]
    assert lines_with(rm.stderr, "dedup: ") == [d.line()]


def test_refusals_leave_an_empty_directory(reads, tmp_path):
    for args, text in (
            (["trim", "-i", reads["r1"], "-o", "o.fq", "--dedup-bases", 32, *STEPS], "--dedup-bases needs --dedup"),
            (["trim", "-i", reads["r1"], "-o", "o.fq", "--dedup", "--dedup-bases", 8], "--dedup-bases takes 16 to 4096, not '8'"),
            (["trim", "-i", reads["r1"], "-o", "o.fq", "--dedup", "--fasta"], "--fasta does not go with --dedup"),
            (["run", "-i", reads["r1"], "-o", "s", "--dedup", "--fasta"], "--fasta does not go with --dedup"),
            (["run", "-i", reads["r1"], "-o", "s", "--dedup-initial-slots", 64], "--dedup-initial-slots needs --dedup"),
            (["run-multi", "--sample", "a", "-i", reads["r1"], "-o", "s", "--dedup", "--dedup-bases", 5000], "--dedup-bases takes 16 to 4096, not '5000'"),
            (["qc", "-i", reads["r1"], "-o", "r.tsv", "--dedup"], "unknown option --dedup"),
            (["smudge", "-d", "db", "-o", "r.tsv", "--dedup"], "unknown option --dedup")):
        r = cli(*args, cwd=tmp_path, ok=False)
        assert r.returncode != 0 and text in r.stderr, r.stderr
        assert os.listdir(tmp_path) == []
    bad = tmp_path / "bad.fq"
    bad.write_bytes(reads["t1"][:5000] + b"@x\nACGT\n+\nII\n")
    r = cli("trim", "-i", reads["r1"], "-i", bad, "-o", "o.fq", "--dedup", *STEPS, cwd=tmp_path, ok=False)   # refused in the middle of the stream
    assert r.returncode != 0 and "bad.fq" in r.stderr and sorted(os.listdir(tmp_path)) == ["bad.fq"]


# ---- run --dedup and run-multi --dedup against their chains ----

def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def write_dup_fastq(paths, reads, rng, share=0.2):
    """the reads as pairs (even, odd) into paths[0] / paths[1] with about `share` of the pairs repeated later in the stream, half of the
    copies with a degraded tail in file 1; returns the number of pairs written"""
    pairs = [(reads[i], reads[i + 1]) for i in range(0, len(reads) - 1, 2)]
    stream = []
    for p in pairs:
        stream.append((p, False))
        if rng.random() < share:
            stream.insert(int(rng.integers(0, len(stream) + 1)), (p, rng.random() < 0.5))
    with open(paths[0], "w") as f1, open(paths[1], "w") as f2:
        for i, ((a, b), poor) in enumerate(stream):
            qa = "I" * len(a)
            if poor:
                cut = int(rng.integers(40, len(a)))
                qa = "I" * cut + "".join(chr(33 + int(q)) for q in rng.integers(2, 25, size=len(a) - cut))
            f1.write("@r%d\n%s\n+\n%s\n" % (i, a, qa))
            f2.write("@r%d\n%s\n+\n%s\n" % (i, b, "#" * len(b) if i % 53 == 0 else "I" * len(b)))
    return len(stream)


def untimed(stdout):
    return [l for l in stdout.splitlines() if " time " not in l]


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: read(os.path.join(od, f)) for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def same_run(mine_dir, chain_dir, got, want, sub="run"):
    a, b = calling_files(mine_dir, "s"), calling_files(chain_dir, "s")
    rows = b["_allele_frequency.txt"].decode().splitlines()
    print("%s --dedup chain: %d calling files, %d lines in allele_frequency.txt" % (sub, len(b), len(rows)))
    assert len(rows) >= 5 and sorted(a) == sorted(b) and len([f for f in b if f != "_model_result.txt"]) == 12   # the comparison is not vacuous
    for f in b:
        assert a[f] == b[f], f
    for f in sorted(os.listdir(chain_dir)):
        if f.startswith(("db", "g.")):
            assert read(os.path.join(mine_dir, f)) == read(os.path.join(chain_dir, f)), f
    assert untimed(got.stdout) == untimed(want.stdout)
    assert lines_with(got.stderr, sub + ": ") == lines_with(want.stderr, sub + ": ")


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    root = tmp_path_factory.mktemp("dedupchain")
    gen = generator("make_build_golden")
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2026)
    half = len(reads) // 2 & ~1
    out = dict(root=root, a=[root / "a1.fq", root / "a2.fq"], b=[root / "b1.fq", root / "b2.fq"])
    write_dup_fastq(out["a"], reads[:half], rng)
    write_dup_fastq(out["b"], reads[:64] + reads[half:], rng)   # the first 32 pairs of a once more: duplicates across the two units
    return out


def test_run_pairs_against_the_chain(raw, tmp_path):
    """two pairs: one table per pair, one `dedup:` line per pair, and a read duplicated across the two pairs survives in both"""
    cd, md = tmp_path / "chain", tmp_path / "mine"
    cd.mkdir()
    md.mkdir()
    trims, inputs = [], []
    for u in ("a", "b"):
        o = [cd / ("%s_%s.fq" % (u, x)) for x in ("o1", "u1", "o2", "u2")]
        t = cli("trim", "-1", raw[u][0], "-2", raw[u][1], "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "--dedup", *WORKFLOW, cwd=cd)
        trims += lines_with(t.stderr, "dedup: ", "trim: ")
        inputs += ["-i", o[0], "-i", o[2]]
    want = cli("run", *inputs, "-o", "s", *MODEL, "--db-out", cd / "db", "--gfa-out", cd / "g", cwd=cd)
    got = cli("run", "-1", raw["a"][0], "-2", raw["a"][1], "-1", raw["b"][0], "-2", raw["b"][1], "-o", "s", *MODEL, "--db-out", md / "db", "--gfa-out", md / "g",
              "--dedup", "--chunk-bytes", 16384, *WORKFLOW, cwd=md)
    same_run(md, cd, got, want)
    assert lines_with(got.stderr, "dedup: ", "trim: ") == trims and [l.split(" ")[0] for l in trims] == ["dedup:", "trim:", "dedup:", "trim:"]
    dup = [int(l.split(" ")[6]) for l in trims[0::2]]
    assert min(dup) > 20
    first = tc.parse_records(read(raw["a"][0]))[0][0][1]
    assert first[:40] in read(cd / "a_o1.fq") + read(cd / "a_u1.fq") and first[:40] in read(cd / "b_o1.fq") + read(cd / "b_u1.fq")
    # without --dedup the duplicates reach the counters: the databases differ
    plain = tmp_path / "plain"
    plain.mkdir()
    cli("run", "-1", raw["a"][0], "-2", raw["a"][1], "-1", raw["b"][0], "-2", raw["b"][1], "-o", "s", "--db-out", plain / "db", *WORKFLOW, cwd=plain)
    assert read(str(plain / "db") + ".kmc_suf") != read(str(md / "db") + ".kmc_suf")


def test_run_single_ended_against_the_chain(raw, tmp_path, monkeypatch):
    """all -i files of a run are one unit: one table over both files, no STEP beside --dedup"""
    cd, md = tmp_path / "chain", tmp_path / "mine"
    cd.mkdir()
    md.mkdir()
    files = [x for f in raw["a"] + raw["b"] for x in ("-i", f)]
    t = cli("trim", *files, "-o", cd / "t.fq", "--dedup", cwd=cd)
    want = cli("run", "-i", cd / "t.fq", "-o", "s", *MODEL, "--db-out", cd / "db", "--gfa-out", cd / "g", cwd=cd)
    got = cli("run", *files, "-o", "s", *MODEL, "--db-out", md / "db", "--gfa-out", md / "g", "--dedup", cwd=md)
    same_run(md, cd, got, want)
    assert lines_with(got.stderr, "dedup: ", "trim: ") == lines_with(t.stderr, "dedup: ", "trim: ") and len(lines_with(got.stderr, "dedup: ")) == 1
    api = tmp_path / "api"
    api.mkdir()
    monkeypatch.chdir(api)
    r = hostapi.run_reads([str(f) for f in raw["a"] + raw["b"]], "s", model="fre", dedup=True)
    assert calling_files(api, "s") == calling_files(md, "s")
    words = lines_with(got.stderr, "dedup: ")[0].split(" ")
    assert (r["dedup"]["units"], r["dedup"]["unique"], r["dedup"]["duplicates"], r["dedup"]["max_copies"]) == tuple(int(words[i]) for i in (2, 4, 6, 8))
    assert r["dedup"]["levels"] == [int(w) for w in words[10:20]]


def test_run_multi_against_the_chain(tmp_path):
    """three samples of the build_mc3_k25 generator at depth 64 (the inputs of the `run-multi STEP...` chain test, here with a fifth of the
    pairs written twice): alpha paired, beta single-ended in two files, gamma paired -- per sample what `run --dedup` does per unit"""
    gen = generator("make_build_multi_golden")
    rng = np.random.default_rng(2027)
    rawd = tmp_path / "raw"
    rawd.mkdir()
    samples = list(gen.make_samples(**dict(gen.CASES["build_mc3_k25"], depth=DEPTH)))
    files = {}
    for name, reads in zip(("alpha", "beta", "gamma"), samples):
        files[name] = [rawd / ("%s_%d.fq" % (name, f)) for f in (1, 2)]
        write_dup_fastq(files[name], list(reads), rng)
    cd, md = tmp_path / "chain", tmp_path / "mine"
    cd.mkdir()
    md.mkdir()
    trims, chain_args, mine_args = [], [], []
    for name in ("alpha", "beta", "gamma"):
        f1, f2 = files[name]
        if name == "beta":
            t = cli("trim", "-i", f1, "-i", f2, "-o", cd / "beta.fq", "--dedup", *WORKFLOW, cwd=cd)
            chain_args += ["--sample", name, "-i", cd / "beta.fq"]
            mine_args += ["--sample", name, "-i", f1, "-i", f2]
        else:
            o = [cd / ("%s_%s.fq" % (name, x)) for x in ("o1", "u1", "o2", "u2")]
            t = cli("trim", "-1", f1, "-2", f2, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "--dedup", *WORKFLOW, cwd=cd)
            chain_args += ["--sample", name, "-i", o[0], "-i", o[2]]
            mine_args += ["--sample", name, "-1", f1, "-2", f2]
        trims += lines_with(t.stderr, "dedup: ", "trim: ")
    want = cli("run-multi", *chain_args, "-o", "s", "--db-out", cd / "db", "--gfa-out", cd / "g", cwd=cd)
    got = cli("run-multi", *mine_args, "-o", "s", "--db-out", md / "db", "--gfa-out", md / "g", "--dedup", *WORKFLOW, cwd=md)
    same_run(md, cd, got, want, "run-multi")
    assert lines_with(got.stderr, "dedup: ", "trim: ") == trims and [l.split(" ")[0] for l in trims] == ["dedup:", "trim:"] * 3
    assert min(int(l.split(" ")[6]) for l in trims[0::2]) > 20
