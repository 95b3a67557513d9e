"""`--adapters` through the command line (trim, run, run-multi) and hostapi, each run checked against a reference made without the
feature: the Python restatement of clip_cases.py clips the input files into plain FASTQ (a dropped read keeps its record with empty
lines, so that the records of a pair stay in step), and the same command then runs on those files without --adapters.  Every output
file and every stdout line must be identical; stderr differs by the `clip:` line and by `bases` of the `trim:` line, which counts the
bases of the records as they were read (the reference reads them clipped: the difference is the clip line's bases_clipped).  The
inputs are the reads of test_gpu_run_trim.py's generator at twice its depth with a seeded adapter read-through in a sixth of them
(clipping and dropping lowers the depth; the calling run should still have rows to compare)."""
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import clip_cases as cc
import gz_cases as gz
import trim_cases as tc

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WORKFLOW = tc.WORKFLOW
DEPTH = 128
MODEL = ["--model", "fre"]
ADAPTERS = cc.make_adapters([33, 41, 58], seed=17, sides=[1, 2, 0])


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def raw_fastq(reads, rng, side):
    """the reads as FASTQ: a sixth run into an adapter of their side after an insert of 0 .. 95 bases; most qualities flat, a quarter
    with a degrading tail"""
    recs = []
    mine = [a for a, s in ADAPTERS if s in (0, side)]
    for i, r in enumerate(reads):
        seq, n = r.encode(), len(r)
        if rng.random() < 1 / 6:
            ad = mine[int(rng.integers(len(mine)))]
            insert = int(rng.integers(0, n - 4))
            seq = (seq[:insert] + ad + cc.rand_bases(__import__("random").Random(i), n))[:n]
        if rng.random() < 0.25:
            cut = int(rng.integers(30, n))
            qual = b"I" * cut + bytes(33 + int(q) for q in rng.integers(2, 25, size=n - cut))
        else:
            qual = b"I" * n
        recs.append((b"r%d" % i, seq, qual))
    return tc.fastq(recs)


def untimed(stdout):
    return [l for l in stdout.splitlines() if " time " not in l]


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def files_of(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d))) if os.path.isfile(os.path.join(str(d), f))}


def as_read_clipped(stderr_lines):
    """the lines with `bases` of every `trim:` line lowered by bases_clipped of the `clip:` line in front of it: what the same command
    says on the files clipped beforehand"""
    out, clipped = [], 0
    for l in stderr_lines:
        w = l.split()
        if w[:1] == ["clip:"]:
            clipped = int(w[w.index("bases_clipped") + 1])
        elif w[:1] == ["trim:"]:
            at = w.index("bases") + 1
            w[at] = str(int(w[at]) - clipped)
            l, clipped = " ".join(w), 0
        out.append(l)
    return out


def clip_line(stats, skipped=0):
    return "clip: adapters %d skipped %d reads_clipped %d dropped %d bases_clipped %d" % (
        len(ADAPTERS), skipped, sum(s["reads_clipped"] for s in stats), sum(s["reads_dropped"] for s in stats), sum(s["bases_clipped"] for s in stats))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """r1 / r2: the raw pair; c1 / c2: the same files clipped by the Python rule (file 1 with the adapters of side 0 and 1, file 2 with
    those of side 0 and 2); ad: the adapter file, with two palindrome-mode entries in front"""
    root = tmp_path_factory.mktemp("clipstream")
    gen = generator("make_build_golden")
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2026)
    out = dict(root=root, ad=root / "adapters.fa")
    out["ad"].write_bytes(cc.adapters_fa(ADAPTERS, prefix_entries=2))
    for side, part in ((1, reads[0::2]), (2, reads[1::2])):
        text = raw_fastq(part, rng, side)
        clipped, st = cc.clip_fastq(text, ADAPTERS, side=side)
        out["t%d" % side], out["k%d" % side], out["s%d" % side] = text, clipped, st
        for name, t in (("r", text), ("c", clipped)):
            out["%s%d" % (name, side)] = root / ("%s%d.fq" % (name, side))
            out["%s%d" % (name, side)].write_bytes(t)
        assert st["reads_clipped"] > 50 and st["reads_dropped"] > 0 and st["bases_clipped"] > 1000, st
    return out


# ---- trim ----

@pytest.mark.parametrize("chunk", [4096, 50000, None])
def test_trim_single_at_three_chunk_sizes(data, tmp_path, chunk):
    """-i files are file 1: both inputs are clipped with the adapters of side 0 and 1"""
    extra = ["--chunk-bytes", chunk] if chunk else []
    c2, s2 = cc.clip_fastq(data["t2"], ADAPTERS, side=1)
    assert c2 != data["k2"]
    (tmp_path / "c2.fq").write_bytes(c2)
    for tag, steps in (("workflow", WORKFLOW), ("minlen", ["MINLEN:1"])):
        w, g = tmp_path / ("want_" + tag), tmp_path / ("got_" + tag)
        for d in (w, g):
            d.mkdir()
        want = cli("trim", "-i", data["c1"], "-i", tmp_path / "c2.fq", "-o", w / "t.fq", "--trimlog", w / "log.txt", *steps, *extra, cwd=w)
        got = cli("trim", "-i", data["r1"], "-i", data["r2"], "-o", g / "t.fq", "--trimlog", g / "log.txt", "--adapters", data["ad"], *steps, *extra, cwd=g)
        assert files_of(g) == files_of(w) and len(files_of(g)) == 2 and got.stdout == want.stdout == ""
        assert as_read_clipped(got.stderr.splitlines()) == [clip_line([data["s1"], s2], skipped=2)] + want.stderr.splitlines()


def test_trim_single_file_2_is_clipped_as_file_1(data, tmp_path):
    """what the loop above relies on, on its own: `trim -i r2` uses the /1 adapters"""
    clipped, st = cc.clip_fastq(data["t2"], ADAPTERS, side=1)
    (tmp_path / "c.fq").write_bytes(clipped)
    want = cli("trim", "-i", tmp_path / "c.fq", "-o", tmp_path / "want.fq", "MINLEN:1", cwd=tmp_path)
    got = cli("trim", "-i", data["r2"], "-o", tmp_path / "got.fq", "--adapters", data["ad"], cwd=tmp_path)   # no STEP beside --adapters
    assert (tmp_path / "got.fq").read_bytes() == (tmp_path / "want.fq").read_bytes()
    assert as_read_clipped(got.stderr.splitlines()) == [clip_line([st], skipped=2)] + want.stderr.splitlines()


@pytest.mark.parametrize("chunk", [4096, 50000, None])
def test_trim_pair_at_three_chunk_sizes(data, tmp_path, chunk):
    extra = ["--chunk-bytes", chunk] if chunk else []
    names = ["-o1", "p1.fq", "-u1", "u1.fq", "-o2", "p2.fq", "-u2", "u2.fq", "--trimlog", "log.txt"]
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    want = cli("trim", "-1", data["c1"], "-2", data["c2"], *names, *WORKFLOW, *extra, cwd=w)
    got = cli("trim", "-1", data["r1"], "-2", data["r2"], *names, "--adapters", data["ad"], "--adapter-seed", 2, "--adapter-score", 10, *WORKFLOW, *extra, cwd=g)
    assert files_of(g) == files_of(w) and len(files_of(g)) == 5 and all(files_of(g).values())
    assert as_read_clipped(got.stderr.splitlines()) == [clip_line([data["s1"], data["s2"]], skipped=2)] + want.stderr.splitlines()


def test_trim_pair_gz_in_and_out_and_hostapi(data, tmp_path):
    for side in (1, 2):
        (tmp_path / ("r%d.fq.gz" % side)).write_bytes(gz.bgzf(data["t%d" % side]))
    names = ["p1.fq.gz", "u1.fq.gz", "p2.fq.gz", "u2.fq.gz"]
    w, g, h = tmp_path / "want", tmp_path / "got", tmp_path / "api"
    for d in (w, g, h):
        d.mkdir()
    flags = [x for pair in zip(["-o1", "-u1", "-o2", "-u2"], names) for x in pair]
    cli("trim", "-1", data["c1"], "-2", data["c2"], *flags, "--gz-out", *WORKFLOW, cwd=w)
    cli("trim", "-1", tmp_path / "r1.fq.gz", "-2", tmp_path / "r2.fq.gz", *flags, "--gz", "--gz-out", "--adapters", data["ad"], *WORKFLOW, cwd=g)
    assert files_of(g) == files_of(w)
    text = gzip.decompress(files_of(g)["p1.fq.gz"])
    assert text.count(b"\n") > 400
    st = hostapi.trim_fastq_pair(str(tmp_path / "r1.fq.gz"), str(tmp_path / "r2.fq.gz"), [str(h / n) for n in names], WORKFLOW, gz=True, gz_out=True,
                                 adapters=str(data["ad"]))
    assert files_of(h) == files_of(w) and st[0]["both"] > 0
    rep = hostapi.clip_report()
    assert (rep["adapters"], rep["skipped"]) == (3, 2)
    for f in ("reads_clipped", "reads_dropped", "bases_clipped", "candidates_scored"):
        assert rep[f] == [data["s1"][f], data["s2"][f]], f
    # other values of seed and score reach the kernel: the reference is clipped with them
    c1, _ = cc.clip_fastq(data["t1"], ADAPTERS, side=1, seed=0, score=25)
    (h / "c1.fq").write_bytes(c1)
    hostapi.trim_fastq(str(h / "c1.fq"), str(h / "want.fq"), WORKFLOW)
    hostapi.trim_fastq(str(data["r1"]), str(h / "got.fq"), WORKFLOW, adapters=str(data["ad"]), adapter_seed=0, adapter_score=25)
    assert (h / "got.fq").read_bytes() == (h / "want.fq").read_bytes() and c1 != data["k1"]


# ---- run, run-multi ----

@pytest.mark.parametrize("name,extra", [("plain", []), ("chunk_carries", ["--chunk-bytes", 4096])])
def test_run_pair_against_the_clipped_files(data, tmp_path, name, extra):
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    common = ["-o", "s", *MODEL, "--db-out", "db", "--gfa-out", "g", *extra, *WORKFLOW]
    want = cli("run", "-1", data["c1"], "-2", data["c2"], *common, cwd=w)
    got = cli("run", "-1", data["r1"], "-2", data["r2"], "--adapters", data["ad"], *common, cwd=g)
    rows = calling_files(w, "s")["_allele_frequency.txt"].decode().splitlines()
    print("run on the clipped pair: L = %s, %d lines in allele_frequency.txt" % (want.stdout.splitlines()[0], len(rows)))
    assert len(rows) >= 5
    assert calling_files(g, "s") == calling_files(w, "s") and files_of(g) == files_of(w)
    assert untimed(got.stdout) == untimed(want.stdout)
    keep = lambda r: [l for l in r.stderr.splitlines() if l.startswith(("clip: ", "trim: ", "run: reads "))]
    assert as_read_clipped(keep(got)) == [clip_line([data["s1"], data["s2"]], skipped=2)] + keep(want)
    # the adapters matter: the raw files without them give another database
    raw = tmp_path / "raw"
    raw.mkdir()
    cli("run", "-1", data["r1"], "-2", data["r2"], "-o", "s", "--db-out", "db", *WORKFLOW, cwd=raw)
    assert files_of(raw)["db.kmc_suf"] != files_of(w)["db.kmc_suf"]


def test_run_single_without_a_step_and_run_reads(data, tmp_path, monkeypatch):
    w, g, h = tmp_path / "want", tmp_path / "got", tmp_path / "api"
    for d in (w, g, h):
        d.mkdir()
    want = cli("run", "-i", data["c1"], "-o", "s", "--db-out", "db", "MINLEN:1", cwd=w)   # (MINLEN:1 drops the empty records, as clipping to 0 does)
    got = cli("run", "-i", data["r1"], "-o", "s", "--db-out", "db", "--adapters", data["ad"], cwd=g)
    assert calling_files(g, "s") == calling_files(w, "s") and files_of(g) == files_of(w) and untimed(got.stdout) == untimed(want.stdout)
    assert [l for l in got.stderr.splitlines() if l.startswith("clip: ")] == [clip_line([data["s1"]], skipped=2)]
    monkeypatch.chdir(h)
    st = hostapi.run_reads(None, "s", pairs=[(str(data["r1"]), str(data["r2"]))], adapters=str(data["ad"]), db_out="db")
    monkeypatch.chdir(w)
    ref = hostapi.run_reads(None, "p", pairs=[(str(data["c1"]), str(data["c2"]))], steps=["MINLEN:1"], db_out="pdb")
    assert {k: v for k, v in st.items() if k != "trim"} == {k: v for k, v in ref.items() if k != "trim"}
    assert files_of(h)["db.kmc_suf"] == files_of(w)["pdb.kmc_suf"]
    assert hostapi.clip_report()["reads_clipped"] == [0, 0]   # the last call took no adapters


def test_run_multi_one_paired_and_one_single_sample(data, tmp_path):
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    # sample b: the second file alone, single-ended: clipped as file 1
    b_clipped, b_stats = cc.clip_fastq(data["t2"], ADAPTERS, side=1)
    (tmp_path / "b.fq").write_bytes(b_clipped)
    common = ["-o", "s", "--db-out", "db", "--gfa-out", "g", *WORKFLOW]
    want = cli("run-multi", "--sample", "a", "-1", data["c1"], "-2", data["c2"], "--sample", "b", "-i", tmp_path / "b.fq", *common, cwd=w)
    # (one file in two samples is refused: sample b reads a copy)
    (tmp_path / "b_raw.fq").write_bytes(data["t2"])
    got = cli("run-multi", "--sample", "a", "-1", data["r1"], "-2", data["r2"], "--sample", "b", "-i", tmp_path / "b_raw.fq", "--adapters", data["ad"], *common, cwd=g)
    assert calling_files(g, "s") == calling_files(w, "s") and files_of(g) == files_of(w)
    assert untimed(got.stdout) == untimed(want.stdout)
    keep = lambda r: [l for l in r.stderr.splitlines() if l.startswith(("clip: ", "trim: "))]
    wt = keep(want)
    assert as_read_clipped(keep(got)) == [clip_line([data["s1"], data["s2"]], skipped=2), wt[0], clip_line([b_stats], skipped=2), wt[1]]


# ---- a record longer than the chunk: the first calls of the stream take no whole record ----

def test_trimlog_with_a_record_longer_than_the_chunk(data, tmp_path):
    """--chunk-bytes 4096 and a first record of 20 000 bases (file 2: 9 000): the stream calls the step with chunks that hold no whole
    record (of both files) while the carry grows; with --adapters and --trimlog those calls ask for the clip ends of no record"""
    rng = __import__("random").Random(31)
    big = []
    for side, n, o in ((1, 20000, 15000), (2, 9000, 8950)):
        ad = [a for a, s in ADAPTERS if s == side][0]
        seq = cc.plant(rng, n, ad, o)
        big.append(tc.fastq([(b"big/%d" % side, seq, b"I" * n)]))
    t = [big[0] + data["t1"][:30000], big[1] + data["t2"][:30000]]
    n = min(len(tc.parse_records(x, final=False)[0]) for x in t)
    t = [x[:tc._end_of(x, n)] for x in t]
    clipped = [cc.clip_fastq(x, ADAPTERS, side=f + 1) for f, x in enumerate(t)]
    assert [tc.parse_records(c[0])[0][0][1].__len__() for c in clipped] == [15000, 8950]
    for f in range(2):
        (tmp_path / ("r%d.fq" % (f + 1))).write_bytes(t[f])
        (tmp_path / ("c%d.fq" % (f + 1))).write_bytes(clipped[f][0])
    names = ["-o1", "p1.fq", "-u1", "u1.fq", "-o2", "p2.fq", "-u2", "u2.fq", "--trimlog", "log.txt", "--chunk-bytes", 4096]
    for tag, w_in, g_in, out, stats in (("pair", ["-1", tmp_path / "c1.fq", "-2", tmp_path / "c2.fq"], ["-1", tmp_path / "r1.fq", "-2", tmp_path / "r2.fq"], names,
                                         [clipped[0][1], clipped[1][1]]),
                                        ("single", ["-i", tmp_path / "c1.fq"], ["-i", tmp_path / "r1.fq"], ["-o", "t.fq", "--trimlog", "log.txt", "--chunk-bytes", 4096],
                                         [clipped[0][1]])):
        w, g = tmp_path / ("want_" + tag), tmp_path / ("got_" + tag)
        for d in (w, g):
            d.mkdir()
        want = cli("trim", *w_in, *out, "MINLEN:1", cwd=w)
        got = cli("trim", *g_in, *out, "--adapters", data["ad"], cwd=g)
        assert files_of(g) == files_of(w) and b"big/1 15000 0 15000 0\n" in files_of(g)["log.txt"]
        assert as_read_clipped(got.stderr.splitlines()) == [clip_line(stats, skipped=2)] + want.stderr.splitlines()
