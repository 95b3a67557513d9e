"""`--adapters f --adapter-pairs` through the command line (trim, run, run-multi) and hostapi, each run checked against a reference made
without the feature: the Python restatement of clip_pair_cases.py clips the two input files into plain FASTQ (a dropped read keeps its
record with empty lines, so that the records of a pair stay in step), and the same command then runs on those files without any
--adapter* option.  Every output file, the trim log and every stdout line must be identical; stderr differs by the `clip:` line,
which is checked by its numbers, and by `bases` of the `trim:` line, which counts the bases of the records as they were read.  The
inputs are the reads of test_gpu_clip_stream.py's generator as pairs, a fifth of them turned into read-through of an insert of 20 ..
99 bases (so that remnants of 1 .. 15 adapter bases occur) and a tenth running into a simple adapter."""
import gzip
import importlib.util
import os
import random
import subprocess

import pytest

from conftest import ROOT

import clip_cases as cc
import clip_pair_cases as pc
import gz_cases as gz
import trim_cases as tc

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WORKFLOW = tc.WORKFLOW
DEPTH = 128
PREFIX = pc.make_prefix_pairs([34], seed=23)
# as in the sequencers' files, the simple adapters of a side start with what reads through behind the insert: RC(P2) in file 1, RC(P1) in file 2
ADAPTERS = [(pc.revcomp(PREFIX[0][1]) + b"ATCTCGTATGCC", 1), (pc.revcomp(PREFIX[0][0]) + b"GTGTAGATCTCG", 2), cc.make_adapters([58], seed=17)[0]]
NAMES = ["-o1", "p1.fq", "-u1", "u1.fq", "-o2", "p2.fq", "-u2", "u2.fq"]


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def raw_pair(reads, seed):
    """(text 1, text 2): reads[2r] and reads[2r + 1] as pair r; a fifth of the pairs are read-through of the first I = 20 .. 99 bases of
    reads[2r] with the prefix pair, one base of each read mutated in half of them; a tenth of the others run into a simple adapter of
    their side; a quarter of all reads have a degrading quality tail"""
    rng = random.Random(seed)
    f1, f2 = [], []
    for r in range(len(reads) // 2):
        s1, s2 = reads[2 * r].encode(), reads[2 * r + 1].encode()
        n1, n2 = len(s1), len(s2)
        u = rng.random()
        if u < 0.2:
            I = rng.randint(20, min(99, n1, n2))
            s1, s2 = pc.read_through(rng, n1, n2, I, *PREFIX[0], insert=s1[:I])
            if rng.random() < 0.5:
                s1, s2 = cc.mutate(rng, s1, 0, n1, 1), cc.mutate(rng, s2, 0, n2, 1)
        elif u < 0.3:
            for side in (1, 2):
                ad = rng.choice([a for a, s in ADAPTERS if s in (0, side)])
                at = rng.randint(0, 95)
                if side == 1:
                    s1 = (s1[:at] + ad + cc.rand_bases(rng, n1))[:n1]
                else:
                    s2 = (s2[:at] + ad + cc.rand_bases(rng, n2))[:n2]
        quals = []
        for n in (n1, n2):
            cut = rng.randint(30, n) if rng.random() < 0.25 else n
            quals.append(b"I" * cut + bytes(33 + rng.randint(2, 24) for _ in range(n - cut)))
        f1.append((b"r%d/1" % r, s1, quals[0]))
        f2.append((b"r%d/2" % r, s2, quals[1]))
    return tc.fastq(f1), tc.fastq(f2)


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


def clip_line(st):
    return "clip: adapters %d pairs %d skipped 0 reads_clipped %d dropped %d bases_clipped %d pairs_clipped %d pairs_dropped %d pairs_too_long %d" % (
        len(ADAPTERS), len(PREFIX), sum(st["reads_clipped"]), sum(st["reads_dropped"]), sum(st["bases_clipped"]), st["pairs_clipped"], st["pairs_dropped"],
        st["pairs_too_long"])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """r1 / r2: the raw pair; per keep_both (False, True) the same files clipped by the Python rule (c1, c2) and its statistics (st);
    ad: the adapter file, the prefix pair in front of the three simple adapters"""
    root = tmp_path_factory.mktemp("clippairstream")
    gen = generator("make_build_golden")
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    t1, t2 = raw_pair(reads, 2027)
    results = pc.pair_results(t1, t2, ADAPTERS, PREFIX)
    out = dict(root=root, ad=root / "adapters.fa", t1=t1, t2=t2, r1=root / "r1.fq", r2=root / "r2.fq", results=results)
    out["ad"].write_bytes(pc.adapters_fa(ADAPTERS, PREFIX))
    out["r1"].write_bytes(t1)
    out["r2"].write_bytes(t2)
    for keep in (False, True):
        texts, st = pc.clip_fastq_pair(t1, t2, ADAPTERS, PREFIX, results=results, keep_both=keep)
        paths = [root / ("c%d_%d.fq" % (f + 1, keep)) for f in range(2)]
        for p, t in zip(paths, texts):
            p.write_bytes(t)
        out[keep] = dict(c1=paths[0], c2=paths[1], st=st, texts=texts)
    st = out[True]["st"]
    # the planted share really clips: pairs by pair mode alone (remnants below 16 bases among them), by simple mode alone and by both
    assert st["pair_only"] > 20 and st["simple_only"] > 50 and st["both"] > 50 and st["pairs_clipped"] > 150, st
    return out


def keep_flag(keep):
    return ["--adapter-keep-both"] if keep else []


# ---- trim ----

@pytest.mark.parametrize("keep", [False, True], ids=["drop_reverse", "keep_both"])
@pytest.mark.parametrize("chunk", [4096, None])
def test_trim_pair_with_a_trimlog(data, tmp_path, keep, chunk):
    extra = ["--chunk-bytes", chunk] if chunk else []
    ref = data[keep]
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    want = cli("trim", "-1", ref["c1"], "-2", ref["c2"], *NAMES, "--trimlog", "log.txt", *WORKFLOW, *extra, cwd=w)
    got = cli("trim", "-1", data["r1"], "-2", data["r2"], *NAMES, "--trimlog", "log.txt", "--adapters", data["ad"], "--adapter-pairs", *keep_flag(keep),
              *WORKFLOW, *extra, cwd=g)
    assert files_of(g) == files_of(w) and len(files_of(g)) == 5 and files_of(g)["p1.fq"] and files_of(g)["log.txt"]
    assert got.stdout == want.stdout == ""
    assert as_read_clipped(got.stderr.splitlines()) == [clip_line(ref["st"])] + want.stderr.splitlines()
    if not keep:   # the reverse read of a clipped pair is dropped: its forward read is unpaired
        assert files_of(g)["u1.fq"].count(b"\n") // 4 > 100


def test_trim_pair_without_a_step_and_other_values(data, tmp_path):
    """no STEP beside the adapters; --adapter-pair-score, --adapter-pair-min and --adapter-seed reach the kernel"""
    raw = [t[:tc._end_of(t, 300)] for t in (data["t1"], data["t2"])]   # (the first 300 pairs: the Python rule runs once more)
    texts, st = pc.clip_fastq_pair(raw[0], raw[1], ADAPTERS, PREFIX, keep_both=True, seed=1, pair_score=20, pair_min=1)
    assert texts != pc.clip_fastq_pair(raw[0], raw[1], ADAPTERS, PREFIX, results=data["results"][:300], keep_both=True)[0]
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    for f in range(2):
        (tmp_path / ("c%d.fq" % (f + 1))).write_bytes(texts[f])
        (tmp_path / ("r%d.fq" % (f + 1))).write_bytes(raw[f])
    want = cli("trim", "-1", tmp_path / "c1.fq", "-2", tmp_path / "c2.fq", *NAMES, "MINLEN:1", cwd=w)
    got = cli("trim", "-1", tmp_path / "r1.fq", "-2", tmp_path / "r2.fq", *NAMES, "--adapters", data["ad"], "--adapter-pairs", "--adapter-keep-both", "--adapter-seed", 1,
              "--adapter-pair-score", 20, "--adapter-pair-min", 1, cwd=g)
    assert files_of(g) == files_of(w)
    assert as_read_clipped(got.stderr.splitlines()) == [clip_line(st)] + want.stderr.splitlines()


def test_trim_pair_gz_in_and_out_and_hostapi(data, tmp_path):
    for side in (1, 2):
        (tmp_path / ("r%d.fq.gz" % side)).write_bytes(gz.bgzf(data["t%d" % side]))
    names = ["p1.fq.gz", "u1.fq.gz", "p2.fq.gz", "u2.fq.gz"]
    w, g, h = tmp_path / "want", tmp_path / "got", tmp_path / "api"
    for d in (w, g, h):
        d.mkdir()
    flags = [x for pair in zip(["-o1", "-u1", "-o2", "-u2"], names) for x in pair]
    ref = data[True]
    cli("trim", "-1", ref["c1"], "-2", ref["c2"], *flags, "--gz-out", *WORKFLOW, cwd=w)
    cli("trim", "-1", tmp_path / "r1.fq.gz", "-2", tmp_path / "r2.fq.gz", *flags, "--gz", "--gz-out", "--adapters", data["ad"], "--adapter-pairs",
        "--adapter-keep-both", *WORKFLOW, cwd=g)
    assert files_of(g) == files_of(w)
    assert gzip.decompress(files_of(g)["p1.fq.gz"]).count(b"\n") > 400
    st = hostapi.trim_fastq_pair(str(tmp_path / "r1.fq.gz"), str(tmp_path / "r2.fq.gz"), [str(h / n) for n in names], WORKFLOW, gz=True, gz_out=True,
                                 adapters=str(data["ad"]), adapter_pairs=True, adapter_keep_both=True)
    assert files_of(h) == files_of(w) and st[0]["both"] > 0
    rep, prep = hostapi.clip_report(), hostapi.clip_pair_report()
    assert (rep["adapters"], rep["skipped"], prep["pairs"]) == (3, 0, 1)
    for f in ("reads_clipped", "reads_dropped", "bases_clipped"):
        assert rep[f] == ref["st"][f], f
    for f in ("pairs_clipped", "pairs_dropped", "pairs_too_long"):
        assert prep[f] == ref["st"][f], f


def test_without_the_switch_the_prefix_entries_are_skipped(data, tmp_path):
    """the same command line without --adapter-pairs: today's line with `skipped 2`, and simple mode alone"""
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    clipped = [cc.clip_fastq(data["t%d" % side], ADAPTERS, side=side) for side in (1, 2)]
    for f in range(2):
        (tmp_path / ("c%d.fq" % (f + 1))).write_bytes(clipped[f][0])
    want = cli("trim", "-1", tmp_path / "c1.fq", "-2", tmp_path / "c2.fq", *NAMES, *WORKFLOW, cwd=w)
    got = cli("trim", "-1", data["r1"], "-2", data["r2"], *NAMES, "--adapters", data["ad"], *WORKFLOW, cwd=g)
    assert files_of(g) == files_of(w)
    line = "clip: adapters 3 skipped 2 reads_clipped %d dropped %d bases_clipped %d" % tuple(sum(c[1][k] for c in clipped) for k in ("reads_clipped", "reads_dropped", "bases_clipped"))
    assert as_read_clipped(got.stderr.splitlines()) == [line] + want.stderr.splitlines()


# ---- run, run-multi ----

def test_run_pair_keep_both_against_the_clipped_files(data, tmp_path):
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    ref = data[True]
    common = ["-o", "s", "--model", "fre", "--db-out", "db", "--gfa-out", "g", *WORKFLOW]
    want = cli("run", "-1", ref["c1"], "-2", ref["c2"], *common, cwd=w)
    got = cli("run", "-1", data["r1"], "-2", data["r2"], "--adapters", data["ad"], "--adapter-pairs", "--adapter-keep-both", *common, cwd=g)
    rows = calling_files(w, "s")["_allele_frequency.txt"].decode().splitlines()
    print("run on the clipped pair: L = %s, %d lines in allele_frequency.txt" % (want.stdout.splitlines()[0], len(rows)))
    assert len(rows) >= 1
    assert calling_files(g, "s") == calling_files(w, "s") and files_of(g) == files_of(w)
    assert untimed(got.stdout) == untimed(want.stdout)
    keep = lambda r: [l for l in r.stderr.splitlines() if l.startswith(("clip: ", "trim: ", "run: reads "))]
    assert as_read_clipped(keep(got)) == [clip_line(ref["st"])] + keep(want)


def test_run_reads_without_keep_both(data, tmp_path, monkeypatch):
    """hostapi.run_reads with adapter_pairs alone: a clipped pair is not counted at all (its reverse read is dropped)"""
    w, h = tmp_path / "want", tmp_path / "api"
    for d in (w, h):
        d.mkdir()
    ref = data[False]
    monkeypatch.chdir(h)
    st = hostapi.run_reads(None, "s", pairs=[(str(data["r1"]), str(data["r2"]))], steps=WORKFLOW, adapters=str(data["ad"]), adapter_pairs=True, db_out="db")
    monkeypatch.chdir(w)
    want = hostapi.run_reads(None, "s", pairs=[(str(ref["c1"]), str(ref["c2"]))], steps=WORKFLOW, db_out="db")
    assert {k: v for k, v in st.items() if k != "trim"} == {k: v for k, v in want.items() if k != "trim"}
    assert files_of(h)["db.kmc_suf"] == files_of(w)["db.kmc_suf"]
    assert st["trim"][0][0]["both"] == want["trim"][0][0]["both"] <= want["trim"][0][0]["reads"] - ref["st"]["pairs_clipped"]
    assert hostapi.clip_pair_report()["pairs"] == 0   # the last call took no adapters


def test_run_multi_two_paired_samples(data, tmp_path):
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    ref = data[True]
    # sample b: the pair the other way round (one file in two samples is refused: it reads copies)
    texts, st_b = pc.clip_fastq_pair(data["t2"], data["t1"], ADAPTERS, PREFIX, keep_both=True)
    for name, t in (("b1.fq", data["t2"]), ("b2.fq", data["t1"]), ("bc1.fq", texts[0]), ("bc2.fq", texts[1])):
        (tmp_path / name).write_bytes(t)
    common = ["-o", "s", "--db-out", "db", "--gfa-out", "g", *WORKFLOW]
    want = cli("run-multi", "--sample", "a", "-1", ref["c1"], "-2", ref["c2"], "--sample", "b", "-1", tmp_path / "bc1.fq", "-2", tmp_path / "bc2.fq", *common, cwd=w)
    got = cli("run-multi", "--sample", "a", "-1", data["r1"], "-2", data["r2"], "--sample", "b", "-1", tmp_path / "b1.fq", "-2", tmp_path / "b2.fq",
              "--adapters", data["ad"], "--adapter-pairs", "--adapter-keep-both", *common, cwd=g)
    assert calling_files(g, "s") == calling_files(w, "s") and files_of(g) == files_of(w)
    assert untimed(got.stdout) == untimed(want.stdout)
    keep = lambda r: [l for l in r.stderr.splitlines() if l.startswith(("clip: ", "trim: "))]
    wt = keep(want)
    assert as_read_clipped(keep(got)) == [clip_line(ref["st"]), wt[0], clip_line(st_b), wt[1]]
