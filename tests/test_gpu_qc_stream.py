"""`ploidyfrost qc`, `trim --report` and `run --report` end to end on files of a few hundred records: the report is the bytes the
Python restatement of qc_cases.py writes, it does not depend on chunking or on how the input is compressed, `--report` leaves every
other output as it is, and the kept stage of a side is the raw stage of `qc` on the files `trim` wrote for that side."""
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import gz_cases as gz
import qc_cases as qc
import trim_cases as tc

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WORKFLOW = tc.WORKFLOW
DEPTH = 128
PAIR_OUT = ["p1.fq", "u1.fq", "p2.fq", "u2.fq"]
PAIR_FLAGS = [x for pair in zip(["-o1", "-u1", "-o2", "-u2"], PAIR_OUT) for x in pair]


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def raw_fastq(reads, rng):
    """the reads as FASTQ: most qualities flat, a quarter with a degrading tail, a tenth with a poor head, some N"""
    recs = []
    for i, r in enumerate(reads):
        seq, n = bytearray(r.encode()), len(r)
        if rng.random() < 0.1:
            seq[int(rng.integers(n))] = ord("N")
        qual = bytearray(b"I" * n)
        if rng.random() < 0.25:
            cut = int(rng.integers(30, n))
            qual[cut:] = bytes(33 + int(q) for q in rng.integers(2, 25, size=n - cut))
        if rng.random() < 0.1:
            qual[:5] = b"#####"
        recs.append((b"r%d" % i, bytes(seq), bytes(qual)))
    return tc.fastq(recs)


def files_of(d, but=()):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d))) if os.path.isfile(os.path.join(str(d), f)) and f not in but}


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def python_report(texts1, texts2=(), steps=None, phred=33):
    t, c = qc.new_tables(), qc.new_clip()
    for side, texts in ((1, texts1), (2, texts2)):
        for text in texts:
            qc.add_chunk(t, c, text, side, phred, True, steps)
    return qc.report_text(t, None, phred), t


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("qcstream")
    gen = generator("make_build_golden")
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2027)
    out = dict(root=root)
    for side, part in ((1, reads[0::2]), (2, reads[1::2])):
        out["t%d" % side] = raw_fastq(part, rng)
        out["r%d" % side] = root / ("r%d.fq" % side)
        out["r%d" % side].write_bytes(out["t%d" % side])
    assert out["t1"].count(b"\n") // 4 >= 300
    return out


# ---- qc ----

def test_qc_writes_the_python_report(data, tmp_path):
    want, tables = python_report([data["t1"]])
    r = cli("qc", "-i", data["r1"], "-o", "rep.tsv", cwd=tmp_path)
    assert (tmp_path / "rep.tsv").read_bytes() == want and sorted(os.listdir(tmp_path)) == ["rep.tsv"]
    assert r.stderr.splitlines() == [qc.side_line(1, tables[0][0])] and r.stdout == ""
    # two sides, and two files on one side
    want2, tables2 = python_report([data["t1"]], [data["t2"], data["t1"]])
    r = cli("qc", "-1", data["r1"], "-2", data["r2"], "-2", data["r1"], "-o", "rep2.tsv", cwd=tmp_path)
    assert (tmp_path / "rep2.tsv").read_bytes() == want2
    assert r.stderr.splitlines() == [qc.side_line(1, tables2[0][0]), qc.side_line(2, tables2[1][0])]
    hostapi.qc_fastq([str(data["r1"])], str(tmp_path / "api.tsv"), paths2=[str(data["r2"]), str(data["r1"])])
    assert (tmp_path / "api.tsv").read_bytes() == want2


def test_qc_does_not_depend_on_chunks_or_compression(data, tmp_path):
    want, _ = python_report([data["t1"]])
    (tmp_path / "b.fq.gz").write_bytes(gz.bgzf(data["t1"]))
    (tmp_path / "p.fq.gz").write_bytes(gzip.compress(data["t1"]))
    for name, args in (("chunk", ["-i", data["r1"], "--chunk-bytes", 4096]), ("gz", ["-i", tmp_path / "b.fq.gz", "--gz"]),
                       ("gz_chunk", ["-i", tmp_path / "b.fq.gz", "--gz", "--chunk-bytes", 4096]), ("plain", ["-i", tmp_path / "p.fq.gz", "--gz-plain"])):
        cli("qc", *args, "-o", name + ".tsv", cwd=tmp_path)
        assert (tmp_path / (name + ".tsv")).read_bytes() == want, name


def test_qc_format_refusal_names_path_and_record(data, tmp_path):
    bad = tmp_path / "bad.fq"
    bad.write_bytes(data["t1"][:2000].rsplit(b"@", 1)[0] + b"@x\nACGT\n+\nII\n")
    r = cli("qc", "-i", data["r1"], "-i", bad, "-o", "rep.tsv", cwd=tmp_path, ok=False)
    n = bad.read_bytes().count(b"\n") // 4
    assert r.returncode != 0 and "qc: %s: record %d: " % (bad, n) in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.fq"]


def test_phred_64_input_under_the_default_offset(data, tmp_path):
    recs, _ = tc.parse_records(data["t1"][:30000], False)
    text = tc.fastq([(h[1:], s, bytes(min(c + 31, 126) for c in q)) for h, s, _, q in recs])
    (tmp_path / "p64.fq").write_bytes(text)
    r = cli("qc", "-i", "p64.fq", "-o", "rep.tsv", cwd=tmp_path)
    rep = (tmp_path / "rep.tsv").read_bytes()
    assert rep.split(b"\n")[1] == b"# phred 33 hint 64" and rep == python_report([text])[0]
    quals = [r[3] for r in tc.parse_records(text)[0]]
    lo, hi = min(min(q) for q in quals), max(max(q) for q in quals)
    assert lo >= 64
    assert r.stderr.splitlines()[-1] == "qc: quality bytes run from %d to %d: the files look like phred 64, not 33" % (lo, hi)
    r = cli("qc", "-i", "p64.fq", "-o", "rep64.tsv", "--phred", 64, cwd=tmp_path)
    assert len(r.stderr.splitlines()) == 1 and (tmp_path / "rep64.tsv").read_bytes() == python_report([text], phred=64)[0]
    # trim under the wrong offset trims nothing and says why it may be so
    r = cli("trim", "-i", "p64.fq", "-o", "out.fq", *WORKFLOW, "--report", "trim.tsv", cwd=tmp_path)
    assert "the files look like phred 64, not 33" in r.stderr.splitlines()[-1]


# ---- trim --report ----

def test_trim_single_report(data, tmp_path):
    w, g = tmp_path / "want", tmp_path / "got"
    for d in (w, g):
        d.mkdir()
    want = cli("trim", "-i", data["r1"], "-i", data["r2"], "-o", "out.fq", "--trimlog", "log.txt", *WORKFLOW, cwd=w)
    got = cli("trim", "-i", data["r1"], "-i", data["r2"], "-o", "out.fq", "--trimlog", "log.txt", *WORKFLOW, "--report", "rep.tsv", "--chunk-bytes", 50000, cwd=g)
    assert files_of(g, but=("rep.tsv",)) == files_of(w) and sorted(os.listdir(g)) == ["log.txt", "out.fq", "rep.tsv"]
    assert got.stderr.splitlines()[: len(want.stderr.splitlines())] == want.stderr.splitlines() and got.stdout == want.stdout
    rep = (g / "rep.tsv").read_bytes()
    assert rep == python_report([data["t1"], data["t2"]], steps=WORKFLOW)[0]
    # raw = qc on the inputs; kept = qc on what trim wrote
    cli("qc", "-i", data["r1"], "-i", data["r2"], "-o", "raw.tsv", cwd=g)
    cli("qc", "-i", "out.fq", "-o", "kept.tsv", cwd=g)
    assert qc.rows_of(rep, 1, "raw") == qc.rows_of((g / "raw.tsv").read_bytes(), 1, "raw")
    assert qc.rows_of(rep, 1, "kept") == qc.rows_of((g / "kept.tsv").read_bytes(), 1, "raw")
    assert len(qc.rows_of(rep, 1, "kept")["position"]) >= 50 and qc.rows_of(rep, 1, "kept") != qc.rows_of(rep, 1, "raw")


def test_trim_pair_report(data, tmp_path):
    w, g, h = tmp_path / "want", tmp_path / "got", tmp_path / "api"
    for d in (w, g, h):
        d.mkdir()
    cli("trim", "-1", data["r1"], "-2", data["r2"], *PAIR_FLAGS, *WORKFLOW, cwd=w)
    cli("trim", "-1", data["r1"], "-2", data["r2"], *PAIR_FLAGS, *WORKFLOW, "--report", "rep.tsv", cwd=g)
    assert files_of(g, but=("rep.tsv",)) == files_of(w)
    rep = (g / "rep.tsv").read_bytes()
    assert rep == python_report([data["t1"]], [data["t2"]], steps=WORKFLOW)[0]
    cli("qc", "-1", data["r1"], "-2", data["r2"], "-o", "raw.tsv", cwd=g)
    cli("qc", "-1", "p1.fq", "-1", "u1.fq", "-2", "p2.fq", "-2", "u2.fq", "-o", "kept.tsv", cwd=g)   # a side's kept records: its -o and -u together
    for side in (1, 2):
        assert qc.rows_of(rep, side, "raw") == qc.rows_of((g / "raw.tsv").read_bytes(), side, "raw")
        assert qc.rows_of(rep, side, "kept") == qc.rows_of((g / "kept.tsv").read_bytes(), side, "raw")
    hostapi.trim_fastq_pair(str(data["r1"]), str(data["r2"]), [str(h / n) for n in PAIR_OUT], WORKFLOW, report=str(h / "rep.tsv"), chunk_bytes=4096)
    assert files_of(h) == files_of(g, but=("raw.tsv", "kept.tsv"))


# ---- run --report ----

def test_run_pair_report(data, tmp_path):
    w, g, t = tmp_path / "want", tmp_path / "got", tmp_path / "trim"
    for d in (w, g, t):
        d.mkdir()
    common = ["-1", data["r1"], "-2", data["r2"], "-o", "s", *WORKFLOW]
    want = cli("run", *common, cwd=w)
    got = cli("run", *common, "--report", "rep.tsv", cwd=g)
    files = calling_files(w, "s")
    assert len(files) == 12 and calling_files(g, "s") == files
    assert files_of(g, but=("rep.tsv",)) == files_of(w) and [l for l in got.stdout.splitlines() if " time " not in l] == [l for l in want.stdout.splitlines() if " time " not in l]
    cli("trim", "-1", data["r1"], "-2", data["r2"], *PAIR_FLAGS, *WORKFLOW, "--report", "rep.tsv", cwd=t)
    assert (g / "rep.tsv").read_bytes() == (t / "rep.tsv").read_bytes()
    assert [l for l in got.stderr.splitlines() if l.startswith("qc: ")] == [qc.side_line(s, python_report([data["t1"]], [data["t2"]])[1][s - 1][0]) for s in (1, 2)]
