"""`--gz` end to end: every sub-command that takes the sequencer's files, on blocked-gzip input with `--gz`, against the same command on
the plain files without it.  Bytes only: every file, stdout, and the command's line on stderr are identical.  The reads are the pair of
tests/test_gpu_run_trim.py's chain (the build_k25 generator at depth 64, seeded qualities: 512 pairs), compressed here in members of
64 KiB less 256 bytes of text as `bgzip` cuts them, plus the end-of-file marker.  A file is about 107 KB: two members as bgzip cuts
it, so `--chunk-bytes 4096` crosses one chunk edge a file there; the carry at almost every edge is what the files cut at 1 000 bytes
(more than a hundred members each, most of them ending inside a record) are for."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import gz_cases as gz
import trim_cases as tc

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WORKFLOW = tc.WORKFLOW
MODEL = ["--model", "fre"]
DEPTH = 64


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def seeded_quality(rng, n):
    x = rng.random()
    if x < 0.04:
        return "#" * n
    if x < 0.29:
        cut = int(rng.integers(30, n))
        return "I" * cut + "".join(chr(33 + int(q)) for q in rng.integers(2, 25, size=n - cut))
    return "I" * n


def fastq_text(reads, rng):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, r, seeded_quality(rng, len(r))) for i, r in enumerate(reads)).encode()


def untimed(stdout):
    return [l for l in stdout.splitlines() if " time " not in l]


def lines_with(text, word):
    return [l for l in text.splitlines() if l.startswith(word)]


def tree(d):
    """every file under d, by its path from d"""
    out = {}
    for dp, _, files in os.walk(str(d)):
        for f in files:
            p = os.path.join(dp, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, str(d))] = fh.read()
    return out


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """r1 / r2 plain, as bgzip cuts them (.gz), and cut at 1 000 bytes so that most members end inside a record (.k.gz)"""
    root = tmp_path_factory.mktemp("gzreads")
    gen = generator("make_build_golden")
    rs = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2025)
    out = {}
    for name, part in (("r1", rs[0::2]), ("r2", rs[1::2])):
        text = fastq_text(part, rng)
        assert len(text) > gz.BGZIP_CUT       # more than one member
        for suffix, data in ((".fq", text), (".fq.gz", gz.bgzf(text)), (".k.fq.gz", gz.bgzf(text, cut=1000))):
            (root / (name + suffix)).write_bytes(data)
            out[name + suffix] = root / (name + suffix)
        assert hostapi.inflate_bgzf(gz.bgzf(text, cut=1000)) == text
    return out


RUN = ["-o", "s", "--db-out", "db", "--gfa-out", "g"] + MODEL


@pytest.fixture(scope="module")
def plain_run(reads, tmp_path_factory):
    d = tmp_path_factory.mktemp("plainrun")
    r = cli("run", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *RUN, *WORKFLOW, cwd=d)
    files = tree(d)
    calling = [f for f in files if f.startswith("PloidyFrost_output") and "model_result" not in f]
    assert len(calling) == 12 and len(files["PloidyFrost_output/s_allele_frequency.txt"].splitlines()) >= 5
    return dict(files=files, stdout=r.stdout, lines=lines_with(r.stderr, "trim: ") + lines_with(r.stderr, "run: reads "))


def test_count(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    w = cli("count", "-k", 25, "-ci", 1, "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "db", "--hist", "h.txt", cwd=a)
    g = cli("count", "-k", 25, "-ci", 1, "-i", reads["r1.fq.gz"], "-i", reads["r2.k.fq.gz"], "-o", "db", "--hist", "h.txt", "--gz", "--chunk-bytes", 30000, cwd=b)
    assert tree(a) == tree(b) and sorted(tree(a)) == ["db.kmc_pre", "db.kmc_suf", "h.txt"]
    assert lines_with(g.stderr, "count: ") == lines_with(w.stderr, "count: ") and len(lines_with(w.stderr, "count: ")) == 1 and g.stdout == w.stdout
    v = cli("count", "-k", 25, "-i", reads["r1.fq.gz"], "-o", "v", "--gz", "-v", cwd=b)
    assert v.returncode == 0


def test_trim_single_and_pair(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    outs = ["-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq", "--trimlog", "log.txt"]
    w = cli("trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *outs, *WORKFLOW, cwd=a)
    g = cli("trim", "-1", reads["r1.fq.gz"], "-2", reads["r2.fq.gz"], *outs, "--gz", *WORKFLOW, cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) == 5 and all(tree(a).values())
    assert lines_with(g.stderr, "trim: ") == lines_with(w.stderr, "trim: ") and len(lines_with(w.stderr, "trim: ")) == 1
    w = cli("trim", "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "t.fq", "--trimlog", "tl.txt", *WORKFLOW, cwd=a)
    g = cli("trim", "-i", reads["r1.k.fq.gz"], "-i", reads["r2.fq"], "-o", "t.fq", "--trimlog", "tl.txt", "--gz", "--chunk-bytes", 4096, *WORKFLOW, cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) == 7
    assert lines_with(g.stderr, "trim: ") == lines_with(w.stderr, "trim: ")


@pytest.mark.parametrize("name,f1,f2,extra", [
    ("bgzip_members", "r1.fq.gz", "r2.fq.gz", []),
    ("one_member_a_chunk", "r1.fq.gz", "r2.fq.gz", ["--chunk-bytes", 4096]),
    ("members_of_1000_bytes", "r1.k.fq.gz", "r2.k.fq.gz", ["--chunk-bytes", 20000]),
    ("second_file_plain", "r1.fq.gz", "r2.fq", [])])
def test_run_pair_with_steps(reads, plain_run, tmp_path, name, f1, f2, extra):
    r = cli("run", "-1", reads[f1], "-2", reads[f2], *RUN, "--gz", *extra, *WORKFLOW, cwd=tmp_path)
    got = tree(tmp_path)
    assert sorted(got) == sorted(plain_run["files"])
    for f in got:
        assert got[f] == plain_run["files"][f], f
    assert untimed(r.stdout) == untimed(plain_run["stdout"])
    assert lines_with(r.stderr, "trim: ") + lines_with(r.stderr, "run: reads ") == plain_run["lines"] and len(plain_run["lines"]) == 2


def test_run_single_without_steps(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    w = cli("run", "-i", reads["r1.fq"], "-i", reads["r2.fq"], *RUN, cwd=a)
    g = cli("run", "-i", reads["r1.k.fq.gz"], "-i", reads["r2.fq.gz"], *RUN, "--gz", "--chunk-bytes", 50000, cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) >= 15
    assert untimed(g.stdout) == untimed(w.stdout) and lines_with(g.stderr, "run: reads ") == lines_with(w.stderr, "run: reads ")
    v = cli("run", "-i", reads["r1.fq.gz"], "-i", reads["r2.fq.gz"], "-o", "v", "--gz", "-v", cwd=b)
    assert v.returncode == 0


def test_run_multi_one_sample_blocked_one_plain(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    tail = ["-o", "m", "--db-out", "db", "--gfa-out", "g"]
    w = cli("run-multi", "--sample", "A", "-i", reads["r1.fq"], "--sample", "B", "-i", reads["r2.fq"], *tail, cwd=a)
    g = cli("run-multi", "--sample", "A", "-i", reads["r1.fq.gz"], "--sample", "B", "-i", reads["r2.fq"], *tail, "--gz", cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) >= 6
    assert untimed(g.stdout) == untimed(w.stdout) and lines_with(g.stderr, "run-multi: ") == lines_with(w.stderr, "run-multi: ")


def test_a_flipped_byte_in_the_seventh_member(reads, tmp_path):
    data = bytearray(reads["r1.k.fq.gz"].read_bytes())
    off = gz.member_offsets(bytes(data))
    assert len(off) > 20
    data[off[6] + 18 + (off[7] - off[6] - 26) // 2] ^= 0x10     # the middle of the seventh member's payload
    clause = hostapi.inflate_bgzf_member(bytes(data[off[6]: off[7]]))[0]
    assert clause != 0
    bad = tmp_path / "bad.fq.gz"
    bad.write_bytes(bytes(data))
    before = sorted(os.listdir(tmp_path))
    want = "%s: member 7, byte %d: %s" % (bad, off[6], hostapi.inflate_clause_text(clause))
    r = cli("count", "-k", 25, "-i", bad, "-o", "db", "--gz", "--chunk-bytes", 3000, cwd=tmp_path, ok=False)
    assert r.returncode != 0 and r.stdout == "" and "count: " + want in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    for extra in ([], ["--chunk-bytes", 100000]):
        r = cli("run", "-1", bad, "-2", reads["r2.fq.gz"], "-o", "s", "--db-out", "db", "--gfa-out", "g", "--gz", *extra, *WORKFLOW, cwd=tmp_path, ok=False)
        assert r.returncode != 0 and r.stdout == "" and "run: " + want in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == before
    with pytest.raises(ValueError) as e:
        hostapi.count_fastq([str(bad)], str(tmp_path / "db"), k=25, gz=True)
    assert str(e.value) == "count: " + want
