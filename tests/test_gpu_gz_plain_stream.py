"""`--gz-plain` end to end: every sub-command that takes the sequencer's files, on plain-gzip input (what gzip and pigz write), against the
same command on the inflated files without the flag.  Bytes only: every file, stdout, and the command's line on stderr are identical.
The reads are the pair of tests/test_gpu_gz_stream.py (512 pairs, about 107 KB a file), here as one gzip member with a file name in its
header (.gz), as two members -- the first stored and the second without matches, so that the file is longer than the 64 KiB the reader
hands over at a time and the second member's stream crosses that edge inside a block; cut inside a record (.2.gz) -- and as blocked
gzip (.bgzf.gz)."""
import os
import struct
import zlib

import numpy as np
import pytest

import gz_cases as gz
import gzp_cases as gp
from test_gpu_gz_stream import RUN, WORKFLOW, cli, fastq_text, generator, lines_with, tree, untimed, DEPTH

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    root = tmp_path_factory.mktemp("gzplainreads")
    gen = generator("make_build_golden")
    rs = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2025)
    out = {}
    for name, part in (("r1", rs[0::2]), ("r2", rs[1::2])):
        text = fastq_text(part, rng)
        cut = 60001
        first = gp.member(text[:cut], gp.raw(text[:cut], 0))
        two = first + gp.member(text[cut:], gp.raw(text[cut:], 6, 8, zlib.Z_HUFFMAN_ONLY), head=gp.header(name=b"lane2.fq", comment=b"second lane"))
        assert len(first) + 1000 < 65536 < len(two) - 8000 and text[cut - 1:cut] != b"\n"
        for suffix, data in ((".fq", text), (".fq.gz", gp.member(text, head=gp.header(name=name.encode() + b".fq"))), (".2.fq.gz", two),
                             (".bgzf.fq.gz", gz.bgzf(text))):
            (root / (name + suffix)).write_bytes(data)
            out[name + suffix] = root / (name + suffix)
        assert hostapi.gunzip_member(two, block_bytes=65536) == text
    return out


@pytest.fixture(scope="module")
def plain_run(reads, tmp_path_factory):
    d = tmp_path_factory.mktemp("plainrun")
    r = cli("run", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *RUN, *WORKFLOW, cwd=d)
    files = tree(d)
    assert len(files["PloidyFrost_output/s_allele_frequency.txt"].splitlines()) >= 5
    return dict(files=files, stdout=r.stdout, lines=lines_with(r.stderr, "trim: ") + lines_with(r.stderr, "run: reads "))


def test_count(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    w = cli("count", "-k", 25, "-ci", 1, "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "db", "--hist", "h.txt", cwd=a)
    g = cli("count", "-k", 25, "-ci", 1, "-i", reads["r1.fq.gz"], "-i", reads["r2.2.fq.gz"], "-o", "db", "--hist", "h.txt", "--gz-plain", "--chunk-bytes", 4096, cwd=b)
    assert tree(a) == tree(b) and sorted(tree(a)) == ["db.kmc_pre", "db.kmc_suf", "h.txt"]
    assert lines_with(g.stderr, "count: ") == lines_with(w.stderr, "count: ") and len(lines_with(w.stderr, "count: ")) == 1 and g.stdout == w.stdout
    st = hostapi.count_fastq([str(reads["r1.fq.gz"]), str(reads["r2.bgzf.fq.gz"])], str(b / "py"), k=25, ci=1, gz="plain")
    assert (b / "py.kmc_suf").read_bytes() == (a / "db.kmc_suf").read_bytes() and st


def test_trim_pair_with_a_log_and_single(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    outs = ["-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq", "--trimlog", "log.txt"]
    w = cli("trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *outs, *WORKFLOW, cwd=a)
    g = cli("trim", "-1", reads["r1.fq.gz"], "-2", reads["r2.bgzf.fq.gz"], *outs, "--gz-plain", *WORKFLOW, cwd=b)   # one plain gzip, one blocked
    assert tree(a) == tree(b) and len(tree(a)) == 5 and all(tree(a).values())
    assert lines_with(g.stderr, "trim: ") == lines_with(w.stderr, "trim: ") and len(lines_with(w.stderr, "trim: ")) == 1
    w = cli("trim", "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "t.fq", *WORKFLOW, cwd=a)
    g = cli("trim", "-i", reads["r1.2.fq.gz"], "-i", reads["r2.fq"], "-o", "t.fq", "--gz-plain", "--chunk-bytes", 4096, *WORKFLOW, cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) == 6
    assert lines_with(g.stderr, "trim: ") == lines_with(w.stderr, "trim: ")


@pytest.mark.parametrize("name,f1,f2,extra", [
    ("both_gzip", "r1.fq.gz", "r2.fq.gz", []),
    ("two_members_small_chunks", "r1.2.fq.gz", "r2.2.fq.gz", ["--chunk-bytes", 4096]),
    ("gzip_and_blocked", "r1.fq.gz", "r2.bgzf.fq.gz", []),
    ("gzip_and_text", "r1.fq", "r2.2.fq.gz", [])])
def test_run_pair_with_steps(reads, plain_run, tmp_path, name, f1, f2, extra):
    r = cli("run", "-1", reads[f1], "-2", reads[f2], *RUN, "--gz-plain", *extra, *WORKFLOW, cwd=tmp_path)
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
    g = cli("run", "-i", reads["r1.2.fq.gz"], "-i", reads["r2.fq.gz"], *RUN, "--gz-plain", "--chunk-bytes", 50000, cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) >= 15
    assert untimed(g.stdout) == untimed(w.stdout) and lines_with(g.stderr, "run: reads ") == lines_with(w.stderr, "run: reads ")


def test_run_multi_one_sample_of_each_kind(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    tail = ["-o", "m", "--db-out", "db", "--gfa-out", "g"]
    third = tmp_path / "r3.fq"
    third.write_bytes(reads["r1.fq"].read_bytes()[:40000].rsplit(b"\n@", 1)[0] + b"\n")
    w = cli("run-multi", "--sample", "A", "-i", reads["r1.fq"], "--sample", "B", "-i", reads["r2.fq"], "--sample", "C", "-i", third, *tail, cwd=a)
    g = cli("run-multi", "--sample", "A", "-i", reads["r1.2.fq.gz"], "--sample", "B", "-i", reads["r2.bgzf.fq.gz"], "--sample", "C", "-i", third, *tail,
            "--gz-plain", cwd=b)
    assert tree(a) == tree(b) and len(tree(a)) >= 6
    assert untimed(g.stdout) == untimed(w.stdout) and lines_with(g.stderr, "run-multi: ") == lines_with(w.stderr, "run-multi: ")


def test_a_flipped_crc_in_the_second_member(reads, tmp_path):
    data = bytearray(reads["r1.2.fq.gz"].read_bytes())
    data[-6] ^= 0x04     # the CRC-32 of the second member's trailer
    bad = tmp_path / "bad.fq.gz"
    bad.write_bytes(bytes(data))
    with pytest.raises(ValueError) as e:
        hostapi.gunzip_member(bytes(data))
    assert (e.value.clause, e.value.member, e.value.byte) == (gp.CLAUSE["crc"], 1, len(data) - 8)
    before = sorted(os.listdir(tmp_path))
    want = "%s: member 2, byte %d: CRC-32 mismatch" % (bad, len(data) - 8)
    r = cli("count", "-k", 25, "-i", bad, "-o", "db", "--gz-plain", cwd=tmp_path, ok=False)
    assert r.returncode != 0 and r.stdout == "" and "count: " + want in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    r = cli("run", "-1", bad, "-2", reads["r2.fq.gz"], "-o", "s", "--db-out", "db", "--gfa-out", "g", "--gz-plain", *WORKFLOW, cwd=tmp_path, ok=False)
    assert r.returncode != 0 and r.stdout == "" and "run: " + want in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    with pytest.raises(ValueError) as e:
        hostapi.count_fastq([str(bad)], str(tmp_path / "db"), k=25, gz="plain")
    assert str(e.value) == "count: " + want
    # a length that differs from ISIZE, and a file that ends inside the second member's stream
    data = bytearray(reads["r1.2.fq.gz"].read_bytes())
    struct.pack_into("<I", data, len(data) - 4, struct.unpack_from("<I", data, len(data) - 4)[0] + 1)
    bad.write_bytes(bytes(data))
    r = cli("count", "-k", 25, "-i", bad, "-o", "db", "--gz-plain", cwd=tmp_path, ok=False)
    assert r.returncode != 0 and "member 2, byte %d: the inflated length differs from ISIZE mod 2^32" % (len(data) - 4) in r.stderr, r.stderr
    bad.write_bytes(bytes(data[:-3000]))
    r = cli("count", "-k", 25, "-i", bad, "-o", "db", "--gz-plain", cwd=tmp_path, ok=False)
    assert r.returncode != 0 and "member 2, byte " in r.stderr and "the file ends inside a deflate block" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
