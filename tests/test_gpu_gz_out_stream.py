"""`--gz-out` end to end: `trim` and `mask` with the flag against the same command without it.  Every read output inflates (Python's gzip)
to the plain run's file, is the same bytes with `--chunk-bytes 4096` as with the default, and is what the host rule makes of the plain
file (hostapi.deflate_bgzf): a function of its text alone.  stdout, the command's line on stderr, the trim log and the database are the
plain run's.  Then `count --gz` on what `trim --gz-out` wrote gives the database `count` gives on the plain files.  The reads are the
pair of tests/test_gpu_gz_stream.py (512 pairs, about 107 KB a file: two members)."""
import gzip
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
DEPTH = 64


def cli(*a, cwd):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def seeded_quality(rng, n):
    x = rng.random()
    if x < 0.04:
        return "#" * n
    if x < 0.29:
        cut = int(rng.integers(30, n))
        return "I" * cut + "".join(chr(33 + int(q)) for q in rng.integers(2, 25, size=n - cut))
    return "I" * n


def tree(d):
    out = {}
    for dp, _, files in os.walk(str(d)):
        for f in files:
            with open(os.path.join(dp, f), "rb") as fh:
                out[os.path.relpath(os.path.join(dp, f), str(d))] = fh.read()
    return out


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    root = tmp_path_factory.mktemp("gzoreads")
    spec = importlib.util.spec_from_file_location("make_build_golden", os.path.join(GOLDEN, "make_build_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rs = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2025)
    out = {}
    for name, part in (("r1", rs[0::2]), ("r2", rs[1::2])):
        text = "".join("@r%d\n%s\n+\n%s\n" % (i, r, seeded_quality(rng, len(r))) for i, r in enumerate(part)).encode()
        assert len(text) > gz.BGZIP_CUT
        for suffix, data in ((".fq", text), (".fq.gz", gz.bgzf(text))):
            (root / (name + suffix)).write_bytes(data)
            out[name + suffix] = root / (name + suffix)
    return out


def with_and_without(tmp_path, args, read_outputs, who, markers=()):
    """args without the flag in a/, with it in b/, with it and --chunk-bytes 4096 in c/; returns the three trees"""
    dirs = [tmp_path / x for x in "abc"]
    for d in dirs:
        d.mkdir()
    plain = cli(*args, cwd=dirs[0])
    runs = [cli(*args, "--gz-out", cwd=dirs[1]), cli(*args, "--gz-out", "--chunk-bytes", 4096, cwd=dirs[2])]
    trees = [tree(d) for d in dirs]
    assert sorted(trees[0]) == sorted(trees[1]) == sorted(trees[2])   # the same names, and no temporary file
    line = [l for l in plain.stderr.splitlines() if l.startswith(who + ": ")]
    assert len(line) == 1
    for r in runs:
        assert r.stdout == plain.stdout and [l for l in r.stderr.splitlines() if l.startswith(who + ": ")] == line
    for name, data in trees[0].items():
        if name in read_outputs:
            assert gzip.decompress(trees[1][name]) == data, name
            assert trees[1][name] == trees[2][name] == hostapi.deflate_bgzf(data), name
            assert trees[1][name].endswith(gz.EOF_MARKER)
            assert (trees[1][name] == gz.EOF_MARKER) == (name in markers) == (data == b""), name
        else:   # the trim log, the database
            assert trees[1][name] == trees[2][name] == data, name
    return trees


PAIR_OUTS = ["-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq"]
PAIR_NAMES = ["o1.fq", "u1.fq", "o2.fq", "u2.fq"]


def test_trim_two_single_inputs_give_one_stream(reads, tmp_path):
    trees = with_and_without(tmp_path, ["trim", "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "t.fq"] + WORKFLOW, ["t.fq"], "trim")
    assert len(trees[0]["t.fq"]) > 2 * 65280 and len(gz.member_offsets(trees[1]["t.fq"])) - 1 >= 4   # whole cuts across the two inputs


def test_trim_pair_all_four_outputs(reads, tmp_path):
    trees = with_and_without(tmp_path, ["trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"]] + PAIR_OUTS + WORKFLOW, PAIR_NAMES, "trim")
    assert all(trees[0][n] for n in PAIR_NAMES)


def test_trim_pair_that_drops_every_read_writes_the_marker(reads, tmp_path):
    with_and_without(tmp_path, ["trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"]] + PAIR_OUTS + ["MINLEN:1000"], PAIR_NAMES, "trim", markers=PAIR_NAMES)


def test_trim_pair_from_blocked_gzip(reads, tmp_path):
    trees = with_and_without(tmp_path, ["trim", "--gz", "-1", reads["r1.fq.gz"], "-2", reads["r2.fq.gz"]] + PAIR_OUTS + WORKFLOW, PAIR_NAMES, "trim")
    plain = tmp_path / "plain"
    plain.mkdir()
    cli("trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *PAIR_OUTS, *WORKFLOW, cwd=plain)
    assert tree(plain) == trees[0]


def test_trim_with_a_trimlog(reads, tmp_path):
    trees = with_and_without(tmp_path, ["trim", "-i", reads["r1.fq"], "-o", "t.fq", "--trimlog", "log.txt"] + WORKFLOW, ["t.fq"], "trim")
    assert trees[0]["log.txt"].count(b"\n") == 512
    pair = tmp_path / "pair"
    pair.mkdir()
    with_and_without(pair, ["trim", "--gz", "-1", reads["r1.fq.gz"], "-2", reads["r2.fq"], "--trimlog", "log.txt"] + PAIR_OUTS + WORKFLOW,
                     PAIR_NAMES, "trim")


def test_mask_against_a_database_and_against_its_own_count(reads, tmp_path):
    db = tmp_path / "db"
    db.mkdir()
    cli("count", "-k", 25, "-ci", 1, "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "db", cwd=db)
    d_dir, k_dir = tmp_path / "d", tmp_path / "k"
    d_dir.mkdir(), k_dir.mkdir()
    trees = with_and_without(d_dir, ["mask", "-d", db / "db", "-i", reads["r1.fq"], "-i", reads["r2.fq"], "-o", "m.fq", "-l", 3], ["m.fq"], "mask")
    trees = with_and_without(k_dir, ["mask", "-k", 25, "-ci", 1, "-i", reads["r1.fq"], "-o", "m.fq", "--auto-cutoffs", "--db-out", "own"], ["m.fq"], "mask")
    assert sorted(trees[0]) == ["m.fq", "own.kmc_pre", "own.kmc_suf"]


def test_count_gz_reads_what_trim_gz_out_wrote(reads, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    cli("trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *PAIR_OUTS, *WORKFLOW, cwd=a)
    cli("trim", "-1", reads["r1.fq"], "-2", reads["r2.fq"], *PAIR_OUTS, *WORKFLOW, "--gz-out", cwd=b)
    w = cli("count", "-k", 25, "-ci", 1, "-i", "o1.fq", "-i", "o2.fq", "-i", "u1.fq", "-o", "db", cwd=a)
    g = cli("count", "-k", 25, "-ci", 1, "-i", "o1.fq", "-i", "o2.fq", "-i", "u1.fq", "-o", "db", "--gz", cwd=b)
    ta, tb = tree(a), tree(b)
    assert ta["db.kmc_pre"] == tb["db.kmc_pre"] and ta["db.kmc_suf"] == tb["db.kmc_suf"]
    assert [l for l in g.stderr.splitlines() if l.startswith("count: ")] == [l for l in w.stderr.splitlines() if l.startswith("count: ")]


def test_hostapi_gz_out(reads, tmp_path):
    plain, packed = tmp_path / "t.fq", tmp_path / "t.fq.gz"
    s0 = hostapi.trim_fastq(str(reads["r1.fq"]), str(plain), WORKFLOW)
    s1 = hostapi.trim_fastq(str(reads["r1.fq"]), str(packed), WORKFLOW, gz_out=True)
    assert s0 == s1 and packed.read_bytes() == hostapi.deflate_bgzf(plain.read_bytes())
    s2 = hostapi.trim_fastq(str(reads["r1.fq"]), str(tmp_path / "again.fq"), WORKFLOW)   # the switch is taken back by the call
    assert s2 == s0 and (tmp_path / "again.fq").read_bytes() == plain.read_bytes()
