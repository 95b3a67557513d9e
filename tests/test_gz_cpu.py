"""`--gz` without a GPU: what `count`, `trim`, `run` and `run-multi` refuse about a gzip input before a device context exists -- gzip
that is not blocked (by name, with the two ways out), another compression method, other flags, a first member that runs past the
file's end -- with nothing left under any output name; that everything refused without `--gz` is still refused with it, in the same
words; that nothing changes without `--gz`; and the same through hostapi's gz= argument."""
import os
import struct
import subprocess
import zlib

import pytest
import torch

from conftest import ROOT

import gz_cases as gz

from ploidyfrost_amd import build, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
STEPS = ["LEADING:10", "MINLEN:20"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


@pytest.fixture()
def files(tmp_path):
    text = gz.fastq(50, seed=1)
    good = gz.bgzf(text)
    c = gz.container_clause_members()
    made = {"in.fq": text, "in2.fq": gz.fastq(50, seed=2), "good.fq.gz": good, "plain.fq.gz": c["flags"][0], "nobc.fq.gz": c["not_blocked"][0],
            "method.fq.gz": c["method"][0], "flags.fq.gz": c["flags_name"][0], "cut.fq.gz": good[:40], "cut12.fq.gz": good[:11],
            "short.fq.gz": c["short"][0], "in.fa": b">s\nACGT\n"}
    for name, data in made.items():
        (tmp_path / name).write_bytes(data)
    return tmp_path, sorted(made)


def commands(path, second=None):
    """the four sub-commands on `path` (and, where a pair is taken, `second` beside it), all with --gz"""
    out = [["count", "-k", "7", "-i", path, "-o", "db", "--gz"],
           ["trim", "-i", path, "-o", "t.fq", "--gz"] + STEPS,
           ["run", "-k", "7", "-i", path, "-o", "r", "--db-out", "rdb", "--gfa-out", "rg", "--gz"],
           ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", path, "-o", "m", "--gz"]]
    if second:
        out += [["trim", "-1", second, "-2", path, "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d", "--gz"] + STEPS,
                ["run", "-k", "7", "-1", second, "-2", path, "-o", "r", "--gz"] + STEPS]
    return out


REFUSALS = [("plain.fq.gz", "flags"), ("nobc.fq.gz", "not_blocked"), ("method.fq.gz", "method"), ("flags.fq.gz", "flags"), ("cut.fq.gz", "past_end"),
            ("cut12.fq.gz", "past_end"), ("short.fq.gz", "short")]


@pytest.mark.parametrize("name,clause", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_name_before_a_device_context(files, name, clause):
    tmp_path, before = files
    text = hostapi.inflate_clause_text(gz.CLAUSE[clause])
    for args in commands(name, "in.fq"):
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and r.stdout == "", (args, r.stdout)
        assert "%s: %s: member 1, byte 0: %s" % (args[0], name, text) in r.stderr, (args, r.stderr)
        assert "no device context" not in r.stderr
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    if clause in ("flags", "not_blocked"):
        assert "bgzip" in text and "decompress" in text


def test_what_is_refused_today_is_refused_with_gz_in_the_same_words(files):
    tmp_path, before = files
    for with_gz, without in zip(commands("in.fa", "in.fq"), commands("in.fa", "in.fq")):
        without = [a for a in without if a != "--gz"]
        r1, r0 = run_cli(*with_gz, cwd=tmp_path), run_cli(*without, cwd=tmp_path)
        assert r1.returncode != 0 and r0.returncode != 0 and r1.stderr == r0.stderr and "the input is FASTA" in r1.stderr, (with_gz, r1.stderr, r0.stderr)
    for args in commands("none.fq.gz"):
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and "cannot read none.fq.gz" in r.stderr, args
    r = run_cli("count", "-k", "7", "-i", "good.fq.gz", "-o", "good.fq", "--hist", "good.fq.gz", "--gz", cwd=tmp_path)
    assert r.returncode != 0 and "the output path is an input path" in r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_nothing_changes_without_gz(files):
    tmp_path, before = files
    for args in commands("good.fq.gz"):
        args = [a for a in args if a != "--gz"]
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and "good.fq.gz: record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is" in r.stderr, (args, r.stderr)
    for sub in (["mask", "-d", "db", "-i", "good.fq.gz", "-o", "o.fq", "-l", "2"], ["build", "-k", "7", "-r", "good.fq.gz", "-o", "g"],
                ["build-multi", "-k", "7", "-r", "in.fq", "-r", "good.fq.gz", "-o", "g"]):
        r = run_cli(*(sub + ["--gz"]), cwd=tmp_path)   # their inputs are this tool's own plain outputs
        assert r.returncode != 0 and "--gz" in r.stderr, (sub, r.stderr)
        r = run_cli(*sub, cwd=tmp_path)
        assert r.returncode != 0 and "the input is gzip-compressed" in r.stderr, (sub, r.stderr)
    assert sorted(os.listdir(tmp_path)) == before
    usage = run_cli().stdout + run_cli().stderr
    assert usage.count("[--gz]") >= 4


def test_blocked_gzip_passes_the_preflight(files):
    """a sound blocked-gzip file is refused only for the device it needs"""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_gz_stream.py runs these commands")
    tmp_path, before = files
    for args in commands("good.fq.gz", "in.fq"):
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and "no device context" in r.stderr and "member" not in r.stderr, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args


def test_hostapi_gz_argument_raises_the_same_refusals(files):
    tmp_path, before = files
    p = lambda name: str(tmp_path / name)   # noqa: E731
    text = hostapi.inflate_clause_text(gz.CLAUSE["not_blocked"])
    calls = [
        ("count", lambda f, **k: hostapi.count_fastq([f], p("db"), k=7, **k)),
        ("trim", lambda f, **k: hostapi.trim_fastq([f], p("t.fq"), STEPS, **k)),
        ("trim", lambda f, **k: hostapi.trim_fastq_pair(p("in.fq"), f, [p(x) for x in "abcd"], STEPS, **k)),
        ("run", lambda f, **k: hostapi.run_reads([f], p("r"), k=7, **k)),
        ("run", lambda f, **k: hostapi.run_reads(None, p("r"), k=7, steps=STEPS, pairs=[(p("in.fq"), f)], **k)),
        ("run-multi", lambda f, **k: hostapi.run_multi_reads([("A", [p("in.fq")]), ("B", [f])], p("m"), k=7, **k)),
    ]
    for who, call in calls:
        with pytest.raises(ValueError) as e:
            call(p("nobc.fq.gz"), gz=True)
        assert str(e.value) == "%s: %s: member 1, byte 0: %s" % (who, p("nobc.fq.gz"), text), who
        with pytest.raises(ValueError) as e:
            call(p("cut.fq.gz"), gz=True)
        assert "member 1, byte 0: the member runs past the end of the file" in str(e.value)
        with pytest.raises(RuntimeError) as e:   # without gz= (and after a call with it) the refusal of old
            call(p("good.fq.gz"))
        assert "the input is gzip-compressed (magic 1f 8b)" in str(e.value), who
        with pytest.raises(ValueError) as e:
            call(p("in.fa"), gz=True)
        assert "the input is FASTA" in str(e.value)
    assert sorted(os.listdir(tmp_path)) == before
