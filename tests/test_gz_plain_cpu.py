"""`--gz-plain` without a GPU: what `count`, `trim`, `run` and `run-multi` refuse about a gzip input before a device context exists --
another compression method, a reserved flag bit, a header that runs past the end of the file, and blocked gzip's own refusals -- with
nothing left under any output name; that plain gzip passes the preflight with `--gz-plain` and is still refused with `--gz` alone and
without either, in today's words; that `mask`, `build` and `build-multi` refuse the flag as they refuse `--gz`; and the same through
hostapi's gz="plain"."""
import os
import subprocess

import pytest
import torch

from conftest import ROOT

import gz_cases as gz
import gzp_cases as gp

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
    good = gp.member(text, head=gp.header(name=b"in.fq"))
    blocked = gz.bgzf(text)
    made = {"in.fq": text, "good.fq.gz": good, "two.fq.gz": good + gp.member(gz.fastq(5, seed=2)), "blocked.fq.gz": blocked,
            "method.fq.gz": good[:2] + b"\x07" + good[3:], "reserved.fq.gz": good[:3] + b"\x28" + good[4:], "cut.fq.gz": good[:13],
            "cut_extra.fq.gz": gp.header(extra=b"0123456789")[:15], "blocked_cut.fq.gz": blocked[:40], "in.fa": b">s\nACGT\n"}
    for name, data in made.items():
        (tmp_path / name).write_bytes(data)
    return tmp_path, sorted(made)


def commands(path, second=None, flag="--gz-plain"):
    """the four sub-commands on `path` (and, where a pair is taken, `second` beside it)"""
    flag = [flag] if flag else []
    out = [["count", "-k", "7", "-i", path, "-o", "db"] + flag,
           ["trim", "-i", path, "-o", "t.fq"] + flag + STEPS,
           ["run", "-k", "7", "-i", path, "-o", "r", "--db-out", "rdb", "--gfa-out", "rg"] + flag,
           ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", path, "-o", "m"] + flag]
    if second:
        out += [["trim", "-1", second, "-2", path, "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d"] + flag + STEPS,
                ["run", "-k", "7", "-1", second, "-2", path, "-o", "r"] + flag + STEPS]
    return out


REFUSALS = [("method.fq.gz", "method"), ("reserved.fq.gz", "reserved_flag"), ("cut.fq.gz", "header_past"), ("cut_extra.fq.gz", "past_end"),   # (FLG = 04: judged as blocked gzip is, in its words)
            ("blocked_cut.fq.gz", "past_end")]


@pytest.mark.parametrize("name,clause", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_name_before_a_device_context(files, name, clause):
    tmp_path, before = files
    text = hostapi.gunzip_clause_text(gp.CLAUSE[clause])
    for args in commands(name, "in.fq"):
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and r.stdout == "", (args, r.stdout)
        assert "%s: %s: member 1, byte 0: %s" % (args[0], name, text) in r.stderr, (args, r.stderr)
        assert "no device context" not in r.stderr
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file


def test_plain_gzip_passes_the_preflight_with_the_flag_only(files):
    tmp_path, before = files
    flags = hostapi.inflate_clause_text(gz.CLAUSE["flags"])
    for name in ("good.fq.gz", "two.fq.gz"):
        for args in commands(name, "in.fq", "--gz"):      # --gz alone: today's refusal, by name
            r = run_cli(*args, cwd=tmp_path)
            assert r.returncode != 0 and "%s: %s: member 1, byte 0: %s" % (args[0], name, flags) in r.stderr and "bgzip" in r.stderr, (args, r.stderr)
        for args in commands(name, "in.fq", None):        # neither flag: gzip is refused as ever
            r = run_cli(*args, cwd=tmp_path)
            assert r.returncode != 0 and name + ": record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is" in r.stderr, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before
    for name in ("good.fq.gz", "two.fq.gz", "blocked.fq.gz"):
        for args in commands(name, "in.fq") + commands(name, "in.fq", "--gz")[:1 if name == "blocked.fq.gz" else 0]:
            r = run_cli(*args, cwd=tmp_path)
            assert "member" not in r.stderr and "gzip" not in r.stderr, (args, r.stderr)
            if not torch.cuda.is_available():   # (with a GPU the command goes on: tests/test_gpu_gz_plain_stream.py compares what it writes)
                assert r.returncode != 0 and "no device context" in r.stderr, (args, r.stderr)
                assert sorted(os.listdir(tmp_path)) == before, args
    r = run_cli("count", "-k", "7", "-i", "good.fq.gz", "-o", "db", "--gz", "--gz-plain", cwd=tmp_path)   # --gz-plain implies --gz, in either order
    assert "member" not in r.stderr
    r = run_cli("count", "-k", "7", "-i", "good.fq.gz", "-o", "db", "--gz-plain", "--gz", cwd=tmp_path)
    assert "member" not in r.stderr


def test_what_is_refused_today_is_refused_in_the_same_words(files):
    tmp_path, before = files
    for with_flag, without in zip(commands("in.fa", "in.fq"), commands("in.fa", "in.fq", None)):
        r1, r0 = run_cli(*with_flag, cwd=tmp_path), run_cli(*without, cwd=tmp_path)
        assert r1.returncode != 0 and r0.returncode != 0 and r1.stderr == r0.stderr and "the input is FASTA" in r1.stderr, (with_flag, r1.stderr, r0.stderr)
    for sub in (["mask", "-d", "db", "-i", "good.fq.gz", "-o", "o.fq", "-l", "2"], ["build", "-k", "7", "-r", "good.fq.gz", "-o", "g"],
                ["build-multi", "-k", "7", "-r", "in.fq", "-r", "good.fq.gz", "-o", "g"]):
        r1, r0 = run_cli(*(sub + ["--gz-plain"]), cwd=tmp_path), run_cli(*(sub + ["--gz"]), cwd=tmp_path)
        assert r1.returncode != 0 and r1.stderr == r0.stderr.replace("--gz", "--gz-plain") and "--gz-plain" in r1.stderr, (sub, r1.stderr, r0.stderr)
    assert sorted(os.listdir(tmp_path)) == before
    usage = run_cli().stdout + run_cli().stderr
    assert usage.count("[--gz-plain]") >= 4 and usage.count("[--gz]") >= 4 and "implies --gz" in usage


def test_hostapi_gz_plain_raises_the_same_refusals(files):
    tmp_path, before = files
    p = lambda name: str(tmp_path / name)   # noqa: E731
    text = hostapi.gunzip_clause_text(gp.CLAUSE["reserved_flag"])
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
            call(p("reserved.fq.gz"), gz="plain")
        assert str(e.value) == "%s: %s: member 1, byte 0: %s" % (who, p("reserved.fq.gz"), text), who
        with pytest.raises(ValueError) as e:   # gz=True keeps its meaning
            call(p("good.fq.gz"), gz=True)
        assert "member 1, byte 0: the gzip flags are not FEXTRA alone" in str(e.value), who
        with pytest.raises(RuntimeError) as e:   # without gz= (and after a call with it) the refusal of old
            call(p("good.fq.gz"))
        assert "the input is gzip-compressed (magic 1f 8b)" in str(e.value), who
    assert sorted(os.listdir(tmp_path)) == before
