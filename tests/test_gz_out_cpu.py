"""`--gz-out` on the command line before a device context exists: the flag shows in the usage of `trim` and `mask`, what the two refuse
today is refused in the same words with it and nothing is left behind, and the other sub-commands refuse it as an unknown option."""
import os
import subprocess

import pytest

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
    made = {"in.fq": gz.fastq(50, seed=1), "in2.fq": gz.fastq(50, seed=2), "good.fq.gz": gz.bgzf(gz.fastq(50, seed=1)), "in.fa": b">s\nACGT\n"}
    for name, data in made.items():
        (tmp_path / name).write_bytes(data)
    return tmp_path, sorted(made)


def test_the_flag_shows_in_the_usage_of_trim_and_mask():
    r = run_cli("trim")
    assert r.returncode != 0 and "[--gz-out]" in r.stderr.split("Usage:")[1]
    everything = run_cli().stdout + run_cli().stderr
    for sub, forms in (("trim", 1), ("mask", 2)):   # the overall usage: `trim`'s first form (the second takes "the same options"), both of `mask`'s
        lines = [l for l in everything.splitlines() if l.startswith("Usage: PloidyFrost %s " % sub) and "[--gz-out]" in l]
        assert len(lines) == forms, (sub, lines)
    assert everything.count("[--gz-out]") == 3   # no other sub-command names it


PAIR = ["-1", "in.fq", "-2", "in2.fq", "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d"]
REFUSED = [   # (arguments, words of the refusal)
    (["trim", "-i", "in.fq", "-o", "in.fq"] + STEPS, "is an input path"),                                    # an output that is an input
    (["trim"] + PAIR[:8] + PAIR[10:] + STEPS, "-o2 <out.fq> is missing"),                                    # a missing pair option
    (["trim", "-1", "in.fq", "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d"] + STEPS, "-2 <r2.fq> is missing"),
    (["trim", "-i", "good.fq.gz", "-o", "t.fq"] + STEPS, "the input is gzip-compressed"),                    # gzip input without --gz
    (["trim"] + PAIR[:2] + ["-2", "good.fq.gz"] + PAIR[4:] + STEPS, "the input is gzip-compressed"),
    (["trim"] + PAIR[:10] + ["-u2", "a"] + STEPS, "two outputs have the same path"),
    (["trim", "-i", "in.fa", "-o", "t.fq"] + STEPS, "the input is FASTA"),
    (["trim", "-i", "in.fq", "-o", "t.fq"], "no step is given"),
    (["mask", "-d", "db", "-i", "in.fq", "-o", "in.fq", "-l", "2"], "is an input path"),
    (["mask", "-d", "db", "-i", "good.fq.gz", "-o", "o.fq", "-l", "2"], "the input is gzip-compressed"),
    (["mask", "-k", "7", "-i", "in.fq", "-o", "o.fq", "-l", "2", "-u", "1"], "is above -u"),
    (["mask", "-d", "db", "-i", "in.fq", "-o", "o.fq"], "the lower threshold is missing"),
    (["mask", "-i", "in.fq", "-o", "o.fq", "-l", "2"], "-d <KMCDatabase> is missing"),
]


@pytest.mark.parametrize("args,words", REFUSED, ids=["%s_%d" % (r[0][0], i) for i, r in enumerate(REFUSED)])
def test_what_is_refused_today_is_refused_in_the_same_words_with_the_flag(files, args, words):
    tmp_path, before = files
    r0 = run_cli(*args, cwd=tmp_path)
    for at in (1, len(args)):   # the flag in front and behind
        r1 = run_cli(*(args[:at] + ["--gz-out"] + args[at:]), cwd=tmp_path)
        assert r0.returncode != 0 and r1.returncode != 0 and r1.stdout == r0.stdout == ""
        assert r1.stderr == r0.stderr, (args, r1.stderr, r0.stderr)
        assert "no device context" not in r1.stderr and (words is None or words in r1.stderr), r1.stderr
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file


def test_gz_out_goes_with_gz_and_gz_plain_on_trim(files):
    tmp_path, before = files
    for flag in ("--gz", "--gz-plain"):   # accepted together: the refusal is the input's, in the words of the flag alone
        r0 = run_cli("trim", "-i", "in.fa", "-o", "t.fq", flag, *STEPS, cwd=tmp_path)
        r1 = run_cli("trim", "-i", "in.fa", "-o", "t.fq", flag, "--gz-out", *STEPS, cwd=tmp_path)
        assert r1.returncode != 0 and r1.stderr == r0.stderr and "the input is FASTA" in r1.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_the_other_sub_commands_refuse_the_flag(files):
    tmp_path, before = files
    for args in (["count", "-k", "7", "-i", "in.fq", "-o", "db"], ["build", "-k", "7", "-r", "in.fq", "-o", "g"],
                 ["build-multi", "-k", "7", "-r", "in.fq", "-r", "in2.fq", "-o", "g"], ["run", "-k", "7", "-i", "in.fq", "-o", "r"],
                 ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", "in2.fq", "-o", "m"]):
        r = run_cli(*(args + ["--gz-out"]), cwd=tmp_path)
        assert r.returncode != 0 and "--gz-out" in r.stderr and "nknown" in r.stderr, (args, r.stderr)
        assert "[--gz-out]" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_hostapi_takes_gz_out_and_raises_the_same_refusals(files):
    tmp_path, before = files
    p = lambda name: str(tmp_path / name)   # noqa: E731
    for gz_out in (False, True):
        with pytest.raises(RuntimeError) as e:
            hostapi.trim_fastq(p("good.fq.gz"), p("t.fq"), STEPS, gz_out=gz_out)
        assert "the input is gzip-compressed" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            hostapi.trim_fastq_pair(p("in.fq"), p("in.fa"), [p(x) for x in "abcd"], STEPS, gz_out=gz_out)
        assert "the input is FASTA" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            hostapi.mask_fastq(p("db"), p("in.fq"), p("in.fq"), lower=2, gz_out=gz_out)
        assert "is an input path" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            hostapi.mask_fastq_counted(p("in.fa"), p("o.fq"), k=7, lower=2, gz_out=gz_out)
        assert "the input is FASTA" in str(e.value)
    assert sorted(os.listdir(tmp_path)) == before
    assert "pfh_reads_gz_out" in hostapi.DECLARED_SYMBOLS
