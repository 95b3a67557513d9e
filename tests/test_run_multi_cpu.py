"""`ploidyfrost run-multi` without a device: the host restatement of K-UNION (csrc/pf_runmulti_rule.hpp) against np.unique, the entry
points and kernel ids, and the sub-command's refusals, which come before a device context exists."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import mask_cases as mc

from ploidyfrost_amd import hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
U64 = np.uint64


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_runmulti_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing
    of it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_runmulti_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_runmulti_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_union_host_equals_unique_of_the_concatenation():
    rng = np.random.default_rng(11)
    for n_sets in (1, 2, 3, 5, 8):   # the odd carry and three rounds
        sets = [np.unique(rng.integers(0, 5000, size=int(rng.integers(0, 1500)), dtype=np.uint64)) for _ in range(n_sets)]
        sets[0] = np.unique(np.concatenate([sets[0], [U64(1) << U64(61), U64(42)]]))
        sets[-1] = np.unique(np.concatenate([sets[-1], [U64(42)]]))
        got = hostapi.union_host(sets)
        assert got.dtype == U64 and np.array_equal(got, np.unique(np.concatenate(sets))), n_sets
    empty = np.zeros(0, dtype=U64)
    assert len(hostapi.union_host([empty, empty])) == 0 and len(hostapi.union_host([])) == 0
    assert np.array_equal(hostapi.union_host([empty, np.array([3, 9], dtype=U64)]), np.array([3, 9], dtype=U64))


def test_union_host_refuses_by_name():
    good = np.array([1, 5, 9], dtype=U64)
    for bad, word in ((np.array([4, 3, 8], dtype=U64), "set 1 is not sorted"), (np.array([4, 4, 8], dtype=U64), "set 1 holds a key twice")):
        try:
            hostapi.union_host([good, bad])
        except RuntimeError as e:
            assert word in str(e)
        else:
            raise AssertionError("not refused: %s" % word)


def test_entry_points_are_declared():
    for s in ("pf_kmer_union", "pf_color_kmers", "pf_release_counts"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_run_multi_fastq", "pfh_union_host"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_UNION == hipapi.K_MASKCOUNT + 1 and hipapi.K_COLORSET == hipapi.K_UNION + 1
    L = hipapi.load_library()
    assert L.pf_kernel_name(hipapi.K_UNION) == b"k_union" and L.pf_kernel_name(hipapi.K_COLORSET) == b"k_colorset"
    assert L.pf_kernel_name(hipapi.K_MASKCOUNT) == b"k_maskcount"
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    tail = text.split("PF_K_MASKCOUNT,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    assert tail.index("PF_K_UNION") < tail.index("PF_K_COLORSET")
    with open(os.path.join(ROOT, "ploidyfrost_amd", "csrc", "pf_runmulti_rule.hpp")) as f:
        rule = f.read()
    assert "UNION_TILE = %d" % hipapi.UNION_TILE in rule and "UNION_ITEMS = %d" % hipapi.UNION_ITEMS in rule
    assert hostapi.RUN_MULTI_STATS_FIELDS[0] == "colors" and hostapi.RUN_MULTI_STATS_FIELDS[-1] == "color_bytes"


def test_cli_refusals(tmp_path):
    for n, seq in (("a.fq", b"ACGT"), ("b.fq", b"ACGA")):
        (tmp_path / n).write_bytes(mc.fastq([seq * 10]))
    os.symlink(tmp_path / "a.fq", tmp_path / "link.fq")
    (tmp_path / "x.fa").write_bytes(b">s\nACGT\n")
    (tmp_path / "x.fq.gz").write_bytes(b"\x1f\x8b\x08\x00rest")
    (tmp_path / "same.gfa").write_bytes(mc.fastq([b"ACGT" * 10]))
    a, b = ["--sample", "A", "-i", "a.fq"], ["--sample", "B", "-i", "b.fq"]
    ok = a + b + ["-o", "r"]
    many = [x for c in range(1025) for x in ("--sample", "s%d" % c, "-i", "a.fq")]
    cases = [
        (["-i", "a.fq"] + ok, "-i a.fq stands before any --sample NAME"),
        (a + ["--sample", "B", "-o", "r"], "sample B has no input"),
        (a + ["--sample", "A", "-i", "b.fq", "-o", "r"], "sample A is given twice"),
        (a + ["--sample", "B", "-i", "a.fq", "-o", "r"], "a.fq: the same file is given in two samples (A and B)"),
        (a + ["--sample", "B", "-i", "link.fq", "-o", "r"], "link.fq: the same file is given in two samples"),
        (many + ["-o", "r"], "more than 1024 samples (--sample): 1025"),
        (["-o", "r"], "no sample"),
        (a + b, "-o <out> is missing"),
        (ok + ["-f", "x.bfg_colors"], "-f does not go with run-multi"),
        (ok + ["-C", "cut.txt"], "-C does not go with run-multi"),
        (ok + ["-d", "db"], "-d does not go with run-multi"),
        (ok + ["-h", "hist.txt"], "-h does not go with run-multi"),
        (ok + ["-l", "5"], "-l does not go with run-multi"),
        (ok + ["-b"], "-b does not go with run-multi"),
        (ok + ["--gpus", "2"], "--gpus is not built into run-multi"),
        (ok + ["--filtered-out", "f.fq"], "--filtered-out is not built"),
        (ok + ["-k", "4"], "a KMC1 database needs -k of at least 5"),
        (ok + ["-k", "32"], "-k goes from 3 to 31"),
        (ok + ["-k", "25", "-g", "24"], "run-multi: -g goes from 1 to k - 2 = 23"),
        (ok + ["-ci", "9", "-cx", "8"], "-ci is above -cx"),
        (ok + ["--model", "fre"], "put --filter-multi \"OPTS\" in front of it"),
        (ok + ["--filter", "-n 6", "--model", "fre"], "--filter reads the single-sample result streams: run-multi has --filter-multi"),
        (ok + ["--model-each-color"], "--model-each-color needs --filter-multi"),
        (ok + ["--frobnicate"], "unknown option --frobnicate"),
        (a + ["--sample", "B", "-i", "x.fa", "-o", "r"], "x.fa: record 1: the input is FASTA"),
        (a + ["--sample", "B", "-i", "x.fq.gz", "-o", "r"], "x.fq.gz: record 1: the input is gzip-compressed"),
        (a + ["--sample", "B", "-i", "same.gfa", "-o", "r", "--gfa-out", "same"], "same.gfa: the output path is an input path"),
    ]
    before = sorted(os.listdir(tmp_path))
    for args, word in cases:
        r = run_cli("run-multi", *args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args[-6:], r.stdout, r.stderr[:400])
        assert sorted(os.listdir(tmp_path)) == before, args[-6:]   # no output, no temporary file, no output directory
    assert "PloidyFrost run-multi" in run_cli().stdout
    try:
        hostapi.run_multi_reads([("A", str(tmp_path / "a.fq")), ("A", str(tmp_path / "b.fq"))], "out")
    except RuntimeError as e:
        assert "sample A is given twice" in str(e)
    else:
        raise AssertionError("not refused")
