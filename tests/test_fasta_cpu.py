"""`--fasta` without a GPU: the host rule of K-FASTA (hostapi.fasta_index, csrc/pf_fasta_rule.hpp) against the Python restatement of
fasta_cases.py on the edge texts, whole and cut; the stand-alone program tests/cpp/test_fasta_rule.cpp under the sanitizers; what the
command line refuses about the flag before a device context exists, with nothing left under any output name; that a FASTA input
without the flag is refused in the words of old by every sub-command; and the declarations."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import fasta_cases as fc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
STEPS = ["LEADING:10", "MINLEN:20"]
TEXTS = fc.edge_texts()


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None, env=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120, env=env)


def same_index(got, want):
    assert got["text"] == want["text"]
    assert np.array_equal(got["read_off"], want["read_off"]) and np.array_equal(got["read_len"], want["read_len"])
    assert (got["bytes_used"], got["records"], got["bases"]) == (want["bytes_used"], want["records"], want["bases"])


# ---- the host rule against the restatement ----

@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_host_rule_against_the_restatement(name, text):
    same_index(hostapi.fasta_index(text, final=True), fc.ref_index(text, True))
    same_index(hostapi.fasta_index(text, final=False), fc.ref_index(text, False))
    for c in fc.cuts_of(text):
        same_index(hostapi.fasta_index(text[:c], final=False), fc.ref_index(text[:c], False))


def test_the_restatement_by_hand():
    r = fc.ref_index(b">a\r\nAC\r\nGT\r\n>b\n\n>c\nTT")
    assert (r["text"], list(r["read_off"]), list(r["read_len"]), r["bytes_used"]) == (b"ACGTTT", [0, 4, 4], [4, 0, 2], 21)
    r = fc.ref_index(b">a\nAC\n>b\nGG\nT", final=False)
    assert (r["text"], list(r["read_len"]), r["bytes_used"]) == (b"AC", [2], 6)
    assert fc.ref_index(b">abc", final=False)["bytes_used"] == 0 and fc.ref_index(b">abc", final=False)["records"] == 0
    assert fc.ref_index(b">a\nAC\rGT\r\r\nTT\r")["text"] == b"AC\rGT\rTT\r"
    assert fc.q_of(b">a x\nACGTA\nCGTAC\n>b\n>c\r\nTT\r\n") == b"@a x\nACGTACGTAC\n+\nIIIIIIIIII\n@b\n\n+\n\n@c\nTT\n+\nII\n"


def test_q_of_f_has_the_records_of_f():
    """the FASTQ index of Q(F) gives the sequences the FASTA rule gives for F"""
    for name, text in TEXTS:
        if b"\r" in text.replace(b"\r\n", b"\n"):
            continue                                   # (a lone '\r' inside a sequence: Q(F)'s sequence line would end in it)
        want = fc.ref_index(text)
        q = fc.q_of(text)
        ix = hostapi.mask_index_fastq(q, final=True)
        assert (ix["clause"], ix["bytes_used"], ix["n_records"]) == ("none", len(q), want["records"]), name
        assert [q[int(o):int(o) + int(n)] for o, n in zip(ix["read_off"], ix["read_len"])] == [want["text"][int(o):int(o) + int(n)] for o, n in zip(want["read_off"], want["read_len"])]


def test_text_in_front_of_the_first_header_is_refused():
    with pytest.raises(ValueError, match="does not start with '>'"):
        hostapi.fasta_index(b"ACGT\n>a\nAC\n")


# ---- the stand-alone program ----

def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_fasta_rule.cpp: the rule header alone, plain g++ with -fsanitize=address,undefined, exact-size heap buffers (host
    code only: nothing of it is loaded into Python or run on a GPU).  The edge texts are handed to it in a file."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "test_fasta_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_fasta_rule.cpp"), "-o", exe], check=True)
    path = tmp_path / "texts.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(t)) + t for _, t in TEXTS))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- the command line ----

@pytest.fixture()
def files(tmp_path):
    (tmp_path / "in.fa").write_bytes(b">s\nACGTACGTAC\nGGTTA\n")
    (tmp_path / "in.fq").write_bytes(b"@s\nACGTACGTACGGTTA\n+\nIIIIIIIIIIIIIII\n")
    return tmp_path


def nothing_left(d):
    assert sorted(os.listdir(d)) == ["in.fa", "in.fq"]


OLD_WORDS = "%s: in.fa: record 1: the input is FASTA (first byte '>'): only FASTQ is %s"


@pytest.mark.parametrize("who,what,args", [
    ("count", "counted", ["count", "-k", "7", "-i", "in.fa", "-o", "db"]),
    ("build", "read", ["build", "-k", "7", "-r", "in.fa", "-o", "g"]),
    ("build-multi", "read", ["build-multi", "-k", "7", "-r", "in.fq", "-r", "in.fa", "-o", "g"]),
    ("run", "read", ["run", "-k", "7", "-i", "in.fa", "-o", "r", "--db-out", "rdb", "--gfa-out", "rg"]),
    ("run-multi", "read", ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", "in.fa", "-o", "m"]),
    ("mask", "masked", ["mask", "-k", "7", "-i", "in.fa", "-o", "m.fq", "-l", "2"]),
    ("trim", "trimmed", ["trim", "-i", "in.fa", "-o", "t.fq"] + STEPS),
], ids=["count", "build", "build-multi", "run", "run-multi", "mask", "trim"])
def test_without_the_flag_fasta_is_refused_in_the_words_of_old(files, who, what, args):
    r = run_cli(*args, cwd=files)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "Error: " + OLD_WORDS % (who, what) + "\n"
    nothing_left(files)


@pytest.mark.parametrize("args,why", [
    (["mask", "-k", "7", "-i", "in.fa", "-o", "m.fq", "-l", "2", "--fasta"], "Error: mask: --fasta is not built into mask"),
    (["trim", "-i", "in.fa", "-o", "t.fq", "--fasta"] + STEPS, "Error: trim: --fasta does not go with trim: FASTA has no qualities to trim"),
    (["run", "-k", "7", "-i", "in.fa", "-o", "r", "--fasta"] + STEPS, "Error: run: --fasta does not go with trim steps or -1 / -2 (FASTA has no qualities to trim)"),
    (["run", "-k", "7", "-1", "in.fa", "-2", "in.fq", "-o", "r", "--fasta"] + STEPS, "Error: run: --fasta does not go with trim steps or -1 / -2"),
    (["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", "in.fa", "-o", "m", "--fasta"] + STEPS,
     "Error: run-multi: --fasta does not go with trim steps or -1 / -2"),
    (["run-multi", "-k", "7", "--sample", "A", "-1", "in.fq", "-2", "in.fa", "-o", "m", "--fasta"] + STEPS, "Error: run-multi: --fasta does not go with trim steps or -1 / -2"),
], ids=["mask", "trim", "run_steps", "run_pair", "run_multi_steps", "run_multi_pair"])
def test_where_the_flag_is_refused_by_name(files, args, why):
    r = run_cli(*args, cwd=files)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith(why), r.stderr
    nothing_left(files)


@pytest.mark.parametrize("args", [
    ["count", "-k", "7", "-i", "in.fa", "-o", "db", "--fasta", "-cx", "0"],
    ["count", "-k", "7", "-i", "in.fa", "-o", "in.fa", "--fasta", "--hist", "in.fa"],
    ["build", "-k", "99", "-r", "in.fa", "-o", "g", "--fasta"],
    ["build-multi", "-k", "7", "-r", "in.fa", "-r", "in.fa", "-o", "g", "--fasta"],
    ["run", "-k", "7", "-i", "missing.fa", "-o", "r", "--fasta"],
    ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fa", "--sample", "A", "-i", "in.fq", "-o", "m", "--fasta"],
], ids=["count_cut", "count_same_path", "build_k", "build_multi_twice", "run_missing", "run_multi_name_twice"])
def test_what_a_sub_command_refuses_today_it_refuses_with_the_flag(files, args):
    with_flag = run_cli(*args, cwd=files)
    without = run_cli(*[a for a in args if a != "--fasta"], cwd=files)
    assert with_flag.returncode == 1 and without.returncode == 1
    first = lambda r: r.stderr.splitlines()[0]
    assert first(with_flag) == first(without) or "FASTA" in first(without)      # (without the flag the FASTA refusal may come first)
    assert "FASTA" not in first(with_flag)
    nothing_left(files)


@pytest.mark.parametrize("args", [
    ["count", "-k", "7", "-i", "in.fa", "-i", "in.fq", "-o", "db", "--fasta"],
    ["build", "-k", "7", "-r", "in.fa", "-o", "g", "--fasta"],
    ["build-multi", "-k", "7", "-r", "in.fq", "-r", "in.fa", "-o", "g", "--fasta"],
    ["run", "-k", "7", "-i", "in.fa", "-o", "r", "--fasta"],
    ["run-multi", "-k", "7", "--sample", "A", "-i", "in.fq", "--sample", "B", "-i", "in.fa", "-o", "m", "--fasta"],
], ids=["count", "build", "build-multi", "run", "run-multi"])
def test_with_the_flag_fasta_passes_the_preflight(files, args):
    """the flag is known and the FASTA input is not refused: with no device to be seen the command gets as far as asking for one
    (what it writes with one: test_gpu_fasta.py)"""
    r = run_cli(*args, cwd=files, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert "FASTA" not in r.stderr and "unknown option" not in r.stderr and "Usage" not in r.stderr, r.stderr
    assert "record " not in r.stderr, r.stderr      # no format refusal either
    if "no device context" in r.stderr:
        assert r.returncode == 1
        nothing_left(files)


def test_hostapi_refuses_as_the_commands_do(files):
    cwd = os.getcwd()
    os.chdir(files)
    try:
        with pytest.raises(RuntimeError, match=r"count: in.fa: record 1: the input is FASTA \(first byte '>'\): only FASTQ is counted"):
            hostapi.count_fastq("in.fa", "db", k=7)
        with pytest.raises(RuntimeError, match="run: --fasta does not go with trim steps"):
            hostapi.run_reads("in.fa", "r", k=7, steps=STEPS, fasta=True)
        with pytest.raises(RuntimeError, match="run-multi: --fasta does not go with trim steps"):
            hostapi.run_multi_reads([("A", "in.fq"), ("B", "in.fa")], "m", k=7, steps=STEPS, fasta=True)
        with pytest.raises(RuntimeError, match="the input is FASTA"):      # the switch is taken back by the call that used it
            hostapi.build_graph("in.fa", "g", k=7)
    finally:
        os.chdir(cwd)
    nothing_left(files)


# ---- names ----

def test_entry_points_are_declared():
    L = hipapi.load_library()
    for s in ("pf_fasta_index", "pf_fasta_index_fetch", "pf_count_fasta", "pf_maskcount_fasta", "pf_color_fasta"):
        assert s in hipapi.DECLARED_SYMBOLS and getattr(L, s)
    H = hostapi.load_library()
    for s in ("pfh_reads_fasta", "pfh_fasta_index", "pfh_fasta_clause_text"):
        assert s in hostapi.DECLARED_SYMBOLS and getattr(H, s)
    assert hipapi.K_FASTA == hipapi.K_GUNZIP + 1 and hipapi.FASTA_TILE == fc.TILE
    header = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    assert "#define PF_FASTA_TILE %d " % fc.TILE in header and "PF_K_FASTA," in header
