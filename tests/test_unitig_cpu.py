"""The rule of `ploidyfrost build` (K-UNITIG) without a GPU: the Python restatement of unitig_cases.py on the example worked by hand,
the host's plain restatement (pfh_unitig_build_host, csrc/pf_unitig_rule.hpp) byte for byte against it on every case and flag
combination, the Python rule against what the reference's Bifrost wrote for the fixtures tests/golden/build_* (under the comparator),
the sub-command's refusals that need no device by their wording, the stand-alone program tests/cpp/test_unitig_rule.cpp under the
sanitizers, and the declarations.

The three tests under "the Python restatement itself" touch unitig_cases.py alone: they pin the reference the other tests are held to
(the rule by hand, the format, what each case is for) and would pass without the feature; they are no coverage of it."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import unitig_cases as uc

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
CASES = uc.cases()
FLAG_FILES = {"none": (False, False), "i": (True, False), "d": (False, True), "id": (True, True)}


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def fixture_reads(name):
    with open(os.path.join(GOLDEN, name, "reads.fq")) as f:
        return [ln.strip() for i, ln in enumerate(f) if i % 4 == 1]


# ---- the Python restatement itself ----

def test_python_rule_by_hand():
    S = uc.kmer_set(uc.HAND_READS, uc.HAND_K)
    assert sorted(S) == ["AAGAC", "ACTCC", "ACTCG", "AGACT", "ATGGA", "CATGG", "CGTAA", "CTCCA", "GACTC", "GCGTA"]
    assert uc.succ(S, "GACTC") == ["ACTCC", "ACTCG"] and uc.link(S, "GACTC") is None and uc.link(S, "AGACT") == "GACTC"
    assert uc.succ(S, "CCATG") == ["CATGG"] and uc.link(S, "CCATG") is None          # its own reverse complement
    for flags, (body, stats) in uc.HAND.items():
        text, st = uc.build(S, uc.HAND_K, *flags)
        assert text == uc.header(uc.HAND_K).encode() + body, flags
        assert {f: st[f] for f in stats} == stats and st["bytes"] == len(text), flags


def test_python_format():
    assert [uc.default_g(k) for k in (31, 25, 15, 14, 7, 6, 3)] == [23, 17, 7, 10, 3, 4, 1]
    assert uc.header(25) == "H\tVN:Z:1.0\tBV:Z:1.0.6\tKL:Z:25\tML:Z:17\n" and uc.header(25, 5).endswith("ML:Z:5\n")
    text, st = uc.build_reads(["acgtn" * 3], 25)
    assert text == uc.header(25).encode() and st["unitigs_out"] == 0 and st["bytes"] == len(text)
    # a closed cycle is written from its smallest canonical k-mer as stored, whatever read it came from
    a, _ = uc.build_reads(["AACCGTGAACC"], 5)
    b, _ = uc.build_reads([uc.revcomp("CCGTGAACCGT")], 5)
    assert a == b == uc.header(5).encode() + b"S\t1\tAACCGTGAACC\n"
    # the comparator: a cycle cut elsewhere and read the other way is the same graph, another sequence is not
    assert uc.same_graph(a, uc.header(5).encode() + b"S\t7\t" + uc.revcomp("CGTGAACCGTG").encode() + b"\nL\t1\t+\t1\t+\t4M\n")
    assert not uc.same_graph(a, uc.header(5).encode() + b"S\t1\tAACCGTGAAC\n")
    assert not uc.same_graph(a, uc.header(7).encode() + b"S\t1\tAACCGTGAACC\n")


def test_cases_cover_what_they_are_for():
    by_name = {name: (k, reads) for name, k, reads in CASES}
    for name, (k, reads) in by_name.items():
        _, want = uc.expected(name, k, reads)
        plain = want[(False, False)][1]
        if name.startswith("chain"):
            assert plain["unitigs_out"] == 1 and plain["longest"] == int(name[5:]) + k - 1, name
        if name.startswith("isolated_x"):
            assert plain["unitigs_out"] == int(name[10:]) and want[(False, True)][1]["unitigs_out"] == 0, name
        if name.startswith("cycle") and name != "cycle_tip":
            assert plain["unitigs_out"] == 1 and plain["longest"] == int(name[5:]) + k - 1 and want[(True, True)][1]["removed"] == 0, name
    st = [uc.expected(n, *by_name[n])[1][(True, False)][1] for n in ("tip_km2", "tip_km1", "tip_k", "tip_kp1")]
    assert [s["removed"] for s in st] == [1, 1, 0, 0] and [s["unitigs_out"] for s in st] == [1, 1, 3, 3]
    two = uc.expected("two_tips", *by_name["two_tips"])[1]
    assert two[(True, False)][1]["removed"] == 2 and two[(True, False)][1]["unitigs_out"] == 1 and two[(False, True)][1]["removed"] == 0
    cyc = uc.expected("cycle_tip", *by_name["cycle_tip"])[1]
    assert cyc[(False, False)][1]["unitigs_out"] == 2 and cyc[(True, True)][1]["unitigs_out"] == 1 and cyc[(True, True)][1]["longest"] == 120 + 10
    iso = [uc.expected(n, *by_name[n])[1][(False, True)][1]["removed"] for n in ("isolated_km1", "isolated_k")]
    assert iso == [1, 0]
    for n in ("short_reads", "empty"):
        assert uc.expected(n, *by_name[n])[1][(True, True)][0] == uc.header(25).encode()
    for n in ("palindrome_k8", "palindrome_k24", "acgt20_k8", "at30_k8"):
        k = by_name[n][0]
        assert any(x == uc.revcomp(x) for x in uc.expected(n, *by_name[n])[0]), n


# ---- pfh_unitig_build_host against it ----

@pytest.mark.parametrize("name,k,reads", CASES, ids=[c[0] for c in CASES])
def test_host_rule_on_every_case(name, k, reads):
    S, want = uc.expected(name, k, reads)
    kmers = np.array(sorted(uc.encode(x) for x in S), dtype=np.uint64)
    for flags in uc.FLAGS:
        text, st = hostapi.unitig_build_host(kmers[::-1], k, *flags)   # (any order)
        assert text == want[flags][0], flags
        assert st == want[flags][1], flags


def test_host_rule_on_a_small_graph_made_for_a_size():
    """the make of the GPU suite's graph of more than one grid pass, small: the host's restatement on all of it, and
    unitig_cases.grid_expected (the rule on the k-mers that have a neighbour, the others merged in as lines of one k-mer) over the
    Python rule, are both the Python rule on all of it, byte for byte"""
    km, parts = uc.grid_case(3000)
    assert len(km) >= 3000 and all(len(p) for p in parts.values())
    lone = ~uc.has_neighbour(km, 25)
    assert 0 < lone.sum() < len(km) and not np.isin(km[lone], np.concatenate([p for n, p in parts.items() if n != "single"])).any()

    def python_rule(keys, k, clip, dele):
        return uc.build({"".join(uc.BASES[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k)) for v in keys}, k, clip, dele)

    for flags in uc.FLAGS:
        want = python_rule(km, 25, *flags)
        assert hostapi.unitig_build_host(km, 25, *flags) == want, flags
        assert uc.grid_expected(km, 25, *flags, python_rule) == want, flags
        assert uc.grid_expected(km, 25, *flags, hostapi.unitig_build_host) == want, flags
    st = python_rule(km, 25, True, False)[1]
    assert st["removed"] == len(parts["tip"]) // 5 + 1 and st["longest"] == 3000 + 24   # every tip, and the one on the cycle


def test_host_rule_g_and_refusals():
    kmers = np.array([uc.encode(x) for x in uc.kmer_set(uc.HAND_READS, 5)], dtype=np.uint64)
    assert hostapi.unitig_build_host(kmers, 5, g=2)[0].startswith(uc.header(5, 2).encode())
    assert hostapi.unitig_build_host(kmers, 5)[0].startswith(uc.header(5).encode())   # None: Bifrost's default
    for g in (0, -1):                                                                     # never "the default"
        with pytest.raises(ValueError, match="g goes from 1 to k - 2"):
            hostapi.unitig_build_host(kmers, 5, g=g)
    for k, g in ((2, None), (32, None)):
        with pytest.raises(ValueError, match="k goes from 3 to 31"):
            hostapi.unitig_build_host(kmers, k, g=g)
    with pytest.raises(ValueError, match="g goes from 1 to k - 2"):
        hostapi.unitig_build_host(kmers, 5, g=4)
    assert hostapi.unitig_no_room_text(1000, 10, 7) == "the buffers of the graph (1000 bytes) do not fit in the free device memory (10 bytes) at 7 distinct k-mers"


# ---- what the reference's Bifrost wrote ----

@pytest.mark.parametrize("name", ["build_k25", "build_k7"])
def test_python_rule_equals_bifrost_on_the_fixtures(name):
    with open(os.path.join(GOLDEN, name, "meta.json")) as f:
        k = json.load(f)["k"]
    S = uc.kmer_set(fixture_reads(name), k)
    stats = {}
    for tag, flags in FLAG_FILES.items():
        text, stats[tag] = uc.build(S, k, *flags)
        with open(os.path.join(GOLDEN, name, tag + ".gfa"), "rb") as f:
            ref = f.read()
        assert ref.startswith(uc.header(k).encode())              # the header line, byte for byte
        assert uc.same_graph(text, ref), tag
        assert len(uc.gfa_sequences(ref)[1]) == stats[tag]["unitigs_out"]
    # not vacuous: tips are removed, and in the k = 25 fixture backbones rejoin (fewer unitigs than the removal alone leaves)
    assert stats["i"]["removed"] > 0
    if name == "build_k25":
        assert stats["i"]["unitigs_out"] < stats["i"]["unitigs"] - stats["i"]["removed"]
    assert stats["none"]["removed"] == 0 and stats["none"]["unitigs_out"] == stats["i"]["unitigs"]
    for tag in FLAG_FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name, tag + ".gfa")) < 300 * 1024
    assert os.path.getsize(os.path.join(GOLDEN, name, "reads.fq")) < 300 * 1024


# ---- the sub-command's refusals that need no device (this passes on a machine without a GPU) ----

def test_cli_refusals(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(uc.fastq(["ACGTTGCATGCATGGGATCCATGCAATGCCGTA"]))
    fa, gz = tmp_path / "in.fa", tmp_path / "in.fq.gz"
    fa.write_bytes(b">s\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    os.link(fq, tmp_path / "same.gfa")   # the output name is the input file
    base = ["build", "-r", fq, "-o", tmp_path / "s"]
    cases = [(base + [opt], "%s is not built" % opt) for opt in ("-s", "-c", "-y", "-f", "-a", "-m", "-n", "-b", "-B", "-l", "-w", "-e")]
    cases += [
        (base + ["-k", "2"], "-k goes from 3 to 31"),
        (base + ["-k", "32"], "-k goes from 3 to 31"),
        (base + ["-k", "0"], "-k takes a positive number, not '0'"),
        (base + ["-k", "25", "-g", "24"], "-g goes from 1 to k - 2 = 23"),
        (base + ["-k", "5", "-g", "4"], "-g goes from 1 to k - 2 = 3"),
        (base + ["-g", "x"], "-g takes a positive number, not 'x'"),
        (["build", "-o", tmp_path / "s"], "-r <reads.fq> is missing"),
        (["build", "-r", fq], "-o <sample> is missing"),
        (["build", "-r", fq, "-o", tmp_path / "same"], "%s: the output path is an input path" % fq),
        (["build", "-r", fq, "-r", fa, "-o", tmp_path / "s"], "%s: record 1: the input is FASTA (first byte '>'): only FASTQ is read" % fa),
        (["build", "-r", gz, "-o", tmp_path / "s"], "%s: record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is read" % gz),
        (["build", "-r", tmp_path / "none.fq", "-o", tmp_path / "s"], "cannot read %s" % (tmp_path / "none.fq")),
        (base + ["--gpus", "2"], "--gpus is not built: the graph is made on one GPU"),
        (base + ["--frobnicate"], "unknown option --frobnicate"),
        (base + ["--chunk-bytes"], "--chunk-bytes needs a value"),
        (base + ["-t"], "-t needs a value"),
    ]
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stderr.startswith("Error: build: ") and r.stdout == "", (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["in.fa", "in.fq", "in.fq.gz", "same.gfa"], args   # no output, no temporary file
    usage = run_cli().stdout
    assert "build -k 25 [-i] [-d] -r <reads.fq>" in usage
    for g in (0, -1, 24):   # the Python call: 0 is outside 1 .. k - 2, not "the default" (that is None)
        with pytest.raises(RuntimeError, match="-g goes from 1 to k - 2 = 23"):
            hostapi.build_graph(str(fq), str(tmp_path / "s"), k=25, g=g)
    assert sorted(os.listdir(tmp_path)) == ["in.fa", "in.fq", "in.fq.gz", "same.gfa"]


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_unitig_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_unitig_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_unitig_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- names ----

def declaration(header, name):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = f.read()
    at = text.index(name + "(")
    return " ".join(text[at: text.index(";", at)].split())


def test_entry_points_are_declared():
    for s in ("pf_unitig_build", "pf_unitig_fetch", "pf_unitig_release"):
        assert s in hipapi.DECLARED_SYMBOLS
    for s in ("pfh_build_fastq", "pfh_unitig_build_host"):
        assert s in hostapi.DECLARED_SYMBOLS
    assert hipapi.K_UNITIG == hipapi.K_TRIM + 1
    L = hipapi.load_library()
    assert L.pf_kernel_name(hipapi.K_UNITIG) == b"k_unitig" and L.pf_kernel_name(hipapi.K_TRIM) == b"k_trim"
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_UNITIG" in text.split("PF_K_TRIM,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    assert declaration("ploidyfrost_hip.h", "int pf_unitig_build") == (
        "int pf_unitig_build(pf_ctx *, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated, pf_unitig_stats *stats)")
    assert declaration("ploidyfrost_hip.h", "int pf_unitig_fetch") == "int pf_unitig_fetch(pf_ctx *, uint64_t first_byte, uint64_t len, char *host)"
    assert declaration("ploidyfrost_hip.h", "int pf_unitig_release") == "int pf_unitig_release(pf_ctx *)"
    assert hipapi.UNITIG_STATS == hostapi.UNITIG_STATS and hipapi.UNITIG_STATS.itemsize == 9 * 8 + 6 * 8
    assert hostapi.UNITIG_STATS_FIELDS == uc.STATS == hipapi.UNITIG_STATS.names[:6]
