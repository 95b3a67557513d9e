"""The rule of `ploidyfrost count` (K-COUNT) without a GPU: the host's plain restatement (pfh_count_reads_host / pfh_count_encode_kmc1,
csrc/pf_count_rule.hpp) against the Python restatement of count_cases.py and against the bytes synth.write_kmc1 writes, counter_bytes at
its boundaries, the stand-alone program tests/cpp/test_count_rule.cpp under the sanitizers, the declarations, and the refusals of
`count` and `mask -k` that come before any device work."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case

import count_cases as cc
import mask_cases as mc

from ploidyfrost_amd import build, hipapi, hostapi, synth

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def host_count(reads, k, **kw):
    text, off, ln = mc.pack(reads)
    return hostapi.count_reads_host(text, off, ln, k, **kw)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- the Python restatement itself, on figures worked out by hand ----

def test_python_rule_by_hand():
    # ACGTACGTNACG, k = 3: ACG CGT GTA TAC ACG CGT | GTN TNA NAC | ACG; CGT is ACG's other strand, TAC is GTA's
    km, ct, st = cc.ref_count([b"ACGTACGTNACG"], 3, ci=1)
    assert km.tolist() == [0b000110, 0b101100] and ct.tolist() == [5, 2]
    assert st == dict(reads=1, bases=12, kmers=10, kmers_bad=3, unique=2, below_min=0, above_max=0, written=2)
    km, ct, st = cc.ref_count([b"ACGTACGTNACG"], 3, both_strands=False, ci=1)
    assert km.tolist() == [0b000110, 0b011011, 0b101100, 0b110001] and ct.tolist() == [3, 2, 1, 1]
    km, ct, st = cc.ref_count([b"ACGTACGTNACG"], 3, ci=3, cx=4)
    assert len(km) == 0 and (st["below_min"], st["above_max"], st["written"]) == (1, 1, 0)
    km, ct, st = cc.ref_count([b"acgtacgtnacg"], 3, ci=1, cs=4)
    assert ct.tolist() == [4, 2]
    # a k-mer equal to its own reverse complement counts once per occurrence
    km, ct, _ = cc.ref_count([b"ACGCGT", b"ACGCGT"], 6, ci=1)
    assert km.tolist() == [0b000110011011] and ct.tolist() == [2]
    assert [cc.counter_bytes(10 ** 9, cs) for cs in (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [1, 2, 2, 3, 3, 4]


# ---- pfh_count_reads_host against it ----

HAND = [([b""], 25), ([b"A"], 3), ([b"ACGT" * 6], 25), ([b"ACGT" * 6 + b"A"], 25), ([b"N" * 40], 25), ([b"acgt" * 20, b"ACGT" * 20], 25),
        ([b"ACGT" * 40], 31), ([b"ACGTN" * 30], 3), ([b"A" * 2000, b"ACGT" * 500], 5), ([b"ACGCGT" * 5], 6), ([b"ACGTACGTNACG"], 3),
        ([b"GATTACA", mc.revcomp(b"GATTACA")], 7), ([], 25)]


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("cut", [dict(ci=1), dict(), dict(ci=1, cx=5), dict(ci=2, cs=3), dict(ci=1, cx=1, cs=1)])
def test_host_rule_on_hand_cases(both, cut):
    for reads, k in HAND:
        assert same(host_count(reads, k, both_strands=both, **cut), cc.ref_count(reads, k, both_strands=both, **cut)), (reads[:1], k)


def test_host_rule_on_seeded_reads():
    reads = mc.make_reads("dip20k", 200, seed=11)
    for both in (True, False):
        want = cc.ref_count(reads, 25, both_strands=both, ci=1, cs=10000)
        assert same(host_count(reads, 25, both_strands=both, ci=1, cs=10000), want)
        assert want[2]["kmers_bad"] > 0 and want[2]["unique"] > 5000 and want[1].max() > 1
    gap = b"\n+\n@x\n"     # not packed: bytes between the reads are nobody's
    text = gap.join(reads)
    off = np.cumsum([0] + [len(r) + len(gap) for r in reads[:-1]])
    assert same(hostapi.count_reads_host(text, off, [len(r) for r in reads], 25), cc.ref_count(reads, 25))


def test_host_refusals_by_name():
    for kw, name in ((dict(ci=0), "ci_zero"), (dict(ci=6, cx=5), "ci_above_cx"), (dict(cs=0), "cs_zero"), (dict(cx=1 << 32), "too_large"),
                     (dict(cs=1 << 32), "too_large"), (dict(ci=1 << 32, cx=1 << 33), "too_large")):
        with pytest.raises(ValueError) as e:
            host_count([b"ACGT" * 10], 25, **kw)
        assert str(e.value).startswith(name + ": "), (kw, str(e.value))
    for k in (2, 32):
        with pytest.raises(ValueError) as e:
            host_count([b"ACGT" * 10], k)
        assert str(e.value).startswith("k: ")
    with pytest.raises(ValueError) as e:     # k = 3 and k = 4 are counted, not written: no prefix length leaves whole suffix bytes
        hostapi.count_encode_kmc1(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 4)
    assert str(e.value).startswith("k_layout: ")


# ---- the writer: the bytes of synth.write_kmc1 ----

@pytest.mark.parametrize("k", [5, 6, 25, 31])
@pytest.mark.parametrize("both", [True, False])
def test_host_encoder_writes_what_write_kmc1_writes(tmp_path, k, both):
    reads = mc.make_reads("dip20k", 200, seed=12) if k >= 25 else [b"A" * 200, b"ACGT" * 50, b"GATTACAGATTACCA" * 9]
    for cut in (dict(ci=1, cs=10000), dict(), dict(ci=1, cx=3, cs=70000)):
        kmers, counts, _ = cc.ref_count(reads, k, both_strands=both, **cut)
        full = dict(cc.DEFAULTS, **cut)
        assert hostapi.count_encode_kmc1(kmers, counts, k, both_strands=both, **full) == cc.kmc1_bytes(tmp_path, kmers, counts, k, both, **full), (k, cut)
    assert hostapi.count_lut_prefix_len(k) == synth.lut_prefix_len(k)
    none = np.zeros(0, dtype=np.uint64)
    assert hostapi.count_encode_kmc1(none, none.astype(np.uint32), k) == cc.kmc1_bytes(tmp_path, none, none.astype(np.uint32), k)


@pytest.mark.parametrize("cs,want", [(255, 1), (256, 2), (65535, 2), (65536, 3), ((1 << 24) - 1, 3), (1 << 24, 4)])
def test_counter_bytes_boundaries(tmp_path, cs, want):
    assert hostapi.count_counter_bytes(10 ** 9, cs) == cc.counter_bytes(10 ** 9, cs) == want
    assert hostapi.count_counter_bytes(cs, 0xFFFFFFFF) == want            # the smaller of the two decides
    kmers = np.array([3, 9, 1 << 40], dtype=np.uint64)
    counts = np.array([1, cs, max(cs - 1, 1)], dtype=np.uint32)
    pre, suf = hostapi.count_encode_kmc1(kmers, counts, 25, ci=1, cs=cs)
    assert (pre, suf) == cc.kmc1_bytes(tmp_path, kmers, counts, 25, ci=1, cs=cs)
    prefix = str(tmp_path / "back")
    with open(prefix + ".kmc_pre", "wb") as f:
        f.write(pre)
    with open(prefix + ".kmc_suf", "wb") as f:
        f.write(suf)
    k2, c2, meta = synth.read_kmc1(prefix)
    assert k2.tolist() == kmers.tolist() and c2.tolist() == counts.tolist() and meta["min_count"] == 1 and meta["max_count"] == 10 ** 9
    assert len(suf) == 8 + 3 * (5 + want)


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_count_rule.cpp: the shared header alone, plain g++ with -fsanitize=address,undefined (host code only: nothing of
    it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_count_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_count_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- names ----

def test_entry_points_are_declared():
    for s in ("pf_count_begin", "pf_count_reads", "pf_count_fastq", "pf_count_finish", "pf_count_abort", "pf_kmc_encode"):
        assert s in hipapi.DECLARED_SYMBOLS
    assert hipapi.K_COUNT == hipapi.K_MASK + 1 and hipapi.KERNELS[-1] == "k_call_model"
    for s in ("pfh_count_fastq", "pfh_mask_fastq_counted", "pfh_count_reads_host", "pfh_count_encode_kmc1"):
        assert s in hostapi.DECLARED_SYMBOLS
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_COUNT," in text.split("PF_K_MASK,")[1].split("PF_K_COUNT_")[0]
    assert hostapi.COUNT_STATS_FIELDS == cc.STATS == hipapi.COUNT_STATS.names
    L = hipapi.load_library()
    assert L.pf_kernel_name(hipapi.K_COUNT) == b"k_count" and L.pf_kernel_name(hipapi.K_MASK) == b"k_mask"


# ---- the sub-commands' refusals: by name, before any device work (this passes on a machine without a GPU) ----

def test_count_cli_refusals(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(mc.fastq([b"ACGT" * 10]))
    fa, gz = tmp_path / "in.fa", tmp_path / "in.fq.gz"
    fa.write_bytes(b">s\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    (tmp_path / "same.kmc_suf").write_bytes(mc.fastq([b"ACGT" * 10]))
    db = tmp_path / "db"
    base = ["count", "-i", fq, "-o", db]
    cases = [
        (["count", "-o", db], "-i <reads.fq> is missing"),
        (["count", "-i", fq], "-o <KMCDatabase> is missing"),
        (base + ["-ci", "0"], "-ci is below 1"),
        (base + ["-ci0"], "-ci is below 1"),
        (base + ["-ci", "6", "-cx", "5"], "-ci is above -cx"),
        (base + ["-ci6", "-cx5"], "-ci is above -cx"),
        (base + ["-cs", "0"], "-cs is below 1"),
        (base + ["-cx", "4294967296"], "go up to 4294967295"),
        (base + ["-cs4294967296"], "go up to 4294967295"),
        (base + ["-ci", "99999999999999999999999"], "go up to 4294967295"),
        (base + ["-k", "2"], "-k goes from 3 to 31"),
        (base + ["-k32"], "-k goes from 3 to 31"),
        (base + ["-k", "x"], "-k takes a number"),
        (base + ["-k", "4"], "a KMC1 database needs -k of at least 5"),
        (base + ["-ci", "-1"], "-ci takes a number"),
        (base + ["-cs"], "-cs needs a value"),
        (base + ["--chunk-bytes", "0"], "--chunk-bytes takes a positive number"),
        (base + ["--initial-slots", "x"], "--initial-slots takes a positive number"),
        (base + ["--frobnicate"], "unknown option --frobnicate"),
        (["count", "-i", fq, "-i", fa, "-o", db], "%s: record 1: the input is FASTA (first byte '>'): only FASTQ is counted" % fa),
        (["count", "-i", gz, "-o", db], "%s: record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is counted" % gz),
        (["count", "-i", tmp_path / "same.kmc_suf", "-o", tmp_path / "same"], "the output path is an input path"),
        (["count", "-i", fq, "-o", db, "--hist", fq], "the output path is an input path"),
        (["count", "-i", tmp_path / "absent.fq", "-o", db], "cannot read"),
    ]
    before = sorted(os.listdir(tmp_path))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args   # no output, no temporary file
    assert "count -k 25" in run_cli().stdout + run_cli().stderr


def test_mask_k_cli_refusals(tmp_path):
    db = load_case("dip20k")["db"]
    fq = tmp_path / "in.fq"
    fq.write_bytes(mc.fastq([b"ACGT" * 10]))
    out = tmp_path / "out.fq"
    with_k = ["mask", "-k", "25", "-i", fq, "-o", out]
    with_d = ["mask", "-d", db, "-i", fq, "-o", out, "-l", "5"]
    cases = [
        (with_d + ["-k", "25"], "-d does not go with -k"),
        (with_d + ["-k25"], "-d does not go with -k"),
        (with_d + ["-ci", "2"], "-ci needs -k"),
        (with_d + ["-cs10000"], "-cs needs -k"),
        (with_d + ["-cx", "9"], "-cx needs -k"),
        (with_d + ["-b"], "-b needs -k"),
        (with_d + ["--db-out", tmp_path / "db"], "--db-out needs -k"),
        (["mask", "-i", fq, "-o", out, "-l", "5"], "-d <KMCDatabase> is missing"),          # neither -d nor -k: as a missing -d is refused
        (with_k, "the lower threshold is missing"),
        (with_k + ["-l", "5", "--auto-cutoffs"], "-l does not go with --auto-cutoffs"),
        (with_k + ["-l", "9", "-u", "8"], "L > U"),
        (with_k + ["-l", "5", "-ci", "0"], "-ci is below 1"),
        (with_k + ["-l", "5", "-ci", "6", "-cx", "5"], "-ci is above -cx"),
        (with_k + ["-l", "5", "-cs", "0"], "-cs is below 1"),
        (with_k + ["-l", "5", "-cx", "4294967296"], "go up to 4294967295"),
        (["mask", "-k", "32", "-i", fq, "-o", out, "-l", "5"], "-k goes from 3 to 31"),
        (["mask", "-k", "2", "-i", fq, "-o", out, "-l", "5"], "-k goes from 3 to 31"),
        (["mask", "-k", "25", "-o", out, "-l", "5"], "-i <reads.fq> is missing"),
        (["mask", "-k", "25", "-i", fq, "-l", "5"], "-o <out.fq> is missing"),
        (["mask", "-k", "25", "-i", fq, "-o", fq, "-l", "5"], "the output path is an input path"),
        (with_k + ["-l", "5", "--db-out"], "--db-out needs a value"),
        (["mask", "-k3", "-i", fq, "-o", out, "-l", "5", "--db-out", tmp_path / "db"], "a KMC1 database needs -k of at least 5"),
    ]
    (tmp_path / "clash.kmc_pre").write_bytes(mc.fastq([b"ACGT" * 10]))
    cases.append((["mask", "-k", "25", "-i", tmp_path / "clash.kmc_pre", "-o", out, "-l", "5", "--db-out", tmp_path / "clash"], "the output path is an input path"))
    before = sorted(os.listdir(tmp_path))
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stdout == "", (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args
    assert "mask -k 25" in run_cli().stdout + run_cli().stderr
