"""K-FASTA (pf_fasta_index, pf_count_fasta, pf_maskcount_fasta; csrc/pf_fasta.hip) against the host restatement of its rule
(csrc/pf_fasta_rule.hpp), its windows against the host rules of K-COUNT and K-MASKCOUNT on the joined sequences, and every sub-command
that takes `--fasta` on a FASTA file F against the same command without the flag on Q(F), F rewritten record by record as FASTQ
(fasta_cases.q_of).  Every comparison is exact: arrays of integers and bytes of files, the statistics lines and stdout (but for
the calling run's clock lines).

Zero-length records: the FASTQ index takes an empty sequence line with an empty quality line, so Q(F) could hold them; the command
tests keep to the reads of the generators all the same (none is empty), and zero-length records are checked by the kernel tests."""
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import fasta_cases as fc
import gz_cases as gz
import mask_cases as mc
import run_cases as rc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
TEXTS = fc.edge_texts()


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def same_index(got, want, what):
    assert got["text"] == want["text"], what
    assert np.array_equal(got["read_off"], want["read_off"]) and np.array_equal(got["read_len"], want["read_len"]), what
    assert (got["bytes_used"], got["records"], got["bases"]) == (want["bytes_used"], want["records"], want["bases"]), what


# ---- the kernel against the host rule ----

@pytest.mark.parametrize("name,text", [t for t in TEXTS if t[1]], ids=[n for n, t in TEXTS if t])
def test_kernel_against_the_host_rule(dev, name, text):
    for final in (True, False):
        same_index(dev.fasta_index(text, final=final), hostapi.fasta_index(text, final=final), (name, final))
    for c in fc.cuts_of(text):   # inside a sequence line, inside a header, behind a '\n', in front of a '>', a single header
        same_index(dev.fasta_index(text[:c], final=False), hostapi.fasta_index(text[:c], final=False), (name, c))


def test_single_header_chunk_gives_nothing(dev):
    for text in (b">abc", b">abc\n", b">abc\nACGT", b">abc\nACGT\nAC\n"):
        got = dev.fasta_index(text, final=False)
        assert (got["records"], got["bytes_used"], got["bases"], got["text"]) == (0, 0, 0, b""), text
    assert dev.fasta_index(b"", final=True)["records"] == 0


def test_about_300_kb_and_a_device_pointer(dev):
    text = fc.big_text()
    assert 250_000 < len(text) < 450_000
    want = hostapi.fasta_index(text, final=True)
    assert want["records"] == 2000 and int(want["read_len"].min()) == 0
    same_index(dev.fasta_index(text, final=True), want, "final")
    same_index(dev.fasta_index(text, final=False), hostapi.fasta_index(text, final=False), "not final")
    on_dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    same_index(dev.fasta_index(on_dev, final=True), want, "device pointer")
    cut = len(text) // 2 + 5
    shifted = torch.frombuffer(bytearray(b"###" + text[:cut]), dtype=torch.uint8).cuda()[3:]       # device memory that is not 16-byte aligned: staged
    same_index(dev.fasta_index(shifted, final=False), hostapi.fasta_index(text[:cut], final=False), "device pointer, unaligned, cut")


def test_text_in_front_of_the_first_header_is_refused(dev):
    with pytest.raises(hipapi.DeviceError, match="pf_fasta_index: record 0 of the chunk: the text does not start with '>'"):
        dev.fasta_index(b"ACGT\n>a\nAC\n")


def test_timed_as_its_own_kernel(dev):
    text = fc.big_text(seed=6, n_records=200)
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        dev.fasta_index(text)
        ms, launches = dev.kernel_time(hipapi.K_FASTA)
        assert launches == 1 and ms > 0
        assert dev.kernel_time(hipapi.K_COUNT)[1] == 0
    finally:
        dev.enable_timing(False)


# ---- windows ----

def count_fasta(d, text, k, cuts=()):
    """F through pf_count_fasta into a fresh count, whole or in chunks cut at `cuts` with the carry a stream keeps"""
    d.count_begin(k, True)
    total = dict.fromkeys(("reads", "bases", "kmers", "kmers_bad"), 0)
    try:
        at = 0
        for end in list(cuts) + [len(text)]:
            used, st = d.count_fasta(text[at:end], final=(end == len(text)))
            at += used
            for f in total:
                total[f] += st[f]
        assert at == len(text)
    except Exception:
        d.count_abort()
        raise
    kmers, counts, fin = d.count_finish(**rc.EVERY)
    return kmers, counts, total, fin


def host_count(text, k):
    r = hostapi.fasta_index(text)
    kmers, counts, st = hostapi.count_reads_host(r["text"], r["read_off"], r["read_len"], k, True, **rc.EVERY)
    return kmers, counts, st


@pytest.mark.parametrize("name,text,k,n_windows", [
    ("windows_cross_the_line_end", b">a\nACGTA\nCGTAC\n", 5, 6),
    ("none_crosses_a_record", b">a\nTTACG\n>b\nTACCA\n", 5, 2),
    ("shorter_than_k", b">a\nACGT\n>b\nACGTACG\nT\n>c\n", 5, 4),
    ("crlf_and_a_non_base", b">a\r\nACGTAC\r\nGTNACG\r\nTACGT\r\n", 5, 13),
])
def test_windows_against_the_host_count(dev, name, text, k, n_windows):
    want_k, want_c, want_st = host_count(text, k)
    kmers, counts, st, fin = count_fasta(dev, text, k)
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c), name
    assert st["kmers"] == n_windows == want_st["kmers"] and st["kmers_bad"] == want_st["kmers_bad"]
    assert (st["reads"], st["bases"]) == (want_st["reads"], want_st["bases"]) == (text.count(b">"), len(hostapi.fasta_index(text)["text"]))
    if name == "none_crosses_a_record":      # joined, the two records would have six windows
        assert st["kmers"] < len(b"TTACGTACCA") - k + 1 and int(counts.sum()) == 2


def test_count_of_the_big_text_whole_and_in_chunks(dev):
    text = fc.big_text(seed=7, n_records=400)
    want_k, want_c, want_st = host_count(text, 25)
    for cuts in ((), (len(text) // 3, len(text) // 2, len(text) // 2 + 1)):
        kmers, counts, st, _ = count_fasta(dev, text, 25, cuts)
        assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c), cuts
        assert st == {f: want_st[f] for f in st}, cuts


def test_a_bad_window_in_front_of_a_line_end_masks_its_neighbours_on_the_next_line(dev):
    """one low-count window that starts two bases in front of a line end: the windows within k - 1 starts of it go, those on the next
    line included (pf_run_rule.hpp), exactly as on the joined sequence"""
    k, n, width = 25, 400, 60
    weak = 2 * width - 2                                   # two bases in front of the end of the second sequence line
    genome, db = mc.synthetic(21, n, k, weak=(weak,))
    db.upload(dev)
    text = fc.fasta([genome], width=width)
    r = hostapi.fasta_index(text)
    assert r["text"] == genome
    table = [(0, n)]
    want_k, want_c, want_st = hostapi.count_masked_host(genome, [0], [n], k, rc.flat_counters(genome, table, db), 10, mc.NO_UPPER)
    dev.count_begin(k, True)
    try:
        used, st = dev.maskcount_fasta(text, 10)
    except Exception:
        dev.count_abort()
        raise
    kmers, counts, _ = dev.count_finish(**rc.EVERY)
    assert used == len(text) and st == want_st
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
    dead = set(range(weak - k + 1, weak + k))
    assert st["kmers_bad"] == 1 and st["kmers_kept"] == n - k + 1 - len(dead)
    fw, rcm = mc.synth.kmers_u64(mc._CODE[np.frombuffer(genome, dtype=np.uint8)], k)
    keys, have = np.minimum(fw, rcm), set(kmers.tolist())
    for p in range(weak - k - 2, weak + k + 3):             # the starts on the next line (p >= 2 * width) among them
        assert (int(keys[p]) in have) == (p not in dead), p


# ---- commands: F with --fasta against Q(F) without ----

def cli(*a, cwd):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """F: the reads of make_build_golden.py's build_k25 case at the depth test_gpu_run.py uses (48), as FASTA at width 60, with one
    record of 20 000 bases in the middle so that --chunk-bytes 4096 has to grow its carry; Q: Q(F)"""
    root = tmp_path_factory.mktemp("fasta")
    gen = generator("make_build_golden")
    reads = [r.encode() for r in gen.make_reads(**dict(gen.CASES["build_k25"], depth=48))]
    long_one = fc.random_seq(np.random.default_rng(3), 20000)
    reads = reads[: len(reads) // 2] + [long_one] + reads[len(reads) // 2:]
    f = fc.fasta(reads, width=60)
    (root / "F.fa").write_bytes(f)
    (root / "Q.fq").write_bytes(fc.q_of(f))
    assert hostapi.fasta_index(f)["records"] == len(reads)
    return {"root": root, "F": root / "F.fa", "Q": root / "Q.fq", "text": f, "reads": reads}


def stdout_of(r):
    """stdout without the calling run's clock lines ("... Cpu time : 0.000286s", "... Real time : 0s"), which no two runs share"""
    return [l for l in r.stdout.splitlines() if " time : " not in l]


def stats_line(r, who):
    lines = [l for l in r.stderr.splitlines() if l.startswith(who + ": reads ") or l.startswith(who + ": colors ")]
    assert len(lines) == 1, r.stderr
    return lines[0]


def files_of(d, skip=()):
    out = {}
    for base, _, names in os.walk(d):
        for n in names:
            p = os.path.join(base, n)
            if n not in skip:
                out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("extra", [[], ["--chunk-bytes", 4096]], ids=["default", "chunk_carries"])
def test_count(inputs, tmp_path, extra):
    args = ["-k", 25, "-ci", 1, "-cs", 10000, "-o", "db", "--hist", "h.txt"] + extra
    got, want = tmp_path / "fa", tmp_path / "fq"
    got.mkdir(), want.mkdir()
    a = cli("count", "-i", inputs["F"], "--fasta", *args, cwd=got)
    b = cli("count", "-i", inputs["Q"], *args, cwd=want)
    assert files_of(got) == files_of(want) and sorted(files_of(got)) == ["db.kmc_pre", "db.kmc_suf", "h.txt"]
    assert stats_line(a, "count") == stats_line(b, "count") and " reads %d " % len(inputs["reads"]) in stats_line(a, "count")
    assert a.stdout == b.stdout


@pytest.mark.parametrize("flags", [["-i", "-d"], []], ids=["id", "none"])
def test_build(inputs, tmp_path, flags):
    got, want = tmp_path / "fa", tmp_path / "fq"
    got.mkdir(), want.mkdir()
    a = cli("build", *flags, "-k", 25, "-r", inputs["F"], "--fasta", "-o", "g", cwd=got)
    b = cli("build", *flags, "-k", 25, "-r", inputs["Q"], "-o", "g", cwd=want)
    assert files_of(got) == files_of(want) and list(files_of(got)) == ["g.gfa"] and len(files_of(got)["g.gfa"]) > 1000
    assert stats_line(a, "build") == stats_line(b, "build")


def test_build_multi_one_fasta_and_one_fastq_colour(inputs, tmp_path):
    """a colour is named by its path as given: both runs get the same relative names in two working directories"""
    reads = [r for r in inputs["reads"] if len(r) < 1000]
    half = len(reads) // 2
    f0 = fc.fasta(reads[:half], width=60)
    q1 = mc.fastq(reads[half:])
    got, want = tmp_path / "fa", tmp_path / "fq"
    for d, s0 in ((got, f0), (want, fc.q_of(f0))):
        d.mkdir()
        (d / "s0").write_bytes(s0)
        (d / "s1").write_bytes(q1)
    a = cli("build-multi", "-i", "-d", "-k", 25, "-r", "s0", "-r", "s1", "--fasta", "-o", "g", cwd=got)
    b = cli("build-multi", "-i", "-d", "-k", 25, "-r", "s0", "-r", "s1", "-o", "g", cwd=want)
    fa, fq = files_of(got, skip=("s0", "s1")), files_of(want, skip=("s0", "s1"))
    assert fa == fq and sorted(fa) == ["g.bfg_colors", "g.gfa"]
    assert stats_line(a, "build-multi") == stats_line(b, "build-multi")


@pytest.mark.parametrize("extra", [[], ["--chunk-bytes", 4096]], ids=["default", "chunk_carries"])
def test_run(inputs, tmp_path, extra):
    got, want = tmp_path / "fa", tmp_path / "fq"
    got.mkdir(), want.mkdir()
    args = ["-o", "r", "--model", "fre", "--db-out", "d", "--gfa-out", "g"] + extra
    a = cli("run", "-i", inputs["F"], "--fasta", *args, cwd=got)
    b = cli("run", "-i", inputs["Q"], *args, cwd=want)
    fa, fq = files_of(got), files_of(want)
    assert fa == fq and len(fa) >= 16, sorted(fa)
    rows = fa[os.path.join("PloidyFrost_output", "r_allele_frequency.txt")].decode().splitlines()
    assert len(rows) >= 5                                      # the comparison is not vacuous
    assert stdout_of(a) == stdout_of(b) and len(stdout_of(a)) >= 10 and int(a.stdout.splitlines()[0]) >= 10
    assert stats_line(a, "run") == stats_line(b, "run")


def test_run_multi_one_fasta_and_one_fastq_sample(tmp_path):
    """the samples of make_build_multi_golden.py's build_mc3_k25 case at the depth test_gpu_run_multi.py uses; sample alpha in two files,
    one FASTA and one FASTQ, sample beta FASTA, sample gamma FASTQ"""
    gen = generator("make_build_multi_golden")
    samples = [[r.encode() for r in s] for s in gen.make_samples(**dict(gen.CASES["build_mc3_k25"], depth=48))]
    third = len(samples[0]) // 3
    fa_parts = {"a0": fc.fasta(samples[0][:third], width=60), "b": fc.fasta(samples[1], width=60)}
    common = {"a1": mc.fastq(samples[0][third:]), "c": mc.fastq(samples[2])}
    got, want = tmp_path / "fa", tmp_path / "fq"
    for d, conv in ((got, lambda t: t), (want, fc.q_of)):
        d.mkdir()
        for n, t in fa_parts.items():
            (d / n).write_bytes(conv(t))
        for n, t in common.items():
            (d / n).write_bytes(t)
    args = ["--sample", "alpha", "-i", "a0", "-i", "a1", "--sample", "beta", "-i", "b", "--sample", "gamma", "-i", "c", "-o", "r", "--model", "fre",
            "--filter-multi", "-v 0.25 -n 6", "--db-out", "d", "--gfa-out", "g"]
    a = cli("run-multi", *args, "--fasta", cwd=got)
    b = cli("run-multi", *args, cwd=want)
    skip = ("a0", "a1", "b", "c")
    fa, fq = files_of(got, skip), files_of(want, skip)
    assert fa == fq and len(fa) >= 16, sorted(fa)
    assert len(fa[os.path.join("PloidyFrost_output", "r_allele_frequency.txt")].decode().splitlines()) >= 5
    assert stdout_of(a) == stdout_of(b) and len(stdout_of(a)) >= 10
    assert [l for l in a.stderr.splitlines() if l.startswith("run-multi: col")] == [l for l in b.stderr.splitlines() if l.startswith("run-multi: col")]


def test_count_of_the_gzip_forms(inputs, tmp_path):
    """`count --gz --fasta` on the blocked-gzip form of F and `count --gz-plain --fasta` on its gzip form against `count --fasta` on F:
    there the kind is the first inflated byte, and the step decides"""
    (tmp_path / "F.fa.bgz").write_bytes(gz.bgzf(inputs["text"]))
    (tmp_path / "F.fa.gz").write_bytes(gzip.compress(inputs["text"], 6))
    args = ["-k", 25, "-ci", 1, "-cs", 10000, "--fasta"]
    want = cli("count", "-i", inputs["F"], "-o", "plain", *args, cwd=tmp_path)
    for flag, name, extra in (("--gz", "F.fa.bgz", []), ("--gz-plain", "F.fa.gz", []), ("--gz", "F.fa.bgz", ["--chunk-bytes", 200000])):
        got = cli("count", "-i", name, "-o", "z", flag, *args, *extra, cwd=tmp_path)
        for suf in (".kmc_pre", ".kmc_suf"):
            assert open(str(tmp_path / "z") + suf, "rb").read() == open(str(tmp_path / "plain") + suf, "rb").read(), (flag, suf)
        assert stats_line(got, "count") == stats_line(want, "count"), flag


def test_hostapi_takes_fasta(inputs, tmp_path):
    want = hostapi.count_fastq(str(inputs["Q"]), str(tmp_path / "q"), k=25, ci=1, cs=10000)
    got = hostapi.count_fastq(str(inputs["F"]), str(tmp_path / "f"), k=25, ci=1, cs=10000, fasta=True)
    assert got == want and got["reads"] == len(inputs["reads"])
    with pytest.raises(RuntimeError, match="the input is FASTA"):       # the switch does not stick
        hostapi.count_fastq(str(inputs["F"]), str(tmp_path / "x"), k=25, ci=1, cs=10000)
    g = hostapi.build_graph(str(inputs["F"]), str(tmp_path / "gf"), k=25, clip_tips=True, del_isolated=True, fasta=True)
    w = hostapi.build_graph(str(inputs["Q"]), str(tmp_path / "gq"), k=25, clip_tips=True, del_isolated=True)
    assert open(tmp_path / "gf.gfa", "rb").read() == open(tmp_path / "gq.gfa", "rb").read()
    assert {f: g[f] for f in g if f != "stage_ms"} == {f: w[f] for f in w if f != "stage_ms"}
