"""K-MASKCOUNT (pf_maskcount_reads / pf_maskcount_fastq, csrc/pf_maskcount.hip) against the host restatement of its rule
(csrc/pf_run_rule.hpp) and against K-MASK followed by K-COUNT, and `ploidyfrost run` against the three-command chain it replaces.
Every comparison is exact: arrays of integers and bytes of files."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import mask_cases as mc
import run_cases as rc

from ploidyfrost_amd import hipapi, hostapi, synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
FIXTURE = os.path.join(ROOT, "tests", "golden", "build_k25", "reads.fq")
TILE = 1024   # pf::MASK_TILE


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def maskcount(d, text, off, ln, k, low, up=mc.NO_UPPER, cuts=()):
    """the reads through pf_maskcount_reads into a fresh count -- in one call, or cut at the read indices `cuts` into several -- and
    the arrays pf_count_finish(ci = 1) gives"""
    d.count_begin(k, True)
    total = dict.fromkeys(hipapi.MASKCOUNT_STATS.names, 0)
    try:
        edges = [0] + list(cuts) + [len(off)]
        for a, b in zip(edges[:-1], edges[1:]):
            if a == b:
                continue
            lo = int(off[a])
            hi = int(off[b - 1]) + int(ln[b - 1])
            st = d.maskcount_reads(text[lo:hi], np.asarray(off[a:b], dtype=np.uint64) - np.uint64(lo), ln[a:b], low, up)
            for f in total:
                total[f] += st[f]
    except Exception:
        d.count_abort()
        raise
    kmers, counts, fin = d.count_finish(**rc.EVERY)
    return kmers, counts, total, fin


def check(d, db, reads, low, up=mc.NO_UPPER, gap=b"", cuts=None):
    """the reads back to back (or with `gap` between them) against the host restatement and against mask-then-count in Python"""
    parts, off, at = [], [], 0
    for r in reads:
        off.append(at)
        parts += [r, gap]
        at += len(r) + len(gap)
    text = b"".join(parts)
    ln = [len(r) for r in reads]
    table = list(zip(off, ln))
    want_k, want_c, want_st = hostapi.count_masked_host(text, off, ln, db.k, rc.flat_counters(text, table, db), low, up)
    comp_k, comp_c, _, _ = rc.composition(text, table, db, low, up)
    assert np.array_equal(want_k, comp_k) and np.array_equal(want_c, comp_c)        # the reference agrees with the composition
    for c in ([()] if cuts is None else [(), cuts]):
        kmers, counts, st, fin = maskcount(d, text, np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint32), db.k, low, up, cuts=c)
        assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c), (len(kmers), len(want_k), c)
        assert st == want_st
        assert fin["written"] == len(want_k) and fin["kmers"] == want_st["kmers"] and fin["kmers_bad"] == want_st["kmers_invalid"]
    return want_k, want_c, want_st


# ---- the kernel, through pf_maskcount_reads ----

@pytest.mark.parametrize("name,weak", [
    ("none", ()), ("first", (0,)), ("last", (2500 - 25,)),
    ("last_of_a_tile", (TILE - 1,)), ("first_of_a_tile", (TILE,)), ("both_sides_of_a_tile_edge", (TILE - 1, TILE)),
    ("victims_in_the_next_tile", (TILE - 3,)), ("victims_in_the_previous_tile", (TILE + 2,)), ("in_the_halo", (TILE - 25, TILE + 24)),
    ("two_k_apart", (300, 300 + 2 * 25)), ("two_k_less_1_apart", (300, 300 + 2 * 25 - 1)),
    ("at_a_word_edge", (639,)), ("behind_a_word_edge", (640,)), ("k_before_a_word_edge", (640 - 25,)), ("k_less_1_before_a_word_edge", (640 - 24,)),
])
def test_bad_windows_by_position_k25(dev, name, weak):
    """one read longer than two tiles at offset 0 of the text: window i is window start i.  A bad window w kills the starts
    w - k + 1 .. w + k - 1 and no others: the start exactly k - 1 away dies, the one exactly k away is kept."""
    k, n = 25, 2500
    genome, db = mc.synthetic(9, n, k, weak=weak)
    db.upload(dev)
    kmers, counts, st = check(dev, db, [genome], 10)
    dead = {p for w in weak for p in range(max(w - k + 1, 0), min(w + k, n - k + 1))}
    assert st["kmers"] == n - k + 1 and st["kmers_bad"] == len(weak) and st["kmers_kept"] == n - k + 1 - len(dead) == len(kmers)
    keys, have = np.minimum(*keys_of(genome, k)), set(kmers.tolist())     # (the genome repeats no k-mer: a key is a window)
    for p in range(n - k + 1):
        assert (int(keys[p]) in have) == (p not in dead), (name, p)
    # the same read deeper in the text: every alignment of the read against the tiles, the 64-bit words and the 16-byte units
    for shift in (1, 15, 63, 1000):
        check(dev, db, [b"", genome], 10, gap=b"#" * shift)


def keys_of(seq, k):
    return synth.kmers_u64(mc._CODE[np.frombuffer(seq, dtype=np.uint8)], k)


@pytest.mark.parametrize("weak", [(33,), (63,), (64,), (94,), (95,), (127,), (128,), (64, 127), (33, 157)])
def test_two_word_edges_k31(dev, weak):
    """k = 31: the 61 bits around a start reach across two edges of the 64-bit words of the bad bitmap"""
    k, n = 31, 400
    genome, db = mc.synthetic(31, n, k, weak=weak)
    db.upload(dev)
    for shift in (0, 1, 33, 34):
        _, _, st = check(dev, db, [b"", genome], 10, gap=b"#" * shift)
        assert st["kmers_bad"] == len(weak)


def test_k3_reads_touching_short_and_exact(dev):
    """k = 3: reads that touch without a gap, reads shorter than k and of exactly k, Ns, lower case, against a database whose counts
    spread over every threshold"""
    k = 3
    reads = rc.random_reads(seed=3, n_reads=400, k=k, length=40) + [b"", b"AC", b"ACG", b"acg", b"ANG", b"ACGT"]
    db = rc.database_of(reads, k)
    db.upload(dev)
    mid = int(np.median(db.counts))
    for low, up in ((0, mc.NO_UPPER), (mid, mc.NO_UPPER), (1, mid), (mid, mid + 50)):
        check(dev, db, reads, low, up, cuts=(100, 250))


@pytest.mark.parametrize("k", [25, 31])
def test_random_reads_one_call_and_three_chunks(dev, k):
    """reads touching without a gap; a text ending mid-tile; low = 0 with Ns; a finite up; lower case; one call against three chunks"""
    reads = rc.random_reads(seed=100 + k, n_reads=300, k=k, genome_len=900, length=120) + [b"A" * (k - 1), b"ACGT" * 8]
    if sum(len(r) for r in reads) % TILE == 0:
        reads.append(b"ACGTA")
    db = rc.database_of(reads, k)
    db.upload(dev)
    for low, up in ((0, mc.NO_UPPER), (2, mc.NO_UPPER), (3, 6), (1, 2)):
        _, _, st = check(dev, db, reads, low, up, cuts=(90, 91))
    assert st["kmers_invalid"] > 0
    long_read = b"".join(reads)[:3 * TILE + 17].replace(b"N", b"A")       # a single read longer than a tile
    check(dev, db, [long_read], 2)


def test_table_of_one_strand(dev):
    """a table uploaded with both_strands = 0 is asked for the window as it reads: the reverse strand's windows are all bad and
    nothing of that read is counted; what is counted is canonical all the same"""
    genome, db = mc.synthetic(5, 400, 25, both_strands=False)
    db.upload(dev)
    fwd, rev = genome[10:160], mc.revcomp(genome[10:160])
    kmers, counts, st = check(dev, db, [fwd, rev, fwd.lower()], 1)
    assert st["kmers_bad"] == 126 and st["kmers_kept"] == 2 * 126 and counts.tolist() == [2] * 126


def test_refusals():
    d = hipapi.Device(0)
    try:
        text, off, ln = b"ACGTACGTAC", [0], [10]
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_reads: no count table is resident"):
            d.maskcount_reads(text, off, ln, 1)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq: no count table is resident"):
            d.maskcount_fastq(mc.fastq([text]), 1)
        _, db = mc.synthetic(2, 100, 25)
        db.upload(d)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_reads: no count is open"):
            d.maskcount_reads(text, off, ln, 1)
        d.count_begin(21, True)
        with pytest.raises(hipapi.DeviceError, match="the open count's k = 21 differs from the count table's k = 25"):
            d.maskcount_reads(text, off, ln, 1)
        d.count_abort()
        d.count_begin(25, False)
        with pytest.raises(hipapi.DeviceError, match="not on both strands"):
            d.maskcount_fastq(mc.fastq([text]), 1)
        d.count_abort()
        d.count_begin(25, True)
        with pytest.raises(hipapi.DeviceError, match="low 5 is above up 4"):
            d.maskcount_reads(text, off, ln, 5, 4)
        kmers, counts, st = d.count_finish(**rc.EVERY)
        assert len(kmers) == 0 and st["kmers"] == 0          # nothing was counted from the refused calls
    finally:
        d.close()


# ---- pf_maskcount_fastq against pf_mask_fastq + pf_count_fastq ----

def fixture_table(k=25):
    text = open(FIXTURE, "rb").read()
    reads = [bytes(text[o:o + n]) for o, n in mc.parse_fastq(text)]
    return text, rc.database_of(reads, k)


def test_fastq_against_mask_then_count_on_device_pointers(dev):
    text, db = fixture_table()
    db.upload(dev)
    low = 10
    # one context masks into a device buffer, a second one counts that buffer
    t_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    t_out = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
    _, used, mst = dev.mask_fastq(t_in, low, out=t_out)
    assert used == len(text)
    second = hipapi.Device(0)
    try:
        second.count_begin(25, True)
        second.count_fastq(t_out[:used])
        want_k, want_c, cst = second.count_finish(**rc.EVERY)
    finally:
        second.close()
    assert len(want_k) > 1000 and mst["kmers_bad"] > 0
    for chunks in (1, 3):
        dev.count_begin(25, True)
        st = dict.fromkeys(hipapi.MASKCOUNT_STATS.names, 0)
        at = 0
        for c in range(chunks):
            end = len(text) if c == chunks - 1 else len(text) * (c + 1) // chunks
            used_c, s = dev.maskcount_fastq(t_in[at:end] if chunks == 1 else text[at:end], low, final=(c == chunks - 1))
            at += used_c
            for f in st:
                st[f] += s[f]
        kmers, counts, fin = dev.count_finish(**rc.EVERY)
        assert at == len(text)
        assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
        assert (st["reads"], st["bases"], st["kmers"], st["kmers_bad"]) == (mst["reads"], mst["bases"], mst["kmers"], mst["kmers_bad"])
        assert st["kmers_kept"] == int(counts.sum()) == cst["kmers"] - cst["kmers_bad"]


def test_fastq_format_error_counts_nothing(dev):
    text, db = fixture_table()
    db.upload(dev)
    recs = text.split(b"\n")
    bad = b"\n".join(recs[:4] + [recs[4][1:]] + recs[5:12]) + b"\n"      # the second record's first line loses its '@'
    dev.count_begin(25, True)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.maskcount_fastq(bad, 10)
    assert e.value.bad_record == 1 and "does not start with '@'" in str(e.value) and "pf_maskcount_fastq" in str(e.value)
    kmers, _, st = dev.count_finish(**rc.EVERY)
    assert len(kmers) == 0 and st["reads"] == 0


def test_timed_as_its_own_kernel(dev):
    genome, db = mc.synthetic(9, 2500, 25, weak=(700,))
    db.upload(dev)
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        dev.count_begin(25, True)
        dev.maskcount_reads(genome, [0], [len(genome)], 10)
        dev.count_abort()
        ms, launches = dev.kernel_time(hipapi.K_MASKCOUNT)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_MASKCOUNT) == 2500 - 24
        assert dev.kernel_time(hipapi.K_MASK)[1] == 0 and dev.kernel_time(hipapi.K_COUNT)[1] == 0
        assert dev.L.pf_kernel_name(hipapi.K_MASKCOUNT) == b"k_maskcount"
    finally:
        dev.enable_timing(False)


# ---- `ploidyfrost run` against the chain it replaces ----

def cli(*a, cwd):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def deeper_reads(path):
    """the generator of tests/golden/make_build_golden.py at twice the fixture's depth.  The chain derives L = max(10, cutoffL) = 10; at
    the fixture's depth of 24 the heterozygous k-mers stand at about 9, below it, the masking removes every bubble and
    allele_frequency.txt comes out empty (measured: 0 rows; 22 rows at depth 48)."""
    spec = importlib.util.spec_from_file_location("make_build_golden", os.path.join(ROOT, "tests", "golden", "make_build_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    s = dict(gen.CASES["build_k25"], depth=48)
    with open(path, "w") as f:
        for i, r in enumerate(gen.make_reads(**s)):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the three commands, once with `build -i -d` and once without: flags -> (directory, L as printed)"""
    root = tmp_path_factory.mktemp("chain")
    reads = root / "reads.fq"
    deeper_reads(reads)
    out = {"reads": reads}
    for tag, flags in (("id", ["-i", "-d"]), ("none", [])):
        d = root / tag
        d.mkdir()
        if tag == "id":
            m = cli("mask", "-k", 25, "-ci", 1, "-cs", 10000, "-i", reads, "-o", d / "filtered.fq", "--auto-cutoffs", "--db-out", d / "db", cwd=d)
            out["L"] = m.stdout
        else:
            shutil.copy(root / "id" / "filtered.fq", d / "filtered.fq")
            for suf in (".kmc_pre", ".kmc_suf"):
                shutil.copy(str(root / "id" / "db") + suf, str(d / "db") + suf)
        cli("build", *flags, "-k", 25, "-r", d / "filtered.fq", "-o", d / "s", cwd=d)
        cli("-g", d / "s.gfa", "-d", d / "db", "-o", "s", "--auto-cutoffs", "--model", "fre", cwd=d)
        out[tag] = d
    return out


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


@pytest.mark.parametrize("name,tag,extra", [("default", "id", []), ("chunk_carries", "id", ["--chunk-bytes", 4096]),
                                            ("keep", "none", ["--keep-tips", "--keep-isolated"])])
def test_run_against_the_chain(chain, tmp_path, name, tag, extra):
    want = calling_files(chain[tag], "s")
    rows = want["_allele_frequency.txt"].decode().splitlines()
    print("chain %s: L = %s, %d calling files, %d lines in allele_frequency.txt" % (tag, chain["L"].strip(), len(want), len(rows)))
    assert len(rows) >= 5, rows[:3]          # (the file has no header line) the comparison is not vacuous
    assert len([f for f in want if f != "_model_result.txt"]) == 12 and "_model_result.txt" in want
    r = cli("run", "-i", chain["reads"], "-o", "r", "--model", "fre", "--db-out", tmp_path / "d", "--gfa-out", tmp_path / "g", *extra, cwd=tmp_path)
    got = calling_files(tmp_path, "r")
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    for suf in (".kmc_pre", ".kmc_suf"):
        assert open(str(tmp_path / "d") + suf, "rb").read() == open(str(chain[tag] / "db") + suf, "rb").read(), suf
    assert open(tmp_path / "g.gfa", "rb").read() == open(chain[tag] / "s.gfa", "rb").read()
    assert r.stdout.splitlines()[0] + "\n" == chain["L"] and int(chain["L"]) >= 10
    assert sorted(os.listdir(tmp_path)) == ["PloidyFrost_output", "d.kmc_pre", "d.kmc_suf", "g.gfa"]      # no temporary file is left
    line = [l for l in r.stderr.splitlines() if l.startswith("run: reads ")]
    assert len(line) == 1 and " lower %d upper " % int(chain["L"]) in line[0]


def test_no_surviving_kmer_ends_with_the_calling_runs_message(tmp_path):
    """every k-mer occurs once or twice, L = 10: the masking leaves nothing and the graph is the header line alone.  `run` says on
    stdout what the calling run says about such a graph (RunCli::failed in pf_cli_run.cpp words it and leaves with EXIT_FAILURE), with that exit status,
    and leaves nothing under an output name."""
    rng = np.random.default_rng(4)
    reads = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=60)) for _ in range(40)]
    fq = tmp_path / "thin.fq"
    fq.write_bytes(mc.fastq(reads + reads[:30]))
    r = tmp_path / "run"
    r.mkdir()
    got = subprocess.run([CLI, "run", "-i", str(fq), "-o", "r", "--db-out", str(r / "d"), "--gfa-out", str(r / "g")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, cwd=r, timeout=300)
    assert got.returncode == 1
    assert got.stdout.splitlines() == ["10", "CompactedDBG::read(): Graph could not be loaded! Exit. (no segments in the GFA file)"]
    assert "run: reads" not in got.stderr
    assert [f for f in os.listdir(r) if not f.startswith("PloidyFrost_output")] == []     # nothing is left under an output name


def test_run_reads_returns_the_numbers_of_the_stderr_line(chain, tmp_path):
    r = cli("run", "-i", chain["reads"], "-o", "r", cwd=tmp_path)
    words = [l for l in r.stderr.splitlines() if l.startswith("run: reads ")][0].split()[1:]
    want = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    cwd = os.getcwd()
    os.makedirs(tmp_path / "api")
    os.chdir(tmp_path / "api")
    try:
        got = hostapi.run_reads(str(chain["reads"]), "r")
    finally:
        os.chdir(cwd)
    assert got == want and tuple(got) == hostapi.RUN_STATS_FIELDS
    assert calling_files(tmp_path / "api", "r") == calling_files(tmp_path, "r")
    assert got["windows_kept"] > 0 and got["unitigs_out"] > 0 and got["lower"] >= 10
