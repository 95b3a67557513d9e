"""K-COUNT (pf_count_* and pf_kmc_encode, csrc/pf_count.hip), the host streaming (hostapi.count_fastq), and the `count` and `mask -k`
sub-commands against the rule restated in Python (count_cases.py): every comparison is equality of the sorted (kmers, counts) and of all
eight statistics, and for the written database equality of its bytes with synth.write_kmc1's."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_case

import count_cases as cc
import mask_cases as mc

from ploidyfrost_amd import hipapi, hostapi, synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
TILE = 1024   # pf::MASK_TILE: window starts a block stages at once (plus a halo of 32 bytes)


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dip_reads():
    """300 seeded reads of dip20k (substitutions, Ns, lower case, both strands) and what the rule gives for them at ci = 1"""
    reads = mc.make_reads("dip20k", 300, seed=41)
    return reads, cc.ref_count(reads, 25, ci=1, cs=10000)


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)


def count_reads(d, reads, k, both_strands=True, initial_slots=0, calls=1, **cut):
    """the reads packed back to back through pf_count_reads (in `calls` calls) and pf_count_finish"""
    d.count_begin(k, both_strands, initial_slots)
    per = max((len(reads) + calls - 1) // calls, 1)
    for at in range(0, max(len(reads), 1), per):
        text, off, ln = mc.pack(reads[at:at + per])
        d.count_reads(text, off, ln)
    return d.count_finish(**dict(cc.DEFAULTS, **cut))


def same(got, want):
    assert got[2] == want[2]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
    return True


def check_reads(d, reads, k, both_strands=True, **kw):
    cut = {c: kw[c] for c in ("ci", "cx", "cs") if c in kw}
    want = cc.ref_count(reads, k, both_strands=both_strands, **cut)
    assert same(count_reads(d, reads, k, both_strands, **kw), want)
    return want


# ---- the kernels, through pf_count_reads ----

@pytest.mark.parametrize("k", [25, 31])
def test_read_lengths(dev, k):
    rng = np.random.default_rng(k)
    genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=3 * TILE))
    lengths = [0, 1, k - 1, k, k + 1, 150, TILE - 1, TILE, TILE + 1, TILE + k - 1, 2 * TILE + 40]
    for n in lengths:
        km, ct, st = check_reads(dev, [genome[5:5 + n]], k, ci=1)
        assert st["kmers"] == max(n - k + 1, 0) == st["written"] and st["kmers_bad"] == 0 and (ct == 1).all()   # a window that straddles a tile edge: once
    km, ct, st = check_reads(dev, [genome[5:5 + n] for n in lengths], k, ci=1)      # all of them packed, tile edges inside reads and between them
    assert ct.max() == len([n for n in lengths if n >= k])


def test_few_keys_every_lane_adds_to_the_same_slots(dev):
    km, ct, st = check_reads(dev, [b"A" * 2000, b"ACGT" * 500], 5, ci=1, cs=10000)
    assert len(km) == 3 and ct.tolist() == [1996, 998, 998]       # AAAAA; ACGTA (= TACGT); CGTAC (= GTACG)
    check_reads(dev, [b"A" * 2000, b"ACGT" * 500], 5, both_strands=False, ci=1)      # (-cs 255 caps the stored value of AAAAA)
    check_reads(dev, [b"ACG" * 700], 3, ci=1)                       # k = 3 is counted (no database can be written of it)


def test_strands(dev):
    rng = np.random.default_rng(3)
    read = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=200))
    km, ct, st = check_reads(dev, [read, mc.revcomp(read)], 25, ci=1)
    assert len(km) == 176 and (ct == 2).all()                        # one record of count 2 per k-mer canonically
    km, ct, st = check_reads(dev, [read, mc.revcomp(read)], 25, both_strands=False, ci=1)
    assert len(km) == 352 and (ct == 1).all()                        # two records with -b
    km, ct, st = check_reads(dev, [b"ACGCGT", b"TTACGCGTAA", b"acgcgt"], 6, ci=1)   # its own reverse complement: once per occurrence
    assert ct[km == 0b000110011011].tolist() == [3]


def test_n_lower_case_and_packed_reads(dev, dip_reads):
    reads, want = dip_reads
    assert want[2]["kmers_bad"] > 0
    assert same(count_reads(dev, reads, 25, ci=1, cs=10000), want)
    a, b = b"ACGTTGCAAGGCTTAACCGGATATCGCGA", b"GGATCCTTAAGCGCGTATATAGCTAGCTA"
    km, ct, st = check_reads(dev, [a, b], 25, ci=1)                  # back to back: no window across the boundary
    assert st["kmers"] == 10 and len(km) == 10
    km, ct, st = check_reads(dev, [a[:24], b[:24]], 25, ci=1)
    assert st["kmers"] == 0 and len(km) == 0
    check_reads(dev, [a[:12] + b"N" + a[13:], a.lower(), b"N" * 60], 5, ci=1)


def test_host_and_device_pointers_alignment_and_determinism(dev, dip_reads):
    reads, want = dip_reads
    text, off, ln = mc.pack(reads)
    results = []
    for mode in ("host", "device", "odd", "host"):
        dev.count_begin(25)
        if mode == "host":
            dev.count_reads(text, off, ln)
        else:
            shift = 1 if mode == "odd" else 0
            t = torch.zeros(len(text) + 16 + shift, dtype=torch.uint8, device="cuda")
            t[shift:shift + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
            o = torch.from_numpy(off.astype(np.int64)).cuda()
            n = torch.from_numpy(ln.astype(np.int32)).cuda()
            torch.cuda.synchronize()
            dev.count_reads(t[shift:shift + len(text)], o, n)
        results.append(dev.count_finish(ci=1, cs=10000))
    for r in results:
        assert same(r, want)
    assert results[0][0].tobytes() == results[3][0].tobytes() and results[0][1].tobytes() == results[3][1].tobytes()   # two runs: the same bits


def test_growth(dev, dip_reads):
    reads, want = dip_reads
    assert want[2]["unique"] > 5000
    assert same(count_reads(dev, reads, 25, initial_slots=64, calls=12, ci=1, cs=10000), want)     # several growths, the table full of keys each time
    assert same(count_reads(dev, reads, 25, initial_slots=64, calls=1, ci=1, cs=10000), want)
    assert same(count_reads(dev, reads, 25, initial_slots=100, calls=5, ci=1, cs=10000), want)     # rounded up to a power of two
    assert same(count_reads(dev, reads, 25, calls=7, ci=1, cs=10000), want)                        # default size, from the first call's bytes


def test_cutoffs(dev):
    rng = np.random.default_rng(5)
    unit = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=60)) for _ in range(8)]
    reads = [u for i, u in enumerate(unit) for _ in range(i + 1)]    # the k-mers of unit i occur i + 1 times
    for cut in (dict(ci=1), dict(ci=2), dict(ci=1, cx=5), dict(ci=1, cs=3), dict(ci=3, cx=6, cs=4), dict(ci=8, cx=8, cs=1)):
        km, ct, st = check_reads(dev, reads, 25, **cut)
        full = dict(cc.DEFAULTS, **cut)
        assert st["unique"] == 8 * 36 and st["below_min"] == (full["ci"] - 1) * 36 and st["above_max"] == max(8 - full["cx"], 0) * 36
        assert ct.max() == min(8, full["cx"], full["cs"])


def test_refusals(dev):
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_finish()
    assert e.value.status == hipapi.PF_ERR_ARG and "pf_count_finish" in str(e.value) and "pf_count_begin comes first" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_reads(b"ACGT" * 10, [0], [40])
    assert e.value.status == hipapi.PF_ERR_ARG and "pf_count_reads" in str(e.value)
    for k in (2, 32):
        with pytest.raises(hipapi.DeviceError) as e:
            dev.count_begin(k)
        assert e.value.status == hipapi.PF_ERR_ARG and "-k goes from 3 to 31" in str(e.value)
    dev.count_begin(25)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_begin(25)
    assert e.value.status == hipapi.PF_ERR_ARG and "a count is open already" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:                      # the table of reads is checked as pf_mask_reads checks it
        dev.count_reads(b"ACGT" * 10, [0, 30], [35, 10])
    assert "read 0 lies outside the text or overlaps the next one" in str(e.value)
    for kw, word in ((dict(ci=0), "-ci is below 1"), (dict(ci=6, cx=5), "-ci is above -cx"), (dict(cs=0), "-cs is below 1"), (dict(cx=1 << 32), "4294967295")):
        with pytest.raises(hipapi.DeviceError) as e:
            dev.count_finish(**dict(cc.DEFAULTS, **kw))
        assert e.value.status == hipapi.PF_ERR_ARG and word in str(e.value)
    dev.count_reads(b"ACGT" * 10, [0], [40])                          # the count is still open and nothing of the refused call was counted
    km, ct, st = dev.count_finish(ci=1)
    assert st["reads"] == 1 and st["kmers"] == 16 and ct.sum() == 16
    dev.count_begin(25)
    dev.count_abort()
    dev.count_abort()                                                 # without a count: nothing to do
    dev.count_begin(25)
    dev.count_abort()


def test_kernel_is_timed_under_its_name(dev, dip_reads):
    reads, _ = dip_reads
    assert dev.L.pf_kernel_name(hipapi.K_COUNT) == b"k_count" and hipapi.KERNELS[-1] == "k_call_model"
    text, off, ln = mc.pack(reads[:100])
    dev.enable_timing(True)
    dev.reset_timing()
    dev.count_begin(25)
    st = dev.count_reads(text, off, ln)
    ms, launches = dev.kernel_time(hipapi.K_COUNT)
    units = dev.kernel_units(hipapi.K_COUNT)
    dev.enable_timing(False)
    dev.count_abort()
    assert launches == 1 and ms > 0 and units == st["kmers"] > 0


# ---- FASTQ, through pf_count_fastq ----

def fastq_in_chunks(d, text, size, k=25, **cut):
    """the text fed in chunks of `size` bytes with the carry, as the host layer feeds it"""
    d.count_begin(k)
    carry, at, reads = b"", 0, 0
    while at < len(text) or carry:
        block = text[at:at + size]
        at += len(block)
        chunk = carry + block
        used, st = d.count_fastq(chunk, final=at >= len(text))
        reads += st["reads"]
        carry = chunk[used:]
        if at >= len(text):
            assert used == len(chunk)
            break
    got = d.count_finish(**dict(cc.DEFAULTS, **cut))
    assert got[2]["reads"] == reads
    return got


def test_fastq_chunks_line_ends_and_last_line(dev, dip_reads):
    reads, want = dip_reads
    for text in (mc.fastq(reads), mc.fastq(reads, crlf=True), mc.fastq(reads, last_newline=False),
                 mc.fastq(reads[:100]) + mc.fastq(reads[100:], crlf=True, last_newline=False, quals={101: b"@" + b"I" * (len(reads[101]) - 1)})):
        assert same(fastq_in_chunks(dev, text, len(text), ci=1, cs=10000), want)
        assert same(fastq_in_chunks(dev, text, 1000, ci=1, cs=10000), want)
    dev.count_begin(25)
    assert dev.count_fastq(b"", final=True)[0] == 0
    km, ct, st = dev.count_finish()
    assert len(km) == 0 and st == dict.fromkeys(cc.STATS, 0)


@pytest.mark.parametrize("name,record,damage", [
    ("does not start with '@'", 7, lambda L: L.__setitem__(28, b"x" + L[28][1:])),
    ("does not start with '+'", 3, lambda L: L.__setitem__(14, b"-")),
    ("quality line's length", 11, lambda L: L.__setitem__(47, L[47][:-1])),
    ("not a multiple of four", 20, lambda L: L.__setitem__(slice(-1, None), [b"@extra", b"ACGT", b""])),
])
def test_fastq_refusals_count_nothing(dev, dip_reads, name, record, damage):
    reads, _ = dip_reads
    lines = mc.fastq(reads[:20]).split(b"\n")
    damage(lines)
    dev.count_begin(25)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_fastq(b"\n".join(lines))
    assert e.value.status == hipapi.PF_ERR_ARG and e.value.bad_record == record
    assert "pf_count_fastq: record %d of the chunk: " % record in str(e.value) and name in str(e.value)
    km, ct, st = dev.count_finish(ci=1)          # nothing counted from the refused chunk
    assert len(km) == 0 and st["reads"] == 0 and st["unique"] == 0


# ---- the encoder, through pf_kmc_encode ----

@pytest.mark.parametrize("k,cs", [(25, 10000), (31, 255), (5, 1 << 24), (6, 70000)])
def test_kmc_encode_is_the_inverse_of_kmc_decode(dev, dip_reads, tmp_path, k, cs):
    reads, _ = dip_reads
    kmers, counts, _ = cc.ref_count(reads, k, ci=1, cs=cs)
    p, cb = synth.lut_prefix_len(k), cc.counter_bytes(10 ** 9, cs)
    rec, lut = dev.kmc_encode(kmers, counts, k, p, cb)
    pre, suf = cc.kmc1_bytes(tmp_path, kmers, counts, k, ci=1, cs=cs)
    assert b"KMCS" + rec.tobytes() + b"KMCS" == suf
    assert lut[-1] == len(kmers) and pre[4:4 + 8 * len(lut)] == lut.tobytes()
    km2, ct2 = dev.kmc_decode(rec, len(kmers), (k - p) // 4, cb, lut, p, k)
    assert np.array_equal(km2, kmers) and np.array_equal(ct2, counts)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.kmc_encode(kmers, counts, k, p + 1, cb)
    assert e.value.status == hipapi.PF_ERR_ARG and "pf_kmc_encode" in str(e.value)


# ---- the host layer and the sub-command ----

@pytest.fixture(scope="module")
def reads_file(tmp_path_factory):
    """1 500 reads, with CRLF records in the middle and no newline at the end, and the rule's answer at kmc's -ci1 -cs10000"""
    d = tmp_path_factory.mktemp("count_reads")
    reads = mc.make_reads("dip20k", 1500, seed=42)
    text = mc.fastq(reads[:500]) + mc.fastq(reads[500:1000], crlf=True, name=b"c") + mc.fastq(reads[1000:], last_newline=False, name=b"t")
    path = d / "reads.fq"
    path.write_bytes(text)
    return dict(dir=d, path=str(path), text=text, reads=reads, want=cc.ref_count(reads, 25, ci=1, cs=10000), record=len(mc.fastq(reads[:1])))


def database_equals(prefix, tmp_path, want, k, both_strands=True, **cut):
    full = dict(cc.DEFAULTS, **cut)
    pre, suf = cc.kmc1_bytes(tmp_path, want[0], want[1], k, both_strands, **full)
    with open(prefix + ".kmc_pre", "rb") as f:
        assert f.read() == pre
    with open(prefix + ".kmc_suf", "rb") as f:
        assert f.read() == suf
    km, ct, meta = synth.read_kmc1(prefix)
    assert np.array_equal(km, want[0]) and np.array_equal(ct, want[1])
    assert (meta["k"], meta["min_count"], meta["max_count"], meta["both_strands"]) == (k, full["ci"], full["cx"], both_strands)
    return True


def test_host_streaming_chunk_sizes(reads_file, tmp_path):
    f = reads_file
    db = str(tmp_path / "db")
    for chunk in (0, 4096, f["record"], f["record"] - 1, 100_000):   # one chunk; many; one record; one byte less (no whole record: the chunk grows)
        st = hostapi.count_fastq([f["path"]], db, ci=1, cs=10000, chunk_bytes=chunk, initial_slots=0 if chunk else 64)
        assert st == f["want"][2], chunk
        assert database_equals(db, tmp_path, f["want"], 25, ci=1, cs=10000)
        assert sorted(os.listdir(tmp_path)) == ["db.kmc_pre", "db.kmc_suf", "want_db.kmc_pre", "want_db.kmc_suf"]


@pytest.mark.parametrize("k,both,cut", [(25, True, dict()), (31, True, dict(ci=1, cs=3)), (31, False, dict(ci=1, cx=5, cs=70000)), (25, False, dict(ci=2, cx=7))])
def test_database_bytes_and_header(reads_file, tmp_path, k, both, cut):
    f = reads_file
    want = cc.ref_count(f["reads"], k, both_strands=both, **cut)
    db = str(tmp_path / "db")
    assert hostapi.count_fastq(f["path"], db, k=k, both_strands=both, **cut) == want[2]
    assert database_equals(db, tmp_path, want, k, both, **cut)
    size = os.path.getsize(db + ".kmc_suf")
    assert size == 8 + len(want[0]) * ((k - synth.lut_prefix_len(k)) // 4 + cc.counter_bytes(dict(cc.DEFAULTS, **cut)["cx"], dict(cc.DEFAULTS, **cut)["cs"]))


def test_cli_two_inputs_hist_and_the_stderr_line(reads_file, tmp_path):
    f = reads_file
    second = tmp_path / "second.fq"
    reads2 = mc.make_reads("dip20k", 200, seed=43)
    second.write_bytes(mc.fastq(reads2))
    both = tmp_path / "both.fq"
    both.write_bytes(f["text"] + b"\n" + mc.fastq(reads2))
    want = cc.ref_count(f["reads"] + reads2, 25, ci=1, cs=10000)
    r = run_cli("count", "-k25", "-ci1", "-cs10000", "-i", f["path"], "-i", second, "-o", tmp_path / "two", "--hist", tmp_path / "two.hist", "--chunk-bytes", 50_000)
    assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
    assert r.stderr == "count: reads %d bases %d kmers %d bad %d unique %d below %d above %d written %d\n" % tuple(want[2][s] for s in cc.STATS)
    assert database_equals(str(tmp_path / "two"), tmp_path, want, 25, ci=1, cs=10000)
    one = run_cli("count", "-k", 25, "-ci", 1, "-cs", 10000, "-i", both, "-o", tmp_path / "one", "-v")     # two inputs equal their concatenation
    assert one.returncode == 0 and one.stderr.startswith(r.stderr) and "stream" in one.stderr and "finish" in one.stderr and "write" in one.stderr
    for ext in (".kmc_pre", ".kmc_suf"):
        assert (tmp_path / ("one" + ext)).read_bytes() == (tmp_path / ("two" + ext)).read_bytes()
    # --hist is byte for byte what `histogram -d` writes from the written database, by the product's own loader
    h = run_cli("histogram", "-d", tmp_path / "two", "-o", tmp_path / "again.hist")
    assert h.returncode == 0, h.stdout + h.stderr
    assert (tmp_path / "two.hist").read_bytes() == (tmp_path / "again.hist").read_bytes() == cc.histogram_text(want[1], 1, 10 ** 9, 10000)
    # defaults: -ci 2 -cs 255, one counter byte
    d = run_cli("count", "-i", f["path"], "-o", tmp_path / "dflt", "--hist", tmp_path / "dflt.hist")
    assert d.returncode == 0, d.stderr
    dflt = cc.ref_count(f["reads"], 25)
    assert database_equals(str(tmp_path / "dflt"), tmp_path, dflt, 25)
    assert (tmp_path / "dflt.hist").read_bytes() == cc.histogram_text(dflt[1], 2, 10 ** 9, 255) == run_cli("histogram", "-d", tmp_path / "dflt").stdout.encode()


@pytest.mark.parametrize("name,record", [("does not start with '@'", 1200), ("quality line's length", 700), ("not a multiple of four", 1500)])
def test_cli_format_refusals_count_records_from_the_start_of_the_file(reads_file, tmp_path, name, record):
    f = reads_file
    lines = f["text"].split(b"\n")
    if "multiple" in name:
        lines += [b"@extra", b"ACGT"]      # (the file had no newline at its end)
    elif "@" in name:
        lines[4 * record] = b"x" + lines[4 * record][1:]
    else:
        q = lines[4 * record + 3]
        lines[4 * record + 3] = q[:-2] + b"\r" if q.endswith(b"\r") else q[:-1]   # one quality byte less
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"\n".join(lines))
    for chunk in (4096, 1 << 20):
        r = run_cli("count", "-ci1", "-i", f["path"], "-i", bad, "-o", tmp_path / "db", "--hist", tmp_path / "h", "--chunk-bytes", chunk)
        assert r.returncode != 0 and r.stdout == ""
        assert "count: %s: record %d: " % (bad, record + 1) in r.stderr and name in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["bad.fq"]   # neither the database, nor the histogram, nor a temporary file


# ---- through the product ----

def test_counted_database_through_the_calling_run(tmp_path):
    """reads = every dip20k unitig once plus 500 seeded reads, counted with kmc's -ci1 -cs10000 of the workflow: the calling run over the
    graph with the counted database writes the twelve files of the run over synth.write_kmc1 of the Python counts"""
    case = load_case("dip20k")
    reads = mc.unitigs("dip20k") + mc.make_reads("dip20k", 500, seed=44)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(mc.fastq(reads))
    want = cc.ref_count(reads, 25, ci=1, cs=10000)
    assert hostapi.count_fastq(str(fq), str(tmp_path / "counted"), ci=1, cs=10000) == want[2]
    synth.write_kmc1(str(tmp_path / "python"), want[0], want[1], 25, counter_size=2, min_count=1, max_count=10 ** 9)
    outs = {}
    for name in ("counted", "python"):
        run = hostapi.Run(case["gfa"], str(tmp_path / name))
        run.set_output_dir(str(tmp_path / ("out_" + name)))
        run.set_unitig_id("g")
        run.find_superbubbles("g")
        run.ploidy_estimation("g", 1, 1000)
        run.close()
        outs[name] = {f: (tmp_path / ("out_" + name) / f).read_bytes() for f in sorted(os.listdir(tmp_path / ("out_" + name)))}
    assert len(outs["counted"]) == 12 and outs["counted"] == outs["python"]
    assert any(len(v) > 0 for v in outs["counted"].values())


# ---- mask -k against the two-command chain ----

@pytest.mark.parametrize("threshold", [("-l", 2), ("--auto-cutoffs",)])
def test_mask_k_equals_count_then_mask_d(reads_file, tmp_path, threshold):
    f = reads_file
    cut = ["-k", 25, "-ci", 1, "-cs", 10000]
    c = run_cli("count", *cut, "-i", f["path"], "-o", tmp_path / "db")
    assert c.returncode == 0, c.stderr
    chain = run_cli("mask", "-d", tmp_path / "db", "-i", f["path"], "-o", tmp_path / "chain.fq", *threshold, "-u", 40)
    assert chain.returncode == 0, chain.stderr
    one = run_cli("mask", *cut, "-i", f["path"], "-o", tmp_path / "one.fq", *threshold, "-u", 40)
    assert one.returncode == 0, one.stderr
    assert (one.stdout, one.stderr) == (chain.stdout, chain.stderr) and one.stderr.startswith("mask: reads 1500 ")
    assert (tmp_path / "one.fq").read_bytes() == (tmp_path / "chain.fq").read_bytes()
    if threshold[0] == "--auto-cutoffs":
        assert one.stdout == run_cli("cutoffL", "-d", tmp_path / "db").stdout and one.stdout.strip().isdigit()
    else:   # against the rule itself: the database is the Python counts
        db = mc.Database.from_arrays(f["want"][0], f["want"][1], 25, True, 1, 10 ** 9)
        want, st = mc.ref_mask_db(f["text"], db, 2, 40)
        assert (tmp_path / "one.fq").read_bytes() == want and st["kmers_bad"] > 0
        assert one.stderr == "mask: reads %d changed %d bases %d masked %d kmers %d bad %d\n" % tuple(st[s] for s in mc.STATS)
    # with --db-out the database is written as well, the same bytes
    two = run_cli("mask", *cut, "-i", f["path"], "-o", tmp_path / "two.fq", *threshold, "-u", 40, "--db-out", tmp_path / "db2", "--chunk-bytes", 30_000)
    assert two.returncode == 0 and (two.stdout, two.stderr) == (chain.stdout, chain.stderr), two.stderr
    assert (tmp_path / "two.fq").read_bytes() == (tmp_path / "chain.fq").read_bytes()
    for ext in (".kmc_pre", ".kmc_suf"):
        assert (tmp_path / ("db2" + ext)).read_bytes() == (tmp_path / ("db" + ext)).read_bytes()
    api = hostapi.mask_fastq_counted(f["path"], str(tmp_path / "api.fq"), ci=1, cs=10000, upper=40, **(dict(lower=2) if threshold[0] == "-l" else dict(auto=True)))
    assert (tmp_path / "api.fq").read_bytes() == (tmp_path / "chain.fq").read_bytes() and api["reads"] == 1500
