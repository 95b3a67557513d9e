"""K-TRIMCOUNT (pf_trim_table_fastq*, pf_count_fastq*_trimmed, pf_maskcount_fastq*_trimmed; csrc/pf_trimcount.hip) against "trim in
Python, then the existing reference on the trimmed reads", and `ploidyfrost run STEP...` / `run-multi STEP...` against the chains they
replace (`trim`, then `run` / `run-multi`).  Every comparison is exact: arrays of integers and bytes of files."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import count_cases as cc
import mask_cases as mc
import run_cases as rc
import trim_cases as tc
import trimrun_cases as trc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
WORKFLOW = tc.WORKFLOW


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def dev_tensor(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def same_table(got, want):
    assert got["n_reads"] == len(want["read_off"])
    assert np.asarray(got["read_off"]).tolist() == want["read_off"] and np.asarray(got["read_len"]).tolist() == want["read_len"]
    assert got["bytes_used"] == want["bytes_used"] and got["n_records"] == want["n_records"] and got["stats"] == want["stats"]


# ---- the table ----

def test_table_of_the_edge_records(dev):
    """lengths 0 .. 1000 at every alignment, and the five 70 000-base reads: the table and trim_fastq's statistics"""
    text = tc.fastq(tc.edge_records())
    for steps in (WORKFLOW, tc.ORDERS[2], ["LEADING:10", "TRAILING:10"]):
        want = trc.table(text, steps)
        assert len(want["read_off"]) > 20 and want["stats"]["dropped"] > 10
        same_table(dev.trim_table_fastq(text, steps), want)


def test_table_of_a_pair_and_pointers(dev):
    """the 400-record pair: both tables, per-file statistics; host pointers and device pointers give the same table"""
    t1, t2 = tc.fastq(tc.make_reads(400, 1)), tc.fastq(tc.make_reads(400, 2))
    want = trc.table_pair(t1, t2, WORKFLOW)
    assert all(x > 0 for x in trc.pair_outcomes(t1, t2, WORKFLOW))
    got = dev.trim_table_fastq_pair(t1, t2, WORKFLOW)
    assert got["n_reads"] == len(want["read_off"][0]) == want["stats"][0]["both"]
    for f in range(2):
        assert got["read_off"][f].tolist() == want["read_off"][f] and got["read_len"][f].tolist() == want["read_len"][f]
    assert got["bytes_used"] == want["bytes_used"] and got["n_records"] == 400 and got["stats"] == want["stats"]
    n = got["n_reads"]
    off = [torch.zeros(401, dtype=torch.int64, device="cuda") for _ in range(2)]
    ln = [torch.zeros(401, dtype=torch.int32, device="cuda") for _ in range(2)]
    on_dev = dev.trim_table_fastq_pair(dev_tensor(t1), dev_tensor(t2), WORKFLOW, read_off=off, read_len=ln)
    assert on_dev["n_reads"] == n and on_dev["stats"] == got["stats"]
    for f in range(2):
        assert off[f][:n].cpu().numpy().tolist() == want["read_off"][f] and ln[f][:n].cpu().numpy().tolist() == want["read_len"][f]
    single = trc.table(t1, WORKFLOW)
    o1, l1 = torch.zeros(401, dtype=torch.int64, device="cuda"), torch.zeros(401, dtype=torch.int32, device="cuda")
    g1 = dev.trim_table_fastq(dev_tensor(t1), WORKFLOW, read_off=o1, read_len=l1)
    assert o1[:g1["n_reads"]].cpu().numpy().tolist() == single["read_off"] and l1[:g1["n_reads"]].cpu().numpy().tolist() == single["read_len"]
    same_table(dev.trim_table_fastq(t1, WORKFLOW), single)


def test_every_record_dropped_counts_nothing(dev):
    text = tc.fastq(tc.make_reads(300, 5))
    steps = ["MINLEN:100000"]
    got = dev.trim_table_fastq(text, steps)
    assert got["n_reads"] == 0 and got["n_records"] == 300 and got["stats"]["dropped"] == 300 and got["bytes_used"] == len(text)
    dev.count_begin(25, True)
    used, ts, st = dev.count_fastq_trimmed(text, steps)
    kmers, _, fin = dev.count_finish(**rc.EVERY)
    assert used == len(text) and ts["reads"] == 300 and ts["kept"] == 0
    assert (st["reads"], st["bases"], st["kmers"]) == (0, 0, 0) and len(kmers) == 0 and fin["kmers"] == 0


def test_pair_chunks_with_different_record_counts(dev):
    """not final, file 1 holds more whole records than file 2: bytes_used per file as pf_trim_fastq_pair gives it"""
    r1, r2 = tc.make_reads(60, 11), tc.make_reads(60, 12)
    t1 = tc.fastq(r1[:50]) + b"@cut\nACG"
    t2 = tc.fastq(r2[:37]) + b"@cut\nACGT\n+\nII"
    want = trc.table_pair(t1, t2, WORKFLOW, final=False)
    assert want["n_records"] == 37 and want["bytes_used"] == [len(tc.fastq(r1[:37])), len(tc.fastq(r2[:37]))]
    got = dev.trim_table_fastq_pair(t1, t2, WORKFLOW, final=False)
    trim = dev.trim_fastq_pair(t1, t2, WORKFLOW, final=False)
    assert got["bytes_used"] == want["bytes_used"] == trim["bytes_used"] and got["n_records"] == 37 and got["stats"] == want["stats"] == trim["stats"]
    for f in range(2):
        assert got["read_off"][f].tolist() == want["read_off"][f] and got["read_len"][f].tolist() == want["read_len"][f]


# ---- count ----

def stream(pieces, call):
    """the pieces as chunks with the carry in front of each; call(chunk, final) -> bytes_used"""
    carry = b""
    for i, p in enumerate(pieces):
        chunk = carry + p
        carry = chunk[call(chunk, i == len(pieces) - 1):]
    assert carry == b""


def add(total, st):
    for f in st:
        total[f] = total.get(f, 0) + st[f]


def count_trimmed(d, k, pieces, steps, phred=33):
    d.count_begin(k, True)
    ts, st = {}, {}
    try:
        def call(chunk, final):
            used, a, b = d.count_fastq_trimmed(chunk, steps, phred, final)
            add(ts, a)
            add(st, b)
            return used
        stream(pieces, call)
    except Exception:
        d.count_abort()
        raise
    kmers, counts, fin = d.count_finish(**rc.EVERY)
    return kmers, counts, ts, st, fin


def check_count(d, text, steps, k, chunks=True):
    want = trc.table(text, steps)
    wk, wc, wst = cc.ref_count(want["reads"], k, both_strands=True, **rc.EVERY)
    # the device composition: K-TRIM into a device buffer, K-COUNT on it
    out = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
    t = d.trim_fastq(dev_tensor(text), steps, out=out)
    d.count_begin(k, True)
    _, cst = d.count_fastq(t["out"]) if len(t["out"]) else (0, dict.fromkeys(hipapi.COUNT_STATS.names, 0))
    ck, ccnt, _ = d.count_finish(**rc.EVERY)
    assert np.array_equal(ck, wk) and np.array_equal(ccnt, wc)
    for pieces in ([text], trc.cut3(text)) if chunks else ([text],):
        kmers, counts, ts, st, fin = count_trimmed(d, k, pieces, steps)
        assert np.array_equal(kmers, wk) and np.array_equal(counts, wc), (len(kmers), len(wk), len(pieces))
        assert ts == want["stats"]
        assert {f: st[f] for f in ("reads", "bases", "kmers", "kmers_bad")} == {f: wst[f] for f in ("reads", "bases", "kmers", "kmers_bad")}
        assert {f: st[f] for f in ("reads", "bases", "kmers", "kmers_bad")} == {f: cst[f] for f in ("reads", "bases", "kmers", "kmers_bad")}
        assert fin["kmers"] == wst["kmers"] and fin["written"] == len(wk)
    return wk, wc, wst


@pytest.mark.parametrize("k", [25, 3])
def test_count_against_trim_then_count(dev, k):
    """reads cut from a short genome (counts above 1, Ns, lower case) with make_reads' quality shapes: against the Python composition,
    against K-TRIM + K-COUNT on the device, one call against three chunks"""
    recs = trc.genome_reads(500, 21)
    text = tc.fastq(recs)
    assert min(tc.outcome_shares(recs)) > 0.05          # dropped, whole, b > 0, e < n are all there
    wk, wc, wst = check_count(dev, text, WORKFLOW, k)
    assert int(wc.max()) > 1 and wst["kmers_bad"] > 0
    check_count(dev, tc.fastq(trc.genome_reads(200, 22), crlf=True, last_newline=False), tc.ORDERS[2], k, chunks=False)


@pytest.mark.parametrize("k", [25, 3])
def test_trimmed_lengths_around_k(dev, k):
    """a read trimmed to k - 1, k and k + 1 bases gives 0, 1 and 2 windows"""
    rng = np.random.default_rng(k)
    for n, windows in ((k - 1, 0), (k, 1), (k + 1, 2)):
        seq = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=n + 60))
        text = tc.fastq([trc.one_read(seq, low_head=40, low_tail=20)])
        kmers, counts, ts, st, fin = count_trimmed(dev, k, [text], ["LEADING:10", "TRAILING:10"])
        assert ts["bases_kept"] == n and st["reads"] == 1 and st["bases"] == n and st["kmers"] == windows == int(counts.sum())
        wk, wc, _ = cc.ref_count([seq[40:40 + n]], k, **rc.EVERY)
        assert np.array_equal(kmers, wk) and np.array_equal(counts, wc)


@pytest.mark.parametrize("b", [1023, 1024])
@pytest.mark.parametrize("e", [2048, 2049])
def test_tile_and_row_step_edges(dev, b, e):
    """one read of 3 000 bases with a low-quality head of b and a tail from e on, under LEADING / TRAILING alone: K-COUNT's 1024-byte
    tile edges and K-TRIM's 256-byte row steps; in front of it a short record so that the line starts at no aligned byte"""
    rng = np.random.default_rng(b * 7 + e)
    seq = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=3000))
    for lead in (b"", b"p" * 7):
        text = tc.fastq([(b"r" + lead, seq, tc.qline([2] * b + [40] * (e - b) + [2] * (3000 - e)))])
        want = trc.table(text, ["LEADING:10", "TRAILING:10"])
        assert want["read_len"] == [e - b] and want["reads"] == [seq[b:e]]
        same_table(dev.trim_table_fastq(text, ["LEADING:10", "TRAILING:10"]), want)
        _, _, wst = check_count(dev, text, ["LEADING:10", "TRAILING:10"], 25, chunks=False)
        assert wst["kmers"] == e - b - 24


def test_count_pair_counts_the_both_kept_reads(dev):
    t1, t2 = tc.fastq(trc.genome_reads(300, 31, genome_seed=3)), tc.fastq(trc.genome_reads(300, 32, genome_seed=3))
    want = trc.table_pair(t1, t2, WORKFLOW)
    assert all(x > 0 for x in trc.pair_outcomes(t1, t2, WORKFLOW))
    for k in (25, 3):
        wk, wc, wst = cc.ref_count(want["reads"][0] + want["reads"][1], k, **rc.EVERY)
        for a, b in ((t1, t2), (dev_tensor(t1), dev_tensor(t2))):
            dev.count_begin(k, True)
            used, ts, st = dev.count_fastq_pair_trimmed(a, b, WORKFLOW)
            kmers, counts, fin = dev.count_finish(**rc.EVERY)
            assert used == [len(t1), len(t2)] and ts == want["stats"]
            assert np.array_equal(kmers, wk) and np.array_equal(counts, wc)
            assert {f: st[f] for f in ("reads", "bases", "kmers", "kmers_bad")} == {f: wst[f] for f in ("reads", "bases", "kmers", "kmers_bad")}
            assert st["reads"] == 2 * want["stats"][0]["both"]


# ---- maskcount ----

def maskcount_trimmed(d, k, pieces, steps, low, up=mc.NO_UPPER):
    d.count_begin(k, True)
    ts, st = {}, {}
    try:
        def call(chunk, final):
            used, a, b = d.maskcount_fastq_trimmed(chunk, steps, low, up, final=final)
            add(ts, a)
            add(st, b)
            return used
        stream(pieces, call)
    except Exception:
        d.count_abort()
        raise
    kmers, counts, fin = d.count_finish(**rc.EVERY)
    return kmers, counts, ts, st, fin


def check_maskcount(d, db, text, steps, low, up=mc.NO_UPPER, chunks=False):
    """against run_cases.composition on the trimmed table (mask in Python, count in Python) and the host restatement's statistics"""
    want = trc.table(text, steps)
    tab = list(zip(want["read_off"], want["read_len"]))
    wk, wc, _, _ = rc.composition(text, tab, db, low, up)
    hk, hc, hst = hostapi.count_masked_host(text, want["read_off"], want["read_len"], db.k, rc.flat_counters(text, tab, db), low, up)
    assert np.array_equal(hk, wk) and np.array_equal(hc, wc)
    for pieces in ([text], trc.cut3(text)) if chunks else ([text],):
        kmers, counts, ts, st, fin = maskcount_trimmed(d, db.k, pieces, steps, low, up)
        assert np.array_equal(kmers, wk) and np.array_equal(counts, wc), (len(kmers), len(wk), len(pieces))
        assert ts == want["stats"] and st == hst
    return wk, wc, hst


def covered_genome(seed, n=150, copies=20):
    rng = np.random.default_rng(seed)
    genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=n))
    return genome, [genome] * copies


def substituted(seq, at):
    return seq[:at] + bytes([b"ACGT"[(b"ACGT".index(seq[at]) + 1) % 4]]) + seq[at + 1:]


@pytest.mark.parametrize("side", ["tail", "head"])
def test_an_error_in_the_trimmed_off_part_masks_nothing(dev, side):
    """a 150-base read of a genome covered many times, with a substitution inside its low-quality tail (base 140, quality 2 from base
    120 on, TRAILING:10) or head (base 5, quality 2 up to base 30, LEADING:10).  The windows over the substitution have count 1 < low,
    but they start in the trimmed-off part: they are no windows.  All 96 windows of the kept 120 bases are counted."""
    k, low = 25, 2
    genome, clean = covered_genome(77)
    if side == "tail":
        rec, steps, kept = trc.one_read(substituted(genome, 140), low_tail=30), ["TRAILING:10"], genome[:120]
    else:
        rec, steps, kept = trc.one_read(substituted(genome, 5), low_head=30), ["LEADING:10"], genome[30:]
    text = tc.fastq([rec])
    assert trc.table(text, steps)["reads"] == [kept]
    db = rc.database_of(clean + [kept], k)            # the table of the trimmed reads' own counts, as `run` uploads it
    db.upload(dev)
    kmers, counts, hst = check_maskcount(dev, db, text, steps, low)
    assert hst["kmers"] == 96 and hst["kmers_bad"] == 0 and hst["kmers_kept"] == 96 == int(counts.sum()) and hst["reads"] == 1 and hst["bases"] == 120


def test_a_bad_window_at_the_last_start_kills_k_starts_and_no_more(dev):
    """the window at start e - k of the trimmed read is genuinely bad: the starts e - 2k + 1 .. e - k die, nothing else"""
    k, e = 25, 120
    genome, db = mc.synthetic(5, 150, k, weak=(e - k,))
    db.upload(dev)
    text = tc.fastq([trc.one_read(genome, low_tail=150 - e)])
    kmers, counts, hst = check_maskcount(dev, db, text, ["TRAILING:10"], 10)
    assert hst["kmers"] == e - k + 1 and hst["kmers_bad"] == 1 and hst["kmers_kept"] == e - 2 * k + 1 == len(kmers)
    fw, rv = hipapi_keys(genome, k)
    have = set(kmers.tolist())
    for p in range(150 - k + 1):
        assert (int(min(fw[p], rv[p])) in have) == (p < e - 2 * k + 1), p


def hipapi_keys(seq, k):
    from ploidyfrost_amd import synth
    return synth.kmers_u64(mc._CODE[np.frombuffer(seq, dtype=np.uint8)], k)


def test_maskcount_random_reads_thresholds_and_chunks(dev):
    k = 25
    text = tc.fastq(trc.genome_reads(400, 41, **trc.DEEP))
    db = rc.database_of(trc.table(text, WORKFLOW)["reads"], k)
    db.upload(dev)
    mid = trc.mid_count(db.counts)
    assert mid > 2
    for low, up in ((0, mc.NO_UPPER), (mid, mc.NO_UPPER), (1, mid)):
        _, _, hst = check_maskcount(dev, db, text, WORKFLOW, low, up, chunks=(low == mid))
    assert hst["kmers_bad"] > 0 and hst["kmers_kept"] > 0 and hst["kmers_invalid"] > 0


def test_maskcount_pair(dev):
    k = 25
    t1, t2 = tc.fastq(trc.genome_reads(300, 51, genome_seed=5, **trc.DEEP)), tc.fastq(trc.genome_reads(300, 52, genome_seed=5, **trc.DEEP))
    want = trc.table_pair(t1, t2, WORKFLOW)
    db = rc.database_of(want["reads"][0] + want["reads"][1], k)
    db.upload(dev)
    low = trc.mid_count(db.counts)
    parts = [rc.composition(t, list(zip(want["read_off"][f], want["read_len"][f])), db, low)[2] for f, t in enumerate((t1, t2))]
    masked_reads = [parts[f][o:o + n] for f in range(2) for o, n in zip(want["read_off"][f], want["read_len"][f])]
    wk, wc, _ = cc.ref_count(masked_reads, k, **rc.EVERY)
    dev.count_begin(k, True)
    used, ts, st = dev.maskcount_fastq_pair_trimmed(t1, t2, WORKFLOW, low)
    kmers, counts, _ = dev.count_finish(**rc.EVERY)
    assert used == [len(t1), len(t2)] and ts == want["stats"]
    assert np.array_equal(kmers, wk) and np.array_equal(counts, wc) and len(wk) > 100
    assert st["reads"] == 2 * want["stats"][0]["both"] and st["kmers_kept"] == int(wc.sum()) and st["kmers_bad"] > 0


# ---- timing, refusals ----

def test_one_call_is_one_launch_of_k_trimcount(dev):
    text = tc.fastq(trc.genome_reads(100, 61))
    db = rc.database_of(trc.table(text, WORKFLOW)["reads"], 25)
    db.upload(dev)
    dev.enable_timing(True)
    try:
        for call in (lambda: dev.count_fastq_trimmed(text, WORKFLOW), lambda: dev.maskcount_fastq_trimmed(text, WORKFLOW, 2),
                     lambda: dev.count_fastq_trimmed(text + b"@half\nACGT\n", WORKFLOW, final=False)):
            dev.reset_timing()
            dev.count_begin(25, True)
            call()
            dev.count_abort()
            ms, launches = dev.kernel_time(hipapi.K_TRIMCOUNT)
            assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_TRIMCOUNT) == 100
            for other in (hipapi.K_TRIM, hipapi.K_COUNT, hipapi.K_MASKCOUNT):
                assert dev.kernel_time(other)[1] == 0
        assert dev.L.pf_kernel_name(hipapi.K_TRIMCOUNT) == b"k_trimcount"
    finally:
        dev.enable_timing(False)


def test_refusals_by_name():
    d = hipapi.Device(0)
    try:
        text = tc.fastq([(b"a", b"ACGTACGTAC", b"IIIIIIIIII")])
        with pytest.raises(hipapi.DeviceError, match="pf_count_fastq_trimmed: no count is open"):
            d.count_fastq_trimmed(text, WORKFLOW)
        with pytest.raises(hipapi.DeviceError, match="pf_count_fastq_pair_trimmed: no count is open"):
            d.count_fastq_pair_trimmed(text, text, WORKFLOW)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_trimmed: no count table is resident"):
            d.maskcount_fastq_trimmed(text, WORKFLOW, 1)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_pair_trimmed: no count table is resident"):
            d.maskcount_fastq_pair_trimmed(text, text, WORKFLOW, 1)
        _, db = mc.synthetic(2, 100, 25)
        db.upload(d)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_trimmed: no count is open"):
            d.maskcount_fastq_trimmed(text, WORKFLOW, 1)
        d.count_begin(21, True)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_trimmed: the open count's k = 21 differs from the count table's k = 25"):
            d.maskcount_fastq_trimmed(text, WORKFLOW, 1)
        d.count_abort()
        d.count_begin(25, False)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_trimmed: the open count is not on both strands"):
            d.maskcount_fastq_trimmed(text, WORKFLOW, 1)
        d.count_abort()
        d.count_begin(25, True)
        with pytest.raises(hipapi.DeviceError, match="pf_maskcount_fastq_trimmed: low 5 is above up 4"):
            d.maskcount_fastq_trimmed(text, WORKFLOW, 5, 4)
        with pytest.raises(hipapi.DeviceError, match="pf_count_fastq_trimmed: no step is given"):
            d.count_fastq_trimmed(text, [])
        with pytest.raises(hipapi.DeviceError, match="pf_count_fastq_trimmed: the quality offset is 33 or 64, not 50"):
            d.count_fastq_trimmed(text, WORKFLOW, phred=50)
        with pytest.raises(hipapi.DeviceError, match="pf_trim_table_fastq: step 1: a value of the step is out of range"):
            d.trim_table_fastq(text, [(hipapi.TRIM_KINDS["LEADING"], 10), (hipapi.TRIM_KINDS["TRAILING"], 94)])
        with pytest.raises(hipapi.DeviceError, match="pf_trim_table_fastq_pair: more than 8 steps"):
            d.trim_table_fastq_pair(text, text, ["MINLEN:1"] * 9)
        with pytest.raises(hipapi.DeviceError, match="pf_count_fastq_pair_trimmed: the final chunks hold different numbers of records") as e:
            d.count_fastq_pair_trimmed(text + text, text, WORKFLOW)
        assert e.value.bad_record == 2 * 1 + 1
        kmers, _, st = d.count_finish(**rc.EVERY)
        assert len(kmers) == 0 and st["kmers"] == 0 and st["reads"] == 0          # nothing was counted from the refused calls
    finally:
        d.close()


def test_a_format_error_counts_nothing(dev):
    recs = trc.genome_reads(20, 71)
    text = tc.fastq(recs)
    lines = text.split(b"\n")
    bad = b"\n".join(lines[:8] + [lines[8][1:]] + lines[9:])      # the third record's first line loses its '@'
    dev.count_begin(25, True)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_fastq_trimmed(bad, WORKFLOW)
    assert e.value.bad_record == 2 and "does not start with '@'" in str(e.value) and "pf_count_fastq_trimmed: record 2 of the chunk" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.count_fastq_pair_trimmed(text, bad, WORKFLOW)
    assert e.value.bad_record == 2 * 2 + 1 and "pf_count_fastq_pair_trimmed: file 2: record 2 of the chunk" in str(e.value)
    kmers, _, st = dev.count_finish(**rc.EVERY)
    assert len(kmers) == 0 and st["reads"] == 0


# ---- `ploidyfrost run STEP...` against the chain it replaces: `trim`, then `run` ----

GOLDEN = os.path.join(ROOT, "tests", "golden")
DEPTH = 64   # see chain()
MODEL = ["--model", "fre"]


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def seeded_quality(rng, n):
    """most reads flat 'I', about a quarter with a tail that degrades from a random cut, a few per cent low throughout"""
    x = rng.random()
    if x < 0.04:
        return "#" * n
    if x < 0.29:
        cut = int(rng.integers(30, n))
        return "I" * cut + "".join(chr(33 + int(q)) for q in rng.integers(2, 25, size=n - cut))
    return "I" * n


def write_fastq(path, reads, rng):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, seeded_quality(rng, len(r))))


def untimed(stdout):
    """stdout without the calling run's lines of measured times (they differ from run to run)"""
    return [l for l in stdout.splitlines() if " time " not in l]


def lines_with(text, word):
    return [l for l in text.splitlines() if l.startswith(word)]


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def read(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The reads of test_gpu_run.py's generator (build_k25: genome 1600, reads of 100) at depth 64, qualities seeded, even records to
    r1.fq, odd ones to r2.fq; then the chain per case: `trim`, then `run` on the trimmed files.  paired: `trim -1 -2 -o1 -u1 -o2 -u2`
    and `run -i o1 -i o2`; single: `trim -i r1 -i r2 -o t.fq` and `run -i t.fq`; keep: the paired one with --keep-tips --keep-isolated.
    Depth 64 is the first depth tried (test_gpu_run.py measured 22 rows at depth 48 untrimmed; trimming lowers the depth).  Measured
    with it: L = 10; paired 405 of 512 pairs kept whole (53 / 49 / 5 forward only, reverse only, neither), 18 rows of
    allele_frequency.txt; single-ended 912 of 1024 reads kept, 22 rows.  The tests print L and the row count and ask for at least 5."""
    root = tmp_path_factory.mktemp("trimchain")
    gen = generator("make_build_golden")
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    rng = np.random.default_rng(2025)
    write_fastq(root / "r1.fq", reads[0::2], rng)
    write_fastq(root / "r2.fq", reads[1::2], rng)
    out = {"r1": root / "r1.fq", "r2": root / "r2.fq"}
    for tag, extra in (("paired", []), ("single", []), ("keep", ["--keep-tips", "--keep-isolated"])):
        d = root / tag
        d.mkdir()
        if tag == "single":
            t = cli("trim", "-i", out["r1"], "-i", out["r2"], "-o", d / "t.fq", *WORKFLOW, cwd=d)
            inputs = ["-i", d / "t.fq"]
        else:
            t = cli("trim", "-1", out["r1"], "-2", out["r2"], "-o1", d / "o1.fq", "-u1", d / "u1.fq", "-o2", d / "o2.fq", "-u2", d / "u2.fq", *WORKFLOW, cwd=d)
            inputs = ["-i", d / "o1.fq", "-i", d / "o2.fq"]
        r = cli("run", *inputs, "-o", "s", *MODEL, "--db-out", d / "db", "--gfa-out", d / "s", *extra, cwd=d)
        out[tag] = dict(dir=d, trim=lines_with(t.stderr, "trim: "), run=lines_with(r.stderr, "run: reads "), L=r.stdout.splitlines()[0], stdout=r.stdout)
    raw = root / "raw"
    raw.mkdir()
    cli("run", "-i", out["r1"], "-i", out["r2"], "-o", "s", "--db-out", raw / "db", cwd=raw)
    out["raw"] = raw
    return out


@pytest.mark.parametrize("name,tag,inputs,extra", [
    ("paired", "paired", "pair", []), ("paired_chunk_carries", "paired", "pair", ["--chunk-bytes", 4096]),
    ("single", "single", "single", []), ("paired_keep", "keep", "pair", ["--keep-tips", "--keep-isolated"])])
def test_run_with_steps_against_the_chain(chain, tmp_path, name, tag, inputs, extra):
    c = chain[tag]
    want = calling_files(c["dir"], "s")
    rows = want["_allele_frequency.txt"].decode().splitlines()
    print("chain %s: L = %s, %d calling files, %d lines in allele_frequency.txt; %s" % (tag, c["L"], len(want), len(rows), c["trim"]))
    assert len(rows) >= 5, rows[:3]          # (the file has no header line) the comparison is not vacuous
    assert len([f for f in want if f != "_model_result.txt"]) == 12 and "_model_result.txt" in want
    # the trimming did something of every kind, and what it did reaches the counters
    words = chain["paired"]["trim"][0].split()
    t = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    assert t["forward_only"] > 0 and t["reverse_only"] > 0 and t["dropped"] > 0 and t["both"] > 0 and t["bases_kept"] < t["bases"]
    assert read(str(c["dir"] / "db") + ".kmc_suf") != read(str(chain["raw"] / "db") + ".kmc_suf")
    files = ["-1", chain["r1"], "-2", chain["r2"]] if inputs == "pair" else ["-i", chain["r1"], "-i", chain["r2"]]
    r = cli("run", *files, "-o", "r", *MODEL, "--db-out", tmp_path / "d", "--gfa-out", tmp_path / "g", *extra, *WORKFLOW, cwd=tmp_path)
    got = calling_files(tmp_path, "r")
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    for suf in (".kmc_pre", ".kmc_suf"):
        assert read(str(tmp_path / "d") + suf) == read(str(c["dir"] / "db") + suf), suf
    assert read(tmp_path / "g.gfa") == read(c["dir"] / "s.gfa")
    assert r.stdout.splitlines()[0] == c["L"] and int(c["L"]) >= 10 and untimed(r.stdout) == untimed(c["stdout"])
    assert sorted(os.listdir(tmp_path)) == ["PloidyFrost_output", "d.kmc_pre", "d.kmc_suf", "g.gfa"]      # no temporary file is left
    mine = [l for l in r.stderr.splitlines() if l.startswith("trim: ") or l.startswith("run: reads ")]
    assert mine == c["trim"] + c["run"] and len(c["trim"]) == 1 and len(c["run"]) == 1      # the trim: line, then the run: line


def test_pair_files_with_different_record_counts(chain, tmp_path):
    short = tmp_path / "short.fq"
    short.write_bytes(b"\n".join(read(chain["r2"]).split(b"\n")[:4 * 300]) + b"\n")      # the first 300 records of r2
    for extra in ([], ["--chunk-bytes", 8192]):
        r = cli("run", "-1", chain["r1"], "-2", short, "-o", "r", "--db-out", tmp_path / "d", *extra, *WORKFLOW, cwd=tmp_path, ok=False)
        assert r.returncode != 0 and r.stdout == ""
        assert "the files of a pair hold the same number of records" in r.stderr and "300" in r.stderr and str(short) in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["short.fq"]
    t = cli("trim", "-1", chain["r1"], "-2", short, "-o1", "a", "-u1", "b", "-o2", "c", "-u2", "d", *WORKFLOW, cwd=tmp_path, ok=False)
    assert t.stderr.replace("trim: ", "run: ", 1).splitlines()[0] == cli("run", "-1", chain["r1"], "-2", short, "-o", "r", *WORKFLOW, cwd=tmp_path, ok=False).stderr.splitlines()[0]


def test_every_read_dropped_ends_as_the_chain_does(chain, tmp_path):
    """MINLEN:100000 keeps nothing: the chain's `trim` writes empty files and its `run` on them says what it says; `run` with the step
    says the same on stdout, leaves with the same status and leaves nothing under an output name"""
    d = tmp_path / "chain"
    d.mkdir()
    cli("trim", "-1", chain["r1"], "-2", chain["r2"], "-o1", d / "o1.fq", "-u1", d / "u1.fq", "-o2", d / "o2.fq", "-u2", d / "u2.fq", "MINLEN:100000", cwd=d)
    assert read(d / "o1.fq") == b"" and read(d / "o2.fq") == b""
    want = cli("run", "-i", d / "o1.fq", "-i", d / "o2.fq", "-o", "s", "--db-out", d / "db", "--gfa-out", d / "g", cwd=d, ok=False)
    e = tmp_path / "mine"
    e.mkdir()
    got = cli("run", "-1", chain["r1"], "-2", chain["r2"], "-o", "s", "--db-out", e / "db", "--gfa-out", e / "g", "MINLEN:100000", cwd=e, ok=False)
    print("the chain's run on the empty files: status %d, stdout %r, stderr %r" % (want.returncode, want.stdout, want.stderr[-300:]))
    assert got.returncode == want.returncode and untimed(got.stdout) == untimed(want.stdout)
    left = lambda p: sorted(f for f in os.listdir(p) if f.startswith(("db.", "g.", "s")) and f != "PloidyFrost_output")
    assert left(e) == left(d) == []


def test_run_reads_with_steps_and_pairs(chain, tmp_path, monkeypatch):
    c = chain["paired"]
    words = c["run"][0].split()[1:]
    want = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    monkeypatch.chdir(tmp_path)
    got = hostapi.run_reads(None, "r", model="fre", steps=WORKFLOW, pairs=[(str(chain["r1"]), str(chain["r2"]))])
    trim = got.pop("trim")
    assert got == want and tuple(got) == hostapi.RUN_STATS_FIELDS
    assert calling_files(tmp_path, "r") == calling_files(c["dir"], "s")
    tw = c["trim"][0].split()
    t = {tw[i]: int(tw[i + 1]) for i in range(1, len(tw), 2)}
    assert len(trim) == 1 and len(trim[0]) == 2
    assert (trim[0][0]["reads"], trim[0][0]["both"], trim[0][0]["only1"], trim[0][0]["only2"], trim[0][0]["neither"]) == \
        (t["pairs"], t["both"], t["forward_only"], t["reverse_only"], t["dropped"])
    assert trim[0][0]["bases_kept"] + trim[0][1]["bases_kept"] == t["bases_kept"]


# ---- `run-multi STEP...` against its chain: one `trim` per unit, then `run-multi` ----

MULTI = ["--model", "fre", "--filter-multi", "-v 0.25 -n 6"]


def test_run_multi_with_steps_against_the_chain(tmp_path, monkeypatch):
    """three samples of the build_mc3_k25 generator at depth 64: alpha paired, beta single-ended in two files, gamma paired in two
    pairs.  Everything `run-multi STEP...` writes equals what one `trim` per unit followed by `run-multi` over the trimmed files writes,
    also with a model per colour."""
    gen = generator("make_build_multi_golden")
    rng = np.random.default_rng(7)
    raw = tmp_path / "raw"
    raw.mkdir()
    samples = list(gen.make_samples(**dict(gen.CASES["build_mc3_k25"], depth=DEPTH)))
    parts = {"alpha": [samples[0][0::2], samples[0][1::2]], "beta": [samples[1][: len(samples[1]) // 3], samples[1][len(samples[1]) // 3:]],
             "gamma": [samples[2][0::4], samples[2][1::4], samples[2][2::4], samples[2][3::4]]}
    files = {}
    for name, ps in parts.items():
        files[name] = []
        for j, p in enumerate(ps):
            write_fastq(raw / ("%s_%d.fq" % (name, j)), p, rng)
            files[name].append(raw / ("%s_%d.fq" % (name, j)))
    d = tmp_path / "chain"
    d.mkdir()
    trims, trimmed = [], {}
    for name in ("alpha", "gamma"):
        trimmed[name] = []
        for u in range(len(files[name]) // 2):
            o = [d / ("%s_%d_%s.fq" % (name, u, x)) for x in ("o1", "u1", "o2", "u2")]
            t = cli("trim", "-1", files[name][2 * u], "-2", files[name][2 * u + 1], "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], *WORKFLOW, cwd=d)
            trims.append((name, lines_with(t.stderr, "trim: ")))
            trimmed[name] += [o[0], o[2]]
    t = cli("trim", "-i", files["beta"][0], "-i", files["beta"][1], "-o", d / "beta.fq", *WORKFLOW, cwd=d)
    trims.insert(1, ("beta", lines_with(t.stderr, "trim: ")))
    trimmed["beta"] = [d / "beta.fq"]
    order = ("alpha", "beta", "gamma")
    chain_args = [x for name in order for x in ["--sample", name] + [y for f in trimmed[name] for y in ("-i", f)]]
    mine_args = [x for name in order for x in ["--sample", name] + ([y for f in files[name] for y in ("-i", f)] if name == "beta" else
                                                                    [y for u in range(len(files[name]) // 2) for y in ("-1", files[name][2 * u], "-2", files[name][2 * u + 1])])]
    want_trim = [l for name in order for n, ls in trims if n == name for l in ls]
    assert len(want_trim) == 4
    for tag, extra in (("plain", []), ("each", MULTI + ["--model-each-color"])):
        cd, md = tmp_path / ("c_" + tag), tmp_path / ("m_" + tag)
        cd.mkdir()
        md.mkdir()
        w = cli("run-multi", *chain_args, "-o", "s", "--db-out", cd / "db", "--gfa-out", cd / "g", *extra, cwd=cd)
        g = cli("run-multi", *mine_args, "-o", "s", "--db-out", md / "db", "--gfa-out", md / "g", *extra, *WORKFLOW, cwd=md)
        want, got = calling_files(cd, "s"), calling_files(md, "s")
        rows = want["_allele_frequency.txt"].decode().splitlines()
        print("run-multi chain (%s): L = %s, %d calling files, %d lines in allele_frequency.txt" % (tag, w.stdout.split()[:3], len(want), len(rows)))
        assert len(rows) >= 5 and sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], f
        assert sorted(os.listdir(md)) == sorted(os.listdir(cd))
        for f in os.listdir(cd):
            if f != "PloidyFrost_output":
                assert read(md / f) == read(cd / f), f
        assert g.stdout.splitlines()[:3] == w.stdout.splitlines()[:3] and untimed(g.stdout) == untimed(w.stdout)
        assert [l for l in g.stderr.splitlines() if l.startswith(("trim: ", "run-multi: col"))] == want_trim + lines_with(w.stderr, "run-multi: col")
    api = tmp_path / "api"
    api.mkdir()
    monkeypatch.chdir(api)
    got = hostapi.run_multi_reads([(n, [str(f) for f in files[n]]) for n in order], "s", steps=WORKFLOW, pairs=["alpha", "gamma"])
    assert calling_files(api, "s") == calling_files(tmp_path / "m_plain", "s")
    assert [len(x) for x in got["trim"]] == [1, 1, 2] and got["trim"][0][0][0]["both"] > 0 and got["trim"][1][0]["kept"] > 0 and got["trim"][2][1][1]["reads"] > 0
