"""K-MASK (pf_mask_reads / pf_mask_fastq, csrc/pf_mask.hip), the host streaming (hostapi.mask_fastq) and the `mask` sub-command against
the rule restated in Python (mask_cases.py): every comparison is byte equality of the output and equality of all six statistics."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case

import hist_cases as hc
import mask_cases as mc

from ploidyfrost_amd import hipapi, hostapi, synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
TILE = 1024   # pf::MASK_TILE: window starts a block stages at once (plus a halo of 32 bytes)
CASES = ["dip20k", "k31_z16", "stranded20k"]


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def golden():
    """case -> (device context with the case's table, its database)"""
    out = {}
    for case in CASES:
        db = mc.Database(load_case(case)["db"])
        d = hipapi.Device(0)
        db.upload(d)
        out[case] = (d, db)
    yield out
    for d, _ in out.values():
        d.close()


def check_reads(d, db, reads, low, up=mc.NO_UPPER, gap=b""):
    """the reads packed back to back (or with `gap` between them) through pf_mask_reads against the rule"""
    parts, off = [], []
    at = 0
    for r in reads:
        off.append(at)
        parts += [r, gap]
        at += len(r) + len(gap)
    text = b"".join(parts)
    ln = [len(r) for r in reads]
    want, want_st = mc.ref_mask_db(text, db, low, up, reads=list(zip(off, ln)))
    got, st = d.mask_reads(text, off, ln, low, up)
    assert got.tobytes() == want, first_difference(got.tobytes(), want)
    assert st == want_st
    return want, want_st


def first_difference(a, b):
    n = min(len(a), len(b))
    at = next((i for i in range(n) if a[i] != b[i]), n)
    return "first difference at byte %d of %d / %d: %r != %r" % (at, len(a), len(b), a[at:at + 40], b[at:at + 40])


def substitute(read, at):
    """the read with the base at `at` replaced by another one (an empty read stays empty)"""
    if not read:
        return read
    return read[:at] + (b"A" if read[at:at + 1] != b"A" else b"C") + read[at + 1:]


def lengths(k):
    return [0, 1, k - 1, k, k + 1, k + 62, k + 63, k + 64, 2 * k - 1, 2 * k, 150]


# ---- the kernels, through pf_mask_reads ----

@pytest.mark.parametrize("case", CASES)
def test_read_lengths(golden, case):
    d, db = golden[case]
    k = db.k
    src = mc.unitigs(case)[0]
    clean = [src[7:7 + n] for n in lengths(k)]
    hit = [substitute(r, len(r) // 2) for r in clean]
    low = max(int(db.meta["min_count"]), 1)
    _, st = check_reads(d, db, clean, low)
    assert st["kmers_bad"] == 0 and st["reads_changed"] == 0 and st["kmers"] == sum(max(n - k + 1, 0) for n in lengths(k))
    _, st = check_reads(d, db, hit, low)
    assert st["kmers_bad"] > 0
    check_reads(d, db, clean + hit, low, gap=b"\n+\n@x\n")      # not packed: bytes between the reads are copied
    check_reads(d, db, mc.make_reads(case, 400, seed=2, k=k), 10, 60)


def test_reverse_complement_against_a_database_of_one_strand(dev):
    genome, db = mc.synthetic(5, 400, 25, both_strands=False)
    db.upload(dev)
    fwd, rev = genome[10:160], mc.revcomp(genome[10:160])
    want, st = check_reads(dev, db, [fwd, rev, fwd.lower()], 1)
    assert want == fwd + b"N" * 150 + fwd.lower() and st["reads_changed"] == 1 and st["kmers_bad"] == 126
    # the canonical twin of the same database finds both
    genome2, both = mc.synthetic(5, 400, 25, both_strands=True)
    both.upload(dev)
    assert genome2 == genome and check_reads(dev, both, [fwd, rev], 1)[1]["kmers_bad"] == 0


@pytest.mark.parametrize("name,weak,low", [
    ("none", (), 10), ("all", (), 21), ("first", (0,), 10), ("last", (2500 - 25,), 10),
    ("k_apart", (300, 325), 10), ("k_plus_1_apart", (300, 326), 10),
    ("last_of_a_tile", (TILE - 1,), 10), ("first_of_a_tile", (TILE,), 10), ("both_sides_of_a_tile_edge", (TILE - 1, TILE), 10),
    ("last_of_the_second_tile", (2 * TILE - 1,), 10), ("in_the_halo", (TILE - 25, TILE + 31), 10),
])
def test_bad_windows_by_position(dev, name, weak, low):
    """one read longer than two tiles plus their halos, at offset 0 of the text, so that window i is window start i of the text"""
    k, n = 25, 2500
    genome, db = mc.synthetic(9, n, k, weak=weak)
    db.upload(dev)
    want, st = check_reads(dev, db, [genome], low)
    assert st["kmers"] == n - k + 1
    if name == "none":
        assert want == genome and st["kmers_bad"] == 0
    elif name == "all":
        assert want == b"N" * n
    else:
        assert st["kmers_bad"] == len(weak)
        masked = [i for i in range(n) if want[i:i + 1] == b"N"]
        assert masked == sorted({j for w in weak for j in range(w, w + k)})
        if name == "k_plus_1_apart":
            assert want[325:326] == genome[325:326] and st["bases_masked"] == 2 * k
        if name == "last_of_a_tile":
            assert want[TILE:TILE + k - 1] == b"N" * (k - 1)   # the mask carries into the next tile's first k - 1 bytes
    # the same read deeper in the text: every alignment of the read against the tiles and the 16-byte units
    for shift in (1, 15, 16, 63, 1000):
        check_reads(dev, db, [b"", genome], low, gap=b"#" * shift)


def test_n_and_lower_case(golden):
    d, db = golden["dip20k"]
    k = db.k
    r = mc.clean_read("dip20k", 150, at=3)
    at_0, at_end = b"N" + r[1:], r[:-1] + b"N"
    every_k = bytearray(r)
    every_k[::k] = b"N" * len(every_k[::k])
    want, st = check_reads(d, db, [at_0, at_end, bytes(every_k), b"N" * 150], 1)
    assert st["bases_masked"] == (k - 1) + (k - 1) + (150 - len(every_k[::k])) and st["reads_changed"] == 3   # the read of Ns: nothing changes
    assert want[:150] == b"N" * k + r[k:]
    # lower case: known k-mers stay as they are; with one error the case is kept outside the mask
    low_read = r.lower()
    err = bytearray(low_read)
    err[70] = ord("a") if err[70] != ord("a") else ord("c")
    want, st = check_reads(d, db, [low_read, bytes(err)], 1)
    assert want[:150] == low_read and st["reads_changed"] == 1
    assert want[150:150 + 70 - k + 1] == bytes(err[:70 - k + 1]) and want[150 + 70 - k + 1:150 + 70 + k] == b"N" * (2 * k - 1)


def test_bounds(golden):
    d, db = golden["dip20k"]
    reads = mc.make_reads("dip20k", 300, seed=4, k=db.k)
    _, st = check_reads(d, db, reads, 0)                      # low = 0: a missing k-mer is not bad
    assert st["kmers_bad"] == 0 and st["reads_changed"] == 0
    top = int(np.median(db.counts))
    _, st = check_reads(d, db, reads, 0, top)                 # up below a present count
    assert 0 < st["kmers_bad"] < st["kmers"]
    check_reads(d, db, reads, top, top)
    with pytest.raises(hipapi.DeviceError) as e:
        d.mask_reads(b"ACGT", [0], [4], 5, 4)
    assert e.value.status == hipapi.PF_ERR_ARG and "pf_mask_reads" in str(e.value) and "above up" in str(e.value)


def test_header_min_count_hides_present_records(dev, tmp_path):
    genome, db = mc.synthetic(12, 600, 25, weak=range(100, 140), weak_count=3)
    prefix = str(tmp_path / "db")
    synth.write_kmc1(prefix, db.file_kmers, db.file_counts, 25, min_count=5, max_count=19)   # the weak records and the count-20 ones both lie outside
    hidden = mc.Database(prefix)
    assert len(hidden.kmers) == 0 and len(hidden.file_kmers) == len(db.file_kmers)
    hidden.upload(dev)
    want, st = check_reads(dev, hidden, [genome], 1)
    assert want == b"N" * 600
    synth.write_kmc1(prefix, db.file_kmers, db.file_counts, 25, min_count=5)
    hidden = mc.Database(prefix)
    hidden.upload(dev)
    want, st = check_reads(dev, hidden, [genome], 1)          # low = 1 would keep the weak windows if the table gave them out
    assert st["kmers_bad"] == 40 and want[100:164] == b"N" * 64 and want[:100] == genome[:100]


def test_packed_reads_do_not_leak_into_each_other(golden):
    d, db = golden["dip20k"]
    r = mc.clean_read("dip20k", 120, at=5)
    bad = r[:119] + (b"A" if r[119:] != b"A" else b"C")      # the last window of the first read is bad; the second read starts right behind it
    want, st = check_reads(d, db, [bad, r, b"", r[:10], r], 1)
    assert want[120:240] == r and st["reads_changed"] == 1 and st["kmers_bad"] == 1 and st["reads"] == 5
    # two reads whose junction reads as k-mers of the database are still two reads: no window starts in the last k - 1 bytes of one
    whole = mc.clean_read("dip20k", 100)
    _, st = check_reads(d, db, [whole[:50], whole[50:]], 1)
    assert st["kmers"] == 2 * (50 - db.k + 1)


def test_no_reads_and_empty_text(golden):
    d, db = golden["dip20k"]
    text = b"no read at all\n" * 9
    got, st = d.mask_reads(text, [], [], 5)
    assert got.tobytes() == text and st == dict.fromkeys(mc.STATS, 0)
    got, st = d.mask_reads(b"", [], [], 5)
    assert len(got) == 0 and st == dict.fromkeys(mc.STATS, 0)
    got, st = d.mask_reads(b"", [0, 0], [0, 0], 5)
    assert st == dict(dict.fromkeys(mc.STATS, 0), reads=2)


def test_table_of_reads_is_checked_by_name(golden):
    d, _ = golden["dip20k"]
    text = b"A" * 100
    for off, ln, who in (([0, 90], [50, 11], 1), ([0, 40], [50, 10], 0), ([60, 0], [10, 10], 0), ([101], [0], 0)):
        with pytest.raises(hipapi.DeviceError) as e:
            d.mask_reads(text, off, ln, 5)
        assert e.value.status == hipapi.PF_ERR_ARG and "pf_mask_reads: read %d " % who in str(e.value)


def test_host_and_device_pointers_alignment_and_determinism(golden):
    import torch
    d, db = golden["dip20k"]
    reads = mc.make_reads("dip20k", 500, seed=6, k=db.k)
    text, off, ln = mc.pack(reads)
    want, want_st = mc.ref_mask_db(text, db, 12, reads=list(zip(off.tolist(), ln.tolist())))
    a, st_a = d.mask_reads(text, off, ln, 12)
    b, st_b = d.mask_reads(text, off, ln, 12)
    assert a.tobytes() == b.tobytes() == want and st_a == st_b == want_st
    t_text = torch.from_numpy(np.frombuffer(b"\0" * 3 + text, dtype=np.uint8).copy()).cuda()
    t_off = torch.from_numpy(off.view(np.int64)).cuda()
    t_len = torch.from_numpy(ln.view(np.int32)).cuda()
    for shift_in, shift_out in ((3, 0), (3, 5), (0, 0), (16, 1)):   # device pointers, 16-byte aligned or not, in and out
        src = t_text[3:] if shift_in == 3 else torch.cat([torch.zeros(shift_in, dtype=torch.uint8, device="cuda"), t_text[3:]])[shift_in:]
        out = torch.full((len(text) + shift_out + 16,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _, st = d.mask_reads(src, t_off, t_len, 12, out=out[shift_out:shift_out + len(text)])
        res = out.cpu().numpy()
        assert res[shift_out:shift_out + len(text)].tobytes() == want and st == want_st
        assert (res[:shift_out] == 7).all() and (res[shift_out + len(text):] == 7).all()   # nothing written around the output
    got, st = d.mask_reads(t_text[3:], off, ln, 12)                     # device text, host table, host out
    assert got.tobytes() == want and st == want_st


def test_kernel_is_timed_under_its_name(golden):
    d, db = golden["dip20k"]
    assert d.L.pf_kernel_name(hipapi.K_MASK) == b"k_mask" and hipapi.KERNELS[-1] == "k_call_model"
    reads = mc.make_reads("dip20k", 100, seed=8, k=db.k)
    text, off, ln = mc.pack(reads)
    d.enable_timing(True)
    d.reset_timing()
    _, st = d.mask_reads(text, off, ln, 10)
    ms, launches = d.kernel_time(hipapi.K_MASK)
    units = d.kernel_units(hipapi.K_MASK)
    d.enable_timing(False)
    assert launches == 1 and ms > 0 and units == st["kmers"] > 0


def test_refused_by_name_without_a_table():
    d = hipapi.Device(0)
    try:
        with pytest.raises(hipapi.DeviceError) as e:
            d.mask_reads(b"ACGT" * 10, [0], [40], 5)
        assert e.value.status == hipapi.PF_ERR_ARG and "pf_mask_reads" in str(e.value) and "count table" in str(e.value)
        with pytest.raises(hipapi.DeviceError) as e:
            d.mask_fastq(mc.fastq([b"ACGT" * 10]), 5)
        assert e.value.status == hipapi.PF_ERR_ARG and "pf_mask_fastq" in str(e.value) and "count table" in str(e.value)
    finally:
        d.close()


# ---- FASTQ, through pf_mask_fastq ----

def check_fastq(d, db, text, low, up=mc.NO_UPPER):
    want, want_st = mc.ref_mask_db(text, db, low, up)
    got, used, st = d.mask_fastq(text, low, up, final=True)
    assert used == len(text) and got.tobytes() == want, first_difference(got.tobytes(), want)
    assert st == want_st
    return want_st


@pytest.mark.parametrize("n_records", [1, 2, 255, 256, 257])
def test_fastq_records(golden, n_records):
    d, db = golden["dip20k"]
    reads = mc.make_reads("dip20k", n_records, seed=n_records, k=db.k)
    quals = {0: b"@" + b"I" * (len(reads[0]) - 1), n_records - 1: b"+" * len(reads[-1])}   # roles come from the line index
    for crlf in (False, True):
        for last_newline in (True, False):
            st = check_fastq(d, db, mc.fastq(reads, crlf=crlf, last_newline=last_newline, quals=quals), 10)
            assert st["reads"] == n_records


def test_fastq_other_cases_and_empty(golden):
    for case in ("k31_z16", "stranded20k"):
        d, db = golden[case]
        check_fastq(d, db, mc.fastq(mc.make_reads(case, 300, seed=1, k=db.k)), 8, 200)
    d, db = golden["dip20k"]
    got, used, st = d.mask_fastq(b"", 5)
    assert len(got) == 0 and used == 0 and st == dict.fromkeys(mc.STATS, 0)
    check_fastq(d, db, b"@only\n\n+\n\n", 5)                       # an empty read
    check_fastq(d, db, mc.fastq([b"", b"ACGT", b"N" * 60]), 5)


def test_fastq_chunks(golden):
    d, db = golden["dip20k"]
    reads = mc.make_reads("dip20k", 40, seed=13, k=db.k)
    head, tail = mc.fastq(reads[:39], crlf=True), mc.fastq(reads[39:], crlf=True)
    want, want_st = mc.ref_mask_db(head, db, 10)
    lines = [len(b"@r0\r\n"), len(b"@r0\r\n") + len(reads[39]) + 2, len(b"@r0\r\n") + len(reads[39]) + 2 + 3]
    cuts = [0, 2, lines[0], lines[0] + 9, lines[1], lines[1] + 1, lines[2], lines[2] + 5, len(tail) - 1]   # inside each of the four lines and at their ends
    for cut in cuts:
        got, used, st = d.mask_fastq(head + tail[:cut], 10, final=False)
        assert used == len(head) and got.tobytes() == want and st == want_st, cut
    got, used, st = d.mask_fastq(head + tail, 10, final=False)
    assert used == len(head + tail) and st["reads"] == 40
    got, used, st = d.mask_fastq(tail[:-1], 10, final=False)     # no whole record
    assert used == 0 and len(got) == 0 and st == dict.fromkeys(mc.STATS, 0)
    got, used, st = d.mask_fastq(b"@r\nACGTACGT", 10, final=False)
    assert used == 0 and st["reads"] == 0


@pytest.mark.parametrize("name,record,damage", [
    ("does not start with '@'", 300, lambda recs: recs.__setitem__(300, b"r" + recs[300][1:])),
    ("does not start with '+'", 2, lambda recs: recs.__setitem__(2, recs[2].replace(b"\n+\n", b"\n-\n"))),
    ("quality line's length", 511, lambda recs: recs.__setitem__(511, recs[511][:-2] + b"\n")),
    ("not a multiple of four", 600, lambda recs: recs.append(b"@extra\nACGT\n")),
    ("does not start with '@'", 0, lambda recs: recs.__setitem__(0, b">" + recs[0][1:])),
])
def test_fastq_refusals(golden, name, record, damage):
    d, db = golden["dip20k"]
    reads = mc.make_reads("dip20k", 600, seed=21, k=db.k)
    recs = [mc.fastq([r], name=b"r%d_" % i) for i, r in enumerate(reads)]
    damage(recs)
    if "multiple" not in name:
        recs[580] = recs[580].replace(b"\n+\n", b"\n?\n")   # a later offender: the smallest record is reported
    text = b"".join(recs)
    out = np.full(len(text), 35, dtype=np.uint8)
    with pytest.raises(hipapi.DeviceError) as e:
        d.mask_fastq(text, 10, final=True, out=out)
    assert e.value.status == hipapi.PF_ERR_ARG and e.value.bad_record == record
    assert "pf_mask_fastq: record %d of the chunk" % record in str(e.value) and name in str(e.value)
    assert (out == 35).all()   # refused before anything was written


# ---- the host streaming and the sub-command ----

def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)


@pytest.fixture(scope="module")
def reads_file(tmp_path_factory):
    """about 3 000 reads, a few hundred KB, with CRLF records in the middle and no newline at the end"""
    d = tmp_path_factory.mktemp("mask_reads")
    db = mc.Database(load_case("dip20k")["db"])
    reads = mc.make_reads("dip20k", 3000, seed=31, k=db.k)
    text = mc.fastq(reads[:1000]) + mc.fastq(reads[1000:2000], crlf=True, name=b"c") + mc.fastq(reads[2000:], last_newline=False, name=b"t")
    path = d / "reads.fq"
    path.write_bytes(text)
    want, st = mc.ref_mask_db(text, db, 12, 60)
    record = len(mc.fastq(reads[:1]))
    return dict(dir=d, path=str(path), text=text, db=db, want=want, stats=st, record=record, first_record=record)


def test_host_streaming_chunk_sizes(reads_file, tmp_path):
    f = reads_file
    out = tmp_path / "out.fq"
    for chunk in (0, 4096, f["record"], f["record"] - 1, 100_000):   # one chunk; many; one record; one byte less (no whole record: the chunk grows)
        st = hostapi.mask_fastq(f["db"].prefix, [f["path"]], str(out), lower=12, upper=60, chunk_bytes=chunk)
        assert out.read_bytes() == f["want"], (chunk, first_difference(out.read_bytes(), f["want"]))
        assert st == dict(f["stats"], lower=12), chunk
        assert sorted(os.listdir(tmp_path)) == ["out.fq"]
        out.unlink()


def test_cli_two_inputs_and_the_stderr_line(reads_file, tmp_path):
    f = reads_file
    second = tmp_path / "second.fq"
    reads2 = mc.make_reads("dip20k", 200, seed=32, k=f["db"].k)
    second.write_bytes(mc.fastq(reads2))
    want2, st2 = mc.ref_mask_db(mc.fastq(reads2), f["db"], 12, 60)
    out = tmp_path / "out.fq"
    r = run_cli("mask", "-d", f["db"].prefix, "-i", f["path"], "-i", second, "-o", out, "-l", 12, "-u", 60, "--chunk-bytes", 50_000)
    assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
    assert out.read_bytes() == f["want"] + want2           # (the first input ends without a newline: inputs are copied as they are)
    total = {s: f["stats"][s] + st2[s] for s in mc.STATS}
    assert r.stderr == "mask: reads %d changed %d bases %d masked %d kmers %d bad %d\n" % tuple(total[s] for s in mc.STATS)


def test_cli_auto_cutoffs(tmp_path):
    meta, prefix, counts = hc.make_single(tmp_path)
    lower = hc.thresholds(counts)[0]
    db = mc.Database(prefix)
    reads = mc.make_reads("dip20k", 1500, seed=33, k=db.k)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(mc.fastq(reads))
    want, st = mc.ref_mask_db(mc.fastq(reads), db, lower)
    assert 0 < st["kmers_bad"] < st["kmers"] and lower != 10
    a, b = tmp_path / "auto.fq", tmp_path / "explicit.fq"
    auto = run_cli("mask", "-d", prefix, "-i", fq, "-o", a, "--auto-cutoffs")
    assert auto.returncode == 0, auto.stderr
    assert auto.stdout == run_cli("cutoffL", "-d", prefix).stdout == "%d\n" % lower
    assert a.read_bytes() == want
    explicit = run_cli("mask", "-d", prefix, "-i", fq, "-o", b, "-l", lower)
    assert explicit.returncode == 0 and explicit.stdout == "" and b.read_bytes() == want and explicit.stderr == auto.stderr
    assert hostapi.mask_fastq(prefix, str(fq), str(tmp_path / "api.fq"), auto=True)["lower"] == lower
    assert (tmp_path / "api.fq").read_bytes() == want


@pytest.mark.parametrize("name,record", [("does not start with '@'", 2500), ("quality line's length", 1200), ("not a multiple of four", 3000)])
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
        r = run_cli("mask", "-d", f["db"].prefix, "-i", f["path"], "-i", bad, "-o", tmp_path / "out.fq", "-l", 12, "--chunk-bytes", chunk)
        assert r.returncode != 0 and r.stdout == ""
        assert "%s: record %d: " % (bad, record + 1) in r.stderr and name in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["bad.fq"]   # neither the output nor its temporary file


def test_kmc2_database_gives_what_its_kmc1_twin_gives(tmp_path):
    prefix2 = load_case("dip_kmc2")["db"]
    kmers, counts, meta = synth.read_kmc(prefix2)
    assert meta["layout"] == "kmc2"
    o = np.argsort(kmers, kind="stable")
    twin = str(tmp_path / "twin")
    synth.write_kmc1(twin, kmers[o], counts[o], meta["k"], min_count=meta["min_count"], max_count=meta["max_count"], both_strands=meta["both_strands"])
    reads = mc.make_reads("dip_kmc2", 800, seed=34, k=meta["k"])
    fq = tmp_path / "reads.fq"
    fq.write_bytes(mc.fastq(reads))
    want, st = mc.ref_mask_db(mc.fastq(reads), mc.Database(prefix2), 10)
    outs = []
    for prefix in (prefix2, twin):
        out = tmp_path / ("out_%s.fq" % os.path.basename(prefix))
        assert hostapi.mask_fastq(prefix, [str(fq)], str(out), lower=10) == dict(st, lower=10)
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] == want
