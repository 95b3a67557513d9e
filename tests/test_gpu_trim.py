"""K-TRIM on the device (pf_trim_fastq / pf_trim_fastq_pair through hipapi, `ploidyfrost trim` through the CLI and hostapi) against the
plain-Python rule of trim_cases.py.  Byte-exact: the output bytes, the (begin, len) arrays and every statistic are equal; there is no
tolerance anywhere.  The shapes are the smallest at which the kernels can go wrong (trim_cases.EDGE_LENGTHS and edge_quals: a row
step of k_trim_intervals is 256 bytes, a lane's unit 16), not workload sizes."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import trim_cases as tc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def edge_text():
    return tc.fastq(tc.edge_records())


@pytest.fixture(scope="module")
def generated():
    """4000 reads (about 1 MB), and a second file of the same number of records with other reads and longer names"""
    a = tc.make_reads(4000, seed=1)
    b = [(name + b" mate/2", seq, qual) for name, seq, qual in tc.make_reads(4000, seed=2)]
    return tc.fastq(a), tc.fastq(b)


def same(got, want):
    assert bytes(got["out"]) == want["out"]
    assert got["bytes_used"] == want["bytes_used"] and got["n_records"] == want["n_records"]
    assert got["begin"].tolist() == want["begin"] and got["len"].tolist() == want["len"]
    assert got["stats"] == want["stats"]


def same_pair(got, want):
    assert [bytes(o) for o in got["out"]] == want["out"]
    assert list(got["bytes_used"]) == want["bytes_used"] and got["n_records"] == want["n_records"]
    for f in range(2):
        assert got["begin"][f].tolist() == want["begin"][f] and got["len"][f].tolist() == want["len"][f]
    assert got["stats"] == want["stats"]


# ---- the edge list, every step order ----

@pytest.mark.parametrize("steps", tc.EDGE_STEPS, ids=lambda s: "_".join(s))
def test_edge_reads(dev, edge_text, steps):
    want = tc.trim_fastq(edge_text, steps)
    same(dev.trim_fastq(edge_text, steps), want)
    assert 0 < want["stats"]["kept"] and want["stats"]["dropped"] > 0


def test_edge_reads_phred64(dev):
    text = tc.fastq(tc.edge_records(phred=64))
    for steps in (tc.WORKFLOW, ["SLIDINGWINDOW:64:20", "LEADING:30"]):
        same(dev.trim_fastq(text, steps, phred=64), tc.trim_fastq(text, steps, phred=64))
    same(dev.trim_fastq(text, tc.WORKFLOW, phred=33), tc.trim_fastq(text, tc.WORKFLOW, phred=33))   # the same bytes read as phred 33


# ---- text shapes ----

def test_every_alignment_of_the_lines(dev):
    """a record whose sequence and quality lines start at every offset 0 .. 15 of a 16-byte unit, trimmed at both ends"""
    q = tc.qline([2] * 7 + [40] * 120 + [2] * 9)
    recs = [(b"n" * a, b"ACGT" * 34, q) for a in range(16)] + [(b"m" * a, b"ACGTA" * 27 + b"C", q) for a in range(16)]
    text = tc.fastq(recs)
    starts, pos = {1: set(), 3: set()}, 0
    for i, line in enumerate(text.split(b"\n")[:-1]):
        if i % 4 in starts:
            starts[i % 4].add(pos % 16)
        pos += len(line) + 1
    assert starts[1] == starts[3] == set(range(16))
    want = tc.trim_fastq(text, tc.WORKFLOW)
    same(dev.trim_fastq(text, tc.WORKFLOW), want)
    assert want["begin"] == [7] * 32 and want["len"] == [120] * 32
    # the output's pieces land at every alignment as well: a kept record is 2 * 120 + header + 4 bytes
    assert len({len(tc.record_bytes(r, 7, 127)) % 16 for r in want["records"]}) >= 8


def test_line_ends_one_record_all_dropped_nothing_trimmed(dev, generated):
    recs = tc.parse_records(generated[0])[0][:300]
    recs = [(r[0][1:], r[1], r[2][1:], r[3]) for r in recs]
    plain = tc.trim_fastq(tc.fastq(recs), tc.WORKFLOW)
    for crlf in (False, True):
        for last_newline in (True, False):
            text = tc.fastq(recs, crlf=crlf, last_newline=last_newline)
            got = dev.trim_fastq(text, tc.WORKFLOW)
            same(got, tc.trim_fastq(text, tc.WORKFLOW))
            assert bytes(got["out"]) == plain["out"] and got["bytes_used"] == len(text)
    one = tc.fastq([(b"only", b"ACGT" * 20, b"I" * 80)], last_newline=False)
    same(dev.trim_fastq(one, tc.WORKFLOW), tc.trim_fastq(one, tc.WORKFLOW))
    low = tc.fastq([(b"r%d" % i, b"A" * n, b"#" * n) for i, n in enumerate((0, 1, 50, 151, 300))])
    got = dev.trim_fastq(low, tc.WORKFLOW)
    same(got, tc.trim_fastq(low, tc.WORKFLOW))
    assert len(got["out"]) == 0 and got["stats"]["kept"] == 0 and got["stats"]["dropped"] == 5
    good = tc.fastq([(b"r%d" % i, b"C" * n, b"plus" * (i % 2), b"I" * n) for i, n in enumerate((50, 51, 64, 151, 256, 257, 1000))])
    got = dev.trim_fastq(good, tc.WORKFLOW)
    assert bytes(got["out"]) == good and got["stats"]["bases_kept"] == got["stats"]["bases"]   # nothing is trimmed: the output is the input
    empty = dev.trim_fastq(b"", tc.WORKFLOW)
    assert empty["n_records"] == 0 and len(empty["out"]) == 0 and empty["bytes_used"] == 0


def test_chunk_cut_inside_each_line_of_the_last_record(dev, generated):
    recs = tc.parse_records(generated[0])[0][:6]
    recs = [(r[0][1:], r[1], r[2][1:], r[3]) for r in recs]
    text, head = tc.fastq(recs), tc.fastq(recs[:5])
    whole = tc.trim_fastq(text, tc.WORKFLOW)
    lines = text[len(head):].split(b"\n")
    cuts, pos = [], len(head)
    for line in lines[:4]:   # the line's first byte, its middle, its newline
        cuts += [pos, pos + len(line) // 2, pos + len(line)]
        pos += len(line) + 1
    for cut in cuts:
        first = dev.trim_fastq(text[:cut], tc.WORKFLOW, final=False)
        same(first, tc.trim_fastq(text[:cut], tc.WORKFLOW, final=False))
        assert first["bytes_used"] == len(head) and first["n_records"] == 5
        second = dev.trim_fastq(text[first["bytes_used"]:], tc.WORKFLOW, final=True)
        assert bytes(first["out"]) + bytes(second["out"]) == whole["out"], cut
    none = dev.trim_fastq(text[:len(tc.fastq(recs[:1])) - 1], tc.WORKFLOW, final=False)   # no whole record: everything is carried
    assert none["bytes_used"] == 0 and none["n_records"] == 0 and len(none["out"]) == 0


# ---- refusals of one chunk ----

def test_refusals_write_nothing(dev, generated):
    text = generated[0][:30000]
    recs, used = tc.parse_records(text, final=False)
    text = text[:used]
    at = tc._end_of(text, 7)
    bad = text[:at] + b"#" + text[at + 1:]   # record 7 starts without '@'
    out = np.full(len(bad) + 1, 0x55, dtype=np.uint8)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.trim_fastq(bad, tc.WORKFLOW, out=out)
    assert e.value.status == hipapi.PF_ERR_ARG and e.value.bad_record == 7 and "does not start with '@'" in str(e.value)
    assert (out == 0x55).all()
    with pytest.raises(hipapi.DeviceError, match="the line count is not a multiple of four"):
        dev.trim_fastq(text[:text.rstrip(b"\n").rfind(b"\n") + 1], tc.WORKFLOW, final=True, out=out)   # the last quality line is missing
    assert (out == 0x55).all()
    for steps, phred, word in (([], 33, "no step is given"), (["MINLEN:1"] * 9, 33, "more than 8 steps"), ([(7, 1, 0)], 33, "step 0: unknown step"),
                               ([(1, 94, 0)], 33, "step 0: a value of the step is out of range"), ([(1, 10, 0), (3, 65, 20)], 33, "step 1: a value of the step is out of range"),
                               (tc.WORKFLOW, 50, "the quality offset is 33 or 64, not 50")):
        with pytest.raises(hipapi.DeviceError) as e:
            dev.trim_fastq(text, steps, phred=phred, out=out)
        assert e.value.status == hipapi.PF_ERR_ARG and word in str(e.value), word
        assert (out == 0x55).all()


# ---- pairs ----

def pair_texts():
    """all four outcomes in one chunk, the two files with different bytes per record"""
    good, bad = b"I" * 60, b"#" * 60
    r1 = [(b"p%d/1" % i, b"A" * 60, (good, good, bad, bad, good)[i % 5]) for i in range(40)]
    r2 = [(b"p%d/2 longer name" % i, b"C" * 60, (good, bad, good, bad, bad)[i % 5]) for i in range(40)]
    return r1, r2


def test_pair_all_four_outcomes(dev):
    r1, r2 = pair_texts()
    t1, t2 = tc.fastq(r1), tc.fastq(r2, crlf=True, last_newline=False)
    want = tc.trim_pair(t1, t2, tc.WORKFLOW)
    same_pair(dev.trim_fastq_pair(t1, t2, tc.WORKFLOW), want)
    s = want["stats"][0]
    assert (s["both"], s["only1"], s["only2"], s["neither"]) == (8, 16, 8, 8) and all(len(o) for o in want["out"])


def test_pair_chunks_with_different_record_counts(dev):
    r1, r2 = pair_texts()
    t1, t2 = tc.fastq(r1[:5]), tc.fastq(r2[:3]) + b"@cut\nACG"
    want = tc.trim_pair(t1, t2, tc.WORKFLOW, final=False)
    got = dev.trim_fastq_pair(t1, t2, tc.WORKFLOW, final=False)
    same_pair(got, want)
    assert got["n_records"] == 3 and list(got["bytes_used"]) == [len(tc.fastq(r1[:3])), len(tc.fastq(r2[:3]))]
    got = dev.trim_fastq_pair(t2, t1, tc.WORKFLOW, final=False)   # the other way round
    same_pair(got, tc.trim_pair(t2, t1, tc.WORKFLOW, final=False))
    none = dev.trim_fastq_pair(t1, t2[:20], tc.WORKFLOW, final=False)   # one file without a whole record: nothing is used of either
    assert none["n_records"] == 0 and list(none["bytes_used"]) == [0, 0] and not any(len(o) for o in none["out"])


def test_pair_refusals_write_nothing(dev):
    r1, r2 = pair_texts()
    t1, t2 = tc.fastq(r1[:5]), tc.fastq(r2[:3])
    outs = [np.full(len(t) + 1, 0x55, dtype=np.uint8) for t in (t1, t1, t2, t2)]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.trim_fastq_pair(t1, t2, tc.WORKFLOW, final=True, outs=outs)
    assert e.value.status == hipapi.PF_ERR_ARG and "the final chunks hold different numbers of records (file 1: 5, file 2: 3)" in str(e.value)
    t2 = tc.fastq(r2[:5])
    at = tc._end_of(t2, 2) + len(b"@p2/2 longer name\n") + 61    # the plus line of record 2 of file 2
    assert t2[at:at + 1] == b"+"
    bad = t2[:at] + b"-" + t2[at + 1:]
    outs = [np.full(len(t) + 1, 0x55, dtype=np.uint8) for t in (t1, t1, bad, bad)]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.trim_fastq_pair(t1, bad, tc.WORKFLOW, outs=outs)
    assert e.value.bad_record == 2 * 2 + 1 and "file 2" in str(e.value) and "third line does not start with '+'" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.trim_fastq_pair(bad, t1, tc.WORKFLOW, outs=[outs[2], outs[3], outs[0], outs[1]])
    assert e.value.bad_record == 2 * 2 + 0 and "file 1" in str(e.value)
    assert all((o == 0x55).all() for o in outs)


# ---- generated reads, device pointers, repeatability, the timer ----

def test_generated_reads_single_and_paired(dev, generated):
    t1, t2 = generated
    want = tc.trim_fastq(t1, tc.WORKFLOW)
    same(dev.trim_fastq(t1, tc.WORKFLOW), want)
    d, w, lead, trail = tc.outcome_shares([(r[0], r[1], r[3]) for r in want["records"]])
    assert min(d, w, lead, trail) >= 0.10
    same_pair(dev.trim_fastq_pair(t1, t2, tc.WORKFLOW), tc.trim_pair(t1, t2, tc.WORKFLOW))


def test_device_pointers_alignment_and_repeatability(dev, generated):
    t1 = generated[0]
    want = tc.trim_fastq(t1, tc.WORKFLOW)
    host = np.frombuffer(t1, dtype=np.uint8)
    for shift in (0, 1, 8):   # the text and the output on the device, 16-byte aligned and not
        buf = torch.zeros(len(t1) + 32, dtype=torch.uint8, device="cuda")
        text = buf[shift: shift + len(t1)]
        text.copy_(torch.from_numpy(host.copy()))
        out = torch.full((len(t1) + 17,), 0x55, dtype=torch.uint8, device="cuda")[shift: shift + len(t1) + 1]
        torch.cuda.synchronize()
        got = dev.trim_fastq(text, tc.WORKFLOW, out=out)
        torch.cuda.synchronize()
        got["out"] = got["out"].cpu().numpy()
        same(got, want)
    first = dev.trim_fastq(t1, tc.WORKFLOW)
    second = dev.trim_fastq(t1, tc.WORKFLOW)
    assert bytes(first["out"]) == bytes(second["out"]) and first["stats"] == second["stats"]
    assert first["begin"].tolist() == second["begin"].tolist() and first["len"].tolist() == second["len"].tolist()


def test_kernel_is_timed_under_its_name(generated):
    d = hipapi.Device(0)
    try:
        d.enable_timing(True)
        r = d.trim_fastq(generated[0], tc.WORKFLOW)
        ms, launches = d.kernel_time(hipapi.K_TRIM)
        assert launches == 1 and ms > 0 and d.kernel_units(hipapi.K_TRIM) == r["n_records"]
        d.trim_fastq_pair(generated[0], generated[1], tc.WORKFLOW)
        assert d.kernel_time(hipapi.K_TRIM)[1] == 2 and d.kernel_units(hipapi.K_TRIM) == 3 * r["n_records"]
        assert d.L.pf_kernel_name(hipapi.K_TRIM).decode() == "k_trim"
    finally:
        d.close()


# ---- the sub-command ----

def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)


def single_line(s):
    return "trim: reads %d kept %d dropped %d bases %d bases_kept %d" % (s["reads"], s["kept"], s["dropped"], s["bases"], s["bases_kept"])


def pair_line(s):
    return "trim: pairs %d both %d forward_only %d reverse_only %d dropped %d bases %d bases_kept %d" % (
        s[0]["reads"], s[0]["both"], s[0]["only1"], s[0]["only2"], s[0]["neither"], s[0]["bases"] + s[1]["bases"], s[0]["bases_kept"] + s[1]["bases_kept"])


def test_cli_single_at_three_chunk_sizes(tmp_path, generated):
    """the smallest --chunk-bytes the option accepts (on a small file: a device call per byte), a value that cuts records, the default"""
    small = tc.fastq(tc.make_reads(12, seed=9), crlf=True, last_newline=False)
    big = generated[0]
    for text, chunks in ((small, (1, 777, None)), (big, (100000, None))):
        fq = tmp_path / "in.fq"
        fq.write_bytes(text)
        want = tc.trim_fastq(text, tc.WORKFLOW)
        for chunk in chunks:
            out, log = tmp_path / "out.fq", tmp_path / "log.txt"
            r = run_cli("trim", "-i", fq, "-o", out, *tc.WORKFLOW, "--trimlog", log, *(("--chunk-bytes", chunk) if chunk else ()))
            assert r.returncode == 0 and r.stdout == "", r.stderr
            assert r.stderr.strip().splitlines()[-1] == single_line(want["stats"]), chunk
            assert out.read_bytes() == want["out"] and log.read_bytes() == tc.trimlog(want), chunk
            assert sorted(os.listdir(tmp_path)) == ["in.fq", "log.txt", "out.fq"]
            out.unlink()
            log.unlink()
    # several inputs, one after the other; -v adds the times
    fq2 = tmp_path / "in2.fq"
    fq2.write_bytes(small)
    r = run_cli("trim", "-i", tmp_path / "in.fq", "-i", fq2, "-o", tmp_path / "out.fq", "-v", *tc.WORKFLOW)
    assert r.returncode == 0 and (tmp_path / "out.fq").read_bytes() == tc.trim_fastq(big, tc.WORKFLOW)["out"] + tc.trim_fastq(small, tc.WORKFLOW)["out"]
    assert "trim: stream " in r.stderr and "device " in r.stderr


def test_cli_pair_at_three_chunk_sizes(tmp_path, generated):
    """the two files have different bytes per record, so the two carries drift apart"""
    small = (tc.fastq(tc.make_reads(12, seed=9)), tc.fastq([(n + b" a much longer name than its mate's", s, q) for n, s, q in tc.make_reads(12, seed=10)]))
    names = ("p1.fq", "u1.fq", "p2.fq", "u2.fq")
    for (t1, t2), chunks in ((small, (1, 500, None)), (generated, (100000, None))):
        f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
        f1.write_bytes(t1)
        f2.write_bytes(t2)
        want = tc.trim_pair(t1, t2, tc.WORKFLOW)
        for chunk in chunks:
            o = [tmp_path / n for n in names]
            log = tmp_path / "log.txt"
            r = run_cli("trim", "-1", f1, "-2", f2, "-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "--trimlog", log, *tc.WORKFLOW,
                        *(("--chunk-bytes", chunk) if chunk else ()))
            assert r.returncode == 0 and r.stdout == "", r.stderr
            assert r.stderr.strip().splitlines()[-1] == pair_line(want["stats"]), chunk
            assert [p.read_bytes() for p in o] == want["out"], chunk
            assert log.read_bytes() == tc.trimlog(want), chunk
            assert sorted(os.listdir(tmp_path)) == sorted(names + ("r1.fq", "r2.fq", "log.txt"))
            for p in o + [log]:
                p.unlink()
    # the same through the host layer's Python binding
    o = [str(tmp_path / n) for n in names]
    st = hostapi.trim_fastq_pair(str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq"), o, tc.WORKFLOW, chunk_bytes=300000)
    assert st == tc.trim_pair(*generated, tc.WORKFLOW)["stats"] and [open(p, "rb").read() for p in o] == tc.trim_pair(*generated, tc.WORKFLOW)["out"]
    st = hostapi.trim_fastq(str(tmp_path / "r1.fq"), o[0], tc.WORKFLOW, trimlog=o[1])
    assert st == tc.trim_fastq(generated[0], tc.WORKFLOW)["stats"]


def test_cli_refusals_mid_stream_leave_nothing(tmp_path, generated):
    t1, t2 = generated
    at = tc._end_of(t1, 3000)
    bad = t1[:at] + b"#" + t1[at + 1:]   # record 3001 starts without '@': the second chunk of 500 000 bytes
    fq, f2 = tmp_path / "bad.fq", tmp_path / "r2.fq"
    fq.write_bytes(bad)
    f2.write_bytes(t2)
    r = run_cli("trim", "-i", fq, "-o", tmp_path / "out.fq", "--trimlog", tmp_path / "log.txt", "--chunk-bytes", 500000, *tc.WORKFLOW)
    assert r.returncode != 0 and "%s: record 3001: the record's first line does not start with '@'" % fq in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.fq", "r2.fq"]
    o = [tmp_path / n for n in ("p1.fq", "u1.fq", "p2.fq", "u2.fq")]
    pair = ["-o1", o[0], "-u1", o[1], "-o2", o[2], "-u2", o[3], "--trimlog", tmp_path / "log.txt", "--chunk-bytes", 500000, *tc.WORKFLOW]
    r = run_cli("trim", "-1", f2, "-2", fq, *pair)
    assert r.returncode != 0 and "%s: record 3001: the record's first line does not start with '@'" % fq in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.fq", "r2.fq"]
    # one file of a pair ends while the other still holds whole records: refused by name with both counts
    short = tmp_path / "short.fq"
    short.write_bytes(t1[:at])
    for chunk in (500000, 100000000):
        r = run_cli("trim", "-1", short, "-2", f2, *pair[:-len(tc.WORKFLOW) - 1], chunk, *tc.WORKFLOW)
        assert r.returncode != 0 and "the files of a pair hold the same number of records" in r.stderr and str(short) in r.stderr and "3000" in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["bad.fq", "r2.fq", "short.fq"]
