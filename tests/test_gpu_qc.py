"""K-QC on the device (pf_qc_begin .. pf_qc_end around pf_qc_fastq, pf_trim_fastq[_pair] and pf_count_fastq_trimmed through hipapi)
against the host's plain restatement of csrc/pf_qc_rule.hpp (hostapi.qc_fastq_chunk; test_qc_cpu.py holds that one to the Python
rule).  Every word of every table is equal; there is no tolerance anywhere.  The shapes are the smallest at which the kernel can go
wrong (a lane's unit is 16 positions, a row step 256, the pooled position bin 1023, the pooled length 1024, a block 16 rows), not
workload sizes."""
import numpy as np
import pytest

import clip_cases as cc
import qc_cases as qc
import trim_cases as tc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
GEN_STEPS = ["LEADING:5", "TRAILING:5", "MINLEN:20"]   # (clip_cases' generated qualities are noise: the workflow's window drops nearly every read)
DROP_ALL = ["MINLEN:100000"]


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 16], seed=3, sides=[0, 1, 2])


@pytest.fixture(scope="module")
def generated():
    """3 000 generated records (more than one block of 16 rows; fewer records than lanes in the last block), and their mates"""
    a = qc.make_reads(3000, 1)
    b = [(name + b" mate/2", seq, qual) for name, seq, qual in qc.make_reads(3000, 2)]
    return tc.fastq(a), tc.fastq(b)


class Report:
    """a report open on the device for the length of a `with`; the host rule accumulates beside it and same() compares every word"""

    def __init__(self, dev, phred=33, adapters=None):
        self.dev, self.phred, self.adapters = dev, phred, adapters
        self.tables, self.clip = qc.new_tables(), qc.new_clip()
        self.had = None if adapters is None else hostapi.clip_parse_adapters(cc.adapters_fa(adapters))

    def __enter__(self):
        self.dev.qc_begin(self.phred)
        if self.adapters is not None:
            self.dev.clip_begin(self.adapters)
        assert not self.dev.qc_tables().any() and not self.dev.qc_clip_table().any()   # an untouched table is all zero
        return self

    def __exit__(self, *exc):
        if self.adapters is not None:
            self.dev.clip_end()
        self.dev.qc_end()

    def host(self, text, side=1, final=True, steps=None):
        h = hostapi.qc_fastq_chunk(text, tables=self.tables, clip=self.clip, side=side, phred=self.phred, final=final, steps=steps, adapters=self.had)
        assert h["clause"] == "none"
        return h

    def same(self):
        got, want = self.dev.qc_tables(), self.tables
        assert np.array_equal(got, want), [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(got != want)[:8]]
        assert np.array_equal(self.dev.qc_clip_table(), self.clip)


# ---- pf_qc_fastq: stage raw ----

@pytest.mark.parametrize("phred", [33, 64])
def test_edge_records(dev, phred):
    """every edge length, names of 1 to 16 bytes, lower case, N and other bytes, qualities below 0 and above 93"""
    text = tc.fastq(qc.edge_records(phred=phred))
    with Report(dev, phred) as r:
        for side in (0, 1):
            h = r.host(text, side + 1)
            assert dev.qc_fastq(text, side) == (h["bytes_used"], h["n_records"])
            r.same()
        t = dev.qc_tables()
        assert t[0][0][qc.W_QUAL_LOW] > 0 and t[0][0][qc.W_READS_NO_ACGT] >= 1 and t[0][0][qc.W_LENGTH + 1024] == 6
        assert phred == 64 or t[0][0][qc.W_QUAL_HIGH] > 0   # (byte 127 at offset 33; offset 64 has no printable byte above 93)
        assert t[0][0][qc.W_POS_BASE + 1023 * 5: qc.W_POS_BASE + 1024 * 5].sum() == 2 * (1 + 2 + 1977)   # the pooled bin: lengths 1024, 1025, 3000
        assert not t[:, 1].any()   # qc_fastq adds to stage raw alone


def test_one_record_and_one_of_every_length_alone(dev):
    for name, seq, qual in qc.edge_records()[:13]:
        text = tc.fastq([(name, seq, qual)])
        with Report(dev) as r:
            r.host(text)
            assert dev.qc_fastq(text) == (len(text), 1)
            r.same()


def test_generated_chunk_and_two_calls_into_one_report(dev, generated):
    with Report(dev) as r:
        r.host(generated[0])
        assert dev.qc_fastq(generated[0])[1] == 3000
        r.same()
        r.host(generated[1])   # a second call adds to the same tables
        dev.qc_fastq(generated[1])
        r.same()
        assert dev.qc_tables()[0][0][qc.W_READS] == 6000


def test_chunk_that_is_not_final_with_its_last_record_cut(dev, generated):
    text = generated[0][:40000]
    with Report(dev) as r:
        h = r.host(text, final=False)
        assert 0 < h["bytes_used"] < len(text)
        assert dev.qc_fastq(text, final=False) == (h["bytes_used"], h["n_records"])
        r.same()
    with Report(dev) as r:   # CRLF, and no last newline
        for t in (tc.fastq(qc.make_reads(40, 4), crlf=True), tc.fastq(qc.make_reads(40, 5), last_newline=False)):
            r.host(t)
            dev.qc_fastq(t)
            r.same()


def test_format_refusal_adds_nothing(dev):
    with Report(dev) as r:
        with pytest.raises(hipapi.DeviceError, match="record 1 of the chunk") as e:
            dev.qc_fastq(b"@r\nACGT\n+\nIIII\n@r2\nACGT\n+\nII\n")
        assert e.value.bad_record == 1
        r.same()


# ---- the trim calls with a report open: both stages ----

@pytest.mark.parametrize("steps", [tc.WORKFLOW, DROP_ALL], ids=["workflow", "drop_all"])
def test_trim_fastq_fills_both_stages(dev, generated, steps):
    text = generated[0] + tc.fastq(qc.edge_records())
    plain = dev.trim_fastq(text, steps)
    with Report(dev) as r:
        got = dev.trim_fastq(text, steps)
        r.host(text, steps=steps)
        r.same()
        kept = dev.qc_tables()[0][1]
        assert kept[qc.W_SEEN] == 1 and kept[qc.W_READS] == got["stats"]["kept"] and kept[qc.W_POS_BASE:qc.W_POS_QSUM].sum() == got["stats"]["bases_kept"]
    # out, begin, len and the statistics are what they are with no report open
    assert bytes(got["out"]) == bytes(plain["out"]) and got["stats"] == plain["stats"]
    assert got["begin"].tolist() == plain["begin"].tolist() and got["len"].tolist() == plain["len"].tolist()
    assert (got["bytes_used"], got["n_records"]) == (plain["bytes_used"], plain["n_records"])


def test_pair_calls_fill_both_sides(dev, generated):
    with Report(dev) as r:
        dev.trim_fastq_pair(generated[0], generated[1], tc.WORKFLOW)
        for side in (1, 2):
            r.host(generated[side - 1], side, steps=tc.WORKFLOW)
        r.same()
        t = dev.qc_tables()
        assert t[0][1][qc.W_READS] > 0 and t[1][1][qc.W_READS] > 0 and not np.array_equal(t[0][1], t[1][1])


def test_a_clip_open(dev, adapters):
    text = tc.fastq(cc.make_reads(600, adapters, seed=9))
    for steps in ([], GEN_STEPS):
        with Report(dev, adapters=adapters) as r:
            dev.trim_fastq(text, steps)
            r.host(text, steps=steps)
            r.same()
            assert dev.qc_clip_table()[0].sum() > 50 and not dev.qc_clip_table()[1].any()
            dev.count_begin(21)
            try:
                dev.count_fastq_trimmed(text, steps)   # K-TRIMCOUNT's hook: the same records once more
            finally:
                dev.count_abort()
            r.host(text, steps=steps)
            r.same()


# ---- the state on the context ----

def test_begin_get_and_end_refusals(dev):
    for call, word in ((lambda: dev.qc_tables(), "pf_qc_get: no report is open"), (lambda: dev.qc_clip_table(), "pf_qc_clip_get: no report is open"),
                       (lambda: dev.qc_fastq(b"@r\nA\n+\nI\n"), "pf_qc_fastq: no report is open"), (lambda: dev.qc_end(), "pf_qc_end: no report is open"),
                       (lambda: dev.qc_begin(50), "pf_qc_begin: the quality offset is 33 or 64, not 50")):
        with pytest.raises(hipapi.DeviceError, match=word):
            call()
    dev.qc_begin()
    try:
        with pytest.raises(hipapi.DeviceError, match="pf_qc_begin: a report is open already"):
            dev.qc_begin()
        with pytest.raises(hipapi.DeviceError, match="side is 0 or 1"):
            dev.qc_fastq(b"@r\nA\n+\nI\n", side=2)
    finally:
        dev.qc_end()


def test_kernel_time_one_launch_a_file_units_are_records(dev, generated):
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        dev.trim_fastq(generated[0], tc.WORKFLOW)   # no report open: nothing is launched
        assert dev.kernel_time(hipapi.K_QC)[1] == 0 and dev.kernel_units(hipapi.K_QC) == 0
        with Report(dev):
            dev.reset_timing()
            dev.qc_fastq(generated[0])
            assert dev.kernel_time(hipapi.K_QC)[1] == 1 and dev.kernel_units(hipapi.K_QC) == 3000
            dev.trim_fastq(generated[0], tc.WORKFLOW)
            assert dev.kernel_time(hipapi.K_QC)[1] == 2 and dev.kernel_units(hipapi.K_QC) == 6000
            dev.trim_fastq_pair(generated[0], generated[1], tc.WORKFLOW)
            ms, n = dev.kernel_time(hipapi.K_QC)
            assert n == 4 and ms > 0 and dev.kernel_units(hipapi.K_QC) == 12000
    finally:
        dev.enable_timing(False)
