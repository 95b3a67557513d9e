"""K-DEDUP on the device (pf_dedup_begin .. pf_dedup_end around pf_trim_fastq[_pair], pf_trim_table_fastq, pf_count_fastq_trimmed and
pf_dedup_keys through hipapi) against the host's plain restatement of csrc/pf_dedup_rule.hpp (hostapi.trim_fastq_chunk_dedup,
hostapi.dedup_units; test_dedup_cpu.py holds those to the Python rule).  Every byte, interval, flag and statistic is equal; there is no
tolerance anywhere.  The shapes are the smallest at which the kernel can go wrong (a lane's word is 16 bases, a row step 256, a block 16
rows, a table of 64 slots that has to grow), not workload sizes."""
import numpy as np
import pytest

import clip_cases as cc
import dedup_cases as dc
import qc_cases as qc
import trim_cases as tc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
STEPS = ["LEADING:10", "TRAILING:10", "MINLEN:30"]
RULE_STATS = ("units", "unique", "duplicates", "max_copies", "levels")


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


class Dedup:
    """a dedup open on the device for the length of a `with`"""

    def __init__(self, dev, bases=0, initial_slots=0):
        self.dev, self.bases, self.slots = dev, bases, initial_slots

    def __enter__(self):
        self.dev.dedup_begin(self.bases, self.slots)
        return self

    def __exit__(self, *exc):
        self.dev.dedup_end()

    def rule_stats(self):
        s = self.dev.dedup_stats()
        return {f: s[f] for f in RULE_STATS}


def same_single(got, want):
    assert bytes(got["out"]) == want["out"] and got["bytes_used"] == want["bytes_used"] and got["n_records"] == want["n_records"]
    assert list(got["begin"]) == list(want["begin"]) and list(got["len"]) == list(want["len"]) and got["stats"] == want["stats"]


def same_pair(got, want):
    assert [bytes(o) for o in got["out"]] == want["outs"] and list(got["bytes_used"]) == list(want["bytes_used"]) and got["n_records"] == want["n_records"]
    for f in range(2):
        assert list(got["begin"][f]) == list(want["begin"][f]) and list(got["len"][f]) == list(want["len"][f]) and got["stats"][f] == want["stats"][f]


def host_stats(keys):
    """the rule's statistics of the units that took part (keys: [n, 2], 0 0 = took no part)"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
    _, st = hostapi.dedup_units(keys[keys.any(axis=1)])
    return {f: st[f] for f in RULE_STATS}


# ---- no dedup open ----

def test_no_dedup_open_then_one_open(dev):
    """with none open the calls give what the host rule of K-TRIM gives, refuse an empty list of steps and launch nothing of K-DEDUP;
    with one open a call is one timed launch whose unit is the units that take part"""
    text = tc.fastq(dc.dup_reads(700, 21))
    want = hostapi.trim_fastq_chunk(text, STEPS)
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        got = dev.trim_fastq(text, STEPS)
        assert bytes(got["out"]) == want["out"] and got["stats"] == want["stats"] and list(got["len"]) == list(want["len"])
        dev.count_begin(21)
        try:
            used, ts, cs = dev.count_fastq_trimmed(text, STEPS)
            assert used == len(text) and ts == want["stats"] and cs["reads"] == want["stats"]["kept"] and cs["bases"] == want["stats"]["bases_kept"]
        finally:
            dev.count_abort()
        with pytest.raises(hipapi.DeviceError, match="no step is given"):
            dev.trim_fastq(text, [])
        assert dev.kernel_time(hipapi.K_DEDUP)[1] == 0 and dev.kernel_units(hipapi.K_DEDUP) == 0
        with pytest.raises(hipapi.DeviceError, match="pf_dedup_stats_get: no dedup is open"):
            dev.dedup_stats()
        with pytest.raises(hipapi.DeviceError, match="pf_dedup_end: no dedup is open"):
            dev.dedup_end()
        with pytest.raises(hipapi.DeviceError, match="pf_dedup_begin: bases is 0 .the whole read. or 16 .. 4096, not 15"):
            dev.dedup_begin(15)
        with Dedup(dev) as d:
            with pytest.raises(hipapi.DeviceError, match="pf_dedup_begin: a dedup is open already"):
                dev.dedup_begin()
            h = hostapi.trim_fastq_chunk_dedup(text, STEPS)
            same_single(dev.trim_fastq(text, STEPS), h)
            ms, n = dev.kernel_time(hipapi.K_DEDUP)
            assert n == 1 and ms > 0 and dev.kernel_units(hipapi.K_DEDUP) == host_stats(h["keys"])["units"] == d.rule_stats()["units"]
            assert h["stats"]["kept"] < want["stats"]["kept"]
        same_single(dev.trim_fastq(text, STEPS), dict(want, begin=want["begin"], len=want["len"]))   # closed: as before
    finally:
        dev.enable_timing(False)


# ---- the key ----

@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("bases", [0, 16, 100])
def test_key_on_edge_reads(dev, bases, crlf):
    """every edge length with its near copies (the last base, a prefix, lower case, another non-ACGT byte), at every alignment mod 16"""
    recs = dc.edge_records()
    text = tc.fastq(recs, crlf=crlf)
    starts, pos = set(), 0
    for name, seq, _ in recs:
        starts.add((pos + len(name) + (3 if crlf else 2)) % 16)
        pos += len(tc.fastq([(name, seq, b"I" * len(seq))], crlf=crlf))
    assert starts == set(range(16))
    h = hostapi.trim_fastq_chunk_dedup(text, [], bases=bases)
    with Dedup(dev, bases) as d:
        same_single(dev.trim_fastq(text, []), h)
        assert d.rule_stats() == host_stats(h["keys"])
    kept = sum(1 for x in h["len"] if x)
    assert 0 < kept < sum(1 for r in recs if len(r[1]))   # (an empty read is dropped by K-TRIM itself and takes no part)


def test_long_reads_loop_over_row_steps(dev):
    rng = __import__("random").Random(9)
    a = dc.rand_seq(rng, 5000)
    recs = [(b"a", a, b"I" * 5000), (b"b", a[:4999] + b"N", b"I" * 5000), (b"c", a, b"I" * 5000), (b"d", a[:257], b"I" * 257), (b"e", a[:256], b"I" * 256),
            (b"f", a[:257], b"I" * 257)]
    text = tc.fastq(recs)
    for bases in (0, 256, 4096):
        h = hostapi.trim_fastq_chunk_dedup(text, [], bases=bases)
        with Dedup(dev, bases):
            same_single(dev.trim_fastq(text, []), h)
    assert [int(x != 0) for x in hostapi.trim_fastq_chunk_dedup(text, [], bases=4096)["len"]] == [1, 0, 0, 1, 1, 0]


# ---- the same key from many lanes at once ----

def test_same_key_race(dev):
    """200 copies of one read interleaved with 300 distinct ones in one call: exactly the first copy is kept"""
    rng = __import__("random").Random(5)
    one = dc.rand_seq(rng, 100)
    recs, copies = [], 0
    for i in range(500):
        if i % 5 in (0, 2):
            recs.append((b"copy%d" % copies, one, b"I" * 100))
            copies += 1
        else:
            recs.append((b"new%d" % i, dc.rand_seq(rng, 100), b"I" * 100))
    assert copies == 200
    text = tc.fastq(recs)
    with Dedup(dev) as d:
        r = dev.trim_fastq(text, ["MINLEN:50"])
        flags = [int(x != 0) for x in r["len"]]
        assert flags == [int(not rec[0].startswith(b"copy") or rec[0] == b"copy0") for rec in recs]
        assert r["stats"]["kept"] == 301 and r["stats"]["bases_kept"] == 30100
        st = d.rule_stats()
        assert st == dict(units=500, unique=301, duplicates=199, max_copies=200, levels=[300, 0, 0, 0, 0, 0, 0, 0, 0, 1])


# ---- across calls ----

def test_chunks_continue_the_stream_and_a_refused_chunk_changes_nothing(dev):
    recs = dc.dup_reads(900, 31, copies_of_one=7)
    text = tc.fastq(recs)
    whole = hostapi.trim_fastq_chunk_dedup(text, STEPS)
    ends = [len(tc.fastq(recs[:n])) for n in (1, 17, 400, 401, len(recs))]
    bad = tc.fastq([(b"bad", b"ACGT" * 10, b"IIII" * 9 + b"II")])   # a quality line shorter than its sequence
    with Dedup(dev) as d:
        pos, out, lens = 0, b"", []
        for i, end in enumerate(ends):
            final = end == len(text)
            chunk = text[pos:end] if final else text[pos:end + 37]   # a non-final chunk carries the head of the next record
            r = dev.trim_fastq(chunk, STEPS, final=final)
            assert r["bytes_used"] == end - pos
            out += bytes(r["out"])
            lens += list(r["len"])
            pos = end
            if i == 2:
                before = dev.dedup_stats()
                with pytest.raises(hipapi.DeviceError):
                    dev.trim_fastq(text[:ends[1]] + bad, STEPS)
                assert dev.dedup_stats() == before
        assert out == whole["out"] and lens == list(whole["len"])
        assert d.rule_stats() == host_stats(whole["keys"])
        # the unit numbers continue: the whole text once more is all duplicates of what the table holds
        again = dev.trim_fastq(text, STEPS)
        assert again["stats"]["kept"] == 0 and len(again["out"]) == 0


# ---- the slot protocol through pf_dedup_keys ----

def test_keys_with_one_h1(dev):
    keys = dc.keys_one_h1(4096)
    with Dedup(dev, initial_slots=64) as d:
        assert dev.dedup_keys(keys).all()
        st = dev.dedup_stats()
        assert st["unique"] == st["units"] == 4096 and st["max_copies"] == 1 and st["slots"] >= 2 * 4096
        assert not dev.dedup_keys(keys).any()
        assert d.rule_stats() == dict(units=8192, unique=4096, duplicates=4096, max_copies=2, levels=[0, 4096] + [0] * 8)


def test_keys_with_one_home_slot_grow_the_table(dev):
    """2 048 distinct keys that share their home slot in every table up to 2^20 slots, given in calls of growing size into a table of 64
    slots: long probe runs, a rehash in front of most calls"""
    keys = dc.keys_one_home(2048)
    assert len({int(k) & 0xFFFFF for k in keys[:, 0]}) == 1
    order = np.random.default_rng(6).permutation(2048)
    stream = np.concatenate([keys[order], keys[order[::3]]])   # every third key once more
    want, want_st = hostapi.dedup_units(stream)
    cuts = [0, 16, 40, 100, 300, 700, 1500, 2048, len(stream)]
    with Dedup(dev, initial_slots=64) as d:
        got = np.concatenate([dev.dedup_keys(stream[a:b]) for a, b in zip(cuts, cuts[1:])])
        assert np.array_equal(got, want)
        st = dev.dedup_stats()
        assert st["growths"] >= 5 and st["slots"] >= 4096
        assert d.rule_stats() == {f: want_st[f] for f in RULE_STATS}


def test_zero_words_and_device_pointers(dev):
    import torch
    keys = np.array([[0, 5], [1, 5], [7, 0], [7, 1], [0, 0], [1, 1]], dtype=np.uint64)
    want, _ = hostapi.dedup_units(keys)
    assert list(want) == [1, 0, 1, 0, 1, 0]
    with Dedup(dev, initial_slots=64):
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        keep = torch.zeros(len(keys), dtype=torch.uint8, device="cuda")
        dev.dedup_keys(dk, keep)
        assert keep.cpu().tolist() == list(want)


# ---- growth ----

def test_a_table_that_grows_decides_as_one_that_does_not(dev):
    recs = dc.dup_reads(5000, 41, share=0.3, length=40)
    text = tc.fastq(recs)
    results = []
    for slots in (64, 0):
        with Dedup(dev, initial_slots=slots):
            r = [dev.trim_fastq(text[a:b], ["MINLEN:20"]) for a, b in ((0, len(tc.fastq(recs[:1000]))), (len(tc.fastq(recs[:1000])), len(text)))]
            results.append((b"".join(bytes(x["out"]) for x in r), [list(x["len"]) for x in r], [x["stats"] for x in r], dev.dedup_stats()))
    (o64, l64, s64, st64), (o0, l0, s0, st0) = results
    assert o64 == o0 and l64 == l0 and s64 == s0
    assert {f: st64[f] for f in RULE_STATS} == {f: st0[f] for f in RULE_STATS} and 1000 < st0["duplicates"] < 2000
    assert st64["growths"] >= 2 and st0["growths"] == 0 and st0["slots"] == 1 << 20 and st64["slots"] >= 2 * 5000


# ---- pairs ----

def test_pairs(dev):
    rng = __import__("random").Random(8)
    a, b, c = (dc.rand_seq(rng, 100) for _ in range(3))
    good, poor = b"I" * 100, b"#" * 100
    r1 = [(b"p0", a, good), (b"p1", a, good), (b"p2", a, good), (b"p3", b, good), (b"p4", c, good), (b"p5", c, good), (b"p6", c, good), (b"p7", a.lower(), good)]
    r2 = [(b"p0", b, good), (b"p1", c, good), (b"p2", b, good), (b"p3", a, good), (b"p4", b, poor), (b"p5", b, good), (b"p6", b, good), (b"p7", b, good)]
    # p1: the same R1, another R2; p2: a copy of p0; p3: p0 swapped; p4: file 2 dropped, no unit; p5: the first intact (c, b); p6 its copy; p7: p0 in lower case
    t1, t2 = tc.fastq(r1), tc.fastq(r2, crlf=True)
    h = hostapi.trim_fastq_chunk_dedup(t1, STEPS, text2=t2)
    assert [int(x != 0) for x in h["len"][0]] == [1, 1, 0, 1, 1, 1, 0, 0] and [int(x != 0) for x in h["len"][1]] == [1, 1, 0, 1, 0, 1, 0, 0]
    assert h["stats"][0]["both"] == 4 and h["stats"][0]["only1"] == 1 and h["stats"][0]["neither"] == 3
    with Dedup(dev) as d:
        same_pair(dev.trim_fastq_pair(t1, t2, STEPS), h)
        assert d.rule_stats() == host_stats(h["keys"]) and d.rule_stats()["units"] == 7
    # generated pairs over several blocks, bases = 16, the table growing
    recs = dc.dup_reads(1500, 51)
    m = dc.mates(recs, 2)
    for i in range(0, 1500, 97):
        m[i] = (m[i][0], m[i][1], b"#" * len(m[i][1]))
    t1, t2 = tc.fastq(recs), tc.fastq(m)
    for bases in (0, 16):
        h = hostapi.trim_fastq_chunk_dedup(t1, STEPS, text2=t2, bases=bases)
        with Dedup(dev, bases, 64) as d:
            same_pair(dev.trim_fastq_pair(t1, t2, STEPS), h)
            assert d.rule_stats() == host_stats(h["keys"])
        with Dedup(dev, bases):
            t = dev.trim_table_fastq_pair(t1, t2, STEPS)
            assert t["n_reads"] == h["stats"][0]["both"] and t["stats"] == h["stats"]
            assert list(t["read_len"][0]) == [x for x, y in zip(h["len"][0], h["len"][1]) if x and y]


# ---- the trimmed counts ----

def test_trimmed_counts_take_the_deduplicated_reads(dev):
    text = tc.fastq(dc.dup_reads(1200, 61))
    h = hostapi.trim_fastq_chunk_dedup(text, STEPS)
    dev.count_begin(21)
    try:
        _, _, want = dev.count_fastq_trimmed(h["out"], ["MINLEN:1"])   # no dedup open: the deduplicated text as it is
    finally:
        dev.count_abort()
    dev.count_begin(21)
    try:
        with Dedup(dev, initial_slots=64) as d:
            used, ts, got = dev.count_fastq_trimmed(text, STEPS)
            assert d.rule_stats() == host_stats(h["keys"])
    finally:
        dev.count_abort()
    assert used == len(text) and ts == h["stats"] and got == want and got["reads"] == h["stats"]["kept"]
    with Dedup(dev):
        t = dev.trim_table_fastq(text, [])   # no step beside an open dedup
        h0 = hostapi.trim_fastq_chunk_dedup(text, [])
        assert t["n_reads"] == h0["stats"]["kept"] and t["stats"] == h0["stats"] and list(t["read_len"]) == [x for x in h0["len"] if x]


# ---- other state open ----

def test_report_open_stage_kept_is_what_is_written(dev):
    text = tc.fastq(dc.dup_reads(800, 71))
    h = hostapi.trim_fastq_chunk_dedup(text, STEPS)
    dev.qc_begin(33)
    try:
        dev.trim_fastq(text, STEPS)
        plain = dev.qc_tables()
    finally:
        dev.qc_end()
    dev.qc_begin(33)
    try:
        with Dedup(dev):
            same_single(dev.trim_fastq(text, STEPS), h)
        both = dev.qc_tables()
    finally:
        dev.qc_end()
    assert np.array_equal(both[0, 0], plain[0, 0])   # stage raw: what it is without a dedup
    want = qc.new_tables()
    hq = hostapi.qc_fastq_chunk(h["out"], tables=want, side=1, phred=33, steps=["MINLEN:1"])   # the written records, as they are
    assert hq["clause"] == "none"
    assert np.array_equal(both[0, 1], want[0, 1]) and int(both[0, 1][qc.W_READS]) == h["stats"]["kept"] < int(plain[0, 1][qc.W_READS])


def test_clip_open_the_key_is_of_the_raw_read(dev):
    """two reads equal before the clip are duplicates whatever the clip leaves of them; the clip's own counters are what they are
    without a dedup"""
    adapters = cc.make_adapters([34], seed=3, sides=[0])
    ad = adapters[0][0] if isinstance(adapters[0], (tuple, list)) else adapters[0]
    ad = ad.encode() if isinstance(ad, str) else bytes(ad)
    rng = __import__("random").Random(12)
    ins = [dc.rand_seq(rng, 60) for _ in range(40)]
    recs = []
    for i in range(200):
        s = ins[i % 40] + ad
        recs.append((b"r%d" % i, s, b"I" * len(s)))
    text = tc.fastq(recs)
    dev.clip_begin(adapters)
    try:
        plain = dev.trim_fastq(text, [])
        clip_plain = dev.clip_stats()
        assert plain["stats"]["kept"] == 200 and all(x == 60 for x in plain["len"])
    finally:
        dev.clip_end()
    dev.clip_begin(adapters)
    try:
        with Dedup(dev) as d:
            r = dev.trim_fastq(text, [])
            assert [int(x) for x in r["len"]] == [60] * 40 + [0] * 160 and r["stats"]["kept"] == 40 and r["stats"]["bases_kept"] == 2400
            assert bytes(r["out"]) == bytes(plain["out"])[: len(r["out"])]
            assert d.rule_stats() == dict(units=200, unique=40, duplicates=160, max_copies=5, levels=[0, 0, 0, 0, 40, 0, 0, 0, 0, 0])
            assert dev.clip_stats() == clip_plain
    finally:
        dev.clip_end()


def test_clip_report_and_dedup_open_together(dev):
    """reads that hold an adapter, a third of them written twice, with a clip, a report and a dedup open at once: the report's clip rows
    and stage raw are what they are without a dedup, stage kept counts exactly the written records, the clip's own counters stay"""
    adapters = cc.make_adapters([34], seed=3, sides=[0])
    ad = bytes(adapters[0][0])
    rng = __import__("random").Random(14)
    recs = []
    for i in range(600):
        if i % 3 == 2:
            seq = recs[rng.randrange(len(recs))][1]                                   # a copy of an earlier read, adapter and tail included
        elif i % 2:
            ins = rng.randrange(40, 66)
            seq = (dc.rand_seq(rng, ins) + ad + dc.rand_seq(rng, 100))[:100]          # read-through at a varying insert size
        else:
            seq = dc.rand_seq(rng, 100)
        recs.append((b"r%d" % i, seq, b"I" * 100))
    text = tc.fastq(recs)
    steps = ["MINLEN:20"]

    def run(dedup):
        dev.qc_begin(33)
        dev.clip_begin(adapters)
        try:
            if dedup:
                dev.dedup_begin()
            try:
                r = dev.trim_fastq(text, steps)
                st = dev.dedup_stats() if dedup else None
            finally:
                if dedup:
                    dev.dedup_end()
            return r, dev.qc_tables(), dev.qc_clip_table(), dev.clip_stats(), st
        finally:
            dev.clip_end()
            dev.qc_end()

    plain, tab0, clip0, cs0, _ = run(False)
    mine, tab1, clip1, cs1, st = run(True)
    assert int(clip0[0].sum()) > 150 and cs0["reads_clipped"][0] > 150      # the clip did something, and the report saw it
    assert np.array_equal(clip1, clip0) and np.array_equal(tab1[0, 0], tab0[0, 0]) and cs1 == cs0
    # the decision: the key is of the raw read, the intervals of the kept units are the clip's
    d, want_len = dc.Dedup(), []
    for rec, ln in zip(recs, plain["len"]):
        want_len.append(int(ln) if ln and d.unit(dc.key_of(rec[1])) else 0)
    assert [int(x) for x in mine["len"]] == want_len and 150 < st["duplicates"] == d.stats()["duplicates"] and st["units"] == d.stats()["units"]
    assert any(0 < a < 100 and b == 0 for a, b in zip(plain["len"], want_len))      # a clipped copy is among the dropped ones
    # stage kept: exactly the written records
    want = qc.new_tables()
    assert hostapi.qc_fastq_chunk(bytes(mine["out"]), tables=want, side=1, phred=33, steps=["MINLEN:1"])["clause"] == "none"
    assert np.array_equal(tab1[0, 1], want[0, 1]) and int(tab1[0, 1][qc.W_READS]) == mine["stats"]["kept"] < int(tab0[0, 1][qc.W_READS])
