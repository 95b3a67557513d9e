"""K-PALIN on the device (pf_clip_begin_pairs .. pf_clip_end around pf_trim_fastq_pair and pf_trim_table_fastq_pair through hipapi)
against the host's plain restatement of palindrome mode in csrc/pf_clip_rule.hpp (hostapi.trim_fastq_pair_chunk_clip;
test_clip_pair_cpu.py holds that one to the Python rule).  Byte-exact: begin, len, the four outputs, the final clip ends of both
files, the trimming statistics, the clip's counters and the pair counters are equal; there is no tolerance anywhere.  The shapes are
the smallest at which the kernel can go wrong (a plane word is 32 positions, a piece 128, a round 16 insert lengths, a prefix 16 .. 128
bases, a read at most 1024), not workload sizes."""
import pytest
import torch

import clip_cases as cc
import clip_pair_cases as pc
import trim_cases as tc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
GEN_STEPS = ["LEADING:5", "TRAILING:5", "MINLEN:20"]   # (the generated qualities are uniform 2 .. 40: the workflow's window drops nearly every read)


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def prefix_pairs():
    return pc.make_prefix_pairs([34], seed=41)


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 20], seed=3, sides=[0, 1, 2])


@pytest.fixture(scope="module")
def generated(prefix_pairs, adapters):
    """2 000 pairs of 30 .. 300 bases, a third read-through; the headers differ in length by r % 17"""
    f1, f2 = pc.make_pairs(2000, prefix_pairs, seed=1, adapters=adapters)
    return tc.fastq(f1), tc.fastq(f2)


class PairClip:
    """a clip with prefix pairs open on the device for the length of a `with`; check() compares a paired call with the host rule, the
    final clip ends of both files with it, and the growth of both sets of counters with what the host rule counted"""

    def __init__(self, dev, adapters, prefix_pairs, **opt):
        self.dev, self.adapters, self.pairs, self.opt = dev, adapters, prefix_pairs, opt
        self.clip_seen = {f: [0, 0] for f in cc.STATS}
        self.pair_seen = dict(pairs_clipped=0, pairs_dropped=0, pairs_too_long=0, candidates_scored=0, bases_clipped=[0, 0])

    def __enter__(self):
        o = self.opt
        self.dev.clip_begin_pairs(self.adapters, self.pairs, o.get("seed", 2), o.get("score", 10), o.get("pair_score", 30), o.get("pair_min", 8),
                                  o.get("keep_both", False))
        assert self.dev.clip_stats() == self.clip_seen and self.dev.clip_pair_stats() == self.pair_seen
        return self

    def __exit__(self, *exc):
        self.dev.clip_end()

    def host(self, t1, t2, steps, final=True, phred=33):
        opt = {k: v for k, v in self.opt.items()}
        return hostapi.trim_fastq_pair_chunk_clip(t1, t2, steps, (self.adapters, self.pairs), phred=phred, final=final, **opt)

    def counters(self, want):
        now, pnow = self.dev.clip_stats(), self.dev.clip_pair_stats()
        for f in cc.STATS:
            assert now[f] == [self.clip_seen[f][j] + want["clip"][f][j] for j in range(2)], f
        for f in pc.PAIR_STATS[:4]:
            assert pnow[f] == self.pair_seen[f] + want["pairs"][f], f
        assert pnow["bases_clipped"] == [self.pair_seen["bases_clipped"][j] + want["pairs"]["bases_clipped"][j] for j in range(2)]
        self.clip_seen, self.pair_seen = now, pnow

    def check(self, t1, t2, steps, final=True, phred=33):
        got = self.dev.trim_fastq_pair(t1, t2, steps, phred=phred, final=final)
        want = self.host(t1, t2, steps, final=final, phred=phred)
        assert want["clause"] == "none"
        m = want["n_records"]
        assert got["n_records"] == m and list(got["bytes_used"]) == want["bytes_used"]
        for f in range(2):
            assert self.dev.clip_last_ends(m, f).tolist() == want["clip_end"][f], f
            assert got["begin"][f].tolist() == want["begin"][f] and got["len"][f].tolist() == want["len"][f], f
            assert got["stats"][f] == want["stats"][f]
        assert [bytes(o) for o in got["out"]] == want["out"]
        self.counters(want)
        return want


def named(recs1, recs2):
    """two FASTQ texts of the records; the names differ in length, so that the lines start at every alignment"""
    a = [(b"e%d%s" % (i, b"." * (i % 17)), s, q) for i, (s, q) in enumerate(recs1)]
    b = [(b"e%d%s/2" % (i, b":" * (i % 5)), s, q) for i, (s, q) in enumerate(recs2)]
    return tc.fastq(a), tc.fastq(b)


def edge_groups():
    groups = {}
    for s1, q1, s2, q2, pairs in pc.edge_pairs():
        g = groups.setdefault(pairs[0], ([], []))
        g[0].append((s1, q1))
        g[1].append((s2, q2))
    return [([p], *named(*g)) for p, g in groups.items()]


# ---- the edge grid and the hand cases ----

@pytest.mark.parametrize("steps", [[], tc.WORKFLOW], ids=["none", "workflow"])
def test_edge_grid(dev, steps):
    """read lengths 0 .. 1025 (equal and unequal) x prefix lengths 16 .. 128 x planted I in {0, 1, n - A}"""
    seen = dict(pairs_clipped=0, pairs_dropped=0, pairs_too_long=0)
    for pairs, t1, t2 in edge_groups():
        for opt in (dict(), dict(keep_both=True, pair_min=1, seed=0), dict(seed=8, pair_score=100, pair_min=16)):
            with PairClip(dev, [], pairs, **opt) as c:
                want = c.check(t1, t2, steps)
                for k in seen:
                    seen[k] += want["pairs"][k]
    assert all(v > 0 for v in seen.values()), seen


def test_hand_cases(dev):
    for s1, q1, s2, q2, ads, pairs, opt, ends in pc.hand_cases():
        t1, t2 = tc.fastq([(b"h", s1, q1)]), tc.fastq([(b"h/2", s2, q2)])
        dev_opt = {k: v for k, v in opt.items() if k != "phred"}
        with PairClip(dev, ads, pairs, **dev_opt) as c:
            want = c.check(t1, t2, [], phred=opt.get("phred", 33))
            assert [want["clip_end"][0][0], want["clip_end"][1][0]] == ends, opt


# ---- generated pairs ----

def test_generated_pairs_with_simple_adapters(dev, prefix_pairs, adapters, generated):
    """prefix pairs with three simple adapters; 2 000 pairs whose lines start at every alignment of a 16-byte unit"""
    t1, t2 = generated
    starts, pos = set(), 0
    for i, line in enumerate(t1.split(b"\n")[:-1]):
        if i % 4 == 1:
            starts.add(pos % 16)
        pos += len(line) + 1
    assert starts == set(range(16))
    with PairClip(dev, adapters, prefix_pairs, keep_both=True) as c:
        want = c.check(t1, t2, [])
        assert want["pairs"]["pairs_clipped"] > 500 and want["clip"]["candidates_scored"][0] > 0
        c.check(t1, t2, GEN_STEPS)
    with PairClip(dev, adapters, prefix_pairs) as c:
        want = c.check(t1, t2, GEN_STEPS)
        assert want["stats"][0]["only1"] > 300   # the reverse read of a clipped pair is dropped


def test_generated_pairs_with_prefix_pairs_alone(dev, prefix_pairs, generated):
    """n_adapters = 0: K-CLIP is not launched; two prefix pairs, the planted one second"""
    t1, t2 = generated
    two = pc.make_prefix_pairs([40], seed=7) + prefix_pairs
    dev.enable_timing(True)
    dev.reset_timing()
    try:
        with PairClip(dev, [], two, keep_both=True, seed=1, pair_score=25, pair_min=3) as c:
            want = c.check(t1, t2, GEN_STEPS)
            assert want["pairs"]["pairs_clipped"] > 500
        ms, launches = dev.kernel_time(hipapi.K_PALIN)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_PALIN) == 2000
        assert dev.kernel_time(hipapi.K_CLIP)[1] == 0
    finally:
        dev.enable_timing(False)


def test_non_final_chunk_where_file_2_holds_fewer_records(dev, prefix_pairs, adapters, generated):
    t1, t2 = generated
    a, b = t1[:30000], t2[:21000]
    with PairClip(dev, adapters, prefix_pairs, keep_both=True) as c:
        want = c.check(a, b, GEN_STEPS, final=False)
        assert 0 < want["n_records"] and want["bytes_used"][0] < len(a) - 2000 and want["bytes_used"][1] > len(b) - 1000
        assert dev.trim_fastq_pair(a[:10], b[:10], GEN_STEPS, final=False)["n_records"] == 0   # no whole record: nothing clipped
        assert dev.clip_last_ends(0, 0).tolist() == []
        c.counters(dict(clip={f: [0, 0] for f in cc.STATS}, pairs=dict(pairs_clipped=0, pairs_dropped=0, pairs_too_long=0, candidates_scored=0, bases_clipped=[0, 0])))


def test_device_text_and_the_table_call(dev, prefix_pairs, adapters, generated):
    """the chunks on device pointers; pf_trim_table_fastq_pair hands on the pairs of which both records are kept, cut to the final ends"""
    t1, t2 = generated
    d1, d2 = (torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda() for t in (t1, t2))
    with PairClip(dev, adapters, prefix_pairs, keep_both=True) as c:
        want = c.host(t1, t2, GEN_STEPS)
        got = dev.trim_fastq_pair(d1, d2, GEN_STEPS)
        assert [bytes(o) for o in got["out"]] == want["out"]
        c.counters(want)
        tab = dev.trim_table_fastq_pair(d1, d2, GEN_STEPS)
        both = [r for r in range(want["n_records"]) if want["len"][0][r] and want["len"][1][r]]
        assert tab["n_reads"] == len(both) > 1000
        for f in range(2):
            assert tab["read_len"][f].tolist() == [want["len"][f][r] for r in both]
            assert dev.clip_last_ends(want["n_records"], f).tolist() == want["clip_end"][f]
        c.counters(want)


def test_single_ended_calls_while_pairs_are_open(dev, prefix_pairs, adapters, generated):
    """a single-ended call clips with the simple adapters only; with none it clips nothing"""
    t1, _ = generated
    text = t1[: t1.index(b"@p200x")]
    with PairClip(dev, adapters, prefix_pairs) as c:
        got = dev.trim_fastq(text, GEN_STEPS)
        want = hostapi.trim_fastq_chunk_clip(text, GEN_STEPS, adapters)
        assert bytes(got["out"]) == want["out"] and dev.clip_stats() == want["clip"]
    with PairClip(dev, [], prefix_pairs) as c:
        got = dev.trim_fastq(text, GEN_STEPS)
        assert bytes(got["out"]) == hostapi.trim_fastq_chunk(text, GEN_STEPS)["out"]
        assert dev.clip_last_ends(got["n_records"], 0).tolist() == [len(r[1]) for r in tc.parse_records(text)[0]]
        assert dev.clip_stats() == {f: [0, 0] for f in cc.STATS}


def test_a_clip_without_pairs_is_what_it_was(dev, adapters, generated):
    """pf_clip_begin on the same input: each file clipped by simple mode alone, as before"""
    t1, t2 = generated
    dev.clip_begin(adapters)
    try:
        got = dev.trim_fastq_pair(t1, t2, GEN_STEPS)
        w = [hostapi.trim_fastq_chunk_clip(t, GEN_STEPS, adapters, side=f + 1) for f, t in enumerate((t1, t2))]
        assert [g.tolist() for g in got["len"]] == [w[0]["len"], w[1]["len"]] and [g.tolist() for g in got["begin"]] == [w[0]["begin"], w[1]["begin"]]
        now = dev.clip_stats()
        assert all(now[f] == [w[0]["clip"][f][0], w[1]["clip"][f][1]] for f in cc.STATS)
        with pytest.raises(hipapi.DeviceError, match="pf_clip_pair_stats_get: the open clip holds no prefix pairs"):
            dev.clip_pair_stats()
    finally:
        dev.clip_end()


def test_refusals_by_name(dev, prefix_pairs, adapters):
    P1, P2 = prefix_pairs[0]
    for ads, pairs, opt, word in (([], [], {}, "pf_clip_begin_pairs: no prefix pair"), ([], prefix_pairs * 9, {}, "more than 8 prefix pairs"),
                                  ([], [(P1, P2[:30])], {}, "prefix pair 0: the two entries of a prefix pair hold the same number of bases"),
                                  ([], prefix_pairs + [(P1[:15], P2[:15])], {}, "prefix pair 1: an adapter holds 16 to 128 bases"),
                                  ([], [(P1, P2[:33] + b"N")], {}, "prefix pair 0: an adapter holds a byte outside ACGTacgt"),
                                  ([(b"ACGT", 0)], prefix_pairs, {}, "adapter 0: an adapter holds 16 to 128 bases"),
                                  ([], prefix_pairs, dict(pair_score=0), "the adapter pair score is 1 to 1000"),
                                  ([], prefix_pairs, dict(pair_min=17), "the fewest adapter bases of a pair are 1 to 16"),
                                  ([], prefix_pairs, dict(seed=9), "the adapter seed is 0 to 8")):
        with pytest.raises(hipapi.DeviceError, match=word):
            dev.clip_begin_pairs(ads, pairs, **opt)
    with pytest.raises(hipapi.DeviceError, match="no clip is open"):
        dev.clip_pair_stats()
    dev.clip_begin_pairs(adapters, prefix_pairs)
    try:
        with pytest.raises(hipapi.DeviceError, match="pf_clip_begin_pairs: a clip is open already"):
            dev.clip_begin_pairs(adapters, prefix_pairs)
    finally:
        dev.clip_end()
