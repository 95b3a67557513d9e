"""K-CLIP on the device (pf_clip_begin .. pf_clip_end around pf_trim_fastq[_pair], pf_trim_table_fastq[_pair] and pf_count_fastq_trimmed
through hipapi) against the host's plain restatement of csrc/pf_clip_rule.hpp (hostapi.trim_fastq_chunk_clip; test_clip_cpu.py holds
that one to the Python rule).  Byte-exact: begin, len, out, the trimming statistics and the clip's counters are equal; there is no
tolerance anywhere.  The shapes are the smallest at which the kernel can go wrong (a row step is 256 bytes with a halo of 128, a
lane's unit 16, an adapter 16 .. 128 bases), not workload sizes."""
import random

import numpy as np
import pytest
import torch

import clip_cases as cc
import trim_cases as tc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
ZERO = {f: [0, 0] for f in cc.STATS}
GEN_STEPS = ["LEADING:5", "TRAILING:5", "MINLEN:20"]   # (the generated qualities are uniform 2 .. 40: the workflow's window drops nearly every read)


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def adapters():
    return cc.make_adapters([34, 58, 16, 128], seed=3, sides=[0, 1, 2, 0])


@pytest.fixture(scope="module")
def generated(adapters):
    """3 000 reads of 30 .. 300 bases, a third with a planted adapter mutated at 0 .. 3 places, and their mates"""
    a = cc.make_reads(3000, adapters, seed=1)
    b = [(name + b" mate/2", seq, qual) for name, seq, qual in cc.make_reads(3000, adapters, seed=2)]
    return tc.fastq(a), tc.fastq(b)


class Clip:
    """a clip open on the device for the length of a `with`; check() compares a call with the host rule and the counters with it"""

    def __init__(self, dev, adapters, seed=2, score=10):
        self.dev, self.adapters, self.seed, self.score = dev, adapters, seed, score
        self.seen = dict(ZERO)

    def __enter__(self):
        self.dev.clip_begin(self.adapters, self.seed, self.score)
        assert self.dev.clip_stats() == ZERO
        return self

    def __exit__(self, *exc):
        self.dev.clip_end()

    def host(self, text, steps, side=1, final=True, phred=33):
        return hostapi.trim_fastq_chunk_clip(text, steps, self.adapters, side=side, seed=self.seed, score=self.score, phred=phred, final=final)

    def counters(self, *wants):
        """the device's counters have grown by what the host rule counted"""
        now = self.dev.clip_stats()
        for f in cc.STATS:
            assert now[f] == [self.seen[f][j] + sum(w["clip"][f][j] for w in wants) for j in range(2)], f
        self.seen = now

    def check(self, text, steps, final=True, phred=33, out=None):
        got = self.dev.trim_fastq(text, steps, phred=phred, final=final, out=out)
        want = self.host(bytes(text) if isinstance(text, (bytes, bytearray)) else bytes(text.cpu().numpy()), steps, final=final, phred=phred)
        assert want["clause"] == "none"
        o = got["out"].cpu().numpy() if isinstance(got["out"], torch.Tensor) else got["out"]
        assert bytes(o) == want["out"]
        assert got["bytes_used"] == want["bytes_used"] and got["n_records"] == want["n_records"]
        assert got["begin"].tolist() == want["begin"] and got["len"].tolist() == want["len"]
        assert got["stats"] == want["stats"]
        self.counters(want)
        return want


def pair_out(t1, t2, w1, w2):
    """o1 u1 o2 u2 from the two files' (begin, len) arrays"""
    out = [bytearray() for _ in range(4)]
    r1, r2 = tc.parse_records(t1)[0], tc.parse_records(t2)[0]
    for r in range(min(len(r1), len(r2))):
        k1, k2 = w1["len"][r] != 0, w2["len"][r] != 0
        if k1:
            out[0 if k2 else 1] += tc.record_bytes(r1[r], w1["begin"][r], w1["begin"][r] + w1["len"][r])
        if k2:
            out[2 if k1 else 3] += tc.record_bytes(r2[r], w2["begin"][r], w2["begin"][r] + w2["len"][r])
    return [bytes(o) for o in out]


def edge_groups():
    """the edge list as one FASTQ text per adapter length; the names differ in length, so that the lines start at every alignment"""
    groups = {}
    for i, (seq, qual, ads) in enumerate(cc.edge_reads()):
        groups.setdefault(ads[0][0], []).append((b"e%d%s" % (i, b"." * (i % 16)), seq, qual))
    return [([(ad, 0)], tc.fastq(recs)) for ad, recs in groups.items()]


# ---- the edge list ----

@pytest.mark.parametrize("steps", [[], tc.WORKFLOW, ["MINLEN:16", "LEADING:31"]], ids=["none", "workflow", "minlen_leading"])
def test_edge_reads(dev, steps):
    outcomes = set()
    for ads, text in edge_groups():
        for seed, score in ((2, 10), (0, 9), (8, 1)):
            with Clip(dev, ads, seed, score) as c:
                want = c.check(text, steps)
                outcomes |= {"clipped"} if want["clip"]["reads_clipped"][0] else set()
                outcomes |= {"dropped"} if want["clip"]["reads_dropped"][0] else set()
                outcomes |= {"untouched"} if want["clip"]["reads_clipped"][0] + want["clip"]["reads_dropped"][0] < want["n_records"] else set()
    assert outcomes == {"clipped", "dropped", "untouched"}


def test_hand_cases(dev):
    for seq, qual, ads, side, seed, score, phred, end in cc.hand_cases():
        text = tc.fastq([(b"h", seq, qual)])
        with Clip(dev, ads, seed, score) as c:
            if side == 1:
                want = c.check(text, [], phred=phred)
                assert want["len"] == [end]
            else:   # file 2 of a pair (file 1 is the same read: its adapters are those of side 0 and 1)
                got = dev.trim_fastq_pair(text, text, [], phred=phred)
                assert got["len"][1].tolist() == [end] and got["len"][0].tolist() == c.host(text, [], side=1, phred=phred)["len"]


# ---- text shapes ----

def test_every_alignment_of_the_lines(dev, adapters):
    """sequence and quality lines that start at every offset 0 .. 15 of a 16-byte unit (a padded name), the adapter at a fixed offset"""
    rng = random.Random(4)
    ad = adapters[0][0]
    recs = []
    for a in range(16):
        for n, o in ((150, 100), (151, 120), (40, -5)):
            recs.append((b"n" * a + b"x" * (n % 7), cc.plant(rng, n, ad, o), bytes(33 + rng.randint(2, 40) for _ in range(n))))
    text = tc.fastq(recs)
    starts, pos = {1: set(), 3: set()}, 0
    for i, line in enumerate(text.split(b"\n")[:-1]):
        if i % 4 in starts:
            starts[i % 4].add(pos % 16)
        pos += len(line) + 1
    assert starts[1] == starts[3] == set(range(16))
    with Clip(dev, adapters) as c:
        want = c.check(text, [])
        assert want["len"] == [100, 120, 0] * 16
        c.check(text, tc.WORKFLOW)


def test_long_reads_across_row_steps(dev, adapters):
    """reads of several 256-byte row steps with the adapter across a step edge, at every alignment of the line"""
    rng = random.Random(6)
    recs = []
    for i, ad in enumerate(a for a, _ in adapters):
        for o in (230, 255, 256, 257, 500, 511, 513, 767, 900):
            for n in (1000, o + 16, o + 17, o + len(ad) - 1):
                seq = cc.mutate(rng, cc.plant(rng, n, ad, o), o, min(n, o + len(ad)), rng.randint(0, 2))
                recs.append((b"L%d" % len(recs) + b"." * (len(recs) % 16), seq, bytes(33 + rng.randint(20, 40) for _ in range(n))))
    recs.append((b"long", cc.plant(rng, 70000, adapters[3][0], 69000), b"I" * 70000))
    text = tc.fastq(recs)
    with Clip(dev, [(a, 0) for a, _ in adapters]) as c:
        want = c.check(text, [])
        # (two of the four lengths hold the adapter whole or but for a base; 16 and 17 bases of a mutated adapter rarely reach T = 10)
        assert want["len"][-1] == 69000 and want["clip"]["reads_clipped"][0] > len(recs) // 3
        c.check(text, ["SLIDINGWINDOW:4:25", "MINLEN:300"])


def test_64_adapters_of_128_and_one_of_16(dev):
    rng = random.Random(8)
    many = cc.make_adapters([128] * 64, seed=12, sides=[i % 3 for i in range(64)])
    recs = []
    for i in range(200):
        n = rng.randint(16, 400)
        ad = many[rng.randrange(64)][0]
        seq = cc.plant(rng, n, ad, rng.randint(-112, n - 16)) if i % 2 else cc.rand_bases(rng, n)
        recs.append((b"m%d" % i, seq, bytes(33 + rng.randint(2, 40) for _ in range(n))))
    t1 = tc.fastq(recs)
    t2 = tc.fastq([(n + b"/2", s, q) for n, s, q in reversed(recs)])
    with Clip(dev, many) as c:
        c.check(t1, [])
        got = dev.trim_fastq_pair(t1, t2, [])
        w1, w2 = c.host(t1, [], side=1), c.host(t2, [], side=2)
        assert [g.tolist() for g in got["len"]] == [w1["len"], w2["len"]] and [bytes(o) for o in got["out"]] == pair_out(t1, t2, w1, w2)
        c.counters(w1, w2)
    one = cc.make_adapters([16], seed=13)
    recs = [(b"s%d" % i, cc.plant(rng, n, one[0][0], o), b"I" * n) for i, (n, o) in enumerate(((16, 0), (17, 1), (40, 24), (40, 25), (300, 250), (300, 284)))]
    with Clip(dev, one, seed=0, score=9) as c:
        want = c.check(tc.fastq(recs), [])
        assert want["len"] == [0, 1, 24, 40, 250, 284]
    with Clip(dev, one, seed=0, score=10) as c:   # 16 matches never reach T = 10
        assert c.check(tc.fastq(recs), [])["clip"]["reads_clipped"] == [0, 0]


# ---- generated reads, single and paired ----

def test_generated_reads_single_and_paired(dev, adapters, generated):
    t1, t2 = generated
    with Clip(dev, adapters) as c:
        want = c.check(t1, [])
        n = want["n_records"]
        assert want["clip"]["reads_clipped"][0] > n // 10 and want["clip"]["reads_dropped"][0] > n // 50
        kept = c.check(t1, GEN_STEPS)
        assert n // 2 < kept["stats"]["kept"] < n and kept["len"] != want["len"]   # the steps act on the clipped interval, and do something
        for steps in ([], GEN_STEPS):
            got = dev.trim_fastq_pair(t1, t2, steps)
            w1, w2 = c.host(t1, steps, side=1), c.host(t2, steps, side=2)
            for f, w in enumerate((w1, w2)):
                assert got["begin"][f].tolist() == w["begin"] and got["len"][f].tolist() == w["len"]
                assert {k: got["stats"][f][k] for k in ("reads", "kept", "dropped", "bases", "bases_kept")} == {k: w["stats"][k] for k in ("reads", "kept", "dropped", "bases", "bases_kept")}
            assert [bytes(o) for o in got["out"]] == pair_out(t1, t2, w1, w2)
            c.counters(w1, w2)
        assert w1["len"] != c.host(t1, GEN_STEPS, side=2)["len"]   # the /1 and /2 adapters make the files' sides differ


def test_chunk_cut_inside_each_line_of_the_last_record(dev, adapters, generated):
    recs = tc.parse_records(generated[0])[0][:6]
    recs = [(r[0][1:], r[1], r[2][1:], r[3]) for r in recs]
    text, head = tc.fastq(recs), tc.fastq(recs[:5])
    lines = text[len(head):].split(b"\n")
    cuts, pos = [], len(head)
    for line in lines[:4]:   # the line's first byte, its middle, its newline
        cuts += [pos, pos + len(line) // 2, pos + len(line)]
        pos += len(line) + 1
    with Clip(dev, adapters) as c:
        whole = c.check(text, [])
        for cut in cuts:
            first = c.check(text[:cut], [], final=False)
            assert first["bytes_used"] == len(head) and first["n_records"] == 5
            second = c.check(text[first["bytes_used"]:], [], final=True)
            assert first["out"] + second["out"] == whole["out"], cut


def test_device_pointers_alignment_and_repeatability(dev, adapters, generated):
    t1 = generated[0][:200000]
    t1 = t1[:tc.parse_records(t1, final=False)[1]]
    host = np.frombuffer(t1, dtype=np.uint8)
    with Clip(dev, adapters) as c:
        for shift in (0, 1, 8):   # the text and the output on the device, 16-byte aligned and not
            buf = torch.zeros(len(t1) + 32, dtype=torch.uint8, device="cuda")
            text = buf[shift: shift + len(t1)]
            text.copy_(torch.from_numpy(host.copy()))
            out = torch.full((len(t1) + 17,), 0x55, dtype=torch.uint8, device="cuda")[shift: shift + len(t1) + 1]
            torch.cuda.synchronize()
            first = c.check(text, tc.WORKFLOW, out=out)
            second = c.check(text, tc.WORKFLOW, out=out)   # twice with the same bytes
            torch.cuda.synchronize()
            assert first == second


# ---- the state: begin, end, what is accepted in between, refusals ----

def test_no_step_is_a_plan_only_while_a_clip_is_open(dev, adapters, generated):
    text = generated[0][:20000]
    text = text[:tc.parse_records(text, final=False)[1]]
    plain = dev.trim_fastq(text, tc.WORKFLOW)
    out = np.full(len(text) + 1, 0x55, dtype=np.uint8)
    with pytest.raises(hipapi.DeviceError, match="pf_trim_fastq: no step is given"):
        dev.trim_fastq(text, [], out=out)
    with Clip(dev, adapters) as c:
        c.check(text, [])
        with pytest.raises(hipapi.DeviceError, match="pf_clip_begin: a clip is open already"):
            dev.clip_begin(adapters)
        for steps, phred, word in ((["MINLEN:1"] * 9, 33, "more than 8 steps"), ([(7, 1, 0)], 33, "step 0: unknown step"), ([], 50, "the quality offset is 33 or 64, not 50")):
            with pytest.raises(hipapi.DeviceError, match=word):
                dev.trim_fastq(text, steps, phred=phred, out=out)
        at = tc._end_of(text, 7)
        with pytest.raises(hipapi.DeviceError) as e:   # a format refusal: nothing is written, nothing is counted
            dev.trim_fastq(text[:at] + b"#" + text[at + 1:], [], out=out)
        assert e.value.bad_record == 7 and (out == 0x55).all()
        c.counters()
        table = dev.trim_table_fastq(text, [])
        assert table["n_records"] == plain["n_records"]
    for fn, args in ((dev.trim_fastq, (text, [])), (dev.trim_table_fastq, (text, [])), (dev.trim_fastq_pair, (text, text, []))):
        with pytest.raises(hipapi.DeviceError, match="no step is given"):
            fn(*args)
    with pytest.raises(hipapi.DeviceError, match="pf_clip_end: no clip is open"):
        dev.clip_end()
    with pytest.raises(hipapi.DeviceError, match="pf_clip_stats_get: no clip is open"):
        dev.clip_stats()
    again = dev.trim_fastq(text, tc.WORKFLOW)   # without a clip: what it was
    assert bytes(again["out"]) == bytes(plain["out"]) and again["stats"] == plain["stats"]


def test_begin_refusals_by_name(dev):
    a16, a129 = b"ACGT" * 4, b"ACGT" * 32 + b"A"
    for ads, kw, word in (([(a16, 0)], dict(seed=9), "the adapter seed is 0 to 8 mismatches"), ([(a16, 0)], dict(score=0), "the adapter score is 1 to 1000"),
                          ([(a16, 0)], dict(score=1001), "the adapter score is 1 to 1000"), ([], {}, "no usable adapter"),
                          ([(a16, 0)] * 65, {}, "more than 64 usable adapters"), ([(a16, 0), (a16[:15], 0)], {}, "adapter 1: an adapter holds 16 to 128 bases"),
                          ([(a129, 0)], {}, "adapter 0: an adapter holds 16 to 128 bases"), ([(a16[:15] + b"N", 1)], {}, "adapter 0: an adapter holds a byte outside ACGTacgt"),
                          ([(a16, 3)], {}, "adapter 0: the side of an adapter is 0")):
        with pytest.raises(hipapi.DeviceError) as e:
            dev.clip_begin(ads, **kw)
        assert e.value.status == hipapi.PF_ERR_ARG and "pf_clip_begin: " + word in str(e.value), word
    with pytest.raises(hipapi.DeviceError, match="no clip is open"):   # none of them opened one
        dev.clip_end()


def test_kernel_is_timed_under_its_name(adapters, generated):
    d = hipapi.Device(0)
    try:
        d.enable_timing(True)
        d.clip_begin(adapters)
        r = d.trim_fastq(generated[0], tc.WORKFLOW)
        ms, launches = d.kernel_time(hipapi.K_CLIP)
        assert launches == 1 and ms > 0 and d.kernel_units(hipapi.K_CLIP) == r["n_records"]
        assert d.kernel_time(hipapi.K_TRIM)[1] == 1 and d.kernel_time(hipapi.K_TRIM)[0] >= ms   # inside the call's own launch
        d.trim_fastq_pair(generated[0], generated[1], [])
        assert d.kernel_time(hipapi.K_CLIP)[1] == 2 and d.kernel_units(hipapi.K_CLIP) == 3 * r["n_records"]
        d.clip_end()
        d.trim_fastq(generated[0], tc.WORKFLOW)
        assert d.kernel_time(hipapi.K_CLIP)[1] == 2 and d.kernel_time(hipapi.K_TRIM)[1] == 3
        assert d.L.pf_kernel_name(hipapi.K_CLIP).decode() == "k_clip"
    finally:
        d.close()


# ---- the table form ----

def table_of(text, w):
    """(read_off, read_len) of the kept records of one file from its (begin, len) arrays"""
    seq_begin, pos = [], 0
    for i, line in enumerate(text.split(b"\n")[:-1]):
        if i % 4 == 1:
            seq_begin.append(pos)
        pos += len(line) + 1
    return seq_begin, w["begin"], w["len"]


def test_table_and_count_forms(dev, adapters, generated):
    t1, t2 = generated[0][:300000], generated[1][:300000]
    n = min(len(tc.parse_records(t, final=False)[0]) for t in (t1, t2))
    t1, t2 = t1[:tc._end_of(t1, n)], t2[:tc._end_of(t2, n)]
    with Clip(dev, adapters) as c:
        for steps in ([], tc.WORKFLOW):
            w1, w2 = c.host(t1, steps, side=1), c.host(t2, steps, side=2)
            got = dev.trim_table_fastq(t1, steps)
            sb, b, ln = table_of(t1, w1)
            keep = [r for r in range(n) if ln[r]]
            assert got["read_off"].tolist() == [sb[r] + b[r] for r in keep] and got["read_len"].tolist() == [ln[r] for r in keep]
            assert got["stats"] == w1["stats"] and got["n_records"] == n and got["bytes_used"] == len(t1)
            c.counters(w1)
            got = dev.trim_table_fastq_pair(t1, t2, steps)
            sb2, b2, ln2 = table_of(t2, w2)
            both = [r for r in range(n) if ln[r] and ln2[r]]
            assert got["read_off"][0].tolist() == [sb[r] + b[r] for r in both] and got["read_len"][0].tolist() == [ln[r] for r in both]
            assert got["read_off"][1].tolist() == [sb2[r] + b2[r] for r in both] and got["read_len"][1].tolist() == [ln2[r] for r in both]
            c.counters(w1, w2)
            # the count of the clipped and trimmed reads is the count of the host rule's output
            dev.count_begin(21)
            try:
                used, ts, cs = dev.count_fastq_trimmed(t1, steps)
                assert used == len(t1) and ts == w1["stats"]
                km1, ct1, _ = dev.count_finish(1)
            except Exception:
                dev.count_abort()
                raise
            c.counters(w1)
            dev.count_begin(21)
            try:
                _, plain = dev.count_fastq(w1["out"])
                km2, ct2, _ = dev.count_finish(1)
            except Exception:
                dev.count_abort()
                raise
            assert {k: cs[k] for k in ("reads", "bases", "kmers")} == {k: plain[k] for k in ("reads", "bases", "kmers")}
            assert np.array_equal(km1, km2) and np.array_equal(ct1, ct2)


# ---- the clip ends of the last call (what the trim log reads) ----

def test_last_ends_are_the_last_call_s(dev, adapters, generated):
    text = generated[0][:40000]
    recs, used = tc.parse_records(text, final=False)
    text = text[:used]
    want = [hostapi.clip_read(r[1], r[3], adapters) for r in recs]
    with Clip(dev, adapters) as c:
        assert dev.clip_last_ends(0).tolist() == []   # before any call: no record is no refusal
        with pytest.raises(hipapi.DeviceError, match="pf_clip_last_ends: the last call clipped no such file"):
            dev.clip_last_ends(1)
        c.check(text, tc.WORKFLOW)
        assert dev.clip_last_ends(len(recs)).tolist() == want and dev.clip_last_ends(3).tolist() == want[:3]
        with pytest.raises(hipapi.DeviceError, match="the last call clipped %d records, not %d" % (len(recs), len(recs) + 1)):
            dev.clip_last_ends(len(recs) + 1)
        with pytest.raises(hipapi.DeviceError, match="the last call clipped no such file"):
            dev.clip_last_ends(1, file=1)
        with pytest.raises(hipapi.DeviceError, match="file is 0 or 1"):
            dev.clip_last_ends(0, file=2)
        # a call that takes no whole record clipped none: the older ends are gone, and asking for none is accepted
        none = dev.trim_fastq(text[:50], [], final=False)
        assert none["n_records"] == 0 and dev.clip_last_ends(0).tolist() == []
        with pytest.raises(hipapi.DeviceError, match="the last call clipped no such file"):
            dev.clip_last_ends(1)
        got = dev.trim_fastq_pair(text, text, [])
        assert got["n_records"] == len(recs) and dev.clip_last_ends(len(recs), file=0).tolist() == want
        assert dev.clip_last_ends(len(recs), file=1).tolist() == [hostapi.clip_read(r[1], r[3], adapters, side=2) for r in recs]
        with pytest.raises(hipapi.DeviceError):   # a refused call clipped none either
            dev.trim_fastq(text, [], phred=50)
        assert dev.clip_last_ends(0).tolist() == []
        with pytest.raises(hipapi.DeviceError, match="the last call clipped no such file"):
            dev.clip_last_ends(1)
