"""The rule of the read quality report (K-QC, `qc`, `--report`; csrc/pf_qc_rule.hpp) restated in plain Python: what a read adds to a
table, the words of a table, the hint about the quality offset, the text of the report -- and the generators and hand-worked records
the tests share.  Integers only; every comparison made with it is exact."""
import random

import numpy as np

import clip_cases as cc
import trim_cases as tc

POS_BINS, LEN_BINS, Q_BINS, GC_BINS, CLASSES, Q_MAX = 1024, 1025, 94, 101, 5, 93
(W_SEEN, W_READS, W_MIN_LEN, W_MAX_LEN, W_MIN_BYTE, W_MAX_BYTE, W_QUAL_LOW, W_QUAL_HIGH, W_READS_NO_ACGT, W_LENGTH) = range(10)
W_QUALITY = W_LENGTH + LEN_BINS
W_READ_QUALITY = W_QUALITY + Q_BINS
W_GC_PERCENT = W_READ_QUALITY + Q_BINS
W_POS_BASE = W_GC_PERCENT + GC_BINS
W_POS_QSUM = W_POS_BASE + POS_BINS * CLASSES
W_POS_Q20 = W_POS_QSUM + POS_BINS
W_POS_Q30 = W_POS_Q20 + POS_BINS
TABLE_WORDS = W_POS_Q30 + POS_BINS
CLIP_WORDS = LEN_BINS
RAW, KEPT = 0, 1
assert TABLE_WORDS == 9515

# the lengths at which the kernel takes another path: a lane's 16 positions, a row step of 256, the pooled bin 1023, the pooled length 1024
EDGE_LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 1022, 1023, 1024, 1025, 3000]


def new_tables():
    return np.zeros((2, 2, TABLE_WORDS), dtype=np.uint64)


def new_clip():
    return np.zeros((2, CLIP_WORDS), dtype=np.uint64)


def base_class(c: int) -> int:
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(c & 0xDF, 4)


def add_record(t, seq: bytes, qual: bytes, b: int, e: int, phred: int = 33):
    """one record with the interval [b, e) into the table t (a list or array of TABLE_WORDS integers)"""
    L = e - b
    if int(t[W_READS]) == 0 or L < int(t[W_MIN_LEN]):
        t[W_MIN_LEN] = L
    no_byte_yet = int(t[W_MAX_LEN]) == 0
    t[W_MAX_LEN] = max(int(t[W_MAX_LEN]), L)
    t[W_READS] += 1
    t[W_LENGTH + min(L, 1024)] += 1
    sum_qc = gc = acgt = 0
    for p in range(b, e):
        bin_ = min(p - b, 1023)
        cls = base_class(seq[p])
        q = qual[p] - phred
        qc = min(max(q, 0), Q_MAX)
        t[W_POS_BASE + bin_ * CLASSES + cls] += 1
        t[W_POS_QSUM + bin_] += qc
        t[W_POS_Q20 + bin_] += q >= 20
        t[W_POS_Q30 + bin_] += q >= 30
        t[W_QUALITY + qc] += 1
        t[W_QUAL_LOW] += q < 0
        t[W_QUAL_HIGH] += q > Q_MAX
        if (no_byte_yet and p == b) or qual[p] < int(t[W_MIN_BYTE]):
            t[W_MIN_BYTE] = qual[p]
        t[W_MAX_BYTE] = max(int(t[W_MAX_BYTE]), qual[p])
        sum_qc += qc
        acgt += cls < 4
        gc += cls in (1, 2)
    if L == 0:
        return
    t[W_READ_QUALITY + sum_qc // L] += 1
    if acgt:
        t[W_GC_PERCENT + 100 * gc // acgt] += 1
    else:
        t[W_READS_NO_ACGT] += 1


def add_chunk(tables, clip, text: bytes, side: int = 1, phred: int = 33, final: bool = True, steps=None, adapters=None, seed: int = 2, score: int = 10):
    """the whole records of one chunk of file `side` (1 or 2): raw, and with steps (a list, may be empty beside adapters) kept and the
    clip curve.  Returns (records, bytes used)."""
    recs, used = tc.parse_records(text, final)
    if not recs:
        return 0, used
    raw, kept = tables[side - 1][RAW], tables[side - 1][KEPT]
    raw[W_SEEN] = 1
    if steps is not None:
        kept[W_SEEN] = 1
    for _, seq, _, qual in recs:
        add_record(raw, seq, qual, 0, len(qual), phred)
        if steps is None:
            continue
        ce = len(qual)
        if adapters is not None:
            ce = cc.clip_read(seq, qual, adapters, side, seed, score, phred)[0]
            if ce < len(qual):
                clip[side - 1][min(ce, 1024)] += 1
        iv = tc.trim_read(tc.quals(qual[:ce], phred), steps)
        if iv and iv[1] > iv[0]:
            add_record(kept, seq, qual, iv[0], iv[1], phred)
    return len(recs), used


def phred_hint(min_byte: int, reads: int) -> int:
    if reads == 0:
        return 0
    if min_byte < 59:
        return 33
    if min_byte >= 64:
        return 64
    return 0


def totals(t):
    base = np.asarray(t[W_POS_BASE:W_POS_QSUM], dtype=np.uint64).reshape(POS_BINS, CLASSES)
    return dict(bases=int(base.sum()), bases_acgt=int(base[:, :4].sum()), gc=int(base[:, 1:3].sum()), q20=int(np.asarray(t[W_POS_Q20:W_POS_Q30]).sum()),
                q30=int(np.asarray(t[W_POS_Q30:TABLE_WORDS]).sum()))


def hint_of(tables) -> int:
    raws = [tables[s][RAW] for s in range(2) if int(tables[s][RAW][W_MAX_LEN]) > 0]
    return phred_hint(min((int(t[W_MIN_BYTE]) for t in raws), default=0), len(raws))


def report_text(tables, clip=None, phred: int = 33) -> bytes:
    """the bytes `qc` and `--report` write"""
    o = ["# ploidyfrost qc 1", "# phred %d hint %d" % (phred, hint_of(tables))]
    seen = [(s, st, tables[s][st]) for s in range(2) for st in range(2) if int(tables[s][st][W_SEEN])]
    name = ("raw", "kept")

    def row(*cells):
        o.append("\t".join(str(int(c)) if not isinstance(c, str) else c for c in cells))

    o.append(">>totals")
    row("side", "stage", "reads", "bases", "bases_acgt", "gc", "q20", "q30", "qual_low", "qual_high", "min_len", "max_len", "min_byte", "max_byte", "reads_no_acgt")
    for s, st, t in seen:
        tt = totals(t)
        row(s + 1, name[st], t[W_READS], tt["bases"], tt["bases_acgt"], tt["gc"], tt["q20"], tt["q30"], t[W_QUAL_LOW], t[W_QUAL_HIGH], t[W_MIN_LEN], t[W_MAX_LEN],
            t[W_MIN_BYTE], t[W_MAX_BYTE], t[W_READS_NO_ACGT])
    o.append(">>position")
    row("side", "stage", "pos", "reads_here", "A", "C", "G", "T", "other", "qsum", "q20", "q30")
    for s, st, t in seen:
        base = np.asarray(t[W_POS_BASE:W_POS_QSUM], dtype=np.uint64).reshape(POS_BINS, CLASSES)
        here = base.sum(axis=1)
        nz = np.nonzero(here)[0]
        for b in range(int(nz[-1]) + 1 if len(nz) else 0):
            row(s + 1, name[st], "%d%s" % (b, "+" if b == 1023 else ""), here[b], *base[b], t[W_POS_QSUM + b], t[W_POS_Q20 + b], t[W_POS_Q30 + b])
    for title, cols, word, bins, pooled in (("length", ("length", "reads"), W_LENGTH, LEN_BINS, True), ("quality", ("quality", "bases"), W_QUALITY, Q_BINS, False),
                                            ("read_quality", ("mean_quality", "reads"), W_READ_QUALITY, Q_BINS, False),
                                            ("gc_percent", ("gc_percent", "reads"), W_GC_PERCENT, GC_BINS, False)):
        o.append(">>" + title)
        row("side", "stage", *cols)
        for s, st, t in seen:
            for i in range(bins):
                if int(t[word + i]):
                    row(s + 1, name[st], "%d%s" % (i, "+" if pooled and i == bins - 1 else ""), t[word + i])
    o.append(">>clip")
    row("side", "clip_end", "reads")
    if clip is not None:
        for s in range(2):
            for i in range(CLIP_WORDS):
                if int(clip[s][i]):
                    row(s + 1, "%d%s" % (i, "+" if i == 1024 else ""), clip[s][i])
    return ("\n".join(o) + "\n").encode()


def side_line(side: int, raw) -> str:
    tt = totals(raw)
    return "qc: side %d reads %d bases %d q20 %d q30 %d gc %d min_len %d max_len %d" % (side, raw[W_READS], tt["bases"], tt["q20"], tt["q30"], tt["gc"], raw[W_MIN_LEN],
                                                                                        raw[W_MAX_LEN])


def rows_of(report: bytes, side: int, stage: str):
    """the rows of every section of a report that belong to (side, stage), without those two columns: {section: [row, ...]}"""
    out, sec = {}, None
    for line in report.decode().split("\n"):
        if line.startswith(">>"):
            sec = line[2:]
            out[sec] = []
        elif sec and sec != "clip" and line.startswith("%d\t%s\t" % (side, stage)):
            out[sec].append(line.split("\t")[2:])
    return out


# ---- generators ----

def edge_records(seed: int = 7, phred: int = 33):
    """a record of every edge length under names of 1 to 16 bytes (lines start at every alignment mod 16): bases with lower case, N and
    other bytes, qualities over the whole range with the bytes below 0 and above 93 among them"""
    rng = random.Random(seed)
    lo, hi = (32, 127) if phred == 33 else (63, 126)
    recs = []
    for i, n in enumerate(EDGE_LENGTHS * 2):
        name = b"r" * (i % 16 + 1)
        seq = bytes(rng.choice(b"ACGTACGTACGTacgtNn.-*R") for _ in range(n))
        if i % 3 == 0:
            qual = bytes(rng.choice((lo, lo + 1, hi - 1, hi, phred + 20, phred + 30, phred + 19, phred + 29)) for _ in range(n))
        else:
            qual = bytes(rng.randrange(phred, phred + 42) for _ in range(n))
        recs.append((name, seq, qual))
    recs.append((b"x", b"NNNN....", bytes([phred + 40] * 8)))          # no ACGT at all
    recs.append((b"gc", b"GCGCgcgcGC", bytes([phred + 2] * 10)))       # gc 100
    return recs


def make_reads(n: int, seed: int, phred: int = 33):
    """n generated records: trim_cases' quality shapes (all four outcomes of the workflow's steps) with N and lower case sprinkled in"""
    rng = random.Random(seed)
    out = []
    for name, seq, qual in tc.make_reads(n, seed, phred):
        s = bytearray(seq)
        for _ in range(len(s) // 40):
            s[rng.randrange(len(s))] = rng.choice(b"Nacgt")
        out.append((name, bytes(s), qual))
    return out


# ---- hand-worked records (phred 33) ----
# r1: ACGTN  qualities 0 19 20 29 30 ("!45>?")      r2: ggcc  qualities 40 40 40 40 ("IIII")      r3: empty
HAND_TEXT = b"@r1\nACGTN\n+\n!45>?\n@r2\nggcc\n+\nIIII\n@r3\n\n+\n\n"


def hand_raw():
    """the raw table of HAND_TEXT, every non-zero word written out"""
    t = [0] * TABLE_WORDS
    t[W_SEEN], t[W_READS], t[W_MIN_LEN], t[W_MAX_LEN], t[W_MIN_BYTE], t[W_MAX_BYTE] = 1, 3, 0, 5, 33, 73
    t[W_LENGTH + 0], t[W_LENGTH + 4], t[W_LENGTH + 5] = 1, 1, 1
    for q, c in ((0, 1), (19, 1), (20, 1), (29, 1), (30, 1), (40, 4)):
        t[W_QUALITY + q] = c
    t[W_READ_QUALITY + 19] = 1      # (0 + 19 + 20 + 29 + 30) // 5 = 98 // 5
    t[W_READ_QUALITY + 40] = 1
    t[W_GC_PERCENT + 50] = 1        # r1: C, G of A C G T
    t[W_GC_PERCENT + 100] = 1       # r2
    base = {0: {0: 1, 2: 1}, 1: {1: 1, 2: 1}, 2: {2: 1, 1: 1}, 3: {3: 1, 1: 1}, 4: {4: 1}}   # position: {class: count}
    for pos, cls in base.items():
        for c, v in cls.items():
            t[W_POS_BASE + pos * CLASSES + c] = v
    for pos, v in enumerate((40, 59, 60, 69, 30)):
        t[W_POS_QSUM + pos] = v
    for pos, v in enumerate((1, 1, 2, 2, 1)):
        t[W_POS_Q20 + pos] = v
    for pos, v in enumerate((1, 1, 1, 1, 1)):
        t[W_POS_Q30 + pos] = v
    return t


HAND_STEPS = ["LEADING:20", "MINLEN:3"]   # r1 -> [2, 5) "GTN"; r2 whole; r3 dropped


def hand_kept():
    t = [0] * TABLE_WORDS
    t[W_SEEN], t[W_READS], t[W_MIN_LEN], t[W_MAX_LEN], t[W_MIN_BYTE], t[W_MAX_BYTE] = 1, 2, 3, 4, 53, 73
    t[W_LENGTH + 3], t[W_LENGTH + 4] = 1, 1
    for q, c in ((20, 1), (29, 1), (30, 1), (40, 4)):
        t[W_QUALITY + q] = c
    t[W_READ_QUALITY + 26] = 1      # 79 // 3
    t[W_READ_QUALITY + 40] = 1
    t[W_GC_PERCENT + 50] = 1        # G of G T
    t[W_GC_PERCENT + 100] = 1
    base = {0: {2: 2}, 1: {3: 1, 2: 1}, 2: {4: 1, 1: 1}, 3: {1: 1}}
    for pos, cls in base.items():
        for c, v in cls.items():
            t[W_POS_BASE + pos * CLASSES + c] = v
    for pos, v in enumerate((60, 69, 70, 40)):
        t[W_POS_QSUM + pos] = v
    for pos, v in enumerate((2, 2, 2, 1)):
        t[W_POS_Q20 + pos] = v
    for pos, v in enumerate((1, 1, 2, 1)):
        t[W_POS_Q30 + pos] = v
    return t


HAND_REPORT = b"""# ploidyfrost qc 1
# phred 33 hint 33
>>totals
side\tstage\treads\tbases\tbases_acgt\tgc\tq20\tq30\tqual_low\tqual_high\tmin_len\tmax_len\tmin_byte\tmax_byte\treads_no_acgt
1\traw\t3\t9\t8\t6\t7\t5\t0\t0\t0\t5\t33\t73\t0
1\tkept\t2\t7\t6\t5\t7\t5\t0\t0\t3\t4\t53\t73\t0
>>position
side\tstage\tpos\treads_here\tA\tC\tG\tT\tother\tqsum\tq20\tq30
1\traw\t0\t2\t1\t0\t1\t0\t0\t40\t1\t1
1\traw\t1\t2\t0\t1\t1\t0\t0\t59\t1\t1
1\traw\t2\t2\t0\t1\t1\t0\t0\t60\t2\t1
1\traw\t3\t2\t0\t1\t0\t1\t0\t69\t2\t1
1\traw\t4\t1\t0\t0\t0\t0\t1\t30\t1\t1
1\tkept\t0\t2\t0\t0\t2\t0\t0\t60\t2\t1
1\tkept\t1\t2\t0\t0\t1\t1\t0\t69\t2\t1
1\tkept\t2\t2\t0\t1\t0\t0\t1\t70\t2\t2
1\tkept\t3\t1\t0\t1\t0\t0\t0\t40\t1\t1
>>length
side\tstage\tlength\treads
1\traw\t0\t1
1\traw\t4\t1
1\traw\t5\t1
1\tkept\t3\t1
1\tkept\t4\t1
>>quality
side\tstage\tquality\tbases
1\traw\t0\t1
1\traw\t19\t1
1\traw\t20\t1
1\traw\t29\t1
1\traw\t30\t1
1\traw\t40\t4
1\tkept\t20\t1
1\tkept\t29\t1
1\tkept\t30\t1
1\tkept\t40\t4
>>read_quality
side\tstage\tmean_quality\treads
1\traw\t19\t1
1\traw\t40\t1
1\tkept\t26\t1
1\tkept\t40\t1
>>gc_percent
side\tstage\tgc_percent\treads
1\traw\t50\t1
1\traw\t100\t1
1\tkept\t50\t1
1\tkept\t100\t1
>>clip
side\tclip_end\treads
"""
