"""The rule of `ploidyfrost trim` (K-TRIM) restated in plain Python from its wording (include/ploidyfrost_hip.h, README), the case lists
of the CPU and GPU tests, and a seeded generator of reads.  Nothing here looks at the C++.

A read is a quality line of n bytes; q[i] = byte - phred (signed).  The state is [b, e) of the read, [0, n) at first, or dropped;
the steps apply in order; a dropped read stays dropped; a read with e == b after the last step is dropped."""
import random

WORKFLOW = ["LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20", "MINLEN:50"]   # step 1.trim of the reference's workflow
STATS = ("reads", "kept", "dropped", "bases", "bases_kept", "both", "only1", "only2", "neither")

# the step orders both test files run: the workflow's, MINLEN first, SLIDINGWINDOW before LEADING, LEADING twice with rising t, each alone
ORDERS = [
    WORKFLOW,
    ["MINLEN:50", "LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20"],
    ["SLIDINGWINDOW:3:20", "LEADING:10", "TRAILING:10", "MINLEN:50"],
    ["LEADING:10", "LEADING:30", "TRAILING:10"],
    ["LEADING:10"], ["TRAILING:10"], ["SLIDINGWINDOW:3:20"], ["MINLEN:50"],
]
# further step sets of the edge list: w = 1, 3, 64, t = 0, eight steps
EDGE_STEPS = ORDERS + [
    ["SLIDINGWINDOW:1:20"], ["SLIDINGWINDOW:64:20"], ["LEADING:3", "TRAILING:3", "SLIDINGWINDOW:64:15", "MINLEN:1"],
    ["LEADING:0", "TRAILING:0", "SLIDINGWINDOW:3:0", "MINLEN:0"],
    ["LEADING:5", "TRAILING:5", "SLIDINGWINDOW:4:15", "LEADING:20", "TRAILING:20", "SLIDINGWINDOW:2:25", "MINLEN:2", "MINLEN:3"],
    ["LEADING:93", "TRAILING:93"],
]


def parse_steps(steps):
    if isinstance(steps, str):
        steps = steps.split()
    out = []
    for s in steps:
        name, *f = s.split(":")
        out.append((name,) + tuple(int(x) for x in f))
    return out


def trim_read(q, steps):
    """q: the qualities (ints).  (b, e), or None for a dropped read."""
    n = len(q)
    b, e = 0, n
    pre = None
    for st in parse_steps(steps):
        if st[0] == "LEADING":
            i = b
            while i < e and q[i] < st[1]:
                i += 1
            if i == e:
                return None
            b = i
        elif st[0] == "TRAILING":
            i = e - 1
            while i >= b and q[i] < st[1]:
                i -= 1
            if i < b:
                return None
            e = i + 1
        elif st[0] == "SLIDINGWINDOW":
            w, t = st[1], st[2]
            m = e - b
            if m < w:
                return None
            if pre is None:   # pre[i] = q[0] + .. + q[i - 1]: a window's badness does not depend on b
                pre = [0] * (n + 1)
                for i in range(n):
                    pre[i + 1] = pre[i] + q[i]
            first_bad = None
            for j in range(m - w + 1):
                if pre[b + j + w] - pre[b + j] < w * t:
                    first_bad = j
                    break
            if first_bad == 0:
                return None
            if first_bad is not None:
                e = b + first_bad - 1 + w
        elif st[0] == "MINLEN":
            if e - b < st[1]:
                return None
        else:
            raise ValueError(st[0])
    return (b, e) if e > b else None


def quals(line: bytes, phred: int = 33):
    return [c - phred for c in line]


def qline(q, phred: int = 33) -> bytes:
    return bytes(x + phred for x in q)


# ---- FASTQ text ----

def fastq(records, crlf=False, last_newline=True) -> bytes:
    """records: (name, seq, qual) or (name, seq, plus, qual); name without '@', plus without '+'"""
    nl = b"\r\n" if crlf else b"\n"
    out = bytearray()
    for rec in records:
        name, seq, plus, qual = rec if len(rec) == 4 else (rec[0], rec[1], b"", rec[2])
        out += b"@" + name + nl + seq + nl + b"+" + plus + nl + qual + nl
    if not last_newline and out:
        del out[-len(nl):]
    return bytes(out)


def parse_records(text: bytes, final=True):
    """([(header, seq, plus, qual) contents], bytes_used): whole records only; with final the last line may lack its newline"""
    lines, pos = [], 0
    while pos < len(text):
        nl = text.find(b"\n", pos)
        if nl < 0:
            if not final:
                break
            lines.append((text[pos:], len(text)))
            pos = len(text)
        else:
            end = nl - 1 if nl > pos and text[nl - 1:nl] == b"\r" else nl
            lines.append((text[pos:end], nl + 1))
            pos = nl + 1
    n = len(lines) // 4
    recs = [tuple(lines[4 * r + i][0] for i in range(4)) for r in range(n)]
    used = len(text) if final else (lines[4 * n - 1][1] if n else 0)
    return recs, used


def record_bytes(rec, b, e) -> bytes:
    return rec[0] + b"\n" + rec[1][b:e] + b"\n" + rec[2] + b"\n" + rec[3][b:e] + b"\n"


def _file_stats(recs, iv):
    kept = sum(1 for x in iv if x)
    return dict(reads=len(recs), kept=kept, dropped=len(recs) - kept, bases=sum(len(r[3]) for r in recs),
                bases_kept=sum(x[1] - x[0] for x in iv if x), both=0, only1=0, only2=0, neither=0)


def trim_fastq(text: bytes, steps, phred: int = 33, final=True):
    recs, used = parse_records(text, final)
    iv = [trim_read(quals(r[3], phred), steps) for r in recs]
    out = b"".join(record_bytes(r, *x) for r, x in zip(recs, iv) if x)
    return dict(out=out, bytes_used=used, n_records=len(recs), begin=[x[0] if x else 0 for x in iv], len=[x[1] - x[0] if x else 0 for x in iv],
                stats=_file_stats(recs, iv), records=recs)


def trim_pair(text1: bytes, text2: bytes, steps, phred: int = 33, final=True):
    """out = [o1, u1, o2, u2]; the smaller whole-record count of the two chunks is taken from each"""
    parsed = [parse_records(t, final) for t in (text1, text2)]
    n = min(len(parsed[0][0]), len(parsed[1][0]))
    recs = [p[0][:n] for p in parsed]
    used = []
    for t, p in zip((text1, text2), parsed):
        if n == len(p[0]):
            used.append(p[1])
        else:   # the end of record n - 1: where record n begins
            used.append(parse_records(t, False)[1] if n == 0 else _end_of(t, n))
    iv = [[trim_read(quals(r[3], phred), steps) for r in rs] for rs in recs]
    out = [bytearray() for _ in range(4)]
    both = only1 = only2 = 0
    for r in range(n):
        k1, k2 = iv[0][r], iv[1][r]
        if k1:
            out[0 if k2 else 1] += record_bytes(recs[0][r], *k1)
        if k2:
            out[2 if k1 else 3] += record_bytes(recs[1][r], *k2)
        both += bool(k1 and k2)
        only1 += bool(k1 and not k2)
        only2 += bool(k2 and not k1)
    stats = [_file_stats(recs[f], iv[f]) for f in range(2)]
    for s in stats:
        s.update(both=both, only1=only1, only2=only2, neither=n - both - only1 - only2)
    return dict(out=[bytes(o) for o in out], bytes_used=used if n else [0, 0], n_records=n,
                begin=[[x[0] if x else 0 for x in v] for v in iv], len=[[x[1] - x[0] if x else 0 for x in v] for v in iv], stats=stats, records=recs)


def _end_of(text: bytes, n_records: int) -> int:
    pos = 0
    for _ in range(4 * n_records):
        pos = text.find(b"\n", pos) + 1
    return pos


def trimlog(results) -> bytes:
    """results: one trim_fastq dict (single-ended) or one trim_pair dict.  A line per record in input order (for a pair: record r of file
    1, then record r of file 2): `<header without '@'> <kept length> <b> <e> <n - e>`; a dropped record gives 0 0 0 0."""
    paired = isinstance(results["stats"], list)
    files = [(results["records"][f], results["begin"][f], results["len"][f]) for f in range(2)] if paired \
        else [(results["records"], results["begin"], results["len"])]
    out = bytearray()
    for r in range(results["n_records"]):
        for recs, begin, ln in files:
            n, b, l = len(recs[r][3]), begin[r], ln[r]
            out += recs[r][0][1:] + (b" %d %d %d %d\n" % (l, b, b + l, n - (b + l)) if l else b" 0 0 0 0\n")
    return bytes(out)


# ---- the hand table (phred 33): q, the interval under WORKFLOW[:3], under SLIDINGWINDOW:3:20 LEADING:10 ----
HAND_STEPS = (["LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20"], ["SLIDINGWINDOW:3:20", "LEADING:10"])
HAND = [
    ([30, 30, 30, 30, 30], (0, 5), (0, 5)),
    ([5, 5, 30, 30, 30, 5], (2, 5), None),
    ([30, 30, 30, 10, 10, 30, 30], (0, 4), (0, 4)),
    ([20, 20, 20], (0, 3), (0, 3)),
    ([20, 20, 19], None, None),
    ([19, 20, 21, 20, 19, 30], (0, 6), (0, 6)),
    ([2, 2, 2, 2], None, None),
    ([30, 30, 5, 30, 30, 30], (0, 6), (0, 6)),
]


# ---- the edge list: the smallest shapes at which the kernels can go wrong ----
ROW_BYTES = 256   # a row step of k_trim_intervals: 16 lanes of 16 bytes
EDGE_LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]
LONG = 70000      # many steps of one row


def edge_quals(n: int, rich: bool = True):
    """(name, qualities) for a read of n bases"""
    hi, lo = 40, 2
    out = [("low", [lo] * n), ("high", [hi] * n)]
    if n >= 1:
        out += [("good_first", [hi] + [lo] * (n - 1)), ("good_last", [lo] * (n - 1) + [hi])]
    if n >= 4:
        out += [("window0_bad", [lo] * 3 + [hi] * (n - 3)), ("last_window_bad", [hi] * (n - 1) + [-19]),
                ("exact", [20] * n), ("exact_minus_one", [20] * (n - 1) + [19]), ("below_offset", [hi] * (n - 2) + [-1, -5]),
                ("top", [92] + [93] * (n - 2) + [92])]
    if rich:
        for edge in (16, 64, ROW_BYTES, 2 * ROW_BYTES, 1000):   # the first bad window straddling a unit, word and row-step edge
            for at in (edge - 2, edge - 1, edge):
                if 3 <= at < n - 1:
                    q = [hi] * n
                    q[at] = -19
                    out.append(("bad_at_%d" % at, q))
        if n >= 130:   # a dip only a wide window sees, and a low head and tail
            q = [hi] * n
            q[70:100] = [12] * 30
            out.append(("dip", q))
            out.append(("head_tail", [lo] * 17 + [hi] * (n - 40) + [lo] * 23))
    return out


def edge_records(phred: int = 33):
    """every edge read as a record; the names differ in length, so that the lines start at every alignment 0 .. 15"""
    recs = []
    for n in EDGE_LENGTHS:
        for name, q in edge_quals(n):
            recs.append((b"e%d_%s" % (n, name.encode()) + b"x" * (len(recs) % 16), b"ACGT" * (n // 4) + b"ACGT"[: n % 4], qline(q, phred)))
    q = [40] * LONG
    for name, qq in (("high", q), ("bad_late", q[:60000] + [3] * 5 + q[60005:]), ("low_head", [2] * 30000 + q[30000:]),
                     ("low_tail", q[:40000] + [2] * 30000), ("low", [2] * LONG)):
        recs.append((b"long_" + name.encode(), b"A" * LONG, qline(qq, phred)))
    return recs


# ---- generated reads ----
GEN_LENGTHS = (30, 49, 50, 51, 100, 150, 151, 250)


def make_reads(n: int, seed: int, phred: int = 33, lengths=GEN_LENGTHS):
    """n records (name, seq, qual), their lengths drawn from `lengths`.  Four quality shapes: flat 36; uniform noise 2..40; flat 36 with a tail that degrades from a
    random cut to 2..24; flat 36 between a head and a tail of quality 2, each of 0..19 bases.  The last shape is drawn twice as
    often as the others, so that all four outcomes of the workflow's steps (dropped, kept whole, b > 0, e < n) are well represented."""
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        ln = rng.choice(lengths)
        shape = rng.choice(("flat", "noise", "tail", "ends", "ends"))
        if shape == "flat":
            q = [36] * ln
        elif shape == "noise":
            q = [rng.randint(2, 40) for _ in range(ln)]
        elif shape == "tail":
            cut = rng.randrange(ln)
            q = [36] * cut + [rng.randint(2, 24) for _ in range(ln - cut)]
        else:
            h, t = rng.randint(0, min(19, ln)), rng.randint(0, 19)
            t = min(t, ln - h)
            q = [2] * h + [36] * (ln - h - t) + [2] * t
        seq = bytes(rng.choice(b"ACGT") for _ in range(ln))
        recs.append((b"r%d/%s" % (i, shape.encode()), seq, qline(q, phred)))
    return recs


def outcome_shares(recs, steps=WORKFLOW, phred: int = 33):
    """shares of dropped, kept whole, b > 0, e < n"""
    d = w = lead = trail = 0
    for _, _, qual in recs:
        iv = trim_read(quals(qual, phred), steps)
        if iv is None:
            d += 1
            continue
        w += iv == (0, len(qual))
        lead += iv[0] > 0
        trail += iv[1] < len(qual)
    n = float(len(recs))
    return d / n, w / n, lead / n, trail / n
