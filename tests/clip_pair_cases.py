"""Palindrome adapter clipping (K-PALIN, `--adapter-pairs`) restated in plain Python, and the cases the CPU and GPU tests share: the
pair rule of csrc/pf_clip_rule.hpp as loops over prefix pairs and insert lengths (clip_cases holds the simple rule it is combined
with), the prefix-pair parser of the adapter file, seeded prefix pairs and read pairs with read-through planted (no vendor adapter
file is used anywhere), hand-worked pairs, and the clipping of whole FASTQ texts that the stream tests take as reference."""
import random

import clip_cases as cc
import trim_cases as tc

WINDOW, MATCH, PENALTY, UNIT = cc.WINDOW, cc.MATCH, cc.PENALTY, cc.UNIT
MAX_PAIRS, MAX_PAIR_READ, MIN_OVERLAP = 8, 1024, 16
READ_LENGTHS = [0, 1, 15, 16, 17, 100, 255, 256, 257, 1024, 1025]
PREFIX_LENGTHS = [16, 33, 34, 64, 65, 128]
PAIR_STATS = ("pairs_clipped", "pairs_dropped", "pairs_too_long", "candidates_scored", "bases_clipped")
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


# ---- the rule ----

def pair_candidate(s1: bytes, q1: bytes, s2: bytes, q2: bytes, P1: bytes, P2: bytes, I: int, seed: int, phred: int):
    """(seed holds, score) of prefix pair (P1, P2) at insert length I; (False, 0) where I lays fewer than 16 positions"""
    p, n1, n2 = len(P1), len(s1), len(s2)
    S1, S2 = P1 + s1, P2 + s2
    T = 2 * p + I
    lo, hi = max(0, p + I - n2), min(T, p + n1)
    if hi - lo < MIN_OVERLAP:
        return False, 0
    valid, match = [], []
    for i in range(lo, hi):
        a, b = S1[i] & 0xDF, S2[T - 1 - i] & 0xDF
        v = a in CODE and b in CODE
        valid.append(v)
        match.append(v and CODE[a] + CODE[b] == 3)
    run = sum(not m for m in match[:WINDOW])
    ok = run <= seed
    for w in range(1, len(match) - WINDOW + 1):
        if ok:
            break
        run += (not match[w + WINDOW - 1]) - (not match[w - 1])
        ok = run <= seed
    if not ok:
        return False, 0
    best = cur = 0
    for x, i in enumerate(range(lo, hi)):
        if not valid[x]:
            v = 0
        elif match[x]:
            v = MATCH
        else:
            j = T - 1 - i
            qs = ([q1[i - p] - phred] if i >= p else []) + ([q2[j - p] - phred] if j >= p else [])
            v = -PENALTY * max(min(qs), 0)
        cur = max(cur + v, 0)
        best = max(best, cur)
    return True, best


def pair_insert(s1, q1, s2, q2, prefix_pairs, seed=2, pair_score=30, pair_min=8, phred=33):
    """(I* or None, too long, candidates scored): prefix pairs in order, I upwards, below the best found so far"""
    n1, n2 = len(s1), len(s2)
    if n1 > MAX_PAIR_READ or n2 > MAX_PAIR_READ:
        return None, True, 0
    best, found, scored = max(min(n1, n2) - pair_min + 1, 0), False, 0
    for P1, P2 in prefix_pairs:
        for I in range(best):
            ok, s = pair_candidate(s1, q1, s2, q2, P1.upper(), P2.upper(), I, seed, phred)
            if not ok:
                continue
            scored += 1
            if s >= UNIT * pair_score:
                best, found = I, True
                break
    return (best if found else None), False, scored


def clip_pair(s1, q1, s2, q2, adapters, prefix_pairs, seed=2, score=10, pair_score=30, pair_min=8, keep_both=False, phred=33):
    """([final clip end of file 1, of file 2], [simple ends], I* or None, too long, pair candidates scored)"""
    simple = [cc.clip_read(s, q, adapters, side, seed, score, phred)[0] if adapters else len(s) for side, (s, q) in ((1, (s1, q1)), (2, (s2, q2)))]
    I, too_long, scored = pair_insert(s1, q1, s2, q2, prefix_pairs, seed, pair_score, pair_min, phred)
    if I is None:
        return list(simple), simple, None, too_long, scored
    return [min(simple[0], I), min(simple[1], I if keep_both else 0)], simple, I, too_long, scored


# ---- the adapter file with prefix pairs ----

def parse_adapter_pairs(text: bytes):
    """(adapters [(sequence, side)], prefix pairs [(P1, P2)]) or ("refusal name", 1-based record) as the rule header refuses the file
    under `--adapter-pairs`"""
    adapters, pairs, done, waiting, record = [], [], [], [], 0
    cur = None   # [name, sequence]

    def close():
        if cur is None:
            return None
        name, seq = cur[0], bytes(cur[1])
        if not cc.MIN_LEN <= len(seq) <= cc.MAX_LEN:
            return "length"
        if not name.startswith(b"Prefix"):
            if len(adapters) == cc.MAX_ADAPTERS:
                return "too_many"
            adapters.append((seq, 1 if name.endswith(b"/1") else 2 if name.endswith(b"/2") else 0))
            return None
        side = 1 if name.endswith(b"/1") else 2 if name.endswith(b"/2") else 0
        if side == 0:
            return "pair_partner"
        x = name[6:-2]
        if x in done:
            return "pair_partner"
        for w in waiting:
            if w[0] != x:
                continue
            if w[1] == side:
                return "pair_partner"
            if len(w[2]) != len(seq):
                return "pair_lengths"
            if len(pairs) == MAX_PAIRS:
                return "too_many_pairs"
            pairs.append((w[2], seq) if side == 2 else (seq, w[2]))
            done.append(x)
            waiting.remove(w)
            return None
        waiting.append((x, side, seq, record))
        return None

    lines = text.split(b"\n")
    ended = bool(lines) and lines[-1] == b""
    if ended:
        lines.pop()
    for i, line in enumerate(lines):
        if (i + 1 < len(lines) or ended) and line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        if line[:1] == b">":
            why = close()
            if why:
                return why, record
            record += 1
            cur = [line[1:].replace(b"\t", b" ").split(b" ")[0], bytearray()]
            continue
        if cur is None:
            return "not_fasta", 0
        for c in line:
            if c & 0xDF not in CODE:
                return "byte", record
        cur[1] += line.upper()
    why = close()
    if why:
        return why, record
    if record == 0:
        return "not_fasta", 0
    if waiting:
        return "pair_partner", waiting[0][3]
    if not pairs:
        return "no_pair", 0
    return adapters, pairs


def make_prefix_pairs(lengths, seed: int):
    rng = random.Random(seed)
    return [(cc.rand_bases(rng, p), cc.rand_bases(rng, p)) for p in lengths]


def adapters_fa(adapters, prefix_pairs, names=None) -> bytes:
    """the prefix pairs (PrefixPE<q>/1, /2) in front of the simple adapters of clip_cases.adapters_fa"""
    out = bytearray()
    for q, (P1, P2) in enumerate(prefix_pairs):
        x = names[q] if names else b"PE%d" % q
        out += b">Prefix" + x + b"/1\n" + P1 + b"\n>Prefix" + x + b"/2 reverse\n" + P2 + b"\n"
    return bytes(out) + (cc.adapters_fa(adapters) if adapters else b"")


# ---- seeded pairs ----

def read_through(rng, n1: int, n2: int, I: int, P1: bytes, P2: bytes, insert: bytes = None):
    """(R1, R2) of an insert of I bases sequenced with the prefix pair: R1 = insert . RC(P2) . random, R2 = RC(insert) . RC(P1) . random"""
    ins = cc.rand_bases(rng, I) if insert is None else insert
    r1 = (ins + revcomp(P2) + cc.rand_bases(rng, n1))[:n1]
    r2 = (revcomp(ins) + revcomp(P1) + cc.rand_bases(rng, n2))[:n2]
    return r1, r2


def make_pairs(n_pairs: int, prefix_pairs, seed: int, lengths=(30, 300), planted: float = 1 / 3, phred: int = 33, adapters=None, remnant=None):
    """n_pairs records per file [(name, seq, qual)]: a share `planted` of the pairs are read-through of a random insert (mutated at
    0 .. 3 places per read), others overlap without read-through or are unrelated; some carry a planted simple adapter; some N and lower
    case; qualities 2 .. 40; header lengths differ by r % 17.  remnant: (lo, hi) = the planted inserts leave lo .. hi adapter bases."""
    rng = random.Random(seed)
    f1, f2 = [], []
    for r in range(n_pairs):
        n1 = rng.randint(*lengths)
        n2 = n1 if rng.random() < 0.7 else rng.randint(*lengths)
        u = rng.random()
        if u < planted:
            P1, P2 = rng.choice(prefix_pairs)
            m = min(n1, n2)
            I = max(0, m - rng.randint(*remnant)) if remnant else rng.randint(0, m)
            s1, s2 = read_through(rng, n1, n2, I, P1, P2)
            s1 = cc.mutate(rng, s1, 0, n1, rng.randint(0, 3))
            s2 = cc.mutate(rng, s2, 0, n2, rng.randint(0, 3))
        elif u < planted + 0.2:   # an insert longer than the reads: they overlap, no adapter
            ins = cc.rand_bases(rng, max(n1, n2) + rng.randint(0, 40))
            s1, s2 = ins[:n1], revcomp(ins)[:n2]
        else:
            s1, s2 = cc.rand_bases(rng, n1), cc.rand_bases(rng, n2)
            if adapters and rng.random() < 0.3 and n1 >= WINDOW:
                ad = rng.choice(adapters)[0]
                s1 = cc.plant(rng, n1, ad, rng.randint(0, n1 - WINDOW))
        if rng.random() < 0.1 and n1:
            at = rng.randrange(n1)
            s1 = s1[:at] + b"N" + s1[at + 1:]
        if rng.random() < 0.1:
            s2 = s2.lower()
        name = b"p%d%s" % (r, b"x" * (r % 17))
        f1.append((name + b"/1", s1, bytes(phred + rng.randint(2, 40) for _ in range(n1))))
        f2.append((name + b" 2", s2, bytes(phred + rng.randint(2, 40) for _ in range(n2))))
    return f1, f2


def edge_pairs(seed: int = 21, pair_min: int = 8):
    """[(s1, q1, s2, q2, prefix pairs)]: every read length (equal, and against its neighbour in the list so that n1 != n2) with every
    prefix length, read-through planted at I in {0, 1, n - A}; qualities 30"""
    rng = random.Random(seed)
    out = []
    for p in PREFIX_LENGTHS:
        pp = make_prefix_pairs([p], rng.randrange(1 << 30))
        for k, n1 in enumerate(READ_LENGTHS):
            for n2 in {n1, READ_LENGTHS[k - 1]}:
                m = min(n1, n2)
                for I in sorted({0, 1, max(m - pair_min, 0)}):
                    if I > m:
                        continue
                    s1, s2 = read_through(rng, n1, n2, I, *pp[0])
                    out.append((s1, b"?" * n1, s2, b"?" * n2, pp))
    return out


# ---- hand-worked pairs: (s1, q1, s2, q2, adapters, prefix pairs, options dict, [end 1, end 2]) ----

def hand_cases():
    rng = random.Random(9)
    P = make_prefix_pairs([34], 31)
    P1, P2 = P[0]
    hi = lambda n: b"I" * n   # q 40
    other = lambda c: next(x for x in b"ACGT" if x != c)
    cases = []

    def add(s1, q1, s2, q2, ends, adapters=(), pairs=P, **opt):
        cases.append((bytes(s1), bytes(q1), bytes(s2), bytes(q2), list(adapters), pairs, opt, ends))

    # 50 matches reach Tp = 30 (3 010 300), 49 do not (2 950 094): reads of n bases of RC(P2) / RC(P1) alone (I = 0) lay 2 n positions
    for n, ends in ((25, [0, 0]), (24, [24, 24])):
        add(revcomp(P2)[:n], hi(n), revcomp(P1)[:n], hi(n), ends)
    # one mismatch of quality 0 among 51 positions leaves 50 matches in one sub-range only when it costs nothing
    s1 = bytearray(revcomp(P2)[:26])
    s1[25] = other(s1[25])
    add(s1, hi(25) + b"!", revcomp(P1)[:25], hi(25), [0, 0])   # 50 matches in a row in front of it
    # the seed with exactly s and s + 1 mismatches: 16 positions laid (A = 8 bases of each read, I = 0), Tp = 1, quality 0
    for s in (0, 1, 2, 8):
        for extra, ends in ((0, [0, 0]), (1, [8, 8])):
            r1 = cc.mutate(rng, revcomp(P2)[:8], 0, 8, (s + extra + 1) // 2)
            r2 = cc.mutate(rng, revcomp(P1)[:8], 0, 8, (s + extra) // 2)
            add(r1, b"!" * 8, r2, b"!" * 8, ends, seed=s, pair_score=1)
    # N is invalid: scores 0 and is a seed mismatch; lower case matches
    ins = cc.rand_bases(rng, 40)
    r1, r2 = read_through(rng, 60, 60, 40, P1, P2, ins)
    add(r1.lower(), hi(60), r2, hi(60), [40, 0])
    n1 = bytearray(r1)
    n1[10] = ord("N")
    add(n1, hi(60), r2, hi(60), [40, 0], seed=0)
    # a mismatch between two read positions is charged the smaller quality.  Prefix pair of 16, reads of 50, I = 39: T = 71, the
    # positions [5, 66) are laid, 61 of them.  One mismatch leaves 60 matches: 3 612 360 less its cost; the longer side alone is at most
    # 53 matches (3 190 918).  Tp = 35 (3 500 000) passes at q 1 (3 602 360) and not at q 30 (3 312 360).
    short = [(P1[:16], P2[:16])]
    r1, r2 = read_through(rng, 50, 50, 39, P1[:16], P2[:16])
    m1 = bytearray(r1)
    m1[20] = other(m1[20])   # i = 36: lies against position 39 - 1 - 20 = 18 of R2
    qa, qb = bytearray(hi(50)), bytearray(hi(50))
    qa[20], qb[18] = 33 + 30, 33 + 1
    add(m1, qa, r2, qb, [39, 0], pairs=short, pair_score=35)       # min(30, 1) = 1
    qa[20], qb[18] = 33 + 1, 33 + 30
    add(m1, qa, r2, qb, [39, 0], pairs=short, pair_score=35)       # min(1, 30) = 1
    qa[20] = 33 + 30
    add(m1, qa, r2, qb, [50, 50], pairs=short, pair_score=35)      # both 30
    # a mismatch under a prefix position is charged the read's quality: position 42 of R2 lies in RC(P1), against i = 12
    m2 = bytearray(r2)
    m2[42] = other(m2[42])
    qb = bytearray(hi(50))
    qb[42] = 33 + 1
    add(r1, hi(50), m2, qb, [39, 0], pairs=short, pair_score=35)
    qb[42] = 33 + 30
    add(r1, hi(50), m2, qb, [50, 50], pairs=short, pair_score=35)
    # negative q under --phred 64: the mismatch costs nothing
    qb = bytearray(b"h" * 50)   # q 40
    qb[42] = 64 - 10
    add(r1, b"h" * 50, m2, qb, [39, 0], pairs=short, pair_score=35, phred=64)
    # I = min(n1, n2) - A is found and + 1 is not; A = 1 finds a single adapter base
    for A in (8, 1):
        for left, ends in ((A, None), (A - 1, "untouched")):
            I = 50 - left
            r1, r2 = read_through(rng, 50, 50, I, P1, P2)
            add(r1, hi(50), r2, hi(50), [50, 50] if ends else [I, 0], pair_min=A)
    # two prefix pairs of which the later gives the smaller I
    Q = make_prefix_pairs([34, 40], 77)
    ins = cc.rand_bases(rng, 30)
    r1, r2 = read_through(rng, 90, 90, 30, Q[1][0], Q[1][1], ins)
    add(r1, hi(90), r2, hi(90), [30, 0], pairs=Q)
    add(r1, hi(90), r2, hi(90), [30, 30], pairs=[Q[1], Q[0]], keep_both=True)
    # the simple end below and above the pair end (file 1: the adapter planted in the insert at 20; file 2: none)
    ad = cc.rand_bases(rng, 30)
    ins = bytearray(cc.rand_bases(rng, 60))
    ins[20:50] = ad
    r1, r2 = read_through(rng, 100, 100, 60, P1, P2, bytes(ins))
    add(r1, hi(100), r2, hi(100), [20, 60], adapters=[(ad, 1)], keep_both=True)
    add(r1, hi(100), r2, hi(100), [20, 0], adapters=[(ad, 1)])
    r1, r2 = read_through(rng, 100, 100, 60, P1, P2)
    ad2 = r1[70:100]   # simple mode sees RC(P2) and what follows at 70: above the pair end
    add(r1, hi(100), r2, hi(100), [60, 60], adapters=[(ad2, 0)], keep_both=True)
    # a tandem-repeat insert passes at a smaller I than the true one: the smallest wins
    ins = b"AT" * 30
    r1, r2 = read_through(rng, 100, 100, 60, P1, P2, ins)
    true = clip_pair(r1, hi(100), r2, hi(100), [], P, keep_both=True)[0]
    add(r1, hi(100), r2, hi(100), true, keep_both=True)
    return cases


# ---- whole FASTQ texts ----

def pair_results(t1: bytes, t2: bytes, adapters, prefix_pairs, **opt):
    """per pair of whole records of two final texts: (simple ends, I* or None, too long) -- what does not depend on keep_both"""
    opt = {k: v for k, v in opt.items() if k != "keep_both"}
    r1, r2 = tc.parse_records(t1, True)[0], tc.parse_records(t2, True)[0]
    return [clip_pair(a[1], a[3], b[1], b[3], adapters, prefix_pairs, **opt)[1:4] for a, b in zip(r1, r2)]


def clip_fastq_pair(t1: bytes, t2: bytes, adapters, prefix_pairs, results=None, **opt):
    """([text 1, text 2] with every read cut to its final clip end (a dropped read keeps its record with empty lines), statistics):
    whole records of final texts.  results: pair_results of the same texts and options, where they are at hand already."""
    r1, r2 = tc.parse_records(t1, True)[0], tc.parse_records(t2, True)[0]
    if results is None:
        results = pair_results(t1, t2, adapters, prefix_pairs, **opt)
    keep_both = opt.get("keep_both", False)
    out = [bytearray(), bytearray()]
    st = dict(reads_clipped=[0, 0], reads_dropped=[0, 0], bases_clipped=[0, 0], pairs_clipped=0, pairs_dropped=0, pairs_too_long=0,
              simple_only=0, pair_only=0, both=0)
    for a, b, (simple, I, too_long) in zip(r1, r2, results):
        ends = list(simple) if I is None else [min(simple[0], I), min(simple[1], I if keep_both else 0)]
        st["pairs_clipped"] += I is not None and I != 0
        st["pairs_dropped"] += I == 0
        st["pairs_too_long"] += too_long
        by_simple = simple[0] != len(a[1]) or simple[1] != len(b[1])
        st["simple_only"] += by_simple and I is None
        st["pair_only"] += I is not None and not by_simple
        st["both"] += I is not None and by_simple
        for f, rec in enumerate((a, b)):
            e, n = ends[f], len(rec[1])
            st["reads_clipped"][f] += e != n and e != 0
            st["reads_dropped"][f] += e != n and e == 0
            st["bases_clipped"][f] += n - e
            out[f] += rec[0] + b"\n" + rec[1][:e] + b"\n" + rec[2] + b"\n" + rec[3][:e] + b"\n"
    return [bytes(o) for o in out], st
