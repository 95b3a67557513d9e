"""Adapter clipping (K-CLIP, `--adapters`) restated in plain Python, and the cases the CPU and GPU tests share: the rule of
csrc/pf_clip_rule.hpp as loops over adapters and offsets, the parser of the adapter file, seeded adapters and reads (no vendor
adapter file is used anywhere), hand-worked reads, and the clipping of whole FASTQ texts that the stream tests take as reference."""
import random

import trim_cases as tc

WINDOW, MIN_LEN, MAX_LEN, MAX_ADAPTERS = 16, 16, 128, 64
MATCH, PENALTY, UNIT = 60206, 10000, 100000
READ_LENGTHS = [0, 1, 15, 16, 17, 100, 255, 256, 257, 1000]
ADAPTER_LENGTHS = [16, 17, 33, 64, 65, 128]
STATS = ("reads_clipped", "reads_dropped", "bases_clipped", "candidates_scored")


# ---- the rule ----

def offset_score(seq: bytes, qual: bytes, ad: bytes, o: int, seed: int, phred: int):
    """(seed holds, score) of adapter `ad` (upper case) at offset o; (False, 0) for an offset that is no candidate"""
    n, m = len(seq), len(ad)
    lo, hi = max(0, o), min(n, o + m)
    if hi - lo < WINDOW:
        return False, 0
    ru = seq[lo:hi].upper()
    mm = [x != y for x, y in zip(ru, ad[lo - o:hi - o])]   # (a byte outside ACGT equals no adapter base)
    run = sum(mm[:WINDOW])
    ok = run <= seed
    for w in range(1, len(mm) - WINDOW + 1):
        if ok:
            break
        run += mm[w + WINDOW - 1] - mm[w - 1]
        ok = run <= seed
    if not ok:
        return False, 0
    best = cur = 0
    for i, bad in enumerate(mm):
        if ru[i] not in b"ACGT":
            v = 0
        elif not bad:
            v = MATCH
        else:
            v = -PENALTY * max(qual[lo + i] - phred, 0)
        cur = max(cur + v, 0)
        best = max(best, cur)
    return True, best


def clip_read(seq: bytes, qual: bytes, adapters, side: int = 1, seed: int = 2, score: int = 10, phred: int = 33):
    """adapters: [(sequence, side)], side 0 = both files.  (clip end, candidates scored): clip end len(seq) = untouched, 0 = dropped."""
    n, best, scored = len(seq), None, 0
    for ad, ad_side in adapters:
        if ad_side not in (0, side):
            continue
        ad = ad.upper()
        for o in range(-(len(ad) - WINDOW), n - WINDOW + 1):
            ok, s = offset_score(seq, qual, ad, o, seed, phred)
            if not ok:
                continue
            scored += 1
            if s >= UNIT * score and (best is None or o < best):
                best = o
    return (n if best is None else max(best, 0)), scored


def parse_adapters(text: bytes):
    """(adapters [(sequence, side)], names, skipped), or ("refusal name", 1-based record) as csrc/pf_clip_rule.hpp refuses the file"""
    adapters, names, skipped, record = [], [], 0, 0
    cur = None   # [name, sequence, prefix]

    def close():
        nonlocal skipped
        if cur is None:
            return None
        if cur[2]:
            skipped += 1
            return None
        if not MIN_LEN <= len(cur[1]) <= MAX_LEN:
            return "length"
        if len(adapters) == MAX_ADAPTERS:
            return "too_many"
        name = cur[0]
        adapters.append((bytes(cur[1]), 1 if name.endswith(b"/1") else 2 if name.endswith(b"/2") else 0))
        names.append(name)
        return None

    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
        ended = True
    else:
        ended = False
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
            name = line[1:].replace(b"\t", b" ").split(b" ")[0]
            cur = [name, bytearray(), name.startswith(b"Prefix")]
            continue
        if cur is None:
            return "not_fasta", 0
        if cur[2]:
            continue
        for c in line:
            if bytes([c]).upper() not in (b"A", b"C", b"G", b"T"):
                return "byte", record
        cur[1] += line.upper()
    why = close()
    if why:
        return why, record
    if record == 0:
        return "not_fasta", 0
    if not adapters:
        return "no_adapter", 0
    return adapters, names, skipped


# ---- seeded adapters and reads ----

def rand_bases(rng, n: int) -> bytes:
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def make_adapters(lengths, seed: int, sides=None):
    rng = random.Random(seed)
    return [(rand_bases(rng, m), 0 if sides is None else sides[i]) for i, m in enumerate(lengths)]


def adapters_fa(adapters, prefix_entries: int = 0, crlf: bool = False, wrap: int = 0) -> bytes:
    """the adapters as a FASTA file: names a0, a1/1, a2/2 by side; `prefix_entries` palindrome-mode entries in front"""
    nl = b"\r\n" if crlf else b"\n"
    out = bytearray()
    for i in range(prefix_entries):
        out += b">PrefixPE/%d" % (i % 2 + 1) + nl + b"GTCA" * 8 + nl
    for i, (ad, side) in enumerate(adapters):
        out += b">a%d%s some words" % (i, (b"", b"/1", b"/2")[side]) + nl
        for at in range(0, len(ad), wrap or len(ad)):
            out += ad[at:at + (wrap or len(ad))] + nl
    return bytes(out)


def plant(rng, n: int, ad: bytes, o: int) -> bytes:
    """a random read of n bases with adapter `ad` laid at offset o (adapter position j on read position o + j)"""
    read = bytearray(rand_bases(rng, n))
    for p in range(max(0, o), min(n, o + len(ad))):
        read[p] = ad[p - o]
    return bytes(read)


def mutate(rng, read: bytes, lo: int, hi: int, k: int) -> bytes:
    """k positions of read[lo:hi] replaced by another base"""
    read = bytearray(read)
    for p in rng.sample(range(lo, hi), min(k, max(hi - lo, 0))):
        read[p] = rng.choice([c for c in b"ACGT" if c != read[p]])
    return bytes(read)


def edge_offsets(n: int, m: int):
    """the offsets of the edge list for a read of n and an adapter of m bases: the first, -1, 0, 1, the last candidate, one beyond it"""
    return sorted({o for o in (-(m - WINDOW), -1, 0, 1, n - WINDOW, n - WINDOW + 1) if -(m - WINDOW) <= o <= n - WINDOW + 1})


def edge_reads(seed: int = 11):
    """[(seq, qual, adapters)]: every read length against every adapter length at every edge offset, qualities 30"""
    rng = random.Random(seed)
    out = []
    for m in ADAPTER_LENGTHS:
        ad = rand_bases(rng, m)
        for n in READ_LENGTHS:
            offsets = edge_offsets(n, m) if n >= WINDOW else [0]
            for o in offsets:
                seq = plant(rng, n, ad, o)
                out.append((seq, bytes([33 + 30]) * n, [(ad, 0)]))
    return out


def make_reads(n_reads: int, adapters, seed: int, lengths=(30, 300), planted: float = 1 / 3, phred: int = 33):
    """n_reads records (name, seq, qual) of lengths[0] .. lengths[1] bases; a share `planted` of them run into one of the adapters at a
    random offset, the adapter mutated at 0 .. 3 places; some N and lower case; qualities 2 .. 40"""
    rng = random.Random(seed)
    recs = []
    for i in range(n_reads):
        n = rng.randint(*lengths)
        seq = rand_bases(rng, n)
        if rng.random() < planted and n >= WINDOW:
            ad = rng.choice(adapters)[0]
            o = rng.randint(-(len(ad) - WINDOW), n - WINDOW)
            seq = plant(rng, n, ad, o)
            seq = mutate(rng, seq, max(0, o), min(n, o + len(ad)), rng.randint(0, 3))
        if rng.random() < 0.1 and n:
            p = rng.randrange(n)
            seq = seq[:p] + b"N" + seq[p + 1:]
        if rng.random() < 0.1:
            seq = seq.lower()
        qual = bytes(phred + rng.randint(2, 40) for _ in range(n))
        recs.append((b"r%d/%s" % (i, b"x" * (i % 17)), seq, qual))
    return recs


# ---- hand-worked reads: (seq, qual, adapters, side, seed, score, phred, clip end) ----

def hand_cases():
    rng = random.Random(5)
    A = rand_bases(rng, 35)
    B = rand_bases(rng, 24)
    head = b"CA" * 15   # 30 bases that look like no adapter
    hi = lambda n: b"I" * n   # q 40
    cases = []
    # 17 matches reach T = 10 (1 023 502 >= 1 000 000), 16 do not (963 296)
    cases.append((A[:17], hi(17), [(A, 0)], 1, 2, 10, 33, 0))
    cases.append((A[:16], hi(16), [(A, 0)], 1, 2, 10, 33, 16))
    cases.append((head + A[:17], hi(47), [(A, 0)], 1, 2, 10, 33, 30))
    cases.append((head + A[:16], hi(46), [(A, 0)], 1, 2, 10, 33, 46))
    # a seed with exactly s and with s + 1 mismatches (one window: an adapter of 16; T = 1 and quality 0 keep the score out of it)
    a16 = rand_bases(rng, 16)
    for s in (0, 1, 2, 8):
        lowq = b"!" * 46
        cases.append((mutate(rng, head + a16, 30, 46, s), lowq, [(a16, 0)], 1, s, 1, 33, 30))
        cases.append((mutate(rng, head + a16, 30, 46, s + 1), lowq, [(a16, 0)], 1, s, 1, 33, 46))
    # two mismatches of quality 93 in the middle: the whole overlap sums to 33 * 60206 - 1 860 000 = 126 798, the 17 matches behind
    # them to 1 023 502
    seq = bytearray(head + A)
    for p in (30 + 16, 30 + 17):
        seq[p] = next(c for c in b"ACGT" if c != seq[p])
    q = bytearray(hi(65))
    q[46] = q[47] = 33 + 93
    cases.append((bytes(seq), bytes(q), [(A, 0)], 1, 2, 10, 33, 30))
    cases.append((bytes(seq[:-1]), bytes(q[:-1]), [(A, 0)], 1, 2, 10, 33, 64))   # 16 matches behind them: not enough
    # lower case matches; N scores 0 and is a seed mismatch
    cases.append(((head + A).lower(), hi(65), [(A, 0)], 1, 2, 10, 33, 30))
    withn = bytearray(head + A)
    withn[40] = ord("N")
    cases.append((bytes(withn), hi(65), [(A, 0)], 1, 0, 10, 33, 30))   # (the 16 clean positions behind the N hold the seed)
    withn = bytearray(head + A[:20])
    withn[35] = withn[44] = ord("N")
    cases.append((bytes(withn), hi(50), [(A, 0)], 1, 1, 10, 33, 50))   # two N in every window of 16: no seed with s = 1
    # negative q (phred 64 on low bytes): a mismatch costs nothing, 18 matches around two of them pass
    seq = mutate(rng, head + A[:20], 38, 40, 2)
    cases.append((seq, b"5" * 50, [(A, 0)], 1, 2, 10, 64, 30))
    cases.append((seq, b"~" * 50, [(A, 0)], 1, 2, 10, 64, 50))   # q 62 each: the best sub-range is 10 matches
    # two adapters pass: the smaller offset wins, whatever their order
    seq = head + B[:20] + A
    for ads in ([(A, 0), (B, 0)], [(B, 0), (A, 0)]):
        cases.append((seq, hi(len(seq)), ads, 1, 2, 10, 33, 30))
    # sides
    for side, ad_side, end in ((1, 1, 30), (2, 1, 65), (1, 2, 65), (2, 2, 30), (1, 0, 30), (2, 0, 30)):
        cases.append((head + A, hi(65), [(A, ad_side)], side, 2, 10, 33, end))
    # the adapter hangs over the read's start: dropped
    cases.append((A[5:] + head, hi(60), [(A, 0)], 1, 2, 10, 33, 0))
    return cases


# ---- whole FASTQ texts ----

def clip_fastq(text: bytes, adapters, side: int = 1, seed: int = 2, score: int = 10, phred: int = 33):
    """(the text with every read cut to its clip end -- a dropped read keeps its record with empty lines, so that the records of a pair
    stay in step; line ends come out as '\\n' --, statistics).  Whole records of a final text."""
    recs, _ = tc.parse_records(text, True)
    out = bytearray()
    st = dict.fromkeys(STATS, 0)
    for head, seq, plus, qual in recs:
        e, scored = clip_read(seq, qual, adapters, side, seed, score, phred)
        st["candidates_scored"] += scored
        st["reads_clipped"] += e != len(seq) and e != 0
        st["reads_dropped"] += e != len(seq) and e == 0
        st["bases_clipped"] += len(seq) - e
        out += head + b"\n" + seq[:e] + b"\n" + plus + b"\n" + qual[:e] + b"\n"
    return bytes(out), st


def trim_fastq(text: bytes, steps, adapters, side: int = 1, seed: int = 2, score: int = 10, phred: int = 33, final: bool = True):
    """what pf_trim_fastq gives for one chunk while a clip is open: trim_cases.trim_fastq with every interval starting at the clip end"""
    recs, used = tc.parse_records(text, final)
    out, begin, ln = bytearray(), [], []
    clip = dict.fromkeys(STATS, 0)
    for r in recs:
        e, scored = clip_read(r[1], r[3], adapters, side, seed, score, phred)
        clip["candidates_scored"] += scored
        clip["reads_clipped"] += e != len(r[1]) and e != 0
        clip["reads_dropped"] += e != len(r[1]) and e == 0
        clip["bases_clipped"] += len(r[1]) - e
        iv = tc.trim_read(tc.quals(r[3][:e], phred), steps) if steps else ((0, e) if e else None)
        if iv and iv[1] == iv[0]:
            iv = None
        if iv:
            out += tc.record_bytes(r, *iv)
        begin.append(iv[0] if iv else 0)
        ln.append(iv[1] - iv[0] if iv else 0)
    return dict(out=bytes(out), bytes_used=used, n_records=len(recs), begin=begin, len=ln, clip=clip)
