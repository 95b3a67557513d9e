"""The rule of duplicate removal (K-DEDUP, `--dedup`; csrc/pf_dedup_rule.hpp) restated in plain Python: the code of a base, the key of
a unit, the decision over a stream, the statistics, and the composition with the trimming of trim_cases.py -- what `trim --dedup`
writes.  Test data: reads with known duplicates, keys that collide on purpose."""
import random

import numpy as np

import trim_cases as tc

M64 = (1 << 64) - 1
SEED1, SEED2, SEED_LEN = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7
SECOND = 1 << 62
LEVELS = 10
STATS = ("units", "unique", "duplicates", "max_copies", "levels")   # (slots and growths belong to a table, not to the rule)


def mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def code(c: int) -> int:
    return {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(c, 4)


def term(word, index, half):
    x = word ^ (index << 48 & M64) ^ mix64(index >> 16)
    return mix64(x ^ SEED1) if half == 0 else mix64(mix64((x + SEED2) & M64) ^ x)


def close(total, l1, l2, pair, half):
    lens = l1 | (l2 << 32)
    h = mix64(total ^ mix64((lens + SEED_LEN * (2 * half + (1 if pair else 0) + 1)) & M64))
    return h or 1


def covered(n, bases):
    return bases if bases and bases < n else n


def key_of(seq1: bytes, seq2=None, bases: int = 0):
    """(h1, h2) of the read seq1, or of the pair (seq1, seq2)"""
    total, cov = [0, 0], [0, 0]
    for f, s in enumerate((seq1,) if seq2 is None else (seq1, seq2)):
        L = cov[f] = covered(len(s), bases)
        for j in range((L + 15) // 16):
            word = 0
            for i, c in enumerate(s[16 * j:min(16 * j + 16, L)]):
                word |= code(c) << (3 * i)
            index = SECOND + j if f else j
            for half in range(2):
                total[half] = (total[half] + term(word, index, half)) & M64
    return tuple(close(total[h], cov[0], cov[1], seq2 is not None, h) for h in range(2))


class Dedup:
    """the decision over a stream: the keys seen so far and their copies"""

    def __init__(self, bases: int = 0):
        self.bases, self.copies = bases, {}

    def unit(self, key) -> bool:
        """a unit that takes part: True = kept (the first of its key)"""
        key = (key[0] or 1, key[1] or 1)
        self.copies[key] = self.copies.get(key, 0) + 1
        return self.copies[key] == 1

    def keys(self, keys):
        return np.array([self.unit((int(a), int(b))) for a, b in keys], dtype=np.uint8)

    def stats(self) -> dict:
        c = list(self.copies.values())
        levels = [0] * LEVELS
        for v in c:
            levels[min(v, LEVELS) - 1] += 1
        return dict(units=sum(c), unique=len(c), duplicates=sum(c) - len(c), max_copies=max(c, default=0), levels=levels)

    def line(self) -> str:
        s = self.stats()
        return "dedup: units %d unique %d duplicates %d max_copies %d levels %s" % (s["units"], s["unique"], s["duplicates"], s["max_copies"],
                                                                                    " ".join(str(v) for v in s["levels"]))

    # ---- composed with trim_cases: what the device calls give for one chunk with this dedup open (no clip) ----
    def trim_fastq(self, text: bytes, steps, phred: int = 33, final=True):
        r = tc.trim_fastq(text, steps, phred, final)
        for i, rec in enumerate(r["records"]):
            if r["len"][i] and not self.unit(key_of(rec[1], None, self.bases)):
                r["stats"]["kept"] -= 1
                r["stats"]["dropped"] += 1
                r["stats"]["bases_kept"] -= r["len"][i]
                r["begin"][i] = r["len"][i] = 0
        r["out"] = b"".join(tc.record_bytes(rec, b, b + l) for rec, b, l in zip(r["records"], r["begin"], r["len"]) if l)
        return r

    def trim_pair(self, text1: bytes, text2: bytes, steps, phred: int = 33, final=True):
        r = tc.trim_pair(text1, text2, steps, phred, final)
        recs, begin, ln, st = r["records"], r["begin"], r["len"], r["stats"]
        for i in range(r["n_records"]):
            if ln[0][i] and ln[1][i] and not self.unit(key_of(recs[0][i][1], recs[1][i][1], self.bases)):
                for f in range(2):
                    st[f]["kept"] -= 1
                    st[f]["dropped"] += 1
                    st[f]["bases_kept"] -= ln[f][i]
                    st[f]["both"] -= 1
                    st[f]["neither"] += 1
                    begin[f][i] = ln[f][i] = 0
        out = [bytearray() for _ in range(4)]
        for i in range(r["n_records"]):
            k1, k2 = ln[0][i] != 0, ln[1][i] != 0
            if k1:
                out[0 if k2 else 1] += tc.record_bytes(recs[0][i], begin[0][i], begin[0][i] + ln[0][i])
            if k2:
                out[2 if k1 else 3] += tc.record_bytes(recs[1][i], begin[1][i], begin[1][i] + ln[1][i])
        r["out"] = [bytes(o) for o in out]
        return r


def trim_line(stats, paired) -> str:
    """the `trim:` line of the command"""
    if paired:
        a, b = stats
        return "trim: pairs %d both %d forward_only %d reverse_only %d dropped %d bases %d bases_kept %d" % (
            a["reads"], a["both"], a["only1"], a["only2"], a["neither"], a["bases"] + b["bases"], a["bases_kept"] + b["bases_kept"])
    return "trim: reads %d kept %d dropped %d bases %d bases_kept %d" % tuple(stats[f] for f in ("reads", "kept", "dropped", "bases", "bases_kept"))


# ---- test data ----

EDGE_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def edge_records(seed=7):
    """(name, seq, qual) of every edge length, each followed by its near copies: an exact copy, one that differs in the last base, one
    that is a base shorter (a prefix), one in lower case, two that hold different non-ACGT bytes at one place.  The names have 1 to 16
    bytes, so that the sequence lines start at every alignment mod 16."""
    rng = random.Random(seed)
    recs = []

    def add(seq):
        name = b"n" * (len(recs) % 16 + 1)
        recs.append((name, seq, b"I" * len(seq)))

    for n in EDGE_LENGTHS:
        s = rand_seq(rng, n)
        add(s)
        add(s)
        if n:
            add(s[:-1] + (b"A" if s[-1:] != b"A" else b"C"))
            add(s[:-1])
            add(s.lower())
            add(s[:n // 2] + b"N" + s[n // 2 + 1:])
            add(s[:n // 2] + b"." + s[n // 2 + 1:])
    return recs


def dup_reads(n, seed, share=0.2, length=100, requalify=0.3, copies_of_one=0):
    """n records of `length` bases of which about `share` repeat the sequence of an earlier one; a share of the copies get other
    (worse) qualities, so that K-TRIM gives them other intervals or drops them.  copies_of_one: that many further copies of record 0,
    spread over the stream."""
    rng = random.Random(seed)
    recs, seqs = [], []
    for i in range(n):
        if seqs and rng.random() < share:
            seq = rng.choice(seqs)
            tag = b"dup"
        else:
            seq = rand_seq(rng, length)
            seqs.append(seq)
            tag = b"new"
        q = [36] * len(seq)
        if rng.random() < requalify:
            cut = rng.randrange(len(seq))
            q = q[:cut] + [rng.randint(2, 24) for _ in range(len(seq) - cut)]
        recs.append((b"r%d/%s" % (i, tag), seq, tc.qline(q)))
    for c in range(copies_of_one):
        at = rng.randrange(1, len(recs) + 1)
        recs.insert(at, (b"c%d/one" % c, recs[0][1], tc.qline([36] * len(recs[0][1]))))
    return recs


def mates(recs, seed):
    """a mate for every record: the mate's sequence is a function of the record's, so that duplicates stay duplicates as pairs"""
    out = []
    for name, seq, _ in recs:
        rng = random.Random(seq + b"/%d" % seed)   # (seeded by the bytes themselves: the same in every process)
        m = rand_seq(rng, len(seq))
        out.append((name + b" 2", m, b"I" * len(m)))
    return out


def keys_one_h1(n, h1=0x1234567, seed=3):
    """n keys with one h1 and distinct h2"""
    rng = random.Random(seed)
    h2 = rng.sample(range(1, 1 << 62), n)
    return np.array([[h1, v] for v in h2], dtype=np.uint64)


def keys_one_home(n, low_bits=20, seed=5):
    """n distinct keys whose h1 agree in their low `low_bits` bits: one home slot in every table of up to 2^low_bits slots"""
    rng = random.Random(seed)
    hi = rng.sample(range(1, 1 << 40), n)
    return np.array([[(v << low_bits) | 0x2B, rng.randrange(1, 1 << 63)] for v in hi], dtype=np.uint64)
