"""Shared by test_mask_cpu.py and test_gpu_mask.py: the rule of `ploidyfrost mask` (K-MASK) restated in Python, and a maker of reads
cut from the unitigs of a golden graph -- so that every window is in the case's database until the maker damages it.

The rule (the issue's one definition; KMC/kmc_api/kmc_file.cpp:904-1090 restated): a read s[0..n) has a counter c_i per window
i in 0 .. n - k; c_i = 0 when the window holds a byte outside ACGTacgt, else the database's count of the window (lower case read as
upper case; both_strands: the canonical form; absent or outside [min_count, max_count]: 0).  Window i is bad when c_i < low or
c_i > up; a byte becomes N when a bad window covers it; everything else is copied."""
import numpy as np

from conftest import load_case

from ploidyfrost_amd import synth

NO_UPPER = 0xFFFFFFFF
STATS = ("reads", "reads_changed", "bases", "bases_masked", "kmers", "kmers_bad")

_CODE = np.full(256, 4, dtype=np.uint8)
for _ch, _v in zip(b"ACGT", range(4)):
    _CODE[_ch] = _v
    _CODE[_ch + 32] = _v


class Database:
    """(sorted k-mers, counts) a look-up may return: the records inside the header's [min_count, max_count]"""

    def __init__(self, prefix):
        kmers, counts, meta = synth.read_kmc(prefix)
        self.prefix, self.meta = prefix, meta
        self.k, self.both_strands = int(meta["k"]), bool(meta["both_strands"])
        self.file_kmers, self.file_counts = kmers, counts   # as pf_upload_counts takes them
        keep = (counts.astype(np.int64) >= int(meta["min_count"])) & (counts.astype(np.int64) <= int(meta["max_count"]))
        o = np.argsort(kmers[keep], kind="stable")
        self.kmers, self.counts = kmers[keep][o], counts[keep][o]

    @classmethod
    def from_arrays(cls, kmers, counts, k, both_strands=True, min_count=1, max_count=0xFFFFFFFF):
        """a database that exists as arrays only (kmers sorted, distinct)"""
        self = cls.__new__(cls)
        self.prefix, self.meta = None, dict(k=k, both_strands=both_strands, min_count=min_count, max_count=max_count)
        self.k, self.both_strands = k, both_strands
        self.file_kmers, self.file_counts = kmers.astype(np.uint64), counts.astype(np.uint32)
        keep = (self.file_counts.astype(np.int64) >= min_count) & (self.file_counts.astype(np.int64) <= max_count)
        self.kmers, self.counts = self.file_kmers[keep], self.file_counts[keep]
        return self

    def upload(self, dev):
        dev.upload_counts(self.file_kmers, self.file_counts, self.meta["min_count"], self.meta["max_count"], self.both_strands, k=self.k)


def counters(seq: bytes, kmers_sorted, counts, k, both_strands):
    """c_i for i in 0 .. n - k (empty for n < k)"""
    n = len(seq)
    if n < k:
        return np.zeros(0, dtype=np.uint32)
    code = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    invalid = np.concatenate([[0], np.cumsum(code == 4)])
    clean = (invalid[k:] - invalid[:-k]) == 0
    fw, rc = synth.kmers_u64(np.where(code == 4, 0, code), k)
    key = np.minimum(fw, rc) if both_strands else fw
    c = np.zeros(n - k + 1, dtype=np.uint32)
    if len(kmers_sorted):
        at = np.minimum(np.searchsorted(kmers_sorted, key), len(kmers_sorted) - 1)
        found = kmers_sorted[at] == key
        c = np.where(found & clean, counts[at], 0).astype(np.uint32)
    return c


def mask_with_counters(seq: bytes, k, c, low, up):
    """(masked read, windows, bad windows, bytes changed)"""
    n = len(seq)
    if n < k:
        return seq, 0, 0, 0
    bad = (c.astype(np.int64) < low) | (c.astype(np.int64) > up)
    cover = np.zeros(n + 1, dtype=np.int64)
    np.add.at(cover, np.flatnonzero(bad), 1)
    np.add.at(cover, np.flatnonzero(bad) + k, -1)
    masked = np.cumsum(cover)[:n] > 0
    src = np.frombuffer(seq, dtype=np.uint8)
    out = np.where(masked, ord("N"), src).astype(np.uint8)
    return out.tobytes(), n - k + 1, int(bad.sum()), int((out != src).sum())


def parse_fastq(text: bytes):
    """[(offset, length)] of the sequence lines: lines end in \\n, a \\r directly before it belongs to the line end, the last line may
    lack its \\n; roles come from the line index"""
    reads, pos, line = [], 0, 0
    while pos < len(text):
        nl = text.find(b"\n", pos)
        end = len(text) if nl < 0 else nl
        stop = end - 1 if (nl >= 0 and end > pos and text[end - 1:end] == b"\r") else end
        if line % 4 == 1:
            reads.append((pos, stop - pos))
        pos = len(text) if nl < 0 else nl + 1
        line += 1
    assert line % 4 == 0, "ref_mask takes whole records"
    return reads


def ref_mask(text: bytes, kmers_sorted, counts, k, low, up, both_strands, reads=None):
    """(output bytes, statistics): the rule on a FASTQ text, or with reads = [(offset, length)] on the reads given explicitly"""
    if reads is None:
        reads = parse_fastq(text)
    out = bytearray(text)
    st = dict.fromkeys(STATS, 0)
    for off, n in reads:
        seq = bytes(text[off:off + n])
        m, windows, bad, changed = mask_with_counters(seq, k, counters(seq, kmers_sorted, counts, k, both_strands), low, up)
        out[off:off + n] = m
        st["reads"] += 1
        st["reads_changed"] += changed > 0
        st["bases"] += n
        st["bases_masked"] += changed
        st["kmers"] += windows
        st["kmers_bad"] += bad
    return bytes(out), st


def ref_mask_db(text, db: Database, low, up=NO_UPPER, reads=None):
    return ref_mask(text, db.kmers, db.counts, db.k, low, up, db.both_strands, reads)


# ---- reads ----

def unitigs(case):
    """the unitig sequences of a golden case's graph, longest first"""
    meta = load_case(case)
    seqs = []
    with open(meta["gfa"], "rb") as f:
        for line in f:
            if line.startswith(b"S\t"):
                seqs.append(line.split(b"\t")[2].strip())
    return sorted(seqs, key=lambda s: (-len(s), s))


COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq: bytes) -> bytes:
    return seq.translate(COMP)[::-1]


def clean_read(case, length, at=0):
    """`length` bytes of the longest unitig of the case: every window is in its database"""
    u = unitigs(case)[0]
    assert len(u) >= at + length, (len(u), at, length)
    return u[at:at + length]


def synthetic(seed, length, k, count=20, weak=(), weak_count=2, both_strands=True):
    """(genome, Database): a random genome whose every window is in the database with `count`, but for the windows listed in `weak`,
    which get `weak_count` -- a single bad window wherever a test wants it (a random genome repeats no k-mer at these lengths)"""
    rng = np.random.default_rng(seed)
    genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=length))
    fw, rc = synth.kmers_u64(_CODE[np.frombuffer(genome, dtype=np.uint8)], k)
    key = np.minimum(fw, rc) if both_strands else fw
    assert len(np.unique(key)) == len(key)
    counts = np.full(len(key), count, dtype=np.uint32)
    counts[list(weak)] = weak_count
    o = np.argsort(key)
    return genome, Database.from_arrays(key[o], counts[o], k, both_strands)


def make_reads(case, n_reads, seed, length=150, sub_rate=0.01, n_rate=0.002, lower_rate=0.1, k=25):
    """seeded reads cut from the unitigs (whole unitigs where they are shorter than `length`), half of them reverse complemented,
    with substitutions, Ns and lower-case runs"""
    rng = np.random.default_rng(seed)
    us = [u for u in unitigs(case) if len(u) >= k]
    weights = np.array([len(u) for u in us], dtype=np.float64)
    weights /= weights.sum()
    reads = []
    for u in rng.choice(len(us), size=n_reads, p=weights):
        s = us[u]
        n = min(len(s), length)
        at = int(rng.integers(0, len(s) - n + 1))
        r = bytearray(s[at:at + n])
        if rng.random() < 0.5:
            r = bytearray(revcomp(bytes(r)))
        for j in np.flatnonzero(rng.random(n) < sub_rate):
            r[j] = b"ACGT"[(b"ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        for j in np.flatnonzero(rng.random(n) < n_rate):
            r[j] = ord("N")
        if rng.random() < lower_rate:
            a = int(rng.integers(0, n))
            b = int(rng.integers(a, n + 1))
            r[a:b] = bytes(r[a:b]).lower()
        reads.append(bytes(r))
    return reads


def fastq(reads, crlf=False, last_newline=True, quals=None, name=b"r"):
    """the reads as FASTQ text; quals[i] overrides read i's quality line"""
    eol = b"\r\n" if crlf else b"\n"
    parts = []
    for i, r in enumerate(reads):
        q = quals[i] if quals and quals.get(i) is not None else b"I" * len(r)
        parts.append(b"@" + name + b"%d" % i + eol + r + eol + b"+" + eol + q + eol)
    text = b"".join(parts)
    if not last_newline and text:
        text = text[:-len(eol)]
    return text


def pack(reads):
    """(text, offsets, lengths): the reads back to back with no separator (the explicit table of pf_mask_reads only)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])[:-1].astype(np.uint64) if reads else np.zeros(0, dtype=np.uint64)
    return b"".join(reads), off, np.array([len(r) for r in reads], dtype=np.uint32)
