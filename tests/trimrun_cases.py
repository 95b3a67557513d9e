"""Shared by test_run_trim_cpu.py and test_gpu_run_trim.py: what `ploidyfrost run STEP...` hands on from a chunk of raw FASTQ
(csrc/pf_trimrun_rule.hpp), from the restatements the suite already has -- trim_cases (K-TRIM's rule) for the intervals,
mask_cases.parse_fastq for the sequence lines -- and seeded inputs.  Nothing here looks at the C++.

The reads handed on are the sequence bytes [seq_begin + b, seq_begin + e) of every whole record the steps keep; for a pair, record r of
a file goes on only when record r of both files is kept."""
import random

import numpy as np

import mask_cases as mc
import trim_cases as tc


def _seq_lines(text: bytes, used: int, n: int):
    return mc.parse_fastq(text[:used])[:n] if n else []


def table(text: bytes, steps, phred: int = 33, final=True):
    """dict: read_off / read_len (lists), reads (the bytes handed on), bytes_used, n_records, stats (trim_cases' of the chunk)"""
    t = tc.trim_fastq(text, steps, phred, final)
    lines = _seq_lines(text, t["bytes_used"], t["n_records"])
    off = [lines[r][0] + t["begin"][r] for r in range(t["n_records"]) if t["len"][r]]
    ln = [t["len"][r] for r in range(t["n_records"]) if t["len"][r]]
    return dict(read_off=off, read_len=ln, reads=[bytes(text[o:o + n]) for o, n in zip(off, ln)], bytes_used=t["bytes_used"],
                n_records=t["n_records"], stats=t["stats"])


def table_pair(text1: bytes, text2: bytes, steps, phred: int = 33, final=True):
    """the same per file: read_off / read_len / reads = [file 1, file 2]; both tables have the same number of entries"""
    t = tc.trim_pair(text1, text2, steps, phred, final)
    n = t["n_records"]
    off, ln, reads = [[], []], [[], []], [[], []]
    lines = [_seq_lines(x, t["bytes_used"][f], n) for f, x in enumerate((text1, text2))]
    for r in range(n):
        if t["len"][0][r] and t["len"][1][r]:
            for f, x in enumerate((text1, text2)):
                o, m = lines[f][r][0] + t["begin"][f][r], t["len"][f][r]
                off[f].append(o)
                ln[f].append(m)
                reads[f].append(bytes(x[o:o + m]))
    return dict(read_off=off, read_len=ln, reads=reads, bytes_used=t["bytes_used"], n_records=n, stats=t["stats"])


def pair_outcomes(text1: bytes, text2: bytes, steps, phred: int = 33):
    s = tc.trim_pair(text1, text2, steps, phred)["stats"][0]
    return s["both"], s["only1"], s["only2"], s["neither"]


def genome_reads(n: int, seed: int, genome_len: int = 1500, sub_rate=0.01, n_rate=0.004, lower_rate=0.15, lengths=tc.GEN_LENGTHS, genome_seed=None):
    """n records (name, seq, qual): the qualities of trim_cases.make_reads (its four shapes), the sequences cut from one short random
    genome on both strands, so that k-mers repeat (counts above 1), with substitutions, Ns and lower-case runs"""
    grng = random.Random((seed if genome_seed is None else genome_seed) * 7919 + 1)   # (the files of a pair share a genome)
    genome = bytes(grng.choice(b"ACGT") for _ in range(genome_len))
    rng = random.Random(seed * 104729 + 2)
    recs = []
    for name, seq, qual in tc.make_reads(n, seed, lengths=lengths):
        m = len(seq)
        at = rng.randrange(genome_len - m + 1)
        r = bytearray(genome[at:at + m])
        if rng.random() < 0.5:
            r = bytearray(mc.revcomp(bytes(r)))
        for j in range(m):
            x = rng.random()
            if x < sub_rate:
                r[j] = b"ACGT"[(b"ACGT".index(r[j]) + rng.randint(1, 3)) % 4]
            elif x < sub_rate + n_rate:
                r[j] = ord("N")
        if m and rng.random() < lower_rate:
            a = rng.randrange(m)
            r[a:] = bytes(r[a:]).lower()
        recs.append((name, bytes(r), qual))
    return recs


def one_read(seq: bytes, low_head: int = 0, low_tail: int = 0, name=b"x"):
    """a record whose first low_head and last low_tail bases have quality 2, the rest 40"""
    n = len(seq)
    return (name, seq, tc.qline([2] * low_head + [40] * (n - low_head - low_tail) + [2] * low_tail))


def cut3(text: bytes):
    """the text cut into three at places that are no record boundaries"""
    a, b = len(text) // 3 + 5, 2 * len(text) // 3 + 11
    return [text[:a], text[a:b], text[b:]]


def mid_count(counts) -> int:
    """a threshold in the middle of the repeated k-mers: the median of the counts above 1 (the k-mers of count 1, one per sequencing
    error and window, outnumber all others, and their median is 1)"""
    c = np.asarray(counts)
    return int(np.median(c[c > 1]))


DEEP = dict(genome_len=300, sub_rate=0.002, n_rate=0.001)   # genome_reads at a depth at which most windows repeat
