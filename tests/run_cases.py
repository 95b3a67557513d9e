"""Shared by test_run_cpu.py and test_gpu_run.py: what `ploidyfrost run`'s second pass (K-MASKCOUNT, csrc/pf_run_rule.hpp) must equal --
the composition it replaces, from the restatements the suite already has: mask_cases.ref_mask (K-MASK's rule) on the text, then
count_cases.ref_count (K-COUNT's rule, both strands, every k-mer kept) on the masked reads."""
import numpy as np

import count_cases as cc
import mask_cases as mc

EVERY = dict(ci=1, cx=0xFFFFFFFF, cs=0xFFFFFFFF)   # pf_count_finish as `build` and `run` close the count


def composition(text: bytes, reads, db: mc.Database, low, up=mc.NO_UPPER):
    """(kmers u64 sorted, counts u32, masked text, K-MASK's statistics) for reads = [(offset, length)]"""
    masked, st = mc.ref_mask_db(text, db, low, up, reads=list(reads))
    kmers, counts, _ = cc.ref_count([masked[o:o + n] for o, n in reads], db.k, both_strands=True, **EVERY)
    return kmers, counts, masked, st


def flat_counters(text: bytes, reads, db: mc.Database):
    """one u32 per byte of the text: the counter of the window that starts there (0 where no window starts)"""
    c = np.zeros(len(text), dtype=np.uint32)
    for o, n in reads:
        w = mc.counters(bytes(text[o:o + n]), db.kmers, db.counts, db.k, db.both_strands)
        c[o:o + len(w)] = w
    return c


def database_of(reads, k, both_strands=True):
    """the database `count -ci 1` would write for these reads: every k-mer with its number of windows"""
    kmers, counts, _ = cc.ref_count(reads, k, both_strands=both_strands, **EVERY)
    return mc.Database.from_arrays(kmers, counts, k, both_strands)


def random_reads(seed, n_reads, k, genome_len=600, length=80, sub_rate=0.02, n_rate=0.005, lower_rate=0.2):
    """seeded reads of random lengths cut from a random genome, both strands, with substitutions, Ns and lower-case runs: windows of
    every count from 1 up, so that a threshold in the middle makes some bad and keeps others"""
    rng = np.random.default_rng(seed)
    genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=genome_len))
    reads = []
    for _ in range(n_reads):
        n = int(rng.integers(0, length + 1))
        at = int(rng.integers(0, genome_len - n + 1))
        r = bytearray(genome[at:at + n])
        if rng.random() < 0.5:
            r = bytearray(mc.revcomp(bytes(r)))
        for j in np.flatnonzero(rng.random(n) < sub_rate):
            r[j] = b"ACGT"[(b"ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        for j in np.flatnonzero(rng.random(n) < n_rate):
            r[j] = ord("N")
        if n and rng.random() < lower_rate:
            a = int(rng.integers(0, n))
            r[a:] = bytes(r[a:]).lower()
        reads.append(bytes(r))
    return reads
