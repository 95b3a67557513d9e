"""Shared by test_hist_cpu.py and test_gpu_hist.py: the threshold rule of the reference restated in Python, and the databases on which
`--auto-cutoffs` is checked end to end (a golden graph's database plus error k-mers that give its histogram the valley a real one has)."""
import math
import os

import numpy as np

from conftest import load_case

from ploidyfrost_amd import synth

HIST_MAX_BINS = 1 << 20


def ref_cutoff_l(rows):
    """cutoffL of src/Main.cpp:200-235 on the second column of a histogram (before the caller's max(10, .))"""
    peak = 1
    while peak < len(rows):
        if rows[peak - 1] < rows[peak]:
            break
        peak += 1
    return int(math.floor(1.25 * (peak - 1) + 0.5))   # C's round(): halves away from zero


def ref_cutoff_u(rows, q=0.998):
    """cutoffH of src/Main.cpp:236-277; None = its "Histogram File is badly Formatted." (v.size() <= 2)"""
    v = [0]
    for r in rows:
        v.append(int(r) + v[-1])
    if len(v) <= 2:
        return None
    cf = int(q * float(v[-1] - v[1]) + float(v[1]))   # size_t cf = frequency * (v.back() - v[1]) + v[1]
    peak = 2
    while peak < len(v):
        if v[peak] > cf:
            break
        peak += 1
    return peak


def db_rows(counts, meta, counter_size):
    """the rows of a database by their definition: count min_count + r for r = 0 .. top - min_count, top = min(max_count, the counter's
    range, 2^20 - 1); records outside [min_count, max_count] left out, counts above top in the last row"""
    mn, mx = int(meta["min_count"]), int(meta["max_count"])
    top = min(mx, (1 << (8 * min(counter_size, 4))) - 1, HIST_MAX_BINS - 1)
    if top < mn:
        return np.zeros(0, dtype=np.uint64)
    c = counts.astype(np.int64)
    c = c[(c >= mn) & (c <= mx)]
    return np.bincount(np.minimum(c, top), minlength=top + 1)[mn:].astype(np.uint64)


def error_kmers(have, k, n, seed):
    """n canonical k-mers that are not among `have`, sorted"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << (2 * k), size=2 * n + 64, dtype=np.uint64)
    x = np.unique(np.minimum(x, synth.revcomp_u64(x, k)))
    x = x[~np.isin(x, have)]
    assert len(x) >= n
    return np.sort(rng.permutation(x)[:n])


def with_errors(kmers, counts, k, per_count, seed):
    """the database plus error k-mers: per_count[i] of them with count i + 1.  Returns (kmers sorted, counts)."""
    n = int(sum(per_count))
    ek = error_kmers(kmers, k, n, seed)
    ec = np.repeat(np.arange(1, len(per_count) + 1, dtype=np.uint32), per_count)
    allk = np.concatenate([kmers, ek])
    allc = np.concatenate([counts.astype(np.uint32), ec])
    o = np.argsort(allk, kind="stable")
    return allk[o], allc[o]


# counts of the error k-mers fall from 1 upward into the valley in front of the graph's own k-mers
ERRORS_SINGLE = [300, 225, 169, 127, 95, 71, 53, 40, 30, 23, 17, 13]
ERRORS_COLORED = [[300, 150, 75, 40, 20, 10, 5, 3, 2, 1, 4, 9],
                  [400, 300, 225, 169, 127, 95, 71, 53, 40, 30, 23, 17, 13, 10, 12, 30],
                  [200, 100, 50, 25, 12, 6, 4, 3, 3, 2, 2, 1, 5, 11]]


def make_single(tmp_dir, case="dip20k"):
    """(meta, db prefix, counts): the golden case's graph with its database plus ERRORS_SINGLE, written under tmp_dir"""
    meta = load_case(case)
    kmers, counts, km = synth.read_kmc(meta["db"])
    o = np.argsort(kmers, kind="stable")
    kmers = kmers[o]
    # The thresholds test a unitig's smallest count (src/CDBG.cpp:1209), so what a derived threshold changes is decided unitig by
    # unitig: every other unitig of the graph is sequenced at depth 14 instead of 20 (multiplicity from the fixture's own counts,
    # jitter 1).  -l 10 keeps both kinds; the lower threshold derived from the valley in front of count 13 drops the shallow ones.
    mult = np.maximum(np.rint(counts[o] / 20.0), 1).astype(np.int64)
    shallow = np.zeros(len(kmers), dtype=bool)
    lut = np.zeros(256, dtype=np.uint8)
    for ch, v in zip(b"ACGT", range(4)):
        lut[ch] = v
    u = 0
    with open(meta["gfa"], "rb") as f:
        for line in f:
            if line.startswith(b"S\t"):
                fw, rc = synth.kmers_u64(lut[np.frombuffer(line.split(b"\t")[2].strip(), dtype=np.uint8)], km["k"])
                if u % 2:
                    shallow[np.searchsorted(kmers, np.minimum(fw, rc))] = True
                u += 1
    counts = np.where(shallow, synth.synth_counts(kmers, mult, depth=14, jitter=1), synth.synth_counts(kmers, mult, depth=20, jitter=1))
    k2, c2 = with_errors(kmers, counts, km["k"], ERRORS_SINGLE, 7)
    prefix = os.path.join(str(tmp_dir), "auto_db")
    synth.write_kmc1(prefix, k2, c2, km["k"])
    return meta, prefix, c2


def make_colored(tmp_dir, case="col3_dip"):
    """(meta, db prefixes, counts per colour): the colored golden case with every colour's database plus its own error k-mers"""
    meta = load_case(case)
    prefixes, all_counts = [], []
    for c, db in enumerate(meta["dbs"]):
        kmers, counts, km = synth.read_kmc(db)
        o = np.argsort(kmers, kind="stable")
        k2, c2 = with_errors(kmers[o], counts[o], km["k"], ERRORS_COLORED[c % len(ERRORS_COLORED)], 11 + c)
        prefix = os.path.join(str(tmp_dir), "auto_db%d" % c)
        synth.write_kmc1(prefix, k2, c2, km["k"], both_strands=bool(km["both_strands"]))
        prefixes.append(prefix)
        all_counts.append(c2)
    return meta, prefixes, all_counts


def thresholds(counts, q=0.998, min_count=1, max_count=65535, counter_size=2):
    rows = db_rows(counts, dict(min_count=min_count, max_count=max_count), counter_size)
    return max(10, ref_cutoff_l(rows)), ref_cutoff_u(rows, q)
