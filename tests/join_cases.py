"""K-COV-JOIN's edge cases and a plain reference of what the join + K-COV compute.

reference_unitig_cov() restates CDBG::readCov(const UnitigMap&) (reference src/CDBG.cpp:66-98) with np.searchsorted on the sorted
keys: for every k-mer of every unitig the count of the form as read if the database holds it, else the count of its reverse
complement, else the k-mer is a miss.  reference_unitig_cov_colored() is the same per colour (src/CCDBG.cpp:123-155: a colour's own
database is asked, a database written without both strands is never looked up).  Neither uses anything of the product beyond
synth.kmers_u64 and synth.revcomp_u64.

The builders are deterministic.  Each returns a Case: a tuple (seqs, k, keys, counts, note) that also carries `info` -- the count
range of the database, whether absent k-mers are meant, whether the table gets a joined array, and, for the cases that must
overflow a wavefront's hand-over list, where the planted run lies.  The hash of pf_device_common.hpp's kmer_lines() is
restated here only to CHOOSE inputs (minimizer_hashes); no expected value comes from it.
"""
from __future__ import annotations

import numpy as np

from ploidyfrost_amd import synth

WAVE_KMERS = 64 * 64      # k-mers of a wavefront of K-COV-JOIN: 64 rows of 64
REST_CAP = WAVE_KMERS // 2   # entries of a wavefront's slice of the hand-over list
LINE_KEYS = 10
MMER = 16
K_MUL = 0x9E3779B1

_BASES = b"ACGT"
_LUT = np.zeros(256, dtype=np.uint8)
for _ch, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    _LUT[_ch] = _v
_B = np.frombuffer(_BASES, dtype=np.uint8)


class Case(tuple):
    """(seqs, k, keys, counts, note) + info"""

    def __new__(cls, seqs, k, keys, counts, note, **info):
        self = super().__new__(cls, (seqs, k, np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32), note))
        self.info = dict(min_count=1, max_count=65535, absent=False, joined=True)
        self.info.update(info)
        return self


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def graph_kmers(seqs, k):
    """(fwd, rc, first): the k-mers of all unitigs laid end to end as they read and reverse-complemented; unitig u's are
    [first[u], first[u + 1])"""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    nk = lens - k + 1
    assert len(seqs) and (nk >= 1).all()
    codes = _LUT[np.frombuffer(b"".join(seqs), dtype=np.uint8)]
    fw, rc = synth.kmers_u64(codes, k)
    base = np.concatenate([[0], np.cumsum(lens)[:-1]])
    first = np.concatenate([[0], np.cumsum(nk)])
    idx = np.repeat(base - first[:-1], nk) + np.arange(first[-1])
    return fw[idx], rc[idx], first


def _find(keys, counts, q):
    """(found bool[n], count u64[n]) of queries q in the sorted distinct keys"""
    if len(keys) == 0:
        return np.zeros(len(q), dtype=bool), np.zeros(len(q), dtype=np.uint64)
    i = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return keys[i] == q, counts[i].astype(np.uint64)


def _kept(keys, counts, min_count, max_count):
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    keep = (counts >= min_count) & (counts <= max_count)   # not retrievable otherwise (KMC/kmc_api/kmc_file.cpp:1459)
    keys, counts = keys[keep], counts[keep]
    o = np.argsort(keys, kind="stable")
    keys, counts = keys[o], counts[o]
    assert (keys[1:] != keys[:-1]).all(), "a database holds a key once"
    return keys, counts


def kmer_counts(seqs, k, keys, counts, min_count, max_count):
    """(found bool[n_kmers], count u64[n_kmers], first): the composite look-up of every graph k-mer"""
    keys, counts = _kept(keys, counts, min_count, max_count)
    fw, rc, first = graph_kmers(seqs, k)
    hit_f, c_f = _find(keys, counts, fw)
    hit_r, c_r = _find(keys, counts, rc)
    return hit_f | hit_r, np.where(hit_f, c_f, np.where(hit_r, c_r, 0)), first


def reference_unitig_cov(seqs, k, keys, counts, min_count, max_count):
    """(sum u64[N], min u32[N], miss u8[N]); a missing k-mer adds nothing to sum and min"""
    found, c, first = kmer_counts(seqs, k, keys, counts, min_count, max_count)
    s = np.add.reduceat(c, first[:-1]).astype(np.uint64)
    m = np.minimum(np.minimum.reduceat(np.where(found, c, 10000), first[:-1]), 10000).astype(np.uint32)   # src/CDBG.cpp:71
    miss = np.maximum.reduceat((~found).astype(np.uint8), first[:-1]).astype(np.uint8)
    return s, m, miss


MISSING = 0xFFFFFFFF


def reference_unitig_cov_colored(seqs, k, dbs, min_count=1, max_count=65535):
    """dbs: (keys, counts[, both_strands]) per colour -> (sum u64, min u32, max u32, miss u8), each [C, N].  min starts at all
    ones and max at 0 (include/ploidyfrost_hip.h); a colour that is never looked up keeps those, sum 0 and miss 0."""
    n = len(seqs)
    s = np.zeros((len(dbs), n), dtype=np.uint64)
    lo = np.full((len(dbs), n), MISSING, dtype=np.uint32)
    hi = np.zeros((len(dbs), n), dtype=np.uint32)
    miss = np.zeros((len(dbs), n), dtype=np.uint8)
    for c, db in enumerate(dbs):
        if len(db) > 2 and not db[2]:
            continue
        found, cnt, first = kmer_counts(seqs, k, db[0], db[1], min_count, max_count)
        s[c] = np.add.reduceat(cnt, first[:-1])
        lo[c] = np.minimum.reduceat(np.where(found, cnt, MISSING), first[:-1])
        hi[c] = np.maximum.reduceat(cnt, first[:-1])
        miss[c] = np.maximum.reduceat((~found).astype(np.uint8), first[:-1])
    return s, lo, hi, miss


# ---- pieces of the builders ------------------------------------------------------------------------------------------------------

def to_bytes(codes) -> bytes:
    return _B[np.asarray(codes, dtype=np.uint8)].tobytes()


def cut(genome, k, kmer_lens):
    """unitigs over consecutive k-mer ranges of one sequence (neighbours overlap in k - 1 bases, as in a compacted graph)"""
    assert sum(kmer_lens) == len(genome) - k + 1
    out, a = [], 0
    for n in kmer_lens:
        out.append(to_bytes(genome[a: a + n + k - 1]))
        a += n
    return out


def single_kmer_unitigs(seqs, k):
    """every k-mer a unitig of its own, in graph order: sum[u] is then the k-mer's count"""
    return [s[i: i + k] for s in seqs for i in range(len(s) - k + 1)]


def canonical_keys(seqs, k):
    fw, rc, _ = graph_kmers(seqs, k)
    return np.unique(np.minimum(fw, rc))


def some_counts(rng, n, lo=1, hi=60000):
    return rng.integers(lo, hi + 1, size=n, dtype=np.uint64).astype(np.uint32)


def mixed_lens(rng, n, longest=200):
    """unitig lengths in k-mers, 1 .. longest, adding up to n"""
    out, left = [], n
    while left:
        x = min(left, int(rng.integers(1, longest + 1)))
        out.append(x)
        left -= x
    return out


def palindrome(rng, k):
    half = rng.integers(0, 4, size=k // 2, dtype=np.uint8)
    return np.concatenate([half, (3 - half)[::-1]])


def rc_bytes(s: bytes) -> bytes:
    return to_bytes((3 - _LUT[np.frombuffer(s, dtype=np.uint8)])[::-1])


def genome_case(k, kmer_lens, seed, note, palindromes=0, **info):
    """a random genome cut into unitigs of the given lengths; the table is its canonical k-mers"""
    rng = np.random.default_rng(seed)
    n = int(sum(kmer_lens))
    g = rng.integers(0, 4, size=n + k - 1, dtype=np.uint8)
    if palindromes:
        assert k % 2 == 0
        for i in range(palindromes):
            at = (i * 97 + 5) % max(1, n - 1)
            at = min(at, len(g) - k)
            g[at: at + k] = palindrome(rng, k)
    seqs = cut(g, k, kmer_lens)
    keys = canonical_keys(seqs, k)
    return Case(seqs, k, keys, some_counts(rng, len(keys)), note, **info)


# ---- the planted minimizer -------------------------------------------------------------------------------------------------------

def minimizer_hashes(keys, k):
    """[n, k - 15]: c * 0x9E3779B1 mod 2^32 of the canonical 16-mers c of every key -- what kmer_lines() takes the minimum of"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.zeros((len(keys), k - MMER + 1), dtype=np.uint64)
    for j in range(k - MMER + 1):
        f = (keys >> np.uint64(2 * j)) & np.uint64(0xFFFFFFFF)
        c = np.minimum(f, synth.revcomp_u64(f, MMER))
        out[:, j] = (c * np.uint64(K_MUL)) & np.uint64(0xFFFFFFFF)
    return out


def planted_mmer():
    """(the canonical 16-mer of smallest non-zero hash, that hash): every k-mer that holds it and no run of sixteen A's or T's has
    it as its minimizer"""
    inv = pow(K_MUL, -1, 1 << 32)
    for h in range(1, 1 << 20):
        c = (h * inv) & 0xFFFFFFFF
        if c <= int(synth.revcomp_u64(np.array([c], dtype=np.uint64), MMER)[0]):
            return c, h
    raise AssertionError


def planted_unitigs(rng, k, n_unitigs):
    """unitigs of 2k - 16 bases with the planted 16-mer in the middle: each of their k - 15 k-mers holds it"""
    c, _ = planted_mmer()
    mm = np.array([(c >> (2 * (MMER - 1 - i))) & 3 for i in range(MMER)], dtype=np.uint8)
    out, seen = [], set()
    while len(out) < n_unitigs:   # (nine free bases a k-mer at k = 25: a unitig that repeats a k-mer of an earlier one is drawn again)
        u = np.concatenate([rng.integers(0, 4, size=k - MMER, dtype=np.uint8), mm, rng.integers(0, 4, size=k - MMER, dtype=np.uint8)])
        fw, rc = synth.kmers_u64(u, k)
        can = set(np.minimum(fw, rc).tolist())
        if len(can) == len(fw) and not (can & seen):
            seen |= can
            out.append(to_bytes(u))
    return out


def filler_unitigs(rng, k, n_kmers, longest=60):
    """ordinary unitigs of a random genome, n_kmers k-mers in all"""
    if n_kmers == 0:
        return []
    g = rng.integers(0, 4, size=n_kmers + k - 1, dtype=np.uint8)
    return cut(g, k, mixed_lens(rng, n_kmers, longest))


def run_case(k, shift, seed, note, run_kmers=WAVE_KMERS + 1, both_orientations=False, flipped=False, tail=WAVE_KMERS // 2, **info):
    """`shift` k-mers of ordinary unitigs, a run of at least run_kmers k-mers that share the planted minimizer (then, for
    both_orientations, the reverse complements of the run's unitigs), ordinary unitigs behind.  info['run'] = the run's k-mer range."""
    rng = np.random.default_rng(seed)
    per = k - MMER + 1
    n_run = (run_kmers + per - 1) // per
    head = filler_unitigs(rng, k, shift)
    run = planted_unitigs(rng, k, n_run)
    back = [rc_bytes(s) for s in run] if both_orientations else []
    seqs = head + run + back + filler_unitigs(rng, k, tail)
    keys = canonical_keys(seqs, k)
    if flipped:   # the run's keys in their larger form
        rk = canonical_keys(run, k)
        keys = np.unique(np.concatenate([np.setdiff1d(keys, rk), synth.revcomp_u64(rk, k)]))
    return Case(seqs, k, keys, some_counts(rng, len(keys)), note, run=(shift, shift + n_run * per),
                run_back=(shift + n_run * per, shift + 2 * n_run * per) if both_orientations else None, **info)


def overflowing_waves(case):
    """the wavefronts that must hand on more than REST_CAP k-mers: those with more than REST_CAP + LINE_KEYS k-mers of one run
    (all of a run's keys name one first line, which holds ten of them)"""
    out = []
    n = int(graph_kmers(case[0], case[1])[2][-1])
    for rng_ in (case.info.get("run"), case.info.get("run_back")):
        if not rng_:
            continue
        for w in range((n + WAVE_KMERS - 1) // WAVE_KMERS):
            inside = min(rng_[1], (w + 1) * WAVE_KMERS) - max(rng_[0], w * WAVE_KMERS)
            if inside - LINE_KEYS > REST_CAP:
                out.append(w)
    return out


def boundary_ms():
    return list(range(1024, 2304 + 1, 16))


def boundary_case(m, k=25, seed=500):
    """a wavefront of m k-mers that are in no table, then k-mers that are; a second wavefront of k-mers that are"""
    rng = np.random.default_rng(seed + m)
    per = 16
    assert m % per == 0 and 0 < m < WAVE_KMERS
    absent = [to_bytes(rng.integers(0, 4, size=per + k - 1, dtype=np.uint8)) for _ in range(m // per)]
    g = rng.integers(0, 4, size=2 * WAVE_KMERS - m + k - 1, dtype=np.uint8)
    present = cut(g, k, [per] * ((2 * WAVE_KMERS - m) // per))
    keys = canonical_keys(present, k)
    return Case(absent + present, k, keys, some_counts(rng, len(keys)), "m = %d absent k-mers in front" % m, absent=True, n_absent_unitigs=m // per)


# ---- the single-sample cases ---------------------------------------------------------------------------------------------------------

def _shape_lens():
    """name -> unitig lengths in k-mers"""
    rng = np.random.default_rng(1)
    out = {}
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        out["n%d" % n] = mixed_lens(rng, n, 40)
    for r in range(1, 7):
        out["rows%d" % r] = mixed_lens(rng, 64 * r, 50)
        out["rows%d_ragged" % r] = mixed_lens(rng, 64 * r - 31, 50)
    for name, n in (("wave", WAVE_KMERS), ("wave_plus1", WAVE_KMERS + 1), ("four_waves", 4 * WAVE_KMERS), ("four_waves_plus1", 4 * WAVE_KMERS + 1)):
        out[name] = mixed_lens(rng, n, 120)
    out["all_k"] = [1] * (WAVE_KMERS + 130)
    out["all_k_plus_1"] = [2] * (WAVE_KMERS // 2 + 67)
    out["one_long"] = [3, 1, 70, 2 * WAVE_KMERS + 900, 2, 1, 130]
    for name, rem in (("ends_lane0", 1), ("ends_lane62", 63), ("ends_lane63", 0)):
        out[name + "_long_last"] = mixed_lens(rng, 64 * 70 + rem - 150 + (64 if rem == 0 else 0), 90) + [150]
        out[name + "_short_last"] = mixed_lens(rng, 64 * 5 + rem - 1 + (64 if rem == 0 else 0), 30) + [1]
    out["every_word_offset"] = [33 + (i * 7) % 65 for i in range(120)]   # lengths 33 .. 97: every p & 31 on many lanes
    return out


SHAPES = _shape_lens()
K_SWEEP = (25, 31, 5, 9, 16, 17, 18, 21, 30)


def _shape(name, k=25):
    return genome_case(k, SHAPES[name], 1000 + sorted(SHAPES).index(name), "shape %s" % name)


def _k_case(k):
    rng = np.random.default_rng(k)
    return genome_case(k, mixed_lens(rng, 2 * WAVE_KMERS + 777, 150), 2000 + k, "k = %d" % k, palindromes=12 if k % 2 == 0 else 0)


def _orientation(kind, k=25, seed=3000):
    rng = np.random.default_rng(seed + k)
    base = genome_case(k, mixed_lens(rng, 20000, 150), seed + k, "stored keys: %s" % kind, palindromes=8 if k % 2 == 0 else 0)
    seqs, _, keys, counts, note = base
    rcs = synth.revcomp_u64(keys, k)
    if kind == "canonical":
        pass
    elif kind == "larger":
        keys = np.maximum(keys, rcs)
    elif kind == "half":
        keys = np.where(rng.random(len(keys)) < 0.5, rcs, keys)
    elif kind == "both500":
        pick = np.flatnonzero(keys != rcs)[::7][:500]
        assert len(pick) == 500
        keys = np.concatenate([keys, rcs[pick]])
        counts = np.concatenate([counts, counts[pick] + 1000]).astype(np.uint32)
    else:
        raise KeyError(kind)
    o = np.argsort(keys)
    return Case(seqs, k, keys[o], counts[o], note)


def _counts(kind):
    rng = np.random.default_rng(4000)
    base = genome_case(25, mixed_lens(rng, 9000, 8), 4001, "counts: %s" % kind)
    seqs, k, keys, counts, note = base
    if kind == "ones":
        return Case(seqs, k, keys, np.ones(len(keys)), note)
    if kind == "all_max":
        return Case(seqs, k, keys, np.full(len(keys), 65535), note)
    if kind in ("wide", "marker_max"):   # 1, max_count and values between; max_count = 2^32 - 1 is the joined array's marker
        mx = (1 << 32) - 2 if kind == "wide" else (1 << 32) - 1
        c = rng.integers(1, mx - 1, size=len(keys), dtype=np.uint64)
        c[::3] = 1
        c[1::3] = (1 << 32) - 2
        return Case(seqs, k, keys, c, note, max_count=mx, joined=kind == "wide")
    if kind == "filtered":
        # the records of every third unitig lie below min_count: those unitigs miss, their neighbours (k - 1 shared bases: the same
        # minimizers, the same lines) are found
        fw, rc, first = graph_kmers(seqs, k)
        can = np.minimum(fw, rc)
        cut_u = np.arange(len(seqs)) % 3 == 1
        low = np.unique(can[np.repeat(cut_u, np.diff(first))])
        c = rng.integers(100, 60000, size=len(keys), dtype=np.uint64)
        c[np.isin(keys, low)] = rng.integers(1, 100, size=int(np.isin(keys, low).sum()), dtype=np.uint64)
        return Case(seqs, k, keys, c, note, min_count=100, max_count=59999, absent=True)
    raise KeyError(kind)


CASES = {}
for _n in SHAPES:
    CASES["shape_" + _n] = (lambda n=_n: _shape(n))
for _k in K_SWEEP:
    CASES["k%d" % _k] = (lambda k=_k: _k_case(k))
for _k in (25, 31):
    CASES["overflow_aligned_k%d" % _k] = (lambda k=_k: run_case(k, 0, 5000 + k, "a run of one minimizer over a whole wavefront"))
    for _s in (1, 63, 2048):
        CASES["overflow_shift%d_k%d" % (_s, _k)] = (lambda k=_k, s=_s: run_case(k, s, 5100 + k + s, "the run shifted by %d k-mers" % s,
                                                                                   run_kmers=2 * WAVE_KMERS + 64))
    CASES["family_both_orientations_k%d" % _k] = (lambda k=_k: run_case(k, 0, 5200 + k, "a family read in both orientations", both_orientations=True))
for _kind in ("canonical", "larger", "half", "both500"):
    CASES["stored_%s" % _kind] = (lambda kind=_kind: _orientation(kind))
CASES["stored_larger_k18"] = lambda: _orientation("larger", k=18)
CASES["stored_half_k18"] = lambda: _orientation("half", k=18)
# (1200 k-mers of the family in one wavefront beside 2748 ordinary ones: that the hand-over stays below REST_CAP -- about 1200 + 460 of
# 2048 -- rests on the ordinary k-mers' one in six, not on construction; test_crowded_list_case_stays_below_the_overflow holds what is)
CASES["crowded_and_larger"] = lambda: run_case(25, 700, 5300, "a family stored in its larger form, handed on by the list", run_kmers=1200, flipped=True)
CASES["crowded_and_larger_overflow"] = lambda: run_case(25, 0, 5301, "a family stored in its larger form over a whole wavefront", flipped=True)
for _kind in ("ones", "all_max", "wide", "marker_max", "filtered"):
    CASES["counts_%s" % _kind] = (lambda kind=_kind: _counts(kind))

MUST_OVERFLOW = [n for n in CASES if n.startswith(("overflow_", "family_")) or n == "crowded_and_larger_overflow"]


# ---- the colored cases: (seqs, k, dbs, note), dbs = [(keys, counts, both_strands)] -----------------------------------------------

def _colour_dbs(rng, keys, n_colors):
    return [(keys, some_counts(rng, len(keys)), 1) for _ in range(n_colors)]


def colored_plain(n_colors, lens=None, k=25, seed=7000):
    rng = np.random.default_rng(seed + n_colors)
    base = genome_case(k, lens if lens is not None else mixed_lens(rng, WAVE_KMERS + 500, 120), seed + n_colors, "")
    return base[0], k, _colour_dbs(rng, base[2], n_colors), "%d colours, every k-mer in every colour" % n_colors


def colored_overflow_base(n_colors, k=25):
    """the single-sample case whose graph and keys colored_overflow() takes (its info says where the run lies)"""
    return run_case(k, 0, 7100 + n_colors, "")


def colored_overflow(n_colors, k=25):
    base = colored_overflow_base(n_colors, k)
    rng = np.random.default_rng(7100 + n_colors)
    return base[0], k, _colour_dbs(rng, base[2], n_colors), "%d colours, a run of one minimizer over a whole wavefront" % n_colors


def colored_variant(kind, k=25, seed=7200):
    rng = np.random.default_rng(seed)
    base = genome_case(k, mixed_lens(rng, WAVE_KMERS + 900, 12), seed, "")
    seqs, _, keys, _, _ = base
    rcs = synth.revcomp_u64(keys, k)
    dbs = _colour_dbs(rng, keys, 3)
    if kind == "absent_in_one":   # colour 1 lacks the k-mers of every fourth unitig, colour 2 those of every fifth
        fw, rc, first = graph_kmers(seqs, k)
        can = np.minimum(fw, rc)
        for c, every in ((1, 4), (2, 5)):
            gone = np.unique(can[np.repeat(np.arange(len(seqs)) % every == 2, np.diff(first))])
            keep = ~np.isin(keys, gone)
            dbs[c] = (keys[keep], dbs[c][1][keep], 1)
    elif kind == "one_colour_alone_larger":   # (one colour: no k-mer is a key twice, the pipelined kernel looks for the smaller form)
        dbs = [(np.sort(np.maximum(keys, rcs)), dbs[0][1], 1)]
    elif kind == "all_colours_larger":
        dbs = [(np.sort(np.maximum(keys, rcs)), d[1], 1) for d in dbs[:2]]
    elif kind == "all_colours_quarter_larger":
        # every colour stores the same random quarter of the k-mers as their larger form: no k-mer is a key twice, so the pipelined
        # kernel runs, misses those k-mers as their smaller form and hands them on -- a quarter of a wavefront's k-mers and the
        # ordinary one in six of the others, about 1500 of REST_CAP (half of them flipped would overflow the slice and leave the
        # answer to the redo branch): the list branch of k_cov_join_colored_rest with keys that are not canonical
        k1 = np.where(rng.random(len(keys)) < 0.25, rcs, keys)
        o = np.argsort(k1)
        dbs = [(k1[o], d[1][o], 1) for d in dbs]
    elif kind == "one_colour_half_larger":
        k1 = np.where(rng.random(len(keys)) < 0.5, rcs, keys)
        o = np.argsort(k1)
        dbs[1] = (k1[o], dbs[1][1][o], 1)
    elif kind == "opposite_forms":
        dbs = [dbs[0], (np.sort(np.maximum(keys, rcs)), dbs[1][1], 1)]
    elif kind == "unread_colour":
        both = np.unique(np.concatenate([keys, rcs]))
        dbs[1] = (both, some_counts(rng, len(both)), 0)
    elif kind == "empty_colour":
        dbs[2] = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 1)
    else:
        raise KeyError(kind)
    return seqs, k, dbs, "colours: %s" % kind


COLORED_SHAPES = list(SHAPES)   # k_cov_join_colored is a copy of the pipeline: every shape again
COLORED_CASES = {}
for _c in (1, 2, 3, 8, 9):
    COLORED_CASES["plain_c%d" % _c] = (lambda c=_c: colored_plain(c))
for _n in COLORED_SHAPES:
    COLORED_CASES["shape_%s_c3" % _n] = (lambda n=_n: colored_plain(3, SHAPES[n], seed=7300 + COLORED_SHAPES.index(n)))
for _c in (2, 8):
    COLORED_CASES["overflow_c%d" % _c] = (lambda c=_c: colored_overflow(c))
for _kind in ("absent_in_one", "one_colour_alone_larger", "all_colours_larger", "all_colours_quarter_larger", "one_colour_half_larger", "opposite_forms", "unread_colour", "empty_colour"):
    COLORED_CASES[_kind] = (lambda kind=_kind: colored_variant(kind))
COLORED_WITH_ABSENT = {"absent_in_one", "empty_colour"}
COLORED_MUST_OVERFLOW = {"overflow_c2": lambda: colored_overflow_base(2), "overflow_c8": lambda: colored_overflow_base(8)}
