"""K-MINZ (ploidyfrost_amd/csrc/pf_minz.hip) edge cases and a plain census of minimizer positions, for tests/test_minz_cases_cpu.py
and tests/test_gpu_minz_edges.py.  No expected value here comes from the kernel or from host/pf_host_minz.cpp: the census restates
the definition at the head of pf_minz.hip with nothing of the kernel's tiling, and the minimizer hash (synth.bifrost_minimizer_hash,
a restatement of Bifrost's RepHash) is used as the definition requires -- to compute the census and to CHOOSE inputs.

The definition.  k-mer p of a unitig of L bases (p = 0 .. L-k) has the window of g-mer positions p+1 .. p+k-g-1: a minimizer may
sit at neither end of its k-mer.  A position is counted ONCE per unitig when its hash equals the minimum of the window of at least
one k-mer; where hashes tie inside a window every tied position counts.  A counted position adds one to the slot
mix64(canonical g-mer) & (slots - 1) of a table of `slots` counters, the canonical g-mer being the smaller of the g-mer and its
reverse complement as 2-bit integers (A0 C1 G2 T3, first base most significant).

The geometry the cases aim at.  The kernel decides TQ = 66 - 2W positions of a unitig per step, W = k - g - 1 being the number of
positions in a window, with W - 1 halo lanes on either side of a step; a unitig has the positions 1 .. pmax = L - g - 1.  Hence
the lengths of lengths_for below, for every pair of PAIRS: W = 1 (no halo, TQ = 64) to W = 29 (TQ = 8).

Case classes at limit 15, held by test_minz_cases_cpu.py::test_case_classes (46 cases in all):
    ties 18, no ties 28, a slot past 255 (the narrowing to 8 bits saturates) 17, a slot exactly at the limit 15.
(At W = 1 a window is one position: nothing ties there, not even in a homopolymer.)"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from ploidyfrost_amd import synth

_B = b"ACGT"
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
M64 = (1 << 64) - 1

LIMITS = (15, 1, 256)

# (k, g) by window size W = k - g - 1
PAIRS = [(31, 29), (5, 3), (3, 1),          # W = 1
         (25, 22),                          # W = 2
         (15, 8), (25, 17), (31, 23),       # W = 6 or 7: the pairs of the fixtures
         (31, 14),                          # W = 16
         (31, 2),                           # W = 28
         (31, 1)]                           # W = 29
USUAL_PAIRS = [(15, 8), (25, 17), (31, 23)]


def rc(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def mix64(x: int) -> int:
    """the finaliser of host/pf_host_minz.cpp (not synth.mix64), restated"""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def canonical(gmer: bytes) -> int:
    fw = 0
    for c in gmer:
        fw = (fw << 2) | _CODE[c]
    rv = 0
    for c in rc(gmer):
        rv = (rv << 2) | _CODE[c]
    return min(fw, rv)


def table_slots(n_kmers: int) -> int:
    """pf_minimizer_table_slots, restated: 2^16, doubled while below half the number of k-mers"""
    cap = 1 << 16
    while cap < n_kmers // 2 and cap < (1 << 30):
        cap <<= 1
    return cap


def n_kmers(seqs, k):
    return sum(len(s) - k + 1 for s in seqs)


def tile(k, g):
    """(W, TQ) of the kernel's steps -- used to choose lengths only"""
    W = k - g - 1
    return W, 66 - 2 * W


_hash_cache = {}


def _rephash(gmer: bytes) -> int:
    h = _hash_cache.get(gmer)
    if h is None:
        h = _hash_cache[gmer] = synth.bifrost_minimizer_hash(gmer)
    return h


def counted_positions(s: bytes, k: int, g: int, hash_fn):
    """(sorted counted positions of one unitig, whether some window holds its minimum at two positions)"""
    L = len(s)
    h = [hash_fn(s[q: q + g]) for q in range(L - g + 1)]
    counted, ties = set(), False
    for p in range(L - k + 1):
        win = range(p + 1, p + k - g)
        m = min(h[q] for q in win)
        hits = [q for q in win if h[q] == m]
        ties = ties or len(hits) > 1
        counted.update(hits)
    return sorted(counted), ties


Census = namedtuple("Census", "table max crowded counters8 flags has_ties")


def _slot_lists(seqs, k, g, slots, hash_fn):
    out, ties = [], False
    slot_of = {}
    for s in seqs:
        pos, t = counted_positions(s, k, g, hash_fn)
        ties = ties or t
        sl = []
        for q in pos:
            gm = s[q: q + g]
            x = slot_of.get(gm)
            if x is None:
                x = slot_of[gm] = mix64(canonical(gm)) & (slots - 1)
            sl.append(x)
        out.append(np.array(sl, dtype=np.int64))
    return out, ties


def _census_from(slot_lists, ties, slots, limit):
    table = np.zeros(slots, dtype=np.int64)
    if slot_lists:
        np.add.at(table, np.concatenate(slot_lists), 1)
    full = table >= limit
    flags = np.array([1 if len(sl) and full[sl].any() else 0 for sl in slot_lists], dtype=np.uint8)
    return Census(table, int(table.max()), int(full.sum()), np.minimum(table, 255).astype(np.uint8), flags, ties)


def reference_census(seqs, k, g, slots, limit, hash_fn=_rephash):
    """The plain census of the unitigs `seqs` (see the head of this file): table (int64 per slot), max, crowded = slots with
    table >= limit, counters8 = min(table, 255), flags[u] = 1 when a counted position of unitig u lies in a slot with
    table >= limit, has_ties.  hash_fn: bytes -> int (default: Bifrost's minimizer hash, cached per g-mer)."""
    if hash_fn is synth.bifrost_minimizer_hash:
        hash_fn = _rephash
    sl, ties = _slot_lists(seqs, k, g, slots, hash_fn)
    return _census_from(sl, ties, slots, limit)


# ---- the order the loader stands the unitigs in before the move -----------------------------------------------------------------

def loader_order(seqs, k):
    """segments longer than k in file order, then the k-length ones, each as the smaller of itself and its reverse complement:
    the order of pf_minimizer_replay_inputs' flags and of pfh_gfa_write_unitig_ids_given_arrays"""
    return [s for s in seqs if len(s) > k] + [min(s, rc(s)) for s in seqs if len(s) == k]


def write_gfa(path, seqs, k, g):
    with open(path, "wb") as f:
        f.write(b"H\tVN:Z:1.0\tBV:Z:1.0.6\tKL:Z:%d\tML:Z:%d\n" % (k, g))
        for i, s in enumerate(seqs):
            f.write(b"S\t%d\t%s\n" % (i + 1, s))


# ---- builders (deterministic) -----------------------------------------------------------------------------------------------------

def _rnd(rng, n, alphabet=_B):
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def lengths_for(k, g):
    """one and two k-mers; a window more; the last position on the last lane of step one and two, and on the lane behind it; the
    ends of the 32-base words of the packed sequence and the bases beside them; 300 and about 2000.  Lengths below k dropped."""
    W, TQ = tile(k, g)
    want = [k, k + 1, k + W - 1, k + W, g + 1 + TQ, g + 2 + TQ, g + 1 + 2 * TQ, g + 2 + 2 * TQ,
            32, 33, 63, 64, 65, 96, 97, 128, 129, 300, 2001]
    return sorted({n for n in want if n >= k})


def lengths_case(k, g):
    rng = np.random.default_rng(1000 * k + g)
    return [_rnd(rng, n) for n in lengths_for(k, g)] + [_rnd(rng, k)]


def lowcomplexity_case(k, g):
    """a homopolymer of 330 bases (every window ties, one slot past 255), di- and trinucleotide repeats, a homopolymer run inside
    random sequence, a reverse-complement palindrome -- and k-length pieces of the same"""
    rng = np.random.default_rng(2000 * k + g)
    half = _rnd(rng, k + 5)
    W, TQ = tile(k, g)
    return [b"A" * 330, (b"AC" * 80)[: max(k, g + 2 + TQ)], (b"ACG" * 60)[: max(k, 150)], (b"GT" * 40)[:k], b"T" * k,
            _rnd(rng, 40) + b"T" * (k + 9) + _rnd(rng, 40), half + rc(half), _rnd(rng, k)]


def planted_core(k, g, seed):
    """the g-mer with the lowest hash of 3000 random ones (as the crowded graphs of test_host_logic_cpu.py choose theirs)"""
    rng = np.random.default_rng(seed)
    return min((_rnd(rng, g) for _ in range(3000)), key=_rephash)


def planted_case(k, g, sharers):
    """`sharers` k-length unitigs that hold one planted g-mer at the window offsets 1 .. k-g-1 in turn, where it is the one
    strict minimum -- then three unitigs each with it at offset 0 and at offset k-g, the two ends, where it must not be
    counted (and no other position of those holds it).  Its slot gets exactly `sharers`.  At g = 1 the flanks avoid the planted
    base and its complement, which random flanks could not.  Returns (unitigs, the planted g-mer)."""
    rng = np.random.default_rng(3000 * k + 10 * g + sharers)
    core = planted_core(k, g, 77 * k + g)
    hc, cc = _rephash(core), canonical(core)
    alphabet = bytes(b for b in _B if bytes([b]) not in (core, rc(core))) if g == 1 else _B
    W = k - g - 1
    seqs = []

    def draw(o, counted):
        for _ in range(20000):
            s = _rnd(rng, o, alphabet) + core + _rnd(rng, k - g - o, alphabet)
            others = [s[q: q + g] for q in range(1, k - g) if q != o]
            if all(_rephash(x) > hc for x in others) if counted else all(canonical(x) != cc for x in others):
                return s
        raise RuntimeError("no flanks found for (%d, %d)" % (k, g))

    for i in range(sharers):
        seqs.append(draw(1 + i % W, True))
    for o in (0, k - g):
        for _ in range(3):
            seqs.append(draw(o, False))
    return seqs, core


def grid_stride_case():
    """more unitigs than the launch has wavefronts (16 blocks of four per CU: 16 384 at 256 CUs): k-length ones, some of them
    through one planted g-mer"""
    k, g = 15, 8
    rng = np.random.default_rng(515)
    core = planted_core(k, g, 99)
    seqs = []
    for i in range(20500):
        if i % 500 == 7:
            o = 1 + (i // 500) % (k - g - 1)
            seqs.append(_rnd(rng, o) + core + _rnd(rng, k - g - o))
        else:
            seqs.append(_rnd(rng, k))
    return seqs


def wide_table_case():
    """more than 131 072 k-mers: the table has 2^17 slots"""
    k = 15
    rng = np.random.default_rng(616)
    seqs = [_rnd(rng, 2000) for _ in range(67)] + [_rnd(rng, k) for _ in range(40)]
    assert n_kmers(seqs, k) > 131072
    return seqs


Case = namedtuple("Case", "name k g seqs slots note")

_BUILDERS = {}
for _k, _g in PAIRS:
    _BUILDERS["lengths_k%d_g%d" % (_k, _g)] = (_k, _g, lambda k=_k, g=_g: lengths_case(k, g), "random unitigs of every length of lengths_for")
    _BUILDERS["lowcx_k%d_g%d" % (_k, _g)] = (_k, _g, lambda k=_k, g=_g: lowcomplexity_case(k, g), "homopolymer of 330, repeats, palindrome")
    _BUILDERS["planted14_k%d_g%d" % (_k, _g)] = (_k, _g, lambda k=_k, g=_g: planted_case(k, g, 14)[0], "one g-mer counted 14 times: one short of the limit")
    _BUILDERS["planted15_k%d_g%d" % (_k, _g)] = (_k, _g, lambda k=_k, g=_g: planted_case(k, g, 15)[0], "one g-mer counted 15 times: exactly the limit")
_BUILDERS["grid_stride"] = (15, 8, grid_stride_case, "20 500 k-length unitigs: the grid-stride loop runs")
_BUILDERS["wide_table"] = (15, 8, wide_table_case, "more than 131 072 k-mers: 2^17 slots")
for _k, _g in USUAL_PAIRS + [(31, 29)]:
    # (what the device sees of a graph: the loader's order, the hand-off's indexing)
    _BUILDERS["mixed_k%d_g%d" % (_k, _g)] = (_k, _g, lambda k=_k, g=_g: lengths_case(k, g)[::3] + planted_case(k, g, 15)[0] + lowcomplexity_case(k, g)[:3],
                                             "long and k-length unitigs interleaved, a crowded slot among them")
del _k, _g

NAMES = list(_BUILDERS)
LARGE = ["grid_stride", "wide_table"]


@lru_cache(maxsize=None)
def case(name):
    """the unitigs of a case in the loader's order (what is uploaded; flags are indexed so), with the table size"""
    k, g, build, note = _BUILDERS[name]
    seqs = loader_order(build(), k)
    return Case(name, k, g, seqs, table_slots(n_kmers(seqs, k)), note)


@lru_cache(maxsize=None)
def _slots_of_case(name):
    c = case(name)
    return _slot_lists(c.seqs, c.k, c.g, c.slots, _rephash)


@lru_cache(maxsize=None)
def reference(name, limit=15):
    """reference_census of a case, computed once and shared (do not write into its arrays)"""
    sl, ties = _slots_of_case(name)
    r = _census_from(sl, ties, case(name).slots, limit)
    for a in (r.table, r.counters8, r.flags):
        a.setflags(write=False)
    return r


def classes(name):
    """the class of a case, at limit 15: ties or none, a slot past 255, a slot exactly at the limit"""
    r = reference(name, 15)
    return dict(ties=r.has_ties, saturated=r.max > 255, at_limit=bool((r.table == 15).any()))


# ---- graphs built to crowd buckets, for the hand-off ---------------------------------------------------------------------------------

def crowded_graphs(seed, k, g):
    """test_host_logic_cpu._crowded_graphs, every segment at least k long (its `mixed` set is shorter than k where g is small:
    those are padded with a fixed text)"""
    from test_host_logic_cpu import _crowded_graphs
    out = {}
    for name, seqs in _crowded_graphs(seed, k, g).items():
        out[name] = [s if len(s) >= k else s + (b"ACGTTGCA" * 4)[: k - len(s)] for s in seqs]
    return out
