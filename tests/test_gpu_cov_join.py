"""K-COV-JOIN (k_cov_join + k_cov_join_rest, and the colored twins) against a plain look-up, on the inputs of tests/join_cases.py:
the shapes of the software pipeline, hand-over lists that overflow, tables whose keys are not canonical, counts at the edges of
their range, contexts that are used again.  Three routes to the same numbers -- pf_unitig_cov (join, then K-COV streams the joined
array), pf_unitig_cov_probe (K-COV probes the table) and join_cases.reference_unitig_cov (np.searchsorted) -- compared with
np.array_equal: all of it is integer work.  tests/test_join_cases_cpu.py holds the reference and the builders' preconditions."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import join_cases as jc  # noqa: E402
from ploidyfrost_amd import hipapi  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(tag, got, want, ok=None):
    got, want = np.asarray(got), np.asarray(want)
    if ok is not None:
        got, want = got[ok], want[ok]
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).ravel())
        pytest.fail("%s: %d of %d differ, first at %d: got %s, expected %s" % (tag, len(bad), got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]]))


def _spans(n, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(6):
        u0 = int(rng.integers(0, n))
        out.append((u0, int(rng.integers(u0 + 1, n + 1))))
    return out + [(0, 1), (n - 1, n)]


def compare(d, ref, tag, joined=True):
    """both routes of a context against the reference: whole range, ragged sub-ranges, single unitigs at either end; then the join
    once more"""
    es, em, emiss = ref
    ok = emiss == 0

    def one(route, u0, u1):
        s, m, x, st = route(u0, u1)
        t = "%s %s [%d, %d)" % (tag, route.__name__, u0, u1)
        _same(t + " miss", x, emiss[u0:u1])
        _same(t + " sum", s, es[u0:u1], ok[u0:u1])
        _same(t + " min", m, em[u0:u1], ok[u0:u1])
        assert st == (hipapi.PF_OK if ok[u0:u1].all() else hipapi.PF_ERR_MISSING_KMER), t
        return s, m, x

    first = one(d.unitig_cov, 0, d.n)
    one(d.unitig_cov_probe, 0, d.n)
    for u0, u1 in _spans(d.n):
        one(d.unitig_cov, u0, u1)
        one(d.unitig_cov_probe, u0, u1)
    if joined:
        d.join_counts()
        again = one(d.unitig_cov, 0, d.n)
        for a, b in zip(first, again):
            _same(tag + " after a second join", b, a)
    else:   # max_count = 2^32 - 1 is the joined array's marker: such a table keeps the probing form
        with pytest.raises(hipapi.DeviceError):
            d.join_counts()


def check(case, seqs=None, tag=""):
    _, k, keys, counts, note = case
    seqs = case[0] if seqs is None else seqs
    info = case.info
    ref = jc.reference_unitig_cov(seqs, k, keys, counts, info["min_count"], info["max_count"])
    assert ref[2].any() == info["absent"]
    assert 2 * int((ref[2] == 0).sum()) >= len(seqs)   # at least half of the unitigs are compared on sum and min
    packed = hipapi.pack_unitigs(seqs)
    for order in ("graph first", "counts first"):
        d = hipapi.Device(0)
        try:
            if order == "graph first":
                d.upload_graph(*packed, k)
                d.upload_counts(keys, counts, info["min_count"], info["max_count"], True)
            else:
                d.upload_counts(keys, counts, info["min_count"], info["max_count"], True, k=k)
                d.upload_graph(*packed, k)
            compare(d, ref, "%s%s (%s), %s" % (tag, note, "k = %d" % k, order), info["joined"])
        finally:
            d.close()


@pytest.mark.parametrize("name", list(jc.CASES))
def test_join_equals_plain_lookup(name):
    check(jc.CASES[name]())


@pytest.mark.parametrize("name", [n for n in jc.CASES if not n.startswith("shape_")])
def test_join_equals_plain_lookup_kmer_by_kmer(name):
    """the same graph cut into one-k-mer unitigs: sum[u] is the count of k-mer u, so a failure names the k-mer"""
    case = jc.CASES[name]()
    check(case, jc.single_kmer_unitigs(case[0], case[1]), "one k-mer a unitig: ")


def test_hand_over_list_at_its_capacity():
    """m absent k-mers in a wavefront are handed on for certain, the present ones when their first line was full (about one in six):
    somewhere in the sweep the hand-over of the first wavefront is within 16 k-mers of the slice's capacity, on either side
    (tests/test_join_cases_cpu.py: test_boundary_sweep_crosses_the_capacity)"""
    for m in jc.boundary_ms():
        check(jc.boundary_case(m))


# ---- a context used again ------------------------------------------------------------------------------------------------------

def _two_graphs():
    big = jc.genome_case(25, jc.mixed_lens(np.random.default_rng(61), 5 * jc.WAVE_KMERS + 321, 150), 6100, "large")
    small = jc.genome_case(25, jc.mixed_lens(np.random.default_rng(62), 97, 20), 6200, "small")
    keys = np.concatenate([big[2], small[2]])
    counts = np.concatenate([big[3], small[3]])
    o = np.argsort(keys)
    assert (np.diff(keys[o]) > 0).all()
    return big, small, keys[o], counts[o]


def test_graphs_of_other_sizes_under_one_table():
    """the hand-over lists and the joined array are sized by the first graph; a smaller and then a larger one follow"""
    big, small, keys, counts = _two_graphs()
    d = hipapi.Device(0)
    d.upload_counts(keys, counts, 1, 65535, True, k=25)
    for g in (big, small, big, small):
        d.upload_graph(*hipapi.pack_unitigs(g[0]), 25)
        compare(d, jc.reference_unitig_cov(g[0], 25, keys, counts, 1, 65535), g[4] + " graph under one table")
    d.close()
    d = hipapi.Device(0)   # the small one first
    d.upload_counts(keys, counts, 1, 65535, True, k=25)
    for g in (small, big):
        d.upload_graph(*hipapi.pack_unitigs(g[0]), 25)
        compare(d, jc.reference_unitig_cov(g[0], 25, keys, counts, 1, 65535), g[4] + " graph under one table, small first")
    d.close()


def test_a_second_table_under_one_graph():
    a = jc.CASES["stored_canonical"]()
    d = hipapi.Device(0)
    d.upload_graph(*hipapi.pack_unitigs(a[0]), a[1])
    for name in ("stored_canonical", "stored_larger", "stored_both500", "stored_half", "stored_canonical"):
        t = jc.CASES[name]()
        assert t[0] == a[0]
        d.upload_counts(t[2], t[3], 1, 65535, True)
        compare(d, jc.reference_unitig_cov(a[0], a[1], t[2], t[3], 1, 65535), "table %s under the same graph" % name)
    half = a[2][::2].copy(), a[3][::2].copy()   # a table that lacks every second key
    d.upload_counts(half[0], half[1], 1, 65535, True)
    ref = jc.reference_unitig_cov(a[0], a[1], half[0], half[1], 1, 65535)
    assert ref[2].any()
    compare(d, ref, "half a table under the same graph")
    d.close()


def test_join_begun_and_read_without_end():
    """pf_join_counts_begin, a traversal beside the look-ups, then the coverage: the reader waits for the join by itself"""
    big, _, keys, counts = _two_graphs()
    d = hipapi.Device(0)
    d.upload_graph(*hipapi.pack_unitigs(big[0]), 25)
    d.upload_counts(keys, counts, 1, 65535, True)
    d.build_adjacency(want_host=False)
    ref = jc.reference_unitig_cov(big[0], 25, keys, counts, 1, 65535)
    for _ in range(2):
        d._check(d.L.pf_join_counts_begin(d.h))
        d.bfs()
        s, m, x, st = d.unitig_cov()
        assert st == hipapi.PF_OK
        _same("sum after begin + bfs", s, ref[0])
        _same("min after begin + bfs", m, ref[1])
        _same("miss after begin + bfs", x, ref[2])
    compare(d, ref, "after begin without end")
    d.close()


# ---- the colored twin -----------------------------------------------------------------------------------------------------------

def compare_colored(d, ref, tag):
    es, elo, ehi, emiss = ref
    ok = emiss == 0

    def one(probe, u0, u1):
        s, lo, hi, x = d.unitig_cov_colored(u0, u1, probe=probe)
        t = "%s %s [%d, %d)" % (tag, "probed" if probe else "joined", u0, u1)
        _same(t + " miss", x, emiss[:, u0:u1])
        _same(t + " sum", s, es[:, u0:u1], ok[:, u0:u1])
        _same(t + " min", lo, elo[:, u0:u1], ok[:, u0:u1])
        _same(t + " max", hi, ehi[:, u0:u1], ok[:, u0:u1])
        return s, lo, hi, x

    first = one(False, 0, d.n)
    one(True, 0, d.n)
    for u0, u1 in _spans(d.n, 3):
        one(False, u0, u1)
        one(True, u0, u1)
    d.join_counts()
    for a, b in zip(first, one(False, 0, d.n)):
        _same(tag + " after a second join", b, a)


@pytest.mark.parametrize("name", list(jc.COLORED_CASES))
def test_colored_join_equals_plain_lookup(name):
    seqs, k, dbs, note = jc.COLORED_CASES[name]()
    ref = jc.reference_unitig_cov_colored(seqs, k, dbs)
    assert bool(ref[3].any()) == (name in jc.COLORED_WITH_ABSENT)
    packed = hipapi.pack_unitigs(seqs)
    d = hipapi.Device(0)
    try:
        d.upload_graph(*packed, k)
        # (the colored table is addressed by the graph's k: the graph comes first; max_count below 2^32 - 1, the joined array's
        # marker, or the table would keep the probing form and the join kernels would not run)
        d.upload_counts_colored(dbs, 1, 65535)
        compare_colored(d, ref, note)
        d.upload_graph(*packed, k)     # the graph again under the resident table: joined on the next call
        compare_colored(d, ref, note + ", graph uploaded again")
    finally:
        d.close()
