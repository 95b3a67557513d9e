"""The plain minimizer census of tests/minz_cases.py against a hand-worked example and against the host pass of
host/pf_host_minz.cpp, and the numbering replay run from real arrays (pfh_gfa_write_unitig_ids_given_arrays).  No GPU."""
import numpy as np
import pytest

import minz_cases as mc
from ploidyfrost_amd import hostapi


@pytest.fixture(scope="module")
def L():
    return hostapi.load_library()


def test_hand_worked_census():
    """k = 5, g = 2: the window of k-mer p is the positions p+1 and p+2.  Unitig ACGTTAGCA has the 2-mers
         position  0   1   2   3   4   5   6   7
         2-mer     AC  CG  GT  TT  TA  AG  GC  CA
         toy hash  0   5   3   3   7   9   9   0
    and the windows {1,2} {2,3} {3,4} {4,5} {5,6} with the minima 3 (at 2), 3 (at 2 and 3: a tie counts both), 3 (at 3), 7 (at 4),
    9 (at 5 and 6).  Positions 0 and 7 have the lowest hash of all and lie in no window: the ends are excluded.  Position 2 is the
    minimum of two windows and counts once.  Counted: 2 3 4 5 6, i.e. GT TT TA AG GC with the canonical values 1 (AC) 0 (AA) 12 (TA)
    2 (AG) 9 (GC)."""
    toy = {b"AC": 0, b"CG": 5, b"GT": 3, b"TT": 3, b"TA": 7, b"AG": 9, b"GC": 9, b"CA": 0, b"TC": 8, b"AT": 4}.__getitem__
    k, g, slots = 5, 2, 1 << 16
    assert mc.counted_positions(b"ACGTTAGCA", k, g, toy) == ([2, 3, 4, 5, 6], True)
    assert mc.counted_positions(b"CGTCA", k, g, toy) == ([1], False)   # GT (3) against TC (8)
    assert mc.counted_positions(b"CATAC", k, g, toy) == ([1], False)   # AT (4) against TA (7)
    assert [mc.canonical(x) for x in (b"GT", b"TT", b"TA", b"AG", b"GC", b"AT")] == [1, 0, 12, 2, 9, 3]
    seqs = [b"ACGTTAGCA", b"CGTCA", b"CATAC"]
    slot = lambda c: mc.mix64(c) & (slots - 1)  # noqa: E731
    want = np.zeros(slots, dtype=np.int64)
    for c, n in ((1, 2), (0, 1), (12, 1), (2, 1), (9, 1), (3, 1)):   # GT is counted in the first two unitigs
        want[slot(c)] += n
    assert len({slot(c) for c in (1, 0, 12, 2, 9, 3)}) == 6
    r = mc.reference_census(seqs, k, g, slots, 2, hash_fn=toy)
    assert np.array_equal(r.table, want) and r.max == 2 and r.crowded == 1 and r.has_ties
    assert r.flags.tolist() == [1, 1, 0] and np.array_equal(r.counters8, want)
    r1 = mc.reference_census(seqs, k, g, slots, 1, hash_fn=toy)
    assert r1.crowded == 6 and r1.flags.tolist() == [1, 1, 1]
    assert mc.reference_census(seqs[1:], k, g, slots, 2, hash_fn=toy).has_ties is False
    # the finaliser, by hand for 1: x ^= x >> 33 leaves 1, the first multiplier, and so on
    x = 0xff51afd7ed558ccd
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & mc.M64
    assert mc.mix64(1) == x ^ (x >> 33) and mc.mix64(0) == 0


def test_table_size_and_lengths():
    assert mc.table_slots(0) == 1 << 16 and mc.table_slots(131072) == 1 << 16 and mc.table_slots(131074) == 1 << 17
    assert mc.case("wide_table").slots == 1 << 17 and len(mc.case("grid_stride").seqs) > 16384
    for k, g in mc.PAIRS:
        W, TQ = mc.tile(k, g)
        ls = mc.lengths_for(k, g)
        assert min(ls) == k and k + 1 in ls and 2001 in ls and all(n >= k for n in ls)
        # the last position (pmax = L - g - 1) on the last lane of a step and on the first of the next
        for n in (g + 1 + TQ, g + 2 + TQ, g + 1 + 2 * TQ, g + 2 + 2 * TQ):
            assert n < k or n in ls
    assert mc.tile(31, 29) == (1, 64) and mc.tile(31, 1) == (29, 8) and mc.tile(25, 17) == (7, 52)


def test_case_classes():
    """the numbers at the head of minz_cases.py"""
    cl = [mc.classes(n) for n in mc.NAMES]
    assert len(cl) == 46
    assert sum(c["ties"] for c in cl) == 18 and sum(not c["ties"] for c in cl) == 28
    assert sum(c["saturated"] for c in cl) == 17 and sum(c["at_limit"] for c in cl) == 15


@pytest.mark.parametrize("k,g", mc.PAIRS)
def test_planted_gmer_is_counted_inside_and_not_at_the_ends(k, g):
    """14 or 15 unitigs hold the planted g-mer inside the window, six at offset 0 or k-g: its slot holds 14 or 15 exactly"""
    for n in (14, 15):
        seqs, core = mc.planted_case(k, g, n)
        assert len(seqs) == n + 6 and all(len(s) == k for s in seqs)
        W = k - g - 1
        assert all(s[1 + i % W: 1 + i % W + g] == core for i, s in enumerate(seqs[:n]))   # every offset 1 .. k-g-1 in turn
        assert [s[:g] == core for s in seqs[n: n + 3]] == [True] * 3 and [s[k - g:] == core for s in seqs[n + 3:]] == [True] * 3
        r = mc.reference("planted%d_k%d_g%d" % (n, k, g), 15)
        assert r.table[mc.mix64(mc.canonical(core)) & (len(r.table) - 1)] == n
        if g >= 3:   # (at g = 1 and 2 the flanks of the end unitigs share their few g-mers: other slots fill up too)
            assert r.max == n and r.crowded == (n == 15) and int(r.flags.sum()) == (15 if n == 15 else 0)
            assert r.flags.sum() == 0 or np.array_equal(np.nonzero(r.flags)[0], np.arange(15))


def _host_counts(L, gfa):
    slots = L.pfh_gfa_minimizer_counts(gfa.encode(), None, 0)
    host = np.zeros(slots, dtype=np.uint8)
    assert L.pfh_gfa_minimizer_counts(gfa.encode(), host.ctypes.data, slots) == slots
    return host


def test_host_pass_against_the_census(L, tmp_path):
    """Check A.  The host pass counts what Bifrost's iterator reports: never more than the census, and the same wherever no
    window has tied minima (the iterator reports a tied position only while it leads the window, the census always)."""
    tied, plain = 0, 0
    for name in mc.NAMES:
        c = mc.case(name)
        gfa = str(tmp_path / "g.gfa")
        mc.write_gfa(gfa, c.seqs, c.k, c.g)
        host = _host_counts(L, gfa)
        r = mc.reference(name, 15)
        assert len(host) == c.slots, name
        assert np.all(host <= r.counters8), name
        if r.has_ties:
            tied += 1
        else:
            plain += 1
            assert np.array_equal(host, r.counters8), name
    assert tied >= 3 and plain >= 3


def _ids(L, gfa, out):
    assert L.pfh_gfa_write_unitig_ids(gfa.encode(), out.encode()) == 0
    return open(out, "rb").read()


def _ids_given(L, gfa, out, counters8, flags):
    counters8, flags = np.ascontiguousarray(counters8, dtype=np.uint8), np.ascontiguousarray(flags, dtype=np.uint8)
    st = L.pfh_gfa_write_unitig_ids_given_arrays(gfa.encode(), out.encode(), counters8.ctypes.data, len(counters8), flags.ctypes.data, len(flags))
    return st, (open(out, "rb").read() if st == 0 else None)


@pytest.mark.parametrize("k,g", mc.PAIRS)
def test_replay_from_the_census_arrays(L, tmp_path, k, g):
    """Check B.  The census' counters and flags (limit 15), handed to the replay in place of its own two passes: the numbering is
    the host-only one."""
    moved = 0
    for name, seqs in mc.crowded_graphs(k + 2, k, g).items():
        gfa = str(tmp_path / ("%s.gfa" % name))
        mc.write_gfa(gfa, seqs, k, g)
        want = _ids(L, gfa, str(tmp_path / "want.txt"))
        order = mc.loader_order(seqs, k)
        r = mc.reference_census(order, k, g, mc.table_slots(mc.n_kmers(order, k)), 15)
        st, got = _ids_given(L, gfa, str(tmp_path / "got.txt"), r.counters8, r.flags)
        assert st == 0 and got == want, name
        moved += L.pfh_gfa_abundant_kmers(gfa.encode())
    if (k, g) in mc.USUAL_PAIRS:
        assert moved > 0   # the replay really ran


def test_replay_refuses_arrays_of_another_geometry(L, tmp_path):
    k, g = 25, 17
    seqs = mc.crowded_graphs(2, k, g)["shorts"]
    gfa, out = str(tmp_path / "g.gfa"), str(tmp_path / "got.txt")
    mc.write_gfa(gfa, seqs, k, g)
    order = mc.loader_order(seqs, k)
    r = mc.reference_census(order, k, g, 1 << 16, 15)
    assert _ids_given(L, gfa, out, r.counters8, r.flags)[0] == 0
    for c8, fl, word in ((r.counters8[:-1], r.flags, b"counters"), (np.concatenate([r.counters8, r.counters8]), r.flags, b"counters"),
                         (r.counters8, r.flags[:-1], b"flags"), (r.counters8, np.append(r.flags, 1), b"flags")):
        st, _ = _ids_given(L, gfa, out, c8, fl)
        assert st != 0 and word in L.pfh_last_error(None)
    assert L.pfh_gfa_write_unitig_ids_given_arrays(gfa.encode(), out.encode(), None, 1 << 16, None, len(order)) != 0


def test_replay_goes_by_the_flags_it_is_given(L, tmp_path):
    """Control.  `shorts` at (25, 17): 50 k-length unitigs share a minimizer, the 35 behind the first 15 move to the end.  With the
    true counters and every flag cleared no unitig is replayed and nothing moves: the flags are what the replay runs from, and a
    missing one changes the numbering (the host derives flags itself only in a later round, after a redirect)."""
    k, g = 25, 17
    seqs = mc.crowded_graphs(2, k, g)["shorts"]
    gfa = str(tmp_path / "g.gfa")
    mc.write_gfa(gfa, seqs, k, g)
    assert L.pfh_gfa_abundant_kmers(gfa.encode()) == 35
    want = _ids(L, gfa, str(tmp_path / "want.txt"))
    order = mc.loader_order(seqs, k)
    r = mc.reference_census(order, k, g, 1 << 16, 15)
    assert r.flags.sum() == 50
    st, got = _ids_given(L, gfa, str(tmp_path / "got.txt"), r.counters8, np.zeros_like(r.flags))
    unmoved = b"".join(b"%d\t%s\n" % (i + 1, s) for i, s in enumerate(order))
    assert st == 0 and got == unmoved and got != want
    # one flag missing (the sixteenth sharer, the first to move): it stays where it was
    fl = r.flags.copy()
    sharers = np.nonzero(fl)[0]
    fl[sharers[15]] = 0
    st, got = _ids_given(L, gfa, str(tmp_path / "got.txt"), r.counters8, fl)
    assert st == 0 and got != want and got.splitlines()[sharers[15]].split(b"\t")[1] == order[sharers[15]]
