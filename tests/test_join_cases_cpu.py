"""tests/join_cases.py kept honest without a GPU: its plain reference against the pinned CPU oracle on committed fixtures, and the
precondition every case builder states (tests/test_gpu_cov_join.py relies on them: it cannot see how many k-mers a wavefront of
K-COV-JOIN hands on)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_case

sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle  # noqa: E402

import join_cases as jc  # noqa: E402
from ploidyfrost_amd import synth  # noqa: E402


# (stranded20k, a database without canonical counting, is not in the list: the oracle reads it per orientation and the composite
# look-up restated here does not apply to it)
@pytest.mark.parametrize("case", ["dip20k", "k31_z16", "dip_kmc2", "strandmix"])
def test_reference_equals_the_oracle(case):
    meta = load_case(case)
    kmers, counts, km = synth.read_kmc(meta["db"])
    assert km["both_strands"]
    o = pyoracle.Oracle(meta["gfa"], meta["db"])
    s, m, miss = jc.reference_unitig_cov(o.sequences(), o.k, kmers, counts, km["min_count"], km["max_count"])
    es, em, emiss = o.unitig_cov()
    assert not miss.any() and not emiss.any()
    assert np.array_equal(s, es) and np.array_equal(m, em)


@pytest.mark.parametrize("case", ["col3_dip", "col3_stranded"])
def test_colored_reference_equals_the_oracle(case, tmp_path):
    meta = load_case(case)
    o = pyoracle.ColoredOracle(meta["gfa"], meta["colors_dump"], meta["dbs"], str(tmp_path))
    seqs = o.sequences()
    dbs = []
    for p in meta["dbs"]:
        km, cnt, hdr = synth.read_kmc(p)
        dbs.append((km, cnt, hdr["both_strands"]))
    s, lo, hi, miss = jc.reference_unitig_cov_colored(seqs, o.k, dbs)
    assert s.shape == (o.n_colors, o.n)
    for cut in ([(5, 1000)] * o.n_colors, meta["cutoffs"], [(25, 45)] * o.n_colors):
        for c in range(o.n_colors):
            low, up = cut[c]
            for u in range(o.n):
                mean, ok = o.unitig_cov_color(c, u, low, up)   # readCovUni: (sum / len, every count inside (low, up) and none missing)
                got_ok = (not miss[c, u]) and lo[c, u] > low and hi[c, u] < up
                assert bool(ok) == bool(got_ok), (case, c, u)
                if ok:
                    assert mean == float(s[c, u]) / (len(seqs[u]) - o.k + 1)


def test_reference_takes_the_form_as_read_first():
    """src/CDBG.cpp:78-82 on a table that holds both forms of a k-mer, by hand"""
    k = 5
    seq = b"ACGTTGCA"   # ACGTT CGTTG GTTGC TTGCA
    fw, rc = synth.kmers_u64(jc._LUT[np.frombuffer(seq, dtype=np.uint8)], k)
    keys = np.array([fw[0], rc[0], rc[1], fw[3]], dtype=np.uint64)
    counts = np.array([7, 70, 5, 20000], dtype=np.uint32)
    o = np.argsort(keys)
    s, m, miss = jc.reference_unitig_cov([seq[:5], seq[1:6], seq[2:7], seq[3:8], seq[:6]], k, keys[o], counts[o], 1, 65535)
    assert list(s) == [7, 5, 0, 20000, 12] and list(m) == [7, 5, 10000, 10000, 5] and list(miss) == [0, 0, 1, 0, 0]
    s, m, miss = jc.reference_unitig_cov([seq[:5], seq[3:8]], k, keys[o], counts[o], 6, 100)   # 5 and 20000 are not retrievable
    assert list(s) == [7, 0] and list(miss) == [0, 1]


@pytest.mark.parametrize("name", list(jc.CASES))
def test_case_is_what_it_says(name):
    case = jc.CASES[name]()
    seqs, k, keys, counts, note = case
    assert (keys[1:] > keys[:-1]).all() and len(keys) == len(counts)
    assert all(len(s) >= k for s in seqs)
    n_kmers = int(jc.graph_kmers(seqs, k)[2][-1])
    assert n_kmers <= 300_000
    s, m, miss = jc.reference_unitig_cov(seqs, k, keys, counts, case.info["min_count"], case.info["max_count"])
    if case.info["absent"]:
        assert miss.any() and 2 * int((miss == 0).sum()) >= len(seqs)   # at least half of the unitigs are compared on sum and min
    else:
        assert not miss.any()
    again = jc.CASES[name]()
    assert again[0] == seqs and np.array_equal(again[2], keys) and np.array_equal(again[3], counts)   # deterministic


def test_shapes_are_the_ones_listed():
    n = {name: sum(v) for name, v in jc.SHAPES.items()}
    assert [n["n%d" % x] for x in (1, 2, 63, 64, 65, 127, 128, 129)] == [1, 2, 63, 64, 65, 127, 128, 129]
    assert [n["rows%d" % r] for r in range(1, 7)] == [64 * r for r in range(1, 7)]
    assert (n["wave"], n["wave_plus1"], n["four_waves"], n["four_waves_plus1"]) == (4096, 4097, 16384, 16385)
    assert set(jc.SHAPES["all_k"]) == {1} and set(jc.SHAPES["all_k_plus_1"]) == {2}
    assert max(jc.SHAPES["one_long"]) > 2 * jc.WAVE_KMERS
    for name, lane in (("ends_lane0", 0), ("ends_lane62", 62), ("ends_lane63", 63)):
        for v in ("_long_last", "_short_last"):
            assert (n[name + v] - 1) % 64 == lane
    # a unitig of 32 k-mers or more has a k-mer at every offset p & 31 of a sequence word, 0 and 31 included
    assert min(jc.SHAPES["every_word_offset"]) >= 32
    assert set(jc.K_SWEEP) == {25, 31, 5, 9, 16, 17, 18, 21, 30}


@pytest.mark.parametrize("k", [16, 18, 30])
def test_even_k_cases_hold_palindromes(k):
    seqs, _, keys, _, _ = jc.CASES["k%d" % k]()
    fw, rc, _ = jc.graph_kmers(seqs, k)
    assert int((fw == rc).sum()) >= 8 and (keys == synth.revcomp_u64(keys, k)).any()


@pytest.mark.parametrize("name", jc.MUST_OVERFLOW + list(jc.COLORED_MUST_OVERFLOW))
def test_overflow_is_guaranteed_by_construction(name):
    """More than REST_CAP of a wavefront's k-mers cannot be in their first line: every k-mer of the run holds the planted 16-mer, no
    16-mer of any key has a smaller hash (so it is the minimizer of all of them and they name one line of ten keys), and the
    run's k-mers are distinct keys of the table."""
    case = jc.CASES[name]() if name in jc.CASES else jc.COLORED_MUST_OVERFLOW[name]()
    seqs, k, keys, counts, note = case
    if name in jc.COLORED_MUST_OVERFLOW:   # the colored case is this graph under these keys in every colour
        cs, ck, dbs, _ = jc.COLORED_CASES[name]()
        assert cs == seqs and ck == k and all(np.array_equal(d[0], keys) and d[2] for d in dbs)
    c, h = jc.planted_mmer()
    assert h >= 1 and int((c * jc.K_MUL) & 0xFFFFFFFF) == h
    hashes = jc.minimizer_hashes(keys, k)
    assert int(hashes.min()) >= h   # (sixteen A's or T's would hash to 0)
    fw, rc, first = jc.graph_kmers(seqs, k)
    can = np.minimum(fw, rc)
    stored = set(keys.tolist())
    for a, b in [r for r in (case.info["run"], case.info["run_back"]) if r]:
        assert (jc.minimizer_hashes(fw[a:b], k) == h).any(axis=1).all()
        assert len(np.unique(can[a:b])) == b - a
        assert all((int(x) in stored) or (int(y) in stored) for x, y in zip(fw[a:b], rc[a:b]))
    waves = jc.overflowing_waves(case)
    assert waves, "no wavefront holds more than REST_CAP + LINE_KEYS k-mers of the run"
    if "shift" in name or "aligned" in name or "family" in name or name in jc.COLORED_MUST_OVERFLOW:
        assert any(case.info["run"][0] <= w * jc.WAVE_KMERS and (w + 1) * jc.WAVE_KMERS <= case.info["run"][1] for w in waves)


def test_crowded_list_case_stays_below_the_overflow():
    """the family stored in its larger form that is meant for the LIST branch of k_cov_join_rest: too few of its k-mers in a wavefront
    to fill the slice by themselves"""
    case = jc.CASES["crowded_and_larger"]()
    assert not jc.overflowing_waves(case)
    a, b = case.info["run"]
    assert b - a >= 1200 and a // jc.WAVE_KMERS == (b - 1) // jc.WAVE_KMERS
    keys, k = case[2], case[1]
    fw, rc, _ = jc.graph_kmers(case[0], k)
    assert np.isin(np.maximum(fw[a:b], rc[a:b]), keys).all() and not np.isin(np.minimum(fw[a:b], rc[a:b]), keys).any()


def test_boundary_sweep_crosses_the_capacity():
    ms = jc.boundary_ms()
    assert ms[0] == 1024 and ms[-1] == 2304 and max(b - a for a, b in zip(ms, ms[1:])) <= 16
    # at m = 1024 the hand-over stays below REST_CAP unless more than a third of the 3072 present k-mers miss their first line; at
    # m = 2304 it is above whatever they do
    assert 1024 + (jc.WAVE_KMERS - 1024) // 3 <= jc.REST_CAP < 2304
    for m in (ms[0], ms[len(ms) // 2], ms[-1]):
        case = jc.boundary_case(m)
        seqs, k, keys, counts, note = case
        first = jc.graph_kmers(seqs, k)[2]
        assert int(first[-1]) == 2 * jc.WAVE_KMERS and int(first[case.info["n_absent_unitigs"]]) == m
        s, mn, miss = jc.reference_unitig_cov(seqs, k, keys, counts, 1, 65535)
        assert miss[: case.info["n_absent_unitigs"]].all() and not miss[case.info["n_absent_unitigs"]:].any()
        assert 2 * int((miss == 0).sum()) > len(seqs)


def test_orientation_cases_store_what_they_say():
    k = 25
    keys = {kind: jc.CASES["stored_" + kind]()[2] for kind in ("canonical", "larger", "half", "both500")}
    rc = {kind: synth.revcomp_u64(v, k) for kind, v in keys.items()}
    assert (keys["canonical"] <= rc["canonical"]).all()
    assert (keys["larger"] >= rc["larger"]).all() and not np.isin(rc["larger"], keys["larger"]).any()
    frac = float((keys["half"] > rc["half"]).mean())
    assert 0.4 < frac < 0.6 and not np.isin(rc["half"], keys["half"]).any()
    assert int(np.isin(rc["both500"], keys["both500"]).sum()) == 1000
    # the forward form wins: the graph reads some of the doubly stored k-mers in each orientation
    seqs = jc.CASES["stored_both500"]()[0]
    fw, r, _ = jc.graph_kmers(seqs, k)
    twice = keys["both500"][np.isin(rc["both500"], keys["both500"])]
    read = fw[np.isin(fw, twice)]
    assert (read < synth.revcomp_u64(read, k)).any() and (read > synth.revcomp_u64(read, k)).any()


@pytest.mark.parametrize("name", list(jc.COLORED_CASES))
def test_colored_case_is_what_it_says(name):
    seqs, k, dbs, note = jc.COLORED_CASES[name]()
    for d in dbs:
        assert (d[0][1:] > d[0][:-1]).all() and len(d[0]) == len(d[1])
    s, lo, hi, miss = jc.reference_unitig_cov_colored(seqs, k, dbs)
    if name == "all_colours_quarter_larger":   # a one-strand table of keys that are not all canonical, the same in every colour
        keys = dbs[0][0]
        rc = synth.revcomp_u64(keys, k)
        assert all(np.array_equal(d[0], keys) for d in dbs) and not np.isin(rc, keys).any() and 0.2 < float((keys > rc).mean()) < 0.3
    if name in jc.COLORED_WITH_ABSENT:
        assert miss.any() and 2 * int((miss == 0).sum()) >= miss.size
        if name == "absent_in_one":   # present in one colour and absent in another
            assert ((miss[0] == 0) & (miss[1] == 1)).any() and ((miss[1] == 0) & (miss[2] == 1)).any()
    else:
        assert not miss.any()
