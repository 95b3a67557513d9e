"""K-HETPAIR on the device (pf_hetpairs through hipapi.Device.hetpairs) against the host's plain restatement of csrc/pf_hetpair_rule.hpp
(hostapi.hetpairs_host; test_hetpair_cpu.py holds that one to the Python rule): the table, the pairs in their order, the counters and
the statistics, word for word.  There is no tolerance anywhere.  The shapes are the smallest at which the kernel can go wrong (a row is
16 lanes, a wavefront takes 64 keys and four of them at a time, a lane 3 x 16 substitutions a turn, HOME_M + 2 = 18 changes the
table's line addressing, k = 31 fills the word), plus one of 200 000 keys for the contention path of the table kernel."""
import numpy as np
import pytest
import torch

import hetpair_cases as hp

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases():
    return hp.small_cases()


def same(got, want, pairs=True):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    for f in ("pair_x", "pair_y", "cov_x", "cov_y"):
        if pairs:
            assert np.array_equal(got[f], want[f]), f
        else:
            assert got[f] is None
    assert np.array_equal(got["table"], want["table"]), np.argwhere(got["table"] != want["table"])[:8]


def upload(dev, km, ct, k):
    dev.upload_counts(km, ct, 1, 0xFFFFFFFF, True, k=k)


CASES = ["k5_all", "k5_every_second_out", "k4_subset0", "k4_subset1", "k4_subset2", "k4_aatt", "hap_k17", "hap_k18", "hap_k25", "hap_k31", "triallelic",
         "two_close", "edges", "w1", "w4096", "n1", "n63", "n64", "n65", "in_range15", "in_range16", "in_range17"]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_host_rule(dev, cases, name):
    km, ct, k, lo, hi = cases[name]
    upload(dev, km, ct, k)
    want = hostapi.hetpairs_host(km, ct, k, lo, hi)
    same(dev.hetpairs(km, ct, k, lo, hi), want)


def test_the_k25_fixture_has_its_725_pairs_in_one_cell(dev, cases):
    km, ct, k, lo, hi = cases["hap_k25"]
    upload(dev, km, ct, k)
    r = dev.hetpairs(km, ct, k, lo, hi)
    assert len(km) == 3701 and r["stats"]["pairs"] == 725 == int(r["table"][20 - lo, 20 - lo]) == int(r["table"].sum())
    assert np.all(r["pair_x"][:-1] < r["pair_x"][1:]) and np.all(r["pair_x"] < r["pair_y"])


def test_no_keys_is_a_valid_call(dev, cases):
    km, ct, k, lo, hi = cases["hap_k25"]
    upload(dev, km, ct, k)   # (a table of the same k is still needed)
    r = dev.hetpairs(km[:0], ct[:0], k, lo, hi)
    assert r["stats"] == {"kmers": 0, "in_range": 0, "one_partner": 0, "many_partners": 0, "pairs": 0}
    assert not r["table"].any() and all(len(r[f]) == 0 for f in ("pair_x", "pair_y", "cov_x", "cov_y"))


def test_pairs_not_wanted_table_not_wanted_and_device_pointers(dev, cases):
    km, ct, k, lo, hi = cases["hap_k25"]
    upload(dev, km, ct, k)
    want = hostapi.hetpairs_host(km, ct, k, lo, hi)
    same(dev.hetpairs(km, ct, k, lo, hi, want_pairs=False), want, pairs=False)
    r = dev.hetpairs(km, ct, k, lo, hi, want_table=False)
    assert r["table"] is None and np.array_equal(r["pair_y"], want["pair_y"]) and r["stats"] == want["stats"]
    r = dev.hetpairs(km, ct, k, lo, hi, want_pairs=False, want_table=False)
    assert r["stats"] == want["stats"]
    # the same arrays in device memory (counters at an address that is 4 but not 16 bytes aligned as well)
    dk = torch.from_numpy(km.view(np.int64)).cuda()
    dc = torch.from_numpy(np.concatenate([[0], ct]).astype(np.uint32).view(np.int32)).cuda()[1:]
    same(dev.hetpairs(dk, dc, k, lo, hi), want)
    same(dev.hetpairs(dk, ct, k, lo, hi), want)   # one of each
    # the table kernel alone, over the compacted counters
    cx, cy = (torch.from_numpy(want[f].view(np.int32)).cuda() for f in ("cov_x", "cov_y"))
    assert np.array_equal(dev.hetpair_table(cx, cy, lo, hi), want["table"])
    assert not dev.hetpair_table(cx, cy, 21, 30).any()   # counters outside the bounds add nothing


def test_all_pairs_in_one_cell(dev):
    """200 000 keys whose pairs all fall into cell (20, 20): the combining path of the table kernel, and more than one wavefront's
    share of every statistic"""
    km, ct, k, lo, hi = hp.one_cell_case()
    upload(dev, km, ct, k)
    want = hostapi.hetpairs_host(km, ct, k, lo, hi)
    assert want["stats"]["pairs"] > 99000 and int(want["table"][0, 0]) == want["stats"]["pairs"]
    same(dev.hetpairs(km, ct, k, lo, hi), want)
    # the same pairs spread over 20 000 cells: the tile in LDS (4 096 slots), the adds of the lanes that find their slot taken, the flush
    ct2 = np.random.default_rng(9).integers(20, 220, size=len(km)).astype(np.uint32)
    upload(dev, km, ct2, k)
    want = hostapi.hetpairs_host(km, ct2, k, 20, 219)
    assert np.count_nonzero(want["table"]) > 3 * 4096
    same(dev.hetpairs(km, ct2, k, 20, 219), want)


def test_refusals_by_name(dev, cases):
    km, ct, k, lo, hi = cases["hap_k25"]
    fresh = hipapi.Device(0)
    try:
        with pytest.raises(hipapi.DeviceError, match="pf_hetpairs: no count table is resident"):
            fresh.hetpairs(km, ct, k, lo, hi)
    finally:
        fresh.close()
    km17, ct17 = cases["hap_k17"][:2]
    upload(dev, km17, ct17, 17)
    with pytest.raises(hipapi.DeviceError, match="pf_hetpairs: the resident count table has k 17, the keys have k 25"):
        dev.hetpairs(km, ct, k, lo, hi)
    dev.upload_counts(km, ct, 1, 0xFFFFFFFF, False, k=k)   # a -b table
    with pytest.raises(hipapi.DeviceError, match="pf_hetpairs: the resident count table was not counted on both strands"):
        dev.hetpairs(km, ct, k, lo, hi)
    upload(dev, km, ct, k)
    for a, b, word in ((0, 10, "lower bound is below 1"), (11, 10, "lower bound is above the upper bound"), (1, 4097, "above 4096")):
        with pytest.raises(hipapi.DeviceError, match=word):
            dev.hetpairs(km, ct, k, a, b)
    same(dev.hetpairs(km, ct, k, lo, hi), hostapi.hetpairs_host(km, ct, k, lo, hi))   # the context is as good as before


def test_timed_as_one_launch_of_its_kernel(dev, cases):
    km, ct, k, lo, hi = cases["hap_k25"]
    upload(dev, km, ct, k)
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        r = dev.hetpairs(km, ct, k, lo, hi)
        ms, launches = dev.kernel_time(hipapi.K_HETPAIR)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_HETPAIR) == r["stats"]["in_range"]
    finally:
        dev.enable_timing(False)
