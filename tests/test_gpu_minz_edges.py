"""K-MINZ (pf_minimizer_crowding, pf_minimizer_replay_inputs) against the plain census of tests/minz_cases.py: integer work, so
every figure is held exactly -- the u32 table, its maximum, the crowded slots, the saturating bytes and the flag of every unitig,
at every window size from 1 to 29, at unitig lengths that end on and beside a step of the kernel and a word of the packed
sequence, with more unitigs than the launch has wavefronts, and with a table of 2^17 slots."""
import numpy as np
import pytest

import minz_cases as mc
from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device()
    yield d
    d.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_census_and_hand_off_are_the_plain_census(dev, name):
    c = mc.case(name)
    dev.upload_graph(*hipapi.pack_unitigs(c.seqs), c.k)
    for limit in mc.LIMITS:
        r = mc.reference(name, limit)
        for again in (False, True):   # the tables are cleared per call: the second answer is the first
            mx, crowded, table = dev.minimizer_crowding(c.g, limit, want_table=True)
            counters8, flags = dev.minimizer_replay_inputs(c.g, limit)
            what = (name, limit, again)
            assert len(table) == c.slots and len(counters8) == c.slots and len(flags) == len(c.seqs), what
            bad = np.nonzero(table != r.table)[0]
            assert len(bad) == 0, (what, bad[:8], table[bad[:8]], r.table[bad[:8]])
            assert (mx, crowded) == (r.max, r.crowded), what
            assert np.array_equal(counters8, r.counters8), what
            assert np.array_equal(flags, r.flags), (what, np.nonzero(flags != r.flags)[0][:8])
            assert dev.minimizer_crowding(c.g, limit) == (r.max, r.crowded), what


def test_bad_arguments_are_refused(dev):
    c = mc.case("lengths_k25_g17")
    dev.upload_graph(*hipapi.pack_unitigs(c.seqs), c.k)
    for g, limit in ((c.k - 1, 15), (0, 15), (c.g, 0)):
        for call in (dev.minimizer_crowding, dev.minimizer_replay_inputs):
            with pytest.raises(hipapi.DeviceError) as e:
                call(g, limit)
            assert e.value.status == hipapi.PF_ERR_ARG, (g, limit)
    assert dev.minimizer_crowding(c.g, 15) == (mc.reference(c.name, 15).max, 0)   # (and the context still answers)
    empty = hipapi.Device()
    try:
        for call in (empty.minimizer_crowding, empty.minimizer_replay_inputs):
            with pytest.raises(hipapi.DeviceError) as e:
                call(17, 15)
            assert e.value.status == hipapi.PF_ERR_ARG
    finally:
        empty.close()


@pytest.mark.parametrize("k,g", mc.USUAL_PAIRS + [(31, 29), (31, 1)])
def test_replay_from_the_device_arrays(dev, tmp_path, k, g):
    """the real hand-off: K-MINZ's counters and flags through the host replay give the host-only numbering"""
    L = hostapi.load_library()
    moved = 0
    for name, seqs in mc.crowded_graphs(k + 2, k, g).items():
        gfa, want, got = (str(tmp_path / x) for x in ("%s.gfa" % name, "want.txt", "got.txt"))
        mc.write_gfa(gfa, seqs, k, g)
        assert L.pfh_gfa_write_unitig_ids(gfa.encode(), want.encode()) == 0
        order = mc.loader_order(seqs, k)
        dev.upload_graph(*hipapi.pack_unitigs(order), k)
        counters8, flags = dev.minimizer_replay_inputs(g, 15)
        assert L.pfh_gfa_write_unitig_ids_given_arrays(gfa.encode(), got.encode(), counters8.ctypes.data, len(counters8),
                                                       flags.ctypes.data, len(flags)) == 0, L.pfh_last_error(None)
        assert open(got, "rb").read() == open(want, "rb").read(), name
        moved += L.pfh_gfa_abundant_kmers(gfa.encode())
    if (k, g) in mc.USUAL_PAIRS:
        assert moved > 0
