"""K-BFS's entry points against each other (csrc/pf_bfs.hip), on the two smallest graphs whose traversals outgrow the wavefront tier:
the lattice of depth 7 (two traversals of more than 128 vertices) and giant7k (one of more than 4096).

The reference is A = Device.bfs(): pf_bfs_candidates, every tier on the device, itself checked against the CPU oracle (the lattice in
test_gpu_kernels.py::test_bfs_big_tier_matches_oracle, giant7k here).  pf_bfs_candidates_split, _begin/_end and _resident hand the
long traversals to the caller instead: what they return must be A with exactly those records left empty.  Bit-exact: integer work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from bfs_cases import lattice_gfa
from conftest import ROOT, load_case

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

from ploidyfrost_amd import hipapi, hostapi  # noqa: E402

pytestmark = pytest.mark.gpu

GRAPHS = ["lattice7", "giant7k"]
_cache = {}


class Graph:
    """a graph resident on a device, and A: the records and the pool of the call that runs every tier on the device (read-only)"""

    def __init__(self, gfa):
        self.o = pyoracle.Oracle(gfa, None)
        self.dev = hipapi.Device(0)
        self.dev.upload_graph(*hipapi.pack_unitigs(self.o.sequences()), self.o.k)
        self.dev.build_adjacency()
        self.rec, self.pool = self.dev.bfs()
        self.rec.setflags(write=False)
        self.pool.setflags(write=False)

    def lists(self, rec=None, pool=None):
        rec, pool = (self.rec, self.pool) if rec is None else (rec, pool)
        return [pool[int(r["list_off"]): int(r["list_off"]) + int(r["n_list"])] for r in rec]


def graph(name, tmp_path_factory) -> Graph:
    if name not in _cache:
        if name == "lattice7":
            gfa = str(tmp_path_factory.mktemp("lattice") / "lattice.gfa")
            lattice_gfa(gfa, depth=7)
        else:
            gfa = load_case(name)["gfa"]
        _cache[name] = Graph(gfa)
    return _cache[name]


def check_handed_over(g: Graph, rec, pool, deferred):
    """`rec` / `pool` are A with the records at `deferred` left to the caller"""
    A = g.rec
    assert len(rec) == len(A)
    d = np.sort(deferred)
    assert len(d) > 0 and len(np.unique(d)) == len(d)
    assert set(np.nonzero(A["n_seen"] > 128)[0].tolist()) <= set(d.tolist())
    empty = np.zeros(len(d), dtype=hipapi.BFS_RECORD)
    empty["entrance"] = A["entrance"][d]
    empty["exit"] = hipapi.NONE
    assert np.array_equal(rec[d], empty)
    rest = np.setdiff1d(np.arange(len(A)), d)
    for f in hipapi.BFS_RECORD.names:
        if f != "list_off":
            assert np.array_equal(rec[f][rest], A[f][rest]), f
    want, got = g.lists(), g.lists(rec, pool)
    for i in rest:
        assert np.array_equal(got[i], want[i]), i


def test_every_tier_on_the_device_matches_the_oracle_on_giant7k(tmp_path_factory):
    g = graph("giant7k", tmp_path_factory)
    huge = 0
    for r, lst in zip(g.rec, g.lists()):
        e = g.o.extract(int(r["entrance"]))
        assert (int(r["outcome"]), int(r["exit"]), int(r["n_seen"])) == (e["outcome"], e["exit"], len(e["seen"]))
        if e["outcome"] != 0:
            assert np.array_equal(lst, e["seen"])
        huge += len(e["seen"]) > 4096
    assert huge >= 1


@pytest.mark.parametrize("name", GRAPHS)
def test_split_and_begin_end_leave_the_long_traversals_to_the_caller(name, tmp_path_factory):
    g = graph(name, tmp_path_factory)
    rec_s, pool_s, def_s = g.dev.bfs_split()
    check_handed_over(g, rec_s, pool_s, def_s)
    try:
        rec_b, pool_b, def_b, ent_b = g.dev.bfs_begin()
    finally:
        g.dev.bfs_end()
    check_handed_over(g, rec_b, pool_b, def_b)
    assert set(def_s.tolist()) == set(def_b.tolist())
    assert np.array_equal(ent_b, g.rec["entrance"][def_b])


@pytest.mark.parametrize("name", GRAPHS)
def test_resident_records_give_the_components_of_the_reference(name, tmp_path_factory):
    g = graph(name, tmp_path_factory)
    _, _, def_s = g.dev.bfs_split()
    n, _, deferred, entrance = g.dev.bfs_resident()
    assert n == len(g.rec)
    assert set(deferred.tolist()) == set(def_s.tolist()) and len(deferred) == len(def_s)
    assert np.array_equal(entrance, g.rec["entrance"][deferred])
    # K-CC over what the call left on the device, the deferred traversals added as the caller that walked them would
    g.dev.side_components(n_records=n, extra=g.rec[deferred], extra_pool=g.pool)
    _, _, labels = g.dev.replay_order(64)
    assert np.array_equal(labels, hostapi.side_components(g.rec, g.pool, g.dev.n))


def test_misuse_is_answered_with_a_status(tmp_path_factory):
    import torch
    g = graph("lattice7", tmp_path_factory)
    dev, L, n = g.dev, g.dev.L, len(g.rec)
    n_deferred = len(dev.bfs_split()[2])
    # a second begin before end
    dev.bfs_begin()
    try:
        with pytest.raises(hipapi.DeviceError) as err:
            dev.bfs_begin()
        assert err.value.status == hipapi.PF_ERR_ARG
    finally:
        dev.bfs_end()
    assert L.pf_bfs_candidates_end(dev.h) == hipapi.PF_OK

    def split(records, n_pool, n_def):
        pool = np.zeros(n_pool, dtype=np.uint32)
        deferred = np.zeros(max(n_def, 1), dtype=np.uint32)
        nr, used, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = L.pf_bfs_candidates_split(dev.h, 0, dev.n, records, n, pool.ctypes.data, n_pool, C.byref(nr), C.byref(used),
                                       deferred.ctypes.data, n_def, C.byref(nd))
        return st, used.value, nd.value

    rec = np.zeros(n, dtype=hipapi.BFS_RECORD)
    st, used, _ = split(rec.ctypes.data, 8, n)
    assert st == hipapi.PF_ERR_OVERFLOW and used > 8
    st, _, needed = split(rec.ctypes.data, 1 << 20, n_deferred - 1)
    assert st == hipapi.PF_ERR_OVERFLOW and needed == n_deferred
    on_device = torch.zeros(n * hipapi.BFS_RECORD.itemsize, dtype=torch.uint8, device="cuda")
    st, _, _ = split(on_device.data_ptr(), 1 << 20, n)
    assert st == hipapi.PF_ERR_ARG
