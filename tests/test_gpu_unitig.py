"""K-UNITIG (pf_unitig_*, csrc/pf_unitig.hip), the host streaming (hostapi.build_graph) and the `build` sub-command against the rule
restated in Python (unitig_cases.py): every comparison of a text is equality of its bytes, every comparison of statistics equality of
all six; against what the reference's Bifrost wrote (tests/golden/build_*) the comparator of unitig_cases.py.  Shapes are the smallest
that reach each path: chains round the powers of two of the jumping rounds, closed cycles, every id width, more k-mers than a block,
and one graph of more k-mers than a whole grid of this device has threads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import count_cases as cc
import unitig_cases as uc

from ploidyfrost_amd import hipapi, hostapi

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
CASES = uc.cases()
FLAG_FILES = {"none": (False, False), "i": (True, False), "d": (False, True), "id": (True, True)}
FLAG_ARGS = {(False, False): [], (True, False): ["-i"], (False, True): ["-d"], (True, True): ["-i", "-d"]}


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)


def keys(S):
    return np.array(sorted(uc.encode(x) for x in S), dtype=np.uint64)


def fixture(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "meta.json")) as f:
        k = json.load(f)["k"]
    with open(os.path.join(d, "reads.fq"), "rb") as f:
        text = f.read()
    reads = text.split(b"\n")[1::4]
    return dict(dir=d, k=k, path=os.path.join(d, "reads.fq"), reads=reads, S=uc.kmer_set(reads, k))


def six(st):
    return {f: st[f] for f in uc.STATS}


# ---- the kernels, through pf_unitig_build ----

@pytest.mark.parametrize("name,k,reads", CASES, ids=[c[0] for c in CASES])
def test_every_case_and_flag_combination(dev, name, k, reads):
    S, want = uc.expected(name, k, reads)
    km = keys(S)
    for flags in uc.FLAGS:
        for again in range(2):   # a release that left something behind shows in the second build of the context
            text, st = dev.unitig_build(km, k, *flags)
            assert text == want[flags][0], (flags, again)
            assert six(st) == want[flags][1], (flags, again)


def test_more_than_one_grid_pass(dev):
    """Every kernel of K-UNITIG strides over its items with one grid of at most (compute units x 8) blocks of 256 threads
    (pf::ctx_grid), so a graph of more k-mers than that many threads makes the kernels over k-mers, over oriented k-mers and, with
    the single k-mers kept (-i alone clips the tips and keeps them), over lines take the stride more than once; the scan, the select
    and the sort run over thousands of tiles.  Tips, rejoined backbones, long chains and closed cycles lie beyond the first pass
    too: keys are random, so sorting scatters them.  The reference is unitig_cases.grid_expected over the host's restatement."""
    per_pass = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    km, parts = uc.grid_case(per_pass + per_pass // 4)
    assert len(km) > per_pass
    for kind in ("tip", "backbone", "cycle", "cycle_tip", "longest", "short"):   # some k-mer of every kind is beyond the first pass of a kernel over k-mers
        assert np.searchsorted(km, parts[kind]).max() >= per_pass, kind
    want_text, want = uc.grid_expected(km, 25, True, False, hostapi.unitig_build_host)
    assert want["unitigs_out"] > per_pass and want["removed"] >= len(parts["tip"]) // 5 and want["longest"] == 3000 + 24
    text, st = dev.unitig_build(km, 25, True, False)
    print("compute units x 8 x 256 = %d, k-mers %d, %s" % (per_pass, len(km), st))
    assert six(st) == want
    assert text == want_text
    assert st["cycles"] == 3 and st["rounds"] == (2 * len(km) - 1).bit_length() + 1   # a closed cycle: the rank stage runs to its cap
    want_text, want = uc.grid_expected(km, 25, True, True, hostapi.unitig_build_host)   # nearly every k-mer dead in the second adjacency pass
    assert want["removed"] > per_pass
    text, st = dev.unitig_build(km, 25, True, True)
    assert six(st) == want
    assert text == want_text


def test_rounds_cycles_and_stage_times(dev):
    by_name = {name: (k, reads) for name, k, reads in CASES}
    for name, (k, reads) in by_name.items():
        if not name.startswith("chain"):
            continue
        m = int(name[5:])   # k-mers; the farthest node is m - 1 links from the start: a round moves something while 2^(round - 1) < m - 1, one more sees nothing move
        _, st = dev.unitig_build(keys(uc.kmer_set(reads, k)), k)
        assert st["rounds"] == 1 + (max(m - 2, 0)).bit_length() and st["cycles"] == 0 and st["cycle_rounds"] == 0, (name, st)
        assert set(st["stage_ms"]) == set(hipapi.UNITIG_STAGES) and all(v >= 0 for v in st["stage_ms"].values())
    for name, n in (("cycle2", 2), ("cycle3", 3), ("cycle64", 64), ("cycle500", 500)):
        k, reads = by_name[name]
        _, st = dev.unitig_build(keys(uc.kmer_set(reads, k)), k, True, True)
        assert st["cycles"] == 1 and st["unitigs"] == 1 and st["removed"] == 0 and 1 <= st["cycle_rounds"] <= n.bit_length() + 1, (name, st)
    k, reads = by_name["cycle_tip"]       # the removal closes the cycle: one unitig more before than closed cycles after
    _, st = dev.unitig_build(keys(uc.kmer_set(reads, k)), k, True, False)
    assert (st["unitigs"], st["removed"], st["unitigs_out"], st["cycles"]) == (2, 1, 1, 1)


def test_device_pointer_g_and_determinism(dev):
    f = fixture("build_k25")
    km = keys(f["S"])
    want = uc.build(f["S"], 25, True, True, g=11)
    on_device = torch.from_numpy(km.view(np.int64)).cuda()
    a = dev.unitig_build(km, 25, True, True, g=11)
    b = dev.unitig_build(on_device, 25, True, True, g=11)
    assert a[0] == b[0] == want[0] and six(a[1]) == six(b[1]) == want[1]
    assert np.array_equal(on_device.cpu().numpy().view(np.uint64), km)   # the input is not written


def test_kernel_is_timed_under_its_name(dev):
    f = fixture("build_k7")
    dev.enable_timing(True)
    dev.reset_timing()
    try:
        dev.unitig_build(keys(f["S"]), 7, True, True)
        ms, launches = dev.kernel_time(hipapi.K_UNITIG)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_UNITIG) == len(f["S"])
        assert dev.L.pf_kernel_name(hipapi.K_UNITIG) == b"k_unitig"
    finally:
        dev.enable_timing(False)
        dev.reset_timing()


def test_refusals(dev):
    km = keys(uc.kmer_set(uc.HAND_READS, 5))
    stats = np.zeros(1, dtype=hipapi.UNITIG_STATS)
    L = dev.L

    def refused(word, *args):
        st = L.pf_unitig_build(dev.h, *args, stats.ctypes.data)
        assert st == hipapi.PF_ERR_ARG and word in L.pf_last_error(dev.h).decode(), (word, st, L.pf_last_error(dev.h))

    p = km.ctypes.data
    refused("k = 2: -k goes from 3 to 31", p, len(km), 2, 1, 0, 0)
    refused("k = 32: -k goes from 3 to 31", p, len(km), 32, 1, 0, 0)
    refused("g = 0: -g goes from 1 to k - 2 = 3", p, len(km), 5, 0, 0, 0)
    refused("g = 4: -g goes from 1 to k - 2 = 3", p, len(km), 5, 4, 0, 0)
    for g in (0, -1, 4):   # the Python call: None alone is the default
        with pytest.raises(RuntimeError, match="-g goes from 1 to k - 2 = 3"):
            dev.unitig_build(km, 5, g=g)
    assert dev.unitig_build(km, 5)[0].startswith(uc.header(5).encode())
    refused("2^31 or more distinct k-mers", p, 1 << 31, 5, 3, 0, 0)           # refused before anything is read
    refused("kmers is needed", None, 3, 5, 3, 0, 0)
    refused("kmers is not aligned", p + 4, 3, 5, 3, 0, 0)
    for bad in (km[::-1].copy(), np.concatenate([km[:3], km[2:]]), np.array([uc.encode("TTTTT")], dtype=np.uint64), np.array([1 << 10], dtype=np.uint64)):
        refused("not sorted distinct canonical k-mers", bad.ctypes.data, len(bad), 5, 3, 0, 0)
    assert L.pf_unitig_fetch(dev.h, 0, 1, stats.ctypes.data) == hipapi.PF_ERR_ARG and "no built graph is held" in L.pf_last_error(dev.h).decode()
    # a second build without a release, and a fetch outside the text
    assert L.pf_unitig_build(dev.h, p, len(km), 5, 3, 1, 1, stats.ctypes.data) == hipapi.PF_OK
    try:
        refused("a built graph is held already (pf_unitig_release comes first)", p, len(km), 5, 3, 1, 1)
        n = int(stats[0]["bytes"])
        buf = np.zeros(n + 8, dtype=np.uint8)
        assert L.pf_unitig_fetch(dev.h, n, 1, buf.ctypes.data) == hipapi.PF_ERR_ARG and "outside the text of %d bytes" % n in L.pf_last_error(dev.h).decode()
        assert L.pf_unitig_fetch(dev.h, 1, n, buf.ctypes.data) == hipapi.PF_ERR_ARG
        assert L.pf_unitig_fetch(dev.h, 0, n, buf.ctypes.data) == hipapi.PF_OK and L.pf_unitig_fetch(dev.h, n, 0, None) == hipapi.PF_OK
        want = uc.build(uc.kmer_set(uc.HAND_READS, 5), 5, True, True)[0]
        assert buf[:n].tobytes() == want
        piece = np.zeros(7, dtype=np.uint8)
        assert L.pf_unitig_fetch(dev.h, 30, 7, piece.ctypes.data) == hipapi.PF_OK and piece.tobytes() == want[30:37]
    finally:
        assert L.pf_unitig_release(dev.h) == hipapi.PF_OK
    assert L.pf_unitig_release(dev.h) == hipapi.PF_OK   # nothing held: nothing to do
    assert dev.unitig_build(km, 5, True, True)[0] == want


# ---- the host streaming and the sub-command ----

@pytest.mark.parametrize("name", ["build_k25", "build_k7"])
def test_cli_on_the_fixture_reads(name, tmp_path):
    f = fixture(name)
    counted = cc.ref_count(f["reads"], f["k"], ci=1, cs=10 ** 9)[2]
    for tag, flags in FLAG_FILES.items():
        want, st = uc.build(f["S"], f["k"], *flags)
        r = run_cli("build", "-k", f["k"], "-r", f["path"], "-o", tmp_path / tag, "-t", 16, *FLAG_ARGS[flags])
        assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
        assert r.stderr == "build: reads %d bases %d kmers %d bad %d distinct %d unitigs %d removed %d unitigs_out %d longest %d bytes %d\n" % (
            counted["reads"], counted["bases"], counted["kmers"], counted["kmers_bad"], st["distinct"], st["unitigs"], st["removed"], st["unitigs_out"],
            st["longest"], st["bytes"])
        got = (tmp_path / (tag + ".gfa")).read_bytes()
        assert got == want
        with open(os.path.join(f["dir"], tag + ".gfa"), "rb") as ref:
            assert uc.same_graph(got, ref.read()), tag
    assert sorted(os.listdir(tmp_path)) == sorted(t + ".gfa" for t in FLAG_FILES)


def test_cli_chunks_table_size_two_inputs_and_verbose(tmp_path):
    f = fixture("build_k25")
    want, st = uc.build(f["S"], 25, True, True, g=9)
    outs = []
    for tag, extra in (("dflt", []), ("chunk", ["--chunk-bytes", 4096]), ("slots", ["--initial-slots", 64]), ("both", ["--chunk-bytes", 4096, "--initial-slots", 64])):
        r = run_cli("build", "-i", "-d", "-k", 25, "-g", 9, "-r", f["path"], "-o", tmp_path / tag, *extra)
        assert r.returncode == 0, r.stderr
        outs.append((tmp_path / (tag + ".gfa")).read_bytes())
    assert all(o == want for o in outs)
    half = len(f["reads"]) // 2
    (tmp_path / "a.fq").write_bytes(uc.fastq(f["reads"][:half]))
    (tmp_path / "b.fq").write_bytes(uc.fastq(f["reads"][half:]))
    r = run_cli("build", "-i", "-d", "-k", 25, "-g", 9, "-r", tmp_path / "a.fq", "-r", tmp_path / "b.fq", "-o", tmp_path / "two", "-v")
    assert r.returncode == 0 and (tmp_path / "two.gfa").read_bytes() == want
    assert all(w in r.stderr for w in ("stream", "finish", "graph", "write", "index", "adjacency", "simplify", "rank", "rounds", "cycles", "emit"))
    api = hostapi.build_graph([str(tmp_path / "a.fq"), str(tmp_path / "b.fq")], str(tmp_path / "api"), k=25, clip_tips=True, del_isolated=True, g=9,
                              chunk_bytes=10000)
    assert (tmp_path / "api.gfa").read_bytes() == want and six(api) == st and api["reads"] == len(f["reads"])


def test_cli_input_without_a_kmer(tmp_path):
    (tmp_path / "short.fq").write_bytes(uc.fastq(["ACGTACGT", "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"]))
    r = run_cli("build", "-i", "-d", "-k", 25, "-r", tmp_path / "short.fq", "-o", tmp_path / "s")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "s.gfa").read_bytes() == uc.header(25).encode()
    assert "distinct 0 unitigs 0 removed 0 unitigs_out 0 longest 0 bytes %d (no k-mer in the input: the header line alone is written)" % len(uc.header(25)) in r.stderr


@pytest.mark.parametrize("name,record", [("does not start with '@'", 200), ("quality line's length", 100), ("not a multiple of four", 384)])
def test_cli_format_refusals_leave_nothing(tmp_path, name, record):
    f = fixture("build_k25")
    lines = open(f["path"], "rb").read().rstrip(b"\n").split(b"\n")
    if "multiple" in name:
        lines += [b"@extra", b"ACGT"]
    elif "@" in name:
        lines[4 * record] = b"x" + lines[4 * record][1:]
    else:
        lines[4 * record + 3] = lines[4 * record + 3][:-1]
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"\n".join(lines))
    for chunk in (4096, 1 << 20):
        r = run_cli("build", "-k", 25, "-r", f["path"], "-r", bad, "-o", tmp_path / "s", "--chunk-bytes", chunk)
        assert r.returncode != 0 and r.stdout == ""
        assert "build: %s: record %d: " % (bad, record + 1) in r.stderr and name in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["bad.fq"]


def test_api_refusals_leave_nothing(tmp_path):
    f = fixture("build_k7")
    for kw, word in ((dict(k=2), "-k goes from 3 to 31"), (dict(k=7, g=6), "-g goes from 1 to k - 2 = 5"), (dict(k=7, g=-1), "-g goes from 1 to k - 2 = 5")):
        with pytest.raises(RuntimeError, match=word):
            hostapi.build_graph(f["path"], str(tmp_path / "s"), **kw)
    with pytest.raises(RuntimeError, match="build: no input"):
        hostapi.build_graph([], str(tmp_path / "s"))
    assert os.listdir(tmp_path) == []


# ---- through the product ----

def test_built_graph_and_counted_database_through_the_calling_run(tmp_path):
    """`build -i -d` and `count -ci1 -cs10000` on the k = 25 fixture reads, then the calling run on the two: the twelve files of the CPU
    oracle on the same graph and database, with a variant site among them"""
    f = fixture("build_k25")
    r = run_cli("build", "-i", "-d", "-k", 25, "-r", f["path"], "-o", tmp_path / "s")
    assert r.returncode == 0, r.stderr
    r = run_cli("count", "-k25", "-ci1", "-cs10000", "-i", f["path"], "-o", tmp_path / "db")
    assert r.returncode == 0, r.stderr
    gfa, db = str(tmp_path / "s.gfa"), str(tmp_path / "db")
    run = hostapi.Run(gfa, db)
    run.set_output_dir(str(tmp_path / "gpu"))
    run.set_unitig_id("g")
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 1, 1000)
    run.close()
    pyoracle.Oracle(gfa, db).run(str(tmp_path / "cpu"), "g", lower=1, upper=1000)
    names = sorted(os.listdir(tmp_path / "cpu"))
    assert len(names) == 12 and sorted(os.listdir(tmp_path / "gpu")) == names
    for n in names:
        assert (tmp_path / "gpu" / n).read_bytes() == (tmp_path / "cpu" / n).read_bytes(), n
    assert (tmp_path / "cpu" / "g_allele_frequency.txt").stat().st_size > 0 and (tmp_path / "cpu" / "g_bifre.txt").stat().st_size > 0
