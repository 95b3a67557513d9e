"""K-COLOR (pf_unitig_build_colored in csrc/pf_unitig.hip, pf_color_* in csrc/pf_color.hip), the host streaming
(hostapi.build_colored_graph) and the `build-multi` sub-command against the host's plain restatement (hostapi.build_colored_host),
which tests/test_unitig_color_cpu.py holds to the Python rule and to the real Bifrost: every comparison of a file is equality of its
bytes, every comparison of statistics equality of all twelve.  Shapes are unitig_color_cases.cases(): the smallest at which a colour
set takes each form, the colour counts round a 64-bit word, strands, removed tips, the edges of the 1024-byte tile, a placement that
overflows, and one graph of more k-mers than a whole grid of this device has threads."""
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
import unitig_color_cases as ucc

from ploidyfrost_amd import hipapi, hostapi

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
CASES = ucc.cases()
FLAG_FILES = {"none": (False, False), "id": (True, True)}
FLAG_ARGS = {(False, False): [], (True, True): ["-i", "-d"]}
TWELVE = uc.STATS + ucc.STATS
CUTOFFS = (2, 1000)


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)


def fixture(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    paths = [os.path.join(d, "s%d.fq" % s) for s in range(meta["samples"])]
    reads = []
    for p in paths:
        with open(p, "rb") as f:
            reads.append(f.read().split(b"\n")[1::4])
    return dict(dir=d, k=meta["k"], paths=paths, reads=reads)


def device_build(dev, tables, k, clip, dele, n_seeds, names):
    """the read-table entries, end to end: (gfa bytes, bfg_colors bytes, the twelve statistics, all of the device's)"""
    dev.count_begin(k, True)
    try:
        for t in tables:
            dev.count_reads(*t)
        km, _, _ = dev.count_finish(ci=1)
    except Exception:
        dev.count_abort()
        raise
    text, st = dev.unitig_build_colored(km, k, clip, dele, None, n_seeds)
    try:
        dev.color_begin(len(tables))
        for c, t in enumerate(tables):
            dev.color_reads(c, *t)
        col, got = dev.color_finish()
    finally:
        dev.unitig_release()
    assert col["lines"] == st["unitigs_out"] == len(got["heads"]) and col["overflow"] == st["overflow"] and col["runs"] == len(got["runs"])
    stats = {f: st[f] for f in uc.STATS}
    stats.update({f: col[f] for f in ucc.STATS})
    return text, hostapi.bfg_colors_bytes(got, k, names, n_seeds), stats, col


# ---- 1-5, 7: the kernels, through the read-table entries ----

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_case_equals_the_host_restatement(dev, case):
    name, k, reads, flags, n_seeds = case
    names = ["c%d" % c for c in range(len(reads))]
    want = hostapi.build_colored_host(reads, k, *flags, n_seeds=n_seeds, names=names)
    tables = [ucc.table(r) for r in reads]
    for again in range(2):   # a release that left something behind shows in the second build of the context
        gfa, col, st, _ = device_build(dev, tables, k, *flags, n_seeds, names)
        assert st == want[2], again
        assert gfa == want[0], again
        assert col == want[1], again
    if name == "tip":
        assert st["windows_unplaced"] > 0 and st["removed"] == 1
    if name == "overflow":
        assert st["overflow"] == want[2]["overflow"] > 0 and b"\tDA:Z:0\n" in gfa


def test_refusals(dev, tmp_path):
    name, k, reads, flags, n_seeds = next(c for c in CASES if c[0] == "colors2")
    km = np.array(sorted(uc.encode(x) for x in uc.kmer_set([r for rs in reads for r in rs], k)), dtype=np.uint64)
    L = dev.L

    def refused(call, word, code=hipapi.PF_ERR_ARG):
        st = call()
        assert st == code and word in L.pf_last_error(dev.h).decode(), (word, st, L.pf_last_error(dev.h))

    refused(lambda: L.pf_color_begin(dev.h, 2), "no coloured graph is held")
    refused(lambda: L.pf_color_finish(dev.h, None), "no colouring is open")
    for n_seeds_bad in (0, 256):
        with pytest.raises(RuntimeError, match="hash seeds goes from 1 to 255"):
            dev.unitig_build_colored(km, k, n_seeds=n_seeds_bad)
    text, st = dev.unitig_build(km, k)   # a plain build holds no colours
    assert b"DA:Z" not in text
    dev.unitig_build_colored(km, k)
    try:
        refused(lambda: L.pf_color_begin(dev.h, 0), "no colour")
        refused(lambda: L.pf_color_begin(dev.h, 1025), "more than 1024 colours")
        refused(lambda: L.pf_color_begin(dev.h, 1 << 31), "more than 1024 colours")
        assert L.pf_color_begin(dev.h, 2) == hipapi.PF_OK
        refused(lambda: L.pf_color_begin(dev.h, 2), "a colouring is open already")
        t = ucc.table(reads[0])
        with pytest.raises(RuntimeError, match="colour 2 of 2"):
            dev.color_reads(2, *t)
        refused(lambda: L.pf_color_fetch(dev.h, None, None, None, None, None), "the colouring is not finished")
        dev.color_reads(0, *t)
        col, got = dev.color_finish()
        assert col["runs"] == 1 and got["runs"].tolist() == [[0, 39]]
        with pytest.raises(RuntimeError, match="the colouring is finished"):
            dev.color_reads(1, *t)
    finally:
        dev.unitig_release()
    refused(lambda: L.pf_color_finish(dev.h, None), "no colouring is open")
    # ids are 32 bits: a unitig of 2^22 k-mers takes 1023 colours and no more (seed 3: no 24 bases of the sequence come twice)
    m = 1 << 22
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(3).integers(0, 4, size=m + 24, dtype=np.uint8)].tobytes()
    dev.count_begin(25, True)
    dev.count_reads(*ucc.table([seq]))
    km = dev.count_finish(ci=1)[0]
    text, st = dev.unitig_build_colored(km, 25)
    try:
        assert st["unitigs_out"] == 1 and st["longest"] == m + 24
        refused(lambda: L.pf_color_begin(dev.h, 1024), "colours times k-mers reach 2^32 (ids of a colour set are 32 bits): 1024 colours, %d k-mers" % m)
        assert L.pf_color_begin(dev.h, 1023) == hipapi.PF_OK   # (not finished: one row would walk 2^32 ids for this one unitig)
    finally:
        dev.unitig_release()


# ---- 9: more than one grid pass ----

def test_more_than_one_grid_pass(dev):
    """Every kernel of K-COLOR strides over its items with one grid of at most (compute units x 8) blocks of 256 threads (pf::ctx_grid):
    the index kernel over k-mers, the mark kernel over tiles of 1024 bytes, the run kernels over rows of 16 lanes, one a line; the
    placement kernels of the coloured build stride over lines.  A graph of more single-k-mer lines than one such pass has threads, each
    k-mer with the colours drawn from a seed, makes every one of them take the stride more than once; the reads of a colour are more
    tiles than a grid has blocks.  At a load of one line a slot the 31 rounds leave lines over, so the overflow slots are numbered
    across passes too.  The reference is unitig_color_cases.grid_expected (the rule over arrays, the host's writer), which the test
    without a GPU holds to the host's restatement at a small size."""
    per_pass = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    n = per_pass + per_pass // 8
    tables, keys, member = ucc.grid_case(n)
    assert len(keys) > per_pass and all(len(t[0]) // 1024 > per_pass // 256 for t in tables)
    names = ["c%d" % c for c in range(len(tables))]
    want = ucc.grid_expected(keys, member, 25, names, hostapi.bfg_colors_bytes)
    assert want[2]["unitigs_out"] == n and want[2]["runs"] > n and want[2]["overflow"] > 0
    gfa, col, st, dstats = device_build(dev, tables, 25, False, False, ucc.SEEDS, names)
    print("compute units x 8 x 256 = %d, lines %d, %s" % (per_pass, n, dstats))
    assert st == want[2]
    assert gfa == want[0]
    assert col == want[1]


# ---- 6: chunking, through the FASTQ entry and the sub-command ----

def test_chunks_of_the_fastq_entry_and_the_sub_command(dev, tmp_path):
    f = fixture("build_mc3_k25")
    names = [str(p) for p in f["paths"]]
    want = hostapi.build_colored_host(f["reads"], 25, True, True, names=names)
    assert all(os.path.getsize(p) > 3 * 4096 for p in f["paths"])
    outs = {}
    for tag, extra in (("one", []), ("chunk", ["--chunk-bytes", 4096]), ("both", ["--chunk-bytes", 4096, "--initial-slots", 64])):
        r = run_cli("build-multi", "-i", "-d", "-k", 25, *[x for p in names for x in ("-r", p)], "-o", tmp_path / tag, *extra, "-v")
        assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
        outs[tag] = ((tmp_path / (tag + ".gfa")).read_bytes(), (tmp_path / (tag + ".bfg_colors")).read_bytes(), r.stderr)
        assert all(w in r.stderr for w in ("stream", "graph", "color", "serialise", "write", "table", "mark", "runs"))
    assert outs["one"][:2] == outs["chunk"][:2] == outs["both"][:2] == want[:2]
    assert outs["one"][2].split("\n")[0] == outs["chunk"][2].split("\n")[0]
    assert sorted(os.listdir(tmp_path)) == sorted(t + e for t in outs for e in (".gfa", ".bfg_colors"))
    # the FASTQ entry itself, a file in pieces that end inside a record: what is not used comes again with the next piece
    km = np.array(sorted(uc.encode(x) for x in uc.kmer_set([r for rs in f["reads"] for r in rs], 25)), dtype=np.uint64)
    text, st = dev.unitig_build_colored(km, 25, True, True)
    try:
        dev.color_begin(3)
        reads_seen = 0
        for c, p in enumerate(f["paths"]):
            data = open(p, "rb").read()
            at = 0
            while at < len(data):
                piece = data[at:at + 5000]
                used, cst = dev.color_fastq(c, piece, final=at + 5000 >= len(data))
                assert used > 0
                at += used
                reads_seen += cst["reads"]
        col, got = dev.color_finish()
    finally:
        dev.unitig_release()
    assert reads_seen == sum(len(r) for r in f["reads"]) == col["reads"]
    assert text == want[0] and hostapi.bfg_colors_bytes(got, 25, names) == want[1]
    assert {s: col[s] for s in ucc.STATS} == {s: want[2][s] for s in ucc.STATS}


def test_input_without_a_kmer_and_refusals_leave_nothing(tmp_path):
    (tmp_path / "a.fq").write_bytes(uc.fastq(["ACGTACGT", "N" * 30]))
    (tmp_path / "b.fq").write_bytes(uc.fastq(["ACGT"]))
    r = run_cli("build-multi", "-k", 25, "-r", "a.fq", "-r", "b.fq", "-o", "s", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    want = hostapi.build_colored_host([["ACGTACGT", "N" * 30], ["ACGT"]], 25, names=["a.fq", "b.fq"])
    assert (tmp_path / "s.gfa").read_bytes() == want[0] == uc.header(25).encode() and (tmp_path / "s.bfg_colors").read_bytes() == want[1]
    assert "colors 2 reads 3 " in r.stderr and "unitigs_out 0 " in r.stderr and "runs 0 overflow 0 color_bytes %d\n" % len(want[1]) in r.stderr
    os.remove(tmp_path / "s.gfa")
    os.remove(tmp_path / "s.bfg_colors")
    f = fixture("build_mc2_k7")
    lines = open(f["paths"][1], "rb").read().rstrip(b"\n").split(b"\n")
    lines[4 * 3 + 3] = lines[4 * 3 + 3][:-1]
    (tmp_path / "bad.fq").write_bytes(b"\n".join(lines))
    r = run_cli("build-multi", "-k", 7, "-r", f["paths"][0], "-r", "bad.fq", "-o", "s", cwd=tmp_path)
    assert r.returncode != 0 and "build-multi: bad.fq: record 4: " in r.stderr and "quality line's length" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "bad.fq"]


# ---- 8: end to end ----

@pytest.mark.parametrize("name", ["build_mc3_k25", "build_mc2_k7"])
def test_fixtures_through_the_sub_command_and_the_calling_run(name, tmp_path):
    f = fixture(name)
    k = f["k"]
    dbs = []
    for s, reads in enumerate(f["reads"]):   # the sample databases from the host's counting restatement
        kmers, counts, _ = hostapi.count_reads_host(*ucc.table(reads), k, ci=1, cs=10000)
        pre, suf = hostapi.count_encode_kmc1(kmers, counts, k, ci=1, cs=10000)
        dbs.append(str(tmp_path / ("db%d" % s)))
        open(dbs[-1] + ".kmc_pre", "wb").write(pre)
        open(dbs[-1] + ".kmc_suf", "wb").write(suf)
    called = 0
    for tag, flags in FLAG_FILES.items():
        text, bits, st = ucc.build(f["reads"], k, *flags)
        out = tmp_path / tag
        r = run_cli("build-multi", "-k", k, *FLAG_ARGS[flags], *[x for p in f["paths"] for x in ("-r", p)], "-o", out, "-t", 16)
        assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
        gfa, col = str(out) + ".gfa", str(out) + ".bfg_colors"
        got_text = open(gfa, "rb").read()
        assert got_text == text
        counted = cc.ref_count([x for rs in f["reads"] for x in rs], k, ci=1, cs=10 ** 9)[2]
        assert r.stderr == ("build-multi: colors %d reads %d bases %d kmers %d bad %d distinct %d unitigs %d removed %d unitigs_out %d longest %d bytes %d "
                            "windows_colored %d windows_unplaced %d runs %d overflow %d color_bytes %d\n" % (
                                len(f["paths"]), counted["reads"], counted["bases"], counted["kmers"], counted["kmers_bad"], st["distinct"], st["unitigs"],
                                st["removed"], st["unitigs_out"], st["longest"], st["bytes"], st["windows_colored"], st["windows_unplaced"], st["runs"],
                                st["overflow"], os.path.getsize(col)))
        c = hostapi.Colors(gfa, col, 2)
        assert c.names == [str(p) for p in f["paths"]]
        for u, got in enumerate(ucc.colors_bits(c, got_text)):
            assert np.array_equal(got, bits[u]), (tag, u)
        with open(os.path.join(f["dir"], tag + ".gfa"), "rb") as ref:
            assert uc.same_graph(got_text, ref.read()), tag
        if k < 25:
            continue   # (the calling run asks for k = 25 databases)
        # the calling run on the built pair against the CPU oracle on the same graph, given a dump composed from the Python rule
        dump = tmp_path / (tag + ".dump.txt")
        dump.write_text(ucc.dump_text(uc.gfa_sequences(text)[1], bits, k, [str(p) for p in f["paths"]]))
        run = hostapi.ColoredRun(gfa, col, dbs, str(tmp_path))
        run.set_output_dir(str(tmp_path / (tag + "_gpu")))
        run.set_unitig_id("g")
        run.find_superbubbles("g")
        run.ploidy_estimation("g", [CUTOFFS] * len(dbs))
        run.close()
        pyoracle.ColoredOracle(gfa, str(dump), dbs, str(tmp_path)).run(str(tmp_path / (tag + "_cpu")), "g", [CUTOFFS] * len(dbs))
        names = sorted(os.listdir(tmp_path / (tag + "_cpu")))
        assert names and sorted(os.listdir(tmp_path / (tag + "_gpu"))) == names
        for n in names:
            assert (tmp_path / (tag + "_gpu") / n).read_bytes() == (tmp_path / (tag + "_cpu") / n).read_bytes(), (tag, n)
        called += (tmp_path / (tag + "_cpu") / "g_allele_frequency.txt").stat().st_size
    assert called > 0 or k < 25   # not vacuous: a site is called on the k = 25 fixture


def test_api_over_the_fixture(tmp_path):
    f = fixture("build_mc2_k7")
    want = hostapi.build_colored_host(f["reads"], 7, True, True, g=3, n_seeds=5, names=[str(p) for p in f["paths"]])
    got = hostapi.build_colored_graph(f["paths"], str(tmp_path / "api"), k=7, clip_tips=True, del_isolated=True, g=3, n_seeds=5, chunk_bytes=700)
    assert (tmp_path / "api.gfa").read_bytes() == want[0] and (tmp_path / "api.bfg_colors").read_bytes() == want[1]
    assert {s: got[s] for s in TWELVE} == want[2] and got["color_bytes"] == len(want[1]) and got["reads"] == sum(len(r) for r in f["reads"])
    assert set(got["times"]) == set(hostapi.COLOR_TIMES) and got["lines"] == want[2]["unitigs_out"]
