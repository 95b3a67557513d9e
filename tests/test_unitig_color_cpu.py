"""The rule of `ploidyfrost build-multi` (K-COLOR) without a GPU: the Python restatement of unitig_color_cases.py against what the
reference's Bifrost wrote and read back for the fixtures tests/golden/build_mc*, the host's plain restatement and writer
(pfh_build_colored_host: csrc/pf_color_rule.hpp, csrc/host/pf_bfg_write.hpp) against the Python rule through this build's own reader
(hostapi.Colors) and byte for byte, the real library's view of the written files where it has been built, the stand-alone program
tests/cpp/test_bfg_write.cpp under the sanitizers, the sub-command's refusals that need no device, and the declarations."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import unitig_cases as uc
import unitig_color_cases as ucc

from ploidyfrost_amd import build, hipapi, hostapi

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
CASES = ucc.cases()
FLAG_FILES = {"none": (False, False), "id": (True, True)}
FIXTURES = ["build_mc3_k25", "build_mc2_k7"]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=120)


def fixture(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    paths = [os.path.join(d, "s%d.fq" % s) for s in range(meta["samples"])]
    reads = []
    for p in paths:
        with open(p, "rb") as f:
            reads.append(f.read().split(b"\n")[1::4])
    return dict(dir=d, k=meta["k"], paths=paths, reads=reads, names=["s%d.fq" % s for s in range(meta["samples"])])


def written(tmp_path, gfa, colors, tag="w"):
    g, c = tmp_path / (tag + ".gfa"), tmp_path / (tag + ".bfg_colors")
    g.write_bytes(gfa)
    c.write_bytes(colors)
    return str(g), str(c)


# ---- 1. the Python rule against Bifrost ----

@pytest.mark.parametrize("name", FIXTURES)
def test_python_rule_equals_bifrost_on_the_fixtures(name):
    f = fixture(name)
    for tag, flags in FLAG_FILES.items():
        text, bits, st = ucc.build(f["reads"], f["k"], *flags)
        with open(os.path.join(f["dir"], tag + ".gfa"), "rb") as fh:
            ref_gfa = fh.read()
        with open(os.path.join(f["dir"], tag + ".colors.txt")) as fh:
            ref_dump = fh.read()
        assert uc.same_graph(text, ref_gfa), tag
        names, ref = ucc.dump_by_sequence(ref_gfa, ref_dump, f["k"])
        assert names == f["names"]
        mine = ucc.by_sequence(uc.gfa_sequences(text)[1], bits)
        assert sorted(mine) == sorted(ref), tag
        for s in mine:
            assert np.array_equal(mine[s], ref[s]), (tag, s)
        assert all(ln.split("\t")[3].startswith("DA:Z:") for ln in ref_gfa.decode().split("\n") if ln.startswith("S"))   # as this build's lines end
        # not vacuous: some unitig carries a colour on part of its k-mers, some colour is missing from some unitig
        assert any(0 < b[c].sum() < b.shape[1] for b in bits for c in range(b.shape[0])) and any(not b[c].any() for b in bits for c in range(b.shape[0]))
        if flags == (True, True):
            assert st["removed"] > 0 and st["windows_unplaced"] > 0
        for n in os.listdir(f["dir"]):
            assert os.path.getsize(os.path.join(f["dir"], n)) < 300 * 1024


# ---- 2. the host restatement against the rule ----

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_restatement_on_every_case(case, tmp_path):
    name, k, reads, flags, n_seeds = case
    text, bits, st, colors, names = ucc.expected(name)
    gfa, col, hst = hostapi.build_colored_host(reads, k, *flags, n_seeds=n_seeds)
    assert gfa == text and hst == st
    assert col == colors                                   # byte for byte what bfg_colors.py's layout and encodings give
    c = hostapi.Colors(*written(tmp_path, gfa, col), 2)    # and what this build's reader makes of them
    assert c.n_colors == len(reads) and c.names == names and c.n == len(bits)
    for u, got in enumerate(ucc.colors_bits(c, gfa)):
        assert np.array_equal(got, bits[u]), u


def test_cases_cover_what_they_are_for():
    form = {}
    for name, k, reads, flags, n_seeds in CASES:
        text, bits, st, colors, names = ucc.expected(name)
        ids = [np.nonzero(b.ravel())[0] for b in bits]
        form[name] = (st, ids)
    assert [int(form[n][1][0][-1]) for n in ("top60", "top61", "top62")] == [59, 60, 61]
    st, ids = form["cross16"]
    assert ids[0][0] < 1 << 16 <= ids[0][-1] and bits_total(ids) > 0
    st, ids = form["five_containers"]
    assert st["runs"] == 1 and len(ids[0]) == 300000
    st, ids = form["alt2500"]
    assert st["runs"] == 2500 and ids[0][-1] < 1 << 16
    assert form["two_full"][0]["runs"] == 1 and len(form["two_full"][1][0]) == 200
    assert form["tip"][0]["windows_unplaced"] == 10 and form["tip"][0]["removed"] == 1 and form["tip_kept"][0]["windows_unplaced"] == 0
    assert form["overflow"][0]["overflow"] > 0 and b"\tDA:Z:0\n" in ucc.expected("overflow")[0]
    for n in (2, 64, 65):   # the colour without a k-mer has a name and no bit
        _, bits, _, _, _ = ucc.expected("colors%d" % n)
        assert not bits[0][n - 2 if n > 2 else n - 1].any() and bits[0][0].all()
    st = form["tile_edges"][0]
    assert st["windows_bad"] > 0 and st["longest"] == 1024 + 2 * 25


def bits_total(ids):
    return sum(len(i) for i in ids)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_restatement_on_the_fixtures(name, tmp_path):
    f = fixture(name)
    for tag, flags in FLAG_FILES.items():
        text, bits, st = ucc.build(f["reads"], f["k"], *flags)
        gfa, col, hst = hostapi.build_colored_host(f["reads"], f["k"], *flags, names=f["names"])
        assert gfa == text and hst == st
        assert col == ucc.colors_file(uc.gfa_sequences(text)[1], bits, f["k"], f["names"])
        c = hostapi.Colors(*written(tmp_path, gfa, col, tag), 2)
        assert c.names == f["names"]
        for u, got in enumerate(ucc.colors_bits(c, gfa)):
            assert np.array_equal(got, bits[u]), (tag, u)


def test_host_restatement_on_a_small_graph_made_for_a_size():
    """the make of the GPU suite's graph of more than one grid pass, small: unitig_color_cases.grid_expected (the rule over arrays, the
    host's writer) is the host's restatement on the same reads, byte for byte, and the Python rule's bits"""
    tables, keys, member = ucc.grid_case(3000)
    names = ["c0", "c1", "c2"]
    reads = [[t[0][i:i + 25] for i in range(0, len(t[0]), 25)] for t in tables]
    assert all(ucc.table(r)[0] == t[0] and np.array_equal(ucc.table(r)[1], t[1]) and np.array_equal(ucc.table(r)[2], t[2]) for r, t in zip(reads, tables))
    for n_seeds in (ucc.SEEDS, 2):
        want = hostapi.build_colored_host(reads, 25, n_seeds=n_seeds, names=names)
        got = ucc.grid_expected(keys, member, 25, names, hostapi.bfg_colors_bytes, n_seeds)
        assert got[0] == want[0] and got[2] == want[2] and got[1] == want[1], n_seeds
        assert want[2]["overflow"] > 0 and want[2]["runs"] > 3000
    text, bits, st = ucc.build(reads, 25, n_seeds=2)
    assert text == want[0] and st == want[2]
    assert [b[:, 0].astype(bool).tolist() for b in bits] == member.T.tolist()


def test_host_restatement_refusals():
    for kw, word in ((dict(k=2), "k goes from 3 to 31"), (dict(k=7, g=6), "g goes from 1 to k - 2"), (dict(k=7, n_seeds=256), "n_seeds goes from 1 to 255")):
        with pytest.raises(ValueError, match=word):
            hostapi.build_colored_host([["ACGTACGTAC"]], **kw)
    with pytest.raises(ValueError, match="more than 1024 colours"):
        hostapi.build_colored_host([["ACGTACGTAC"]] * 1025, 7)
    assert hostapi.color_no_room_text(1000, 10, 3, 7) == (
        "the colour planes and the table (1000 bytes) do not fit in the free device memory (10 bytes) at 3 colours and 7 k-mers of the graph")
    gfa, col, st = hostapi.build_colored_host([["ACGT"], []], 7)   # no k-mer anywhere: two names, no set
    assert gfa == uc.header(7).encode() and st["unitigs_out"] == 0 and st["runs"] == 0 and b"c0\nc1\n" in col


# ---- 3. the real library's view ----

@pytest.mark.parametrize("name", ["top62", "cross16", "five_containers", "alt2500", "colors65", "tip", "overflow"])
def test_real_bifrost_reads_the_written_files_the_same_way(name, tmp_path):
    if not os.path.exists(pyoracle.REF_COLORS_DUMP):
        pytest.skip("reference Bifrost (oracle/_ref/colors_dump) not built here")
    _, k, reads, flags, n_seeds = next(c for c in CASES if c[0] == name)
    text, bits, st, colors, names = ucc.expected(name)
    gfa, col, _ = hostapi.build_colored_host(reads, k, *flags, n_seeds=n_seeds)
    g, c = written(tmp_path, gfa, col)
    r = subprocess.run([pyoracle.REF_COLORS_DUMP, g, c], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got_names, got = ucc.dump_by_sequence(gfa, r.stdout, k)
    assert got_names == names
    want = ucc.by_sequence(uc.gfa_sequences(text)[1], bits)
    assert sorted(got) == sorted(want)
    for s in want:
        assert np.array_equal(got[s], want[s]), s
    assert all(row[3] == 0 for row in ucc.read_dump(r.stdout)[1])   # n_full_enc


# ---- 4. the stand-alone program ----

def test_standalone_writer_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_bfg_write.cpp: the rule and writer headers alone, plain g++ with -fsanitize=address,undefined (host code only:
    nothing of it is loaded into Python or run on a GPU)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "test_bfg_write")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_bfg_write.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- 5. the sub-command's refusals that need no device ----

def test_cli_refusals(tmp_path):
    fq, fq2 = tmp_path / "a.fq", tmp_path / "b.fq"
    fq.write_bytes(uc.fastq(["ACGTTGCATGCATGGGATCCATGCAATGCCGTA"]))
    fq2.write_bytes(uc.fastq(["TTGCATGCATGGGATCCATGCAATGCCGTAAC"]))
    fa, gz = tmp_path / "in.fa", tmp_path / "in.fq.gz"
    fa.write_bytes(b">s\nACGT\n")
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    os.link(fq, tmp_path / "same.bfg_colors")   # an output name is an input file
    os.link(fq2, tmp_path / "b_again.fq")       # the same file under another name
    listing = sorted(os.listdir(tmp_path))
    base = ["build-multi", "-r", fq, "-r", fq2, "-o", tmp_path / "s"]
    cases = [(base + [opt], "%s is not built" % opt) for opt in ("-s", "-y", "-f", "-a", "-m", "-n", "-b", "-B", "-l", "-w", "-e")]
    cases += [
        (base + ["-k", "2"], "-k goes from 3 to 31"),
        (base + ["-k", "32"], "-k goes from 3 to 31"),
        (base + ["-k", "25", "-g", "24"], "-g goes from 1 to k - 2 = 23"),
        (base + ["-g", "x"], "-g takes a positive number, not 'x'"),
        (["build-multi", "-o", tmp_path / "s"], "-r <reads.fq> is missing"),
        (["build-multi", "-r", fq], "-o <sample> is missing"),
        (["build-multi", "-r", fq, "-r", fq2, "-o", tmp_path / "same"], "%s: the output path is an input path" % fq),
        (["build-multi", "-r", fq, "-r", fa, "-o", tmp_path / "s"], "%s: record 1: the input is FASTA (first byte '>'): only FASTQ is read" % fa),
        (["build-multi", "-r", gz, "-o", tmp_path / "s"], "%s: record 1: the input is gzip-compressed (magic 1f 8b): only plain FASTQ is read" % gz),
        (["build-multi", "-r", fq, "-r", tmp_path / "none.fq", "-o", tmp_path / "s"], "cannot read %s" % (tmp_path / "none.fq")),
        (base + ["-r", fq], "%s: the same file is given twice (-r 1 and -r 3): a colour is a file" % fq),
        (base + ["-r", tmp_path / "b_again.fq"], "%s: the same file is given twice (-r 2 and -r 3): a colour is a file" % (tmp_path / "b_again.fq")),
        (["build-multi", "-o", tmp_path / "s"] + [x for i in range(1025) for x in ("-r", "f%d.fq" % i)], "more than 1024 colours (-r files): 1025"),
        (base + ["--gpus", "2"], "--gpus is not built: the graph is made on one GPU"),
        (base + ["--frobnicate"], "unknown option --frobnicate"),
        (base + ["--chunk-bytes"], "--chunk-bytes needs a value"),
    ]
    for args, word in cases:
        r = run_cli(*args, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stderr and r.stderr.startswith("Error: build-multi: ") and r.stdout == "", (args[:8], r.stderr)
        assert sorted(os.listdir(tmp_path)) == listing, args[:8]   # no output, no temporary file
    usage = run_cli().stdout
    assert "build-multi -k 25 [-i] [-d] -r <s0.fq> -r <s1.fq>" in usage
    # `build -c` stays refused as it was, with a pointer behind it
    r = run_cli("build", "-r", fq, "-o", tmp_path / "s", "-c", cwd=tmp_path)
    assert r.returncode != 0 and r.stderr.startswith("Error: build: -c is not built (a single-sample graph") and "`build-multi`" in r.stderr
    for kw, word in ((dict(k=2), "-k goes from 3 to 31"), (dict(n_seeds=256), "hash seeds goes from 1 to 255")):
        with pytest.raises(RuntimeError, match=word):
            hostapi.build_colored_graph([str(fq), str(fq2)], str(tmp_path / "s"), **kw)
    with pytest.raises(RuntimeError, match="the same file is given twice"):
        hostapi.build_colored_graph([str(fq), str(fq)], str(tmp_path / "s"))
    assert sorted(os.listdir(tmp_path)) == listing


# ---- names ----

def test_entry_points_are_declared():
    for s in ("pf_unitig_build_colored", "pf_color_begin", "pf_color_reads", "pf_color_fastq", "pf_color_finish", "pf_color_fetch"):
        assert s in hipapi.DECLARED_SYMBOLS and hasattr(hipapi.load_library(), s)
    for s in ("pfh_build_colored_fastq", "pfh_build_colored_host", "pfh_bfg_colors_bytes", "pfh_color_no_room_text"):
        assert s in hostapi.DECLARED_SYMBOLS and hasattr(hostapi.load_library(), s)
    assert hipapi.COLOR_STATS == hostapi.COLOR_STATS and hipapi.COLOR_STATS.itemsize == 13 * 8
    assert hostapi.COLOR_STATS_FIELDS == ucc.STATS and hipapi.COLOR_SEEDS == hostapi.COLOR_SEEDS == ucc.SEEDS == 31
    L = hostapi.load_library()   # the hash the device places with is the one this build's reader looks sets up with
    from ploidyfrost_amd import bfg_colors
    assert L.pfh_bifrost_kmer_hash(0x0123456789ABCDEF, ucc.seed_of(3)) == bfg_colors.kmer_hash(0x0123456789ABCDEF, ucc.seed_of(3))
