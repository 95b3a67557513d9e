"""K-UNION (pf_kmer_union, csrc/pf_union.hip) against np.unique over the concatenation, K-COLORSET (pf_color_kmers, csrc/pf_color.hip)
against K-COLOR over the same reads, and `ploidyfrost run-multi` against the chain of C + 2 commands it replaces (the rule:
csrc/pf_runmulti_rule.hpp).  Every comparison is exact: arrays of integers and bytes of files."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first, as everywhere: it binds the HIP runtime the libraries share)

from conftest import GOLDEN, ROOT

import mask_cases as mc
import run_cases as rc

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
T = hipapi.UNION_TILE      # merged positions a block takes
ITEMS = hipapi.UNION_ITEMS   # ... and a lane
U64 = np.uint64


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


# ---- K-UNION ----

def arr(x):
    return np.ascontiguousarray(np.asarray(x, dtype=U64))


def distinct(rng, n, hi=1 << 50):
    """n sorted distinct keys below hi"""
    pool = np.unique(rng.integers(0, hi, size=2 * n + 8, dtype=np.uint64))
    return arr(np.sort(rng.choice(pool, size=n, replace=False)))


def pair_at(pos, after=300):
    """A and B whose one common key stands at merged positions pos - 1 (A's) and pos (B's): pos - 1 smaller keys, split between both"""
    small = np.arange(pos - 1, dtype=U64) * U64(2)
    x = U64(2 * pos + 10)
    tail = x + U64(1) + np.arange(after, dtype=U64) * U64(3)
    a = np.concatenate([small[0::2], [x], tail[0::2]])
    b = np.concatenate([small[1::2], [x], tail[1::2]])
    return [arr(a), arr(b)]


def union_cases():
    rng = np.random.default_rng(20261019)
    full = distinct(rng, 3 * T + 5)
    even, odd = arr(np.arange(0, 2 * T + 6, 2)), arr(np.arange(1, 2 * T + 7, 2))
    low, high = arr(np.arange(10, 10 + T + 3)), arr(np.arange(1 << 20, (1 << 20) + 2 * T + 1))
    cases = [("one_set", [full]), ("one_empty_set", [arr([])]), ("two_empty", [arr([]), arr([])]), ("empty_beside_full", [arr([]), full]),
             ("full_beside_empty", [full, arr([])]), ("equal", [full, full.copy()]), ("interleaved", [even, odd]), ("a_below_b", [low, high]),
             ("b_below_a", [high, low]), ("pair_on_tile_edge", pair_at(T)), ("pair_on_second_tile_edge", pair_at(2 * T)),
             ("pair_on_lane_edge", pair_at(ITEMS * 5)), ("pair_on_lane_edge_of_the_second_tile", pair_at(T + ITEMS * 7))]
    for na in (T - 1, T, T + 1, 2 * T + 1):
        for nb in (T - 1, T, T + 1, 2 * T + 1):
            pool = distinct(rng, (na + nb) * 3 // 4 + 2)   # a quarter of the keys lie in both
            cases.append(("sizes_%d_%d" % (na, nb), [arr(np.sort(rng.choice(pool, size=min(na, len(pool)), replace=False))),
                                                     arr(np.sort(rng.choice(pool, size=min(nb, len(pool)), replace=False)))]))
    for c in (3, 5, 8):   # the odd carry, three rounds; key 777 lies in every set
        sets = []
        for j in range(c):
            own = distinct(rng, 700 + 97 * j, hi=1 << 30)
            sets.append(arr(np.unique(np.concatenate([own, [U64(777)]]))))
        cases.append(("in_all_of_%d" % c, sets))
    hi_bit = U64(1) << U64(61)   # as at k = 31
    cases.append(("bit_61", [arr(np.unique(np.concatenate([distinct(rng, T + 9), distinct(rng, 40) | hi_bit]))),
                             arr(np.unique(distinct(rng, 2 * T) | hi_bit)), arr([hi_bit, hi_bit | U64(5)])]))
    return cases


UNION_CASES = union_cases()


@pytest.mark.parametrize("case", UNION_CASES, ids=[c[0] for c in UNION_CASES])
def test_union_equals_unique_of_the_concatenation(dev, case):
    name, sets = case
    for s in sets:
        assert len(s) < 2 or bool(np.all(s[1:] > s[:-1])), name   # the case itself is sorted and distinct
    want = np.unique(np.concatenate(sets)) if sets else arr([])
    got = dev.kmer_union(sets)
    assert got.dtype == U64 and np.array_equal(got, want), (name, len(got), len(want))
    assert np.array_equal(dev.kmer_union(sets), got)            # the same array on every call
    assert np.array_equal(hostapi.union_host(sets), want)       # ... and from the host restatement
    if name.startswith("pair_on"):
        assert len(want) == len(sets[0]) + len(sets[1]) - 1


def test_union_takes_device_tensors_and_leaves_them_alone(dev):
    rng = np.random.default_rng(5)
    sets = [distinct(rng, T + 17), distinct(rng, 3 * T)]
    tens = [torch.from_numpy(s.view(np.int64).copy()).to("cuda") for s in sets]
    got = dev.kmer_union(tens)
    assert np.array_equal(got, np.unique(np.concatenate(sets)))
    for t, s in zip(tens, sets):
        assert np.array_equal(t.cpu().numpy().view(U64), s)


def test_union_refusals(dev):
    good = arr([1, 5, 9])
    with pytest.raises(hipapi.DeviceError) as e:
        dev.kmer_union([good, arr([4, 3, 8])])
    assert "pf_kmer_union" in str(e.value) and "set 1 is not sorted" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.kmer_union([arr([2, 2, 7]), good])
    assert "pf_kmer_union" in str(e.value) and "set 0 holds a key twice" in str(e.value)
    big = np.arange(3 * T, dtype=U64)
    big[2 * T + 1] = big[2 * T]          # a repeat far from the front, in a later block of the check
    with pytest.raises(hipapi.DeviceError) as e:
        dev.kmer_union([good, good, arr(big)])
    assert "set 2 holds a key twice" in str(e.value)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.kmer_union([])
    assert "pf_kmer_union: no set" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        hostapi.union_host([good, arr([4, 3, 8])])
    assert "set 1 is not sorted" in str(e.value)
    assert np.array_equal(dev.kmer_union([good, arr([5, 6])]), arr([1, 5, 6, 9]))   # the context is as good as before


# ---- K-COLORSET against K-COLOR ----

def fixture(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    return dict(k=meta["k"], data=[open(os.path.join(d, "s%d.fq" % s), "rb").read() for s in range(meta["samples"])])


def kmers_of(dev, k, files):
    """the sorted distinct canonical k-mers of whole FASTQ files (ci = 1)"""
    dev.count_begin(k, True)
    try:
        for data in files:
            used, _ = dev.count_fastq(data, final=True)
            assert used == len(data)
        km, _, _ = dev.count_finish(**rc.EVERY)
    except Exception:
        dev.count_abort()
        raise
    return km


def colour(dev, k, f, flags, route):
    """the coloured graph of all files, coloured by `route`; (what pf_color_fetch returns, statistics, the route's own numbers)"""
    km = kmers_of(dev, k, f["data"])
    _, st = dev.unitig_build_colored(km, k, *flags)
    try:
        dev.color_begin(len(f["data"]))
        own = route(dev)
        col, got = dev.color_finish()
    finally:
        dev.unitig_release()
    return got, col, st, own


def same_fetch(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("heads", "m", "slot", "run_off", "runs"))


@pytest.fixture(scope="module")
def per_file_kmers(dev):
    """route B's keys, counted once: fixture -> one array per file"""
    out = {}
    for name in ("build_mc3_k25", "build_mc2_k7"):
        f = fixture(name)
        out[name] = (f, [kmers_of(dev, f["k"], [data]) for data in f["data"]])
    return out


@pytest.mark.parametrize("flags", [(False, False), (True, True)], ids=["none", "id"])
@pytest.mark.parametrize("name", ["build_mc3_k25", "build_mc2_k7"])
def test_colour_from_keys_equals_colour_from_reads(dev, per_file_kmers, name, flags):
    f, keys = per_file_kmers[name]

    def from_reads(d):
        for c, data in enumerate(f["data"]):
            used, _ = d.color_fastq(c, data, final=True)
            assert used == len(data)

    def from_keys(d):
        return [d.color_kmers(c, keys[c]) for c in range(len(keys))]

    def from_keys_twice(d):   # the same set given again: the same planes
        from_keys(d)
        return from_keys(d)

    a, col_a, st_a, _ = colour(dev, f["k"], f, flags, from_reads)
    b, col_b, st_b, own = colour(dev, f["k"], f, flags, from_keys)
    c, _, _, own2 = colour(dev, f["k"], f, flags, from_keys_twice)
    assert same_fetch(a, b) and same_fetch(a, c)
    assert col_a["runs"] == col_b["runs"] and col_a["lines"] == col_b["lines"] and col_a["overflow"] == col_b["overflow"]
    live = int(a["m"].sum())
    unplaced = sum(s["kmers_unplaced"] for s in own)
    print("%s %s: %d lines, %d live k-mers (%% 32 = %d), %d runs, keys %s, unplaced %d" %
          (name, flags, len(a["m"]), live, live % 32, col_a["runs"], [len(x) for x in keys], unplaced))
    for s, x in zip(own, keys):
        assert s["kmers"] == len(x) == s["kmers_colored"] + s["kmers_unplaced"]
    assert own == own2
    assert col_a["runs"] > 0 and live > 0
    if flags == (False, False):
        assert unplaced == 0 and st_a["removed"] == 0          # nothing removed: every key of every file is a vertex
    else:
        assert (unplaced > 0) == (st_a["removed"] > 0)          # a key -i / -d removed colours nothing
    if name == "build_mc3_k25":
        assert live % 32 != 0                                   # the last colour's plane ends inside a word
        if flags == (True, True):
            assert unplaced > 0


def test_colour_from_keys_edges_and_refusals(dev, per_file_kmers):
    f, keys = per_file_kmers["build_mc2_k7"]
    k, n_col = f["k"], len(keys)
    km = kmers_of(dev, k, f["data"])
    absent = next(x for x in range(4 ** k) if x not in set(km.tolist()))
    with pytest.raises(hipapi.DeviceError) as e:
        dev.color_kmers(0, keys[0])
    assert "pf_color_kmers: no colouring is open" in str(e.value)
    dev.unitig_build_colored(km, k, False, False)
    try:
        dev.color_begin(n_col)
        assert dev.color_kmers(0, arr([])) == dict(kmers=0, kmers_colored=0, kmers_unplaced=0)          # n = 0
        assert dev.color_kmers(1, arr([absent])) == dict(kmers=1, kmers_colored=0, kmers_unplaced=1)     # a key the graph does not hold
        assert dev.color_kmers(1, arr([0xFFFFFFFFFFFFFFFF])) == dict(kmers=1, kmers_colored=0, kmers_unplaced=1)
        with pytest.raises(hipapi.DeviceError) as e:
            dev.color_kmers(n_col, keys[0])
        assert "pf_color_kmers: colour %d of %d" % (n_col, n_col) in str(e.value)
        # mixed with the reads' route: colour 0 from its reads, the last colour from its keys
        used, _ = dev.color_fastq(0, f["data"][0], final=True)
        assert used == len(f["data"][0])
        for c in range(1, n_col):
            st = dev.color_kmers(c, keys[c])
            assert st["kmers_colored"] == len(keys[c])
        _, mixed = dev.color_finish()
        with pytest.raises(hipapi.DeviceError) as e:
            dev.color_kmers(0, keys[0])
        assert "the colouring is finished" in str(e.value)
    finally:
        dev.unitig_release()

    def from_reads(d):
        for c, data in enumerate(f["data"]):
            d.color_fastq(c, data, final=True)

    want, _, _, _ = colour(dev, k, f, (False, False), from_reads)
    assert same_fetch(mixed, want)


def test_each_kernel_is_timed_under_its_own_name(dev, per_file_kmers):
    f, keys = per_file_kmers["build_mc2_k7"]
    km = kmers_of(dev, f["k"], f["data"])
    dev.enable_timing(True)
    try:
        dev.reset_timing()
        got = dev.kmer_union(keys)
        assert np.array_equal(got, km)      # the union of the files' k-mers is the k-mers of the files together
        ms, launches = dev.kernel_time(hipapi.K_UNION)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_UNION) == sum(len(x) for x in keys)
        assert dev.kernel_time(hipapi.K_COLORSET)[1] == 0
        dev.unitig_build_colored(km, f["k"], False, False)
        try:
            dev.color_begin(len(keys))
            dev.color_kmers(0, keys[0])
            dev.color_finish()
        finally:
            dev.unitig_release()
        ms, launches = dev.kernel_time(hipapi.K_COLORSET)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_COLORSET) == len(keys[0])
        assert dev.kernel_time(hipapi.K_UNION)[1] == 1
        assert dev.L.pf_kernel_name(hipapi.K_UNION) == b"k_union" and dev.L.pf_kernel_name(hipapi.K_COLORSET) == b"k_colorset"
    finally:
        dev.enable_timing(False)


# ---- `ploidyfrost run-multi` against the chain it replaces ----

NAMES = ["alpha", "beta", "gamma"]
MODEL = ["--model", "fre", "--filter-multi", "-v 0.25 -n 6"]
DEPTH = 48   # per sample; see chain()


def cli(*a, cwd):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def write_samples(root):
    """the generator of tests/golden/make_build_multi_golden.py (the build_mc3_k25 case) at DEPTH; sample 0 split over two files.
    Returns per sample its list of files."""
    spec = importlib.util.spec_from_file_location("make_build_multi_golden", os.path.join(GOLDEN, "make_build_multi_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    s = dict(gen.CASES["build_mc3_k25"], depth=DEPTH)
    files = []
    for c, reads in enumerate(gen.make_samples(**s)):
        parts = [reads[: len(reads) // 3], reads[len(reads) // 3:]] if c == 0 else [reads]
        mine = []
        for j, part in enumerate(parts):
            p = root / ("s%d_%d.fq" % (c, j))
            with open(p, "w") as f:
                for i, r in enumerate(part):
                    f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
            mine.append(p)
        files.append(mine)
    return files


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The C + 2 commands of the parent commit, with `build-multi -i -d` and without, run with cwd in the masked files' directory so
    that the colour names are the bare NAMEs.  Chosen numbers: the build_mc3_k25 generator (3 samples, genome 800, reads of 100) at
    depth 48 per sample, sample 0 cut into two files after a third of its reads.  Measured with the parent commit's commands: L = 10 for
    every sample and 28 rows of allele_frequency.txt, with -i -d and without (the first depth tried; the fixture's own depth of 16
    leaves every heterozygous k-mer below L).  The test prints the row count and asks for at least 5."""
    root = tmp_path_factory.mktemp("multichain")
    files = write_samples(root)
    out = {"files": files, "L": []}
    for tag, flags in (("id", ["-i", "-d"]), ("none", [])):
        d = root / tag
        d.mkdir()
        for c, name in enumerate(NAMES):
            if tag == "id":
                m = cli("mask", "-k", 25, "-ci", 1, "-cs", 10000, *[x for p in files[c] for x in ("-i", p)], "-o", d / name, "--auto-cutoffs",
                        "--db-out", d / ("db%d" % c), cwd=d)
                out["L"].append(m.stdout)
            else:
                for src in (name, "db%d.kmc_pre" % c, "db%d.kmc_suf" % c):
                    (d / src).write_bytes((root / "id" / src).read_bytes())
        cli("build-multi", *flags, "-k", 25, *[x for n in NAMES for x in ("-r", n)], "-o", "s", cwd=d)
        (d / "dbs.txt").write_text("".join("%s\n" % (d / ("db%d" % c)) for c in range(len(NAMES))))
        cli("-g", "s.gfa", "-f", "s.bfg_colors", "-d", "dbs.txt", "--auto-cutoffs", "-o", "s", *MODEL, cwd=d)
        out[tag] = d
    return out


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def sample_args(files):
    return [x for c, name in enumerate(NAMES) for x in (["--sample", name] + [y for p in files[c] for y in ("-i", p)])]


@pytest.mark.parametrize("name,tag,extra", [("default", "id", []), ("chunk_carries", "id", ["--chunk-bytes", 4096]),
                                            ("keep", "none", ["--keep-tips", "--keep-isolated"])])
def test_run_multi_against_the_chain(chain, tmp_path, name, tag, extra):
    want = calling_files(chain[tag], "s")
    rows = want["_allele_frequency.txt"].decode().splitlines()
    print("chain %s: L = %s, %d calling files, %d lines in allele_frequency.txt" % (tag, [x.strip() for x in chain["L"]], len(want), len(rows)))
    assert len(rows) >= 5, rows[:3]          # (the file has no header line) the comparison is not vacuous
    assert len([f for f in want if f != "_model_result.txt"]) == 12 and "_model_result.txt" in want
    r = cli("run-multi", *sample_args(chain["files"]), "-o", "r", *MODEL, "--db-out", tmp_path / "d", "--gfa-out", tmp_path / "g", *extra, cwd=tmp_path)
    got = calling_files(tmp_path, "r")
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    for c in range(len(NAMES)):
        for suf in (".kmc_pre", ".kmc_suf"):
            assert open(str(tmp_path / ("d%d" % c)) + suf, "rb").read() == open(str(chain[tag] / ("db%d" % c)) + suf, "rb").read(), (c, suf)
    assert open(tmp_path / "g.gfa", "rb").read() == open(chain[tag] / "s.gfa", "rb").read()
    assert open(tmp_path / "g.bfg_colors", "rb").read() == open(chain[tag] / "s.bfg_colors", "rb").read()
    assert r.stdout.splitlines()[:len(NAMES)] == [x.strip() for x in chain["L"]] and all(int(x) >= 10 for x in chain["L"])
    assert sorted(os.listdir(tmp_path)) == sorted(["PloidyFrost_output", "g.gfa", "g.bfg_colors"] +
                                                  ["d%d%s" % (c, s) for c in range(len(NAMES)) for s in (".kmc_pre", ".kmc_suf")])   # no temporary file
    line = [l for l in r.stderr.splitlines() if l.startswith("run-multi: colors ")]
    per = [l for l in r.stderr.splitlines() if l.startswith("run-multi: color ")]
    assert len(line) == 1 and len(per) == len(NAMES)
    for c, l in enumerate(per):
        assert l.startswith("run-multi: color %d lower %d upper " % (c, int(chain["L"][c])))


def test_run_multi_each_color_against_the_chain(chain, tmp_path):
    d = chain["id"]
    cli("-g", "s.gfa", "-f", "s.bfg_colors", "-d", "dbs.txt", "--auto-cutoffs", "-o", "e", *MODEL, "--model-each-color", cwd=d)
    want = calling_files(d, "e")
    each = sorted(f for f in want if f.startswith("_color") and f.endswith("_model_result.txt"))
    print("per-colour results of the chain:", each)
    assert each, sorted(want)
    cli("run-multi", *sample_args(chain["files"]), "-o", "r", *MODEL, "--model-each-color", cwd=tmp_path)
    got = calling_files(tmp_path, "r")
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    assert os.listdir(tmp_path) == ["PloidyFrost_output"]


def test_run_multi_reads_returns_the_numbers_of_the_stderr_lines(chain, tmp_path):
    r = cli("run-multi", *sample_args(chain["files"]), "-o", "r", cwd=tmp_path)
    lines = r.stderr.splitlines()
    words = [l for l in lines if l.startswith("run-multi: colors ")][0].split()[1:]
    want = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    want["color"] = []
    for l in (l for l in lines if l.startswith("run-multi: color ")):
        w = l.split()[3:]
        want["color"].append({w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
    cwd = os.getcwd()
    os.makedirs(tmp_path / "api")
    os.chdir(tmp_path / "api")
    try:
        got = hostapi.run_multi_reads([(n, [str(p) for p in fs]) for n, fs in zip(NAMES, chain["files"])], "r")
    finally:
        os.chdir(cwd)
    assert got == want and tuple(got) == hostapi.RUN_MULTI_STATS_FIELDS + ("color",)
    assert all(tuple(c) == hostapi.RUN_MULTI_COLOR_FIELDS for c in got["color"])
    assert calling_files(tmp_path / "api", "r") == calling_files(tmp_path, "r")
    assert got["colors"] == 3 and got["windows_kept"] > 0 and got["unitigs_out"] > 0 and got["kmers_colored"] > 0 and got["color_bytes"] > 0
    assert got["kmers_colored"] + got["kmers_unplaced"] == sum(c["kept"] for c in got["color"])
    assert got["distinct_kept"] <= sum(c["kept"] for c in got["color"])


def test_no_surviving_kmer_ends_with_the_coloured_calling_runs_message(tmp_path):
    """every k-mer occurs once or twice, L = 10: the masking leaves nothing in any sample.  `run-multi` says on stdout what the coloured
    calling run says about a graph that could not be loaded, leaves with its exit status and leaves nothing under an output name."""
    rng = np.random.default_rng(4)
    for n in ("a", "b"):
        reads = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=60)) for _ in range(40)]
        (tmp_path / (n + ".fq")).write_bytes(mc.fastq(reads + reads[:30]))
    r = tmp_path / "run"
    r.mkdir()
    got = subprocess.run([CLI, "run-multi", "--sample", "a", "-i", str(tmp_path / "a.fq"), "--sample", "b", "-i", str(tmp_path / "b.fq"), "-o", "r",
                          "--db-out", str(r / "d"), "--gfa-out", str(r / "g")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=r, timeout=300)
    assert got.returncode == 1
    out = got.stdout.splitlines()
    assert out[:2] == ["10", "10"] and len(out) == 3 and out[2].startswith("ColoredCDBG::read(): Graph could not be loaded! Exit. (")
    assert "run-multi: colors" not in got.stderr
    assert [f for f in os.listdir(r) if not f.startswith("PloidyFrost_output")] == []     # nothing is left under an output name


def test_refusals_that_need_no_device(tmp_path):
    fq = tmp_path / "a.fq"
    fq.write_bytes(mc.fastq([b"ACGT" * 10]))
    (tmp_path / "b.fq").write_bytes(mc.fastq([b"ACGA" * 10]))
    os.symlink(fq, tmp_path / "link.fq")
    (tmp_path / "x.fa").write_bytes(b">r\nACGT\n")
    (tmp_path / "x.fq.gz").write_bytes(b"\x1f\x8b\x08\x00")
    a, b = ["--sample", "A", "-i", "a.fq"], ["--sample", "B", "-i", "b.fq"]
    many = [x for c in range(1025) for x in ("--sample", "s%d" % c, "-i", "a.fq")]
    cases = [(["-i", "a.fq"] + a, "stands before any --sample"), (a + ["--sample", "B"], "sample B has no input"),
             (a + ["--sample", "A", "-i", "b.fq"], "sample A is given twice"), (a + ["--sample", "B", "-i", "a.fq"], "the same file is given in two samples"),
             (a + ["--sample", "B", "-i", "link.fq"], "the same file is given in two samples"), (many, "more than 1024 samples"),
             (a + b + ["-f", "x"], "-f does not go with run-multi"), (a + b + ["-C", "x"], "-C does not go"), (a + b + ["-d", "x"], "-d does not go"),
             (a + b + ["-h", "x"], "-h does not go"), (a + b + ["-l", "3"], "-l does not go"), (a + b + ["-b"], "-b does not go"),
             (a + b + ["--gpus", "2"], "--gpus is not built into run-multi"), (a + b + ["--filtered-out", "x"], "--filtered-out is not built"),
             (a + b + ["-k", "4"], "-k"), (a + b + ["-k", "32"], "-k"), (a + b + ["-g", "24"], "-g"), (a + b + ["-ci", "9", "-cx", "3"], "-ci"),
             (a + ["--sample", "B", "-i", "x.fa"], "FASTA"), (a + ["--sample", "B", "-i", "x.fq.gz"], "gzip"),
             (a + b + ["--model", "fre"], "--filter-multi"), (a + b + ["--filter", "-n 6", "--model", "fre"], "--filter "),
             (a + b + ["--model-each-color"], "--model-each-color needs --filter-multi")]
    for args, word in cases:
        r = subprocess.run([CLI, "run-multi"] + args + ["-o", "out"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp_path, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (args[-4:], r.stderr[:300])
        assert sorted(os.listdir(tmp_path)) == ["a.fq", "b.fq", "link.fq", "x.fa", "x.fq.gz"], args[-4:]
    # an output that is an input
    os.symlink(fq, tmp_path / "g.gfa")
    r = subprocess.run([CLI, "run-multi"] + a + b + ["--gfa-out", "g", "-o", "out"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp_path,
                       timeout=60)
    assert r.returncode != 0 and "the output path is an input path" in r.stderr, r.stderr[:300]
    with pytest.raises(RuntimeError) as e:
        hostapi.run_multi_reads([("A", str(fq)), ("A", str(tmp_path / "b.fq"))], "out")
    assert "sample A is given twice" in str(e.value)
