"""`ploidyfrost smudge` and `run --smudge` end to end: `smudge -d` on a database written from the k = 25 fixture of hetpair_cases.py is the
bytes the Python restatement writes (report and pairs file), `--auto-cutoffs` takes what `cutoffL -d` / `cutoffU -d` print, `smudge -k`
on reads is `count` followed by `smudge -d` whatever the chunking, and `run --smudge` leaves every other output of `run` as it is and
writes the report `smudge -d` writes for the run's own database and bounds."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

import hetpair_cases as hp
import trim_cases as tc

from ploidyfrost_amd import hostapi, synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K, LO, HI = 25, 10, 100
DEPTH = 64


def cli(*a, cwd, ok=True):
    r = subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, timeout=300)
    assert not ok or r.returncode == 0, (a, r.stdout[-2000:], r.stderr[-2000:])
    return r


def files_of(d, but=()):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d))) if os.path.isfile(os.path.join(str(d), f)) and f not in but}


def calling_files(d, prefix):
    od = os.path.join(str(d), "PloidyFrost_output")
    return {f[len(prefix):]: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od)) if f.startswith(prefix + "_")}


def stats_line(st):
    return "smudge: kmers %d in_range %d one_partner %d many_partners %d pairs %d" % tuple(st[f] for f in ("kmers", "in_range", "one_partner", "many_partners", "pairs"))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the k = 25 fixture as a database, its Python result, and reads of two haplotypes (the generator of the build goldens at depth 64)
    with the database `count` writes for them"""
    root = tmp_path_factory.mktemp("smudge")
    km, ct = hp.haplotypes(K)
    synth.write_kmc1(str(root / "fix"), km, ct, K)
    spec = importlib.util.spec_from_file_location("make_build_golden", os.path.join(GOLDEN, "make_build_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], depth=DEPTH)))
    half = len(reads) // 2
    for name, part in (("a.fq", reads[:half]), ("b.fq", reads[half:])):
        (root / name).write_bytes(tc.fastq([(b"r%d" % i, r.encode(), b"I" * len(r)) for i, r in enumerate(part)]))
    cli("count", "-k", K, "-ci", 1, "-cs", 10000, "-i", root / "a.fq", "-i", root / "b.fq", "-o", root / "reads_db", cwd=root)
    return dict(root=root, fix=root / "fix", want=hp.hetpairs(km, ct, K, LO, HI), a=root / "a.fq", b=root / "b.fq", reads_db=root / "reads_db")


def test_smudge_d_writes_the_python_report(data, tmp_path):
    w = data["want"]
    assert w["stats"]["pairs"] == 725
    r = cli("smudge", "-d", data["fix"], "-l", LO, "-u", HI, "-o", "out", cwd=tmp_path)
    assert (tmp_path / "out_smudge.tsv").read_bytes() == hp.report(w["table"], w["stats"], K, LO, HI) and sorted(os.listdir(tmp_path)) == ["out_smudge.tsv"]
    assert r.stderr.splitlines() == [stats_line(w["stats"])] and r.stdout == ""
    r = cli("smudge", "-d", data["fix"], "-l", LO, "-u", HI, "-o", "n", "-n", 20, "-v", cwd=tmp_path)
    assert (tmp_path / "n_smudge.tsv").read_bytes() == hp.report(w["table"], w["stats"], K, LO, HI, 20)
    lines = r.stderr.splitlines()
    assert lines[:2] == [stats_line(w["stats"]), "smudge: proposed ploidy 2 (AB, 725 of 725 pairs)"] and lines[2].startswith("smudge: load ") and len(lines) == 3
    res = hostapi.smudge(str(tmp_path / "api"), db=str(data["fix"]), lower=LO, upper=HI, n=20)
    assert (tmp_path / "api_smudge.tsv").read_bytes() == (tmp_path / "n_smudge.tsv").read_bytes()
    assert res["stats"] == w["stats"] and (res["k"], res["lower"], res["upper"], res["clamped"]) == (K, LO, HI, 0)
    assert (res["proposed_p"], res["proposed_m"], res["proposed_pairs"], res["all_pairs"]) == (2, 1, 725, 725)


def test_a_refused_call_does_not_spoil_the_next_one(data, tmp_path):
    """the C entry points share one error string: a call that follows a refusal starts with it cleared"""
    w = data["want"]
    with pytest.raises(RuntimeError, match="above 4096"):
        hostapi.smudge(str(tmp_path / "o"), db=str(data["fix"]), lower=LO, upper=5000)
    assert os.listdir(tmp_path) == []
    res = hostapi.smudge(str(tmp_path / "o"), db=str(data["fix"]), lower=LO, upper=HI)
    assert res["stats"] == w["stats"] and (tmp_path / "o_smudge.tsv").read_bytes() == hp.report(w["table"], w["stats"], K, LO, HI)
    with pytest.raises(RuntimeError, match="smudge: no input|either a database or inputs"):
        hostapi.smudge(str(tmp_path / "p"), inputs=[], lower=LO, upper=HI)
    res = hostapi.smudge(str(tmp_path / "p"), inputs=[str(data["a"]), str(data["b"])], lower=LO, upper=HI)
    assert (tmp_path / "p_smudge.tsv").exists() and res["stats"]["kmers"] > 0 and sorted(os.listdir(tmp_path)) == ["o_smudge.tsv", "p_smudge.tsv"]


def test_pairs_file_is_the_restatement_s(data, tmp_path):
    w = data["want"]
    cli("smudge", "-d", data["fix"], "-l", LO, "-u", HI, "-o", "out", "--pairs", "pairs.tsv", cwd=tmp_path)
    assert (tmp_path / "pairs.tsv").read_bytes() == hp.pairs_text(w, K) and sorted(os.listdir(tmp_path)) == ["out_smudge.tsv", "pairs.tsv"]
    assert (tmp_path / "out_smudge.tsv").read_bytes() == hp.report(w["table"], w["stats"], K, LO, HI)
    # bounds that leave no pair: an empty pairs file, a report without cells
    cli("smudge", "-d", data["fix"], "-l", 21, "-u", 39, "-o", "none", "--pairs", "none.tsv", cwd=tmp_path)
    assert (tmp_path / "none.tsv").read_bytes() == b"" and b">>table\ncov_a\tcov_b\tpairs\n>>total\n" in (tmp_path / "none_smudge.tsv").read_bytes()


def test_auto_cutoffs_are_what_the_cutoff_commands_print(data, tmp_path):
    lower = int(cli("cutoffL", "-d", data["reads_db"], cwd=tmp_path).stdout)
    upper = int(cli("cutoffU", "-d", data["reads_db"], cwd=tmp_path).stdout)
    upper_q = int(cli("cutoffU", "-d", data["reads_db"], 0.9, cwd=tmp_path).stdout)
    print("auto cut-offs of the reads: lower %d upper %d (q 0.9: %d)" % (lower, upper, upper_q))
    assert 1 <= lower <= upper_q <= upper < lower + 4096
    r = cli("smudge", "-d", data["reads_db"], "--auto-cutoffs", "-o", "auto", "-n", DEPTH // 2, cwd=tmp_path)
    assert r.stdout == "lower %d upper %d\n" % (lower, upper)
    cli("smudge", "-d", data["reads_db"], "-l", lower, "-u", upper, "-o", "given", "-n", DEPTH // 2, cwd=tmp_path)
    rep = (tmp_path / "auto_smudge.tsv").read_bytes()
    assert rep == (tmp_path / "given_smudge.tsv").read_bytes() and rep.split(b"\n")[1] == b"# k 25 lower %d upper %d n %d" % (lower, upper, DEPTH // 2)
    pairs = int(rep.split(b">>totals\n")[1].split(b"\n")[1].split(b"\t")[4])
    print("pairs of the reads:", pairs)
    assert pairs >= 100   # 13 substitutions x 25 windows in the genome; the reads' errors take some away
    r = cli("smudge", "-d", data["reads_db"], "--auto-cutoffs", "-q", 0.9, "-o", "q", cwd=tmp_path)
    assert r.stdout == "lower %d upper %d\n" % (lower, upper_q)


def test_smudge_k_is_count_followed_by_smudge_d(data, tmp_path):
    cli("smudge", "-d", data["reads_db"], "--auto-cutoffs", "-o", "want", "-n", DEPTH // 2, "--pairs", "want_pairs.tsv", cwd=tmp_path)
    want, want_pairs = (tmp_path / "want_smudge.tsv").read_bytes(), (tmp_path / "want_pairs.tsv").read_bytes()
    assert want_pairs.count(b"\n") >= 100
    for name, extra in (("whole", []), ("chunks", ["--chunk-bytes", 4096])):
        d = tmp_path / name
        d.mkdir()
        r = cli("smudge", "-k", K, "-i", data["a"], "-i", data["b"], "--auto-cutoffs", "-o", "got", "-n", DEPTH // 2, "--pairs", "got_pairs.tsv", *extra, cwd=d)
        assert (d / "got_smudge.tsv").read_bytes() == want and (d / "got_pairs.tsv").read_bytes() == want_pairs, name
        assert sorted(os.listdir(d)) == ["got_pairs.tsv", "got_smudge.tsv"] and r.stdout.startswith("lower ")
    res = hostapi.smudge(str(tmp_path / "api"), inputs=[str(data["a"]), str(data["b"])], auto=True, n=DEPTH // 2, k=K, chunk_bytes=8192)
    assert (tmp_path / "api_smudge.tsv").read_bytes() == want and res["stats"]["pairs"] == want_pairs.count(b"\n")


def test_run_smudge_leaves_run_as_it_is(data, tmp_path):
    w, g, s = tmp_path / "want", tmp_path / "got", tmp_path / "smudge"
    for d in (w, g, s):
        d.mkdir()
    common = ["-i", data["a"], "-i", data["b"], "-o", "s", "--db-out", "db"]
    want = cli("run", *common, cwd=w)
    got = cli("run", *common, "--smudge", "--smudge-n", DEPTH // 2, "--smudge-pairs", "pairs.tsv", cwd=g)
    files = calling_files(w, "s")
    got_files = calling_files(g, "s")
    rep = got_files.pop("_smudge.tsv")
    assert len(files) >= 10 and got_files == files
    assert files_of(g, but=("pairs.tsv",)) == files_of(w) and sorted(os.listdir(g)) == sorted(os.listdir(w) + ["pairs.tsv"])
    time_free = lambda text: [l for l in text.splitlines() if " time " not in l]
    assert time_free(got.stdout) == time_free(want.stdout)
    run_line = [l for l in want.stderr.splitlines() if l.startswith("run: reads ")]
    assert len(run_line) == 1 and run_line == [l for l in got.stderr.splitlines() if l.startswith("run: reads ")]
    assert [l for l in got.stderr.splitlines() if not l.startswith("smudge: ")] == want.stderr.splitlines()
    words = run_line[0].split()
    lower, upper = int(words[words.index("lower") + 1]), int(words[words.index("upper") + 1])
    assert upper < lower + 4096
    # the report and the pairs file of `smudge -d` on the run's own database with the run's bounds
    r = cli("smudge", "-d", g / "db", "-l", lower, "-u", upper, "-n", DEPTH // 2, "-o", "x", "--pairs", "x_pairs.tsv", cwd=s)
    assert rep == (s / "x_smudge.tsv").read_bytes() and (g / "pairs.tsv").read_bytes() == (s / "x_pairs.tsv").read_bytes()
    assert [l for l in got.stderr.splitlines() if l.startswith("smudge: ")] == r.stderr.splitlines()
    assert int(r.stderr.split(" pairs ")[1].split()[0]) >= 100
    # the same through the Python entry point
    a = tmp_path / "api"
    a.mkdir()
    cwd = os.getcwd()
    os.chdir(a)
    try:
        res = hostapi.run_reads([str(data["a"]), str(data["b"])], "s", smudge=True, smudge_n=DEPTH // 2)
    finally:
        os.chdir(cwd)
    assert calling_files(a, "s")["_smudge.tsv"] == rep and (res["lower"], res["upper"]) == (lower, upper)
    assert stats_line(res["smudge"]["stats"]) == r.stderr.splitlines()[0]
