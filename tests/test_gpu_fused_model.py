"""The ploidy estimate in the same run (`--model`, Run.set_model): K-GMM fed from the result text while it is resident on the
device (ploidyfrost_amd/csrc/pf_call_model.hip).  Pinned to the reference binary's own `_model_result.txt` files
(tests/golden/model/fixture_*_expected.txt, written by tests/golden/make_model_golden.py), to the file readers of
`PloidyFrost model` element for element, and to the two-command chain byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, compare_outputs, golden_cases, load_case

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
MODEL = os.path.join(GOLDEN, "model")
TEN = ["alignseq", "allele_frequency", "bicov", "bifre", "tricov", "trifre", "tetracov", "tetrafre", "pentacov", "pentafre"]

PINS = [
    ("hex30k", ["--model", "cov", "--model-ploidy", "1:6"], "fixture_cov"),
    ("tet60k", ["--model", "cov", "--model-q", "0.2", "--model-ploidy", "1:4"], "fixture_cov_q"),   # every row fails the integer test: all NaN
    ("tet60k", ["--model", "fre"], "fixture_fre"),
]


def cli(meta, extra, cwd):
    return subprocess.run([CLI, "-g", meta["gfa"], "-d", meta["db"], "-o", "g", "-t", "1"] + meta["args"] + extra, cwd=cwd,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("case,extra,expected", PINS, ids=[p[2] for p in PINS])
def test_cli_result_file_is_the_reference_binarys(case, extra, expected, tmp_path):
    meta = load_case(case)
    r = cli(meta, extra, tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    with open(out / "g_model_result.txt") as got, open(os.path.join(MODEL, expected + "_expected.txt")) as exp:
        text = got.read()
        assert text == exp.read()
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))   # the twelve calling files, same run
    assert text.splitlines()[-1] in r.stdout.splitlines()                          # the estimate is printed as well


@pytest.mark.parametrize("case,extra,expected", PINS, ids=[p[2] for p in PINS])
def test_cli_model_only_writes_the_result_and_no_calling_file(case, extra, expected, tmp_path):
    meta = load_case(case)
    r = cli(meta, extra + ["--model-only"], tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    with open(out / "g_model_result.txt") as got, open(os.path.join(MODEL, expected + "_expected.txt")) as exp:
        assert got.read() == exp.read()
    for suf in TEN:
        assert not (out / ("g_%s.txt" % suf)).exists(), suf
    for suf in ("Unitig_Id", "super_bubble"):   # findSuperBubble's files are written as ever
        with open(out / ("g_%s.txt" % suf), "rb") as a, open(os.path.join(meta["dir"], "expected", "g_%s.txt" % suf), "rb") as b:
            assert a.read() == b.read(), suf


def open_run(meta, out):
    op = meta["opts"]
    run = hostapi.Run(meta["gfa"], meta["db"], z=int(op["-z"]), M=float(op["-M"]), D=float(op["-D"]), G=float(op["-G"]))
    run.set_output_dir(str(out))
    run.set_unitig_id("g")
    return run


def readers(out, source, q):
    m = hostapi.Gmm()
    if source == "cov":
        m.read_cov(os.path.join(str(out), "g"), q)
    else:
        m.read_fre(os.path.join(str(out), "g_allele_frequency.txt"), q)
    return m.values()


def check_values(run, meta, out, combos=(("cov", 0.0), ("cov", 0.05), ("fre", 0.0), ("fre", 0.05))):
    """the device array against the file readers on the files of the same run.  Where the readers refuse those files -- a coverage row
    that sums to 0, a frequency that is "nan": fixture stranded20k has both -- the sub-command fails, and the one-command run must
    fail with the same error (naming stream and row) after it has written the calling files, and leave the run usable."""
    op = meta["opts"]
    pre = os.path.join(meta["dir"], "expected", "g")
    for source, q in combos:
        refusal = None
        try:   # (the run's files are the fixture's, byte for byte: what the readers say of them is known beforehand)
            m = hostapi.Gmm()
            m.read_cov(pre, q) if source == "cov" else m.read_fre(pre + "_allele_frequency.txt", q)
        except RuntimeError as e:
            refusal = str(e)
        run.set_model(source, q=q, lo=1, hi=1, max_iter=1)
        run.find_superbubbles("g")
        if refusal is not None:
            with pytest.raises(Exception) as e:
                run.ploidy_estimation("g", int(op["-l"]), int(op["-u"]))
            word = "sums to 0" if source == "cov" else "not a number"
            assert word in refusal and word in str(e.value) and "row " in str(e.value) and "of stream _" in str(e.value), (refusal, str(e.value))
            with pytest.raises(RuntimeError, match=word):
                readers(out, source, q)
            assert not (out / "g_model_result.txt").exists()   # nothing was fitted
            continue
        run.ploidy_estimation("g", int(op["-l"]), int(op["-u"]))
        got, exp = run.model_values(), readers(out, source, q)
        assert got.dtype == np.float64 and len(got) == len(exp), (source, q, len(got), len(exp))
        assert np.array_equal(got, exp), (source, q)
        assert run.model_result()["values"] == len(exp)


@pytest.mark.parametrize("case", golden_cases())
def test_value_array_equals_the_readers_on_the_files_of_the_same_run(case, tmp_path):
    meta = load_case(case)
    run = open_run(meta, tmp_path)
    check_values(run, meta, tmp_path)
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(tmp_path))
    run.close()


@pytest.mark.parametrize("variant", ["numeric_text", "alignseq_text", "align_pieces_1", "align_pieces_many", "small_batches", "ref_threads_2"])
def test_value_array_under_every_way_the_text_is_made(variant, tmp_path, monkeypatch):
    meta = load_case("tet60k")
    if variant == "numeric_text":
        monkeypatch.setenv("PF_NUMERIC_ASCII", "1")
    if variant == "alignseq_text":
        monkeypatch.setenv("PF_ALIGNSEQ_ASCII", "1")
    run = open_run(meta, tmp_path)
    if variant == "align_pieces_1":
        run.set_batch_bubbles(16)   # pieces of 64 bubbles, one piece an alignment range
        run.set_align_pieces(1)
    if variant == "align_pieces_many":
        run.set_batch_bubbles(8)    # pieces of 32 bubbles, eight (>= 4) an alignment range
        run.set_align_pieces(8)
    if variant == "small_batches":
        run.set_batch_bubbles(5)
    if variant == "ref_threads_2":
        run.set_reference_threads(2)
    check_values(run, meta, tmp_path)
    if variant != "ref_threads_2":
        assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(tmp_path))
    run.close()


@pytest.mark.parametrize("case", ["hex30k", "tet60k"])
@pytest.mark.parametrize("source", ["cov", "fre"])
def test_same_bytes_as_the_two_command_chain(case, source, tmp_path):
    meta = load_case(case)
    r = cli(meta, ["--model", source], tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    arg = ["-f", str(out / "g")] if source == "cov" else ["-g", str(out / "g_allele_frequency.txt")]
    r2 = subprocess.run([CLI, "model"] + arg + ["-o", "chain"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r2.returncode == 0, r2.stdout
    with open(out / "g_model_result.txt", "rb") as a, open(tmp_path / "chain_model_result.txt", "rb") as b:
        one, two = a.read(), b.read()
    assert len(one) > 0 and one == two


def test_model_result_of_the_facade_is_what_the_file_says(tmp_path):
    meta = load_case("hex30k")
    run = open_run(meta, tmp_path)
    run.set_model("cov", lo=1, hi=6)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    res = run.model_result()
    assert sorted(res["fits"]) == [1, 2, 3, 4, 5, 6]
    with open(tmp_path / "g_model_result.txt") as got, open(os.path.join(MODEL, "fixture_cov_expected.txt")) as exp:
        text = got.read()
        assert text == exp.read()
    assert text.splitlines()[-1] == "estimated ploidy level is : %g" % res["ploidy"]
    best = min(res["fits"], key=lambda g: res["fits"][g]["aic"])
    assert res["ploidy"] == best + 1
    for g, f in res["fits"].items():
        assert ("AIC : %g" % f["aic"]) in text and np.allclose(f["means"], np.arange(1, g + 1) / (g + 1))
    run.set_model(None)   # off again: the next pass writes no result and launches nothing new
    os.remove(tmp_path / "g_model_result.txt")
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    assert not (tmp_path / "g_model_result.txt").exists() and run.model_result()["fits"] == {}
    run.close()


@pytest.mark.parametrize("extra,word", [
    (["--model", "cov", "-f", "graph.bfg_colors"], "--model"),
    (["--model", "cov", "--gpus", "2"], "--gpus"),
    (["--model", "both"], "--model both"),
    (["--model", "cov", "--model-ploidy", "0:3"], "--model-ploidy"),
    (["--model", "fre", "--model-ploidy", "1:17"], "--model-ploidy"),
])
def test_refusals_name_the_option_and_write_nothing(extra, word, tmp_path):
    meta = load_case("tet60k")
    r = subprocess.run([CLI, "-g", meta["gfa"], "-d", meta["db"], "-o", "g"] + meta["args"] + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.startswith("Error:") and word in r.stderr and len(r.stderr.strip().splitlines()) == 1
    assert os.listdir(tmp_path) == []


def test_a_run_without_the_option_writes_no_result_file(tmp_path):
    meta = load_case("tet60k")
    r = cli(meta, [], tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))
    assert not [f for f in os.listdir(out) if "model_result" in f]
    assert "estimated ploidy level" not in r.stdout


def test_model_only_copies_no_calling_text_from_the_device(tmp_path):
    meta = load_case("tet60k")
    run = open_run(meta, tmp_path / "all")
    run.set_model("cov", lo=1, hi=2)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    normal = run.text_bytes_fetched()
    values = run.model_values()
    assert normal > 0
    run.close()
    run = open_run(meta, tmp_path / "only")
    run.set_model("cov", lo=1, hi=2, only=True)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    assert run.text_bytes_fetched() == 0
    assert np.array_equal(run.model_values(), values) and len(values) > 0
    with open(tmp_path / "all" / "g_model_result.txt", "rb") as a, open(tmp_path / "only" / "g_model_result.txt", "rb") as b:
        assert a.read() == b.read()
    for suf in TEN:
        assert not (tmp_path / "only" / ("g_%s.txt" % suf)).exists(), suf
    # a run without a model fetches its text as ever
    run.set_model(None)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    assert run.text_bytes_fetched() > 0
    run.close()
