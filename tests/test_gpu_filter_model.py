"""The row filter in front of the model of the same run (`--model ... --filter "<opts>"`, Run.set_filter; kernels in
ploidyfrost_amd/csrc/pf_call_model.hip, rule in csrc/pf_filter_rows.hpp): held byte for byte to the three-command chain
`ploidyfrost` / `ploidyfrost filter` / `ploidyfrost model`, and element for element to the shared rule on the host."""
import os
import subprocess

import numpy as np
import pytest

from conftest import compare_outputs, load_case
from filter_cases import CLI, HAND_SETS, HAND_TABLES, OPTION_SETS, R_ERROR, TABLES, read_tables, run_filter, write_tables

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
TEN = ["alignseq", "allele_frequency", "bicov", "bifre", "tricov", "trifre", "tetracov", "tetrafre", "pentacov", "pentafre"]


def sh(args, cwd):
    return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def call(meta, extra, cwd):
    return sh(["-g", meta["gfa"], "-d", meta["db"], "-o", "g", "-t", "1"] + meta["args"] + extra, cwd)


def chain_result(prefix, words, source, cwd, name="chain"):
    """`filter -i prefix -o f <words>` then `model -g f_allele_frequency.txt` / `model -f f`: the bytes of the result file"""
    run_filter(prefix, words, str(cwd / "f"))
    arg = ["-f", str(cwd / "f")] if source == "cov" else ["-g", str(cwd / "f_allele_frequency.txt")]
    r = sh(["model"] + arg + ["-o", name], cwd)
    assert r.returncode == 0, r.stdout
    with open(cwd / (name + "_model_result.txt"), "rb") as f:
        return f.read(), r.stdout


@pytest.mark.parametrize("words", [s[0] for s in OPTION_SETS[:3]], ids=[s[0].replace(" ", "") for s in OPTION_SETS[:3]])
@pytest.mark.parametrize("source", ["cov", "fre"])
@pytest.mark.parametrize("case", ["hex30k", "tet60k"])
def test_same_bytes_as_the_three_command_chain(case, source, words, tmp_path):
    meta = load_case(case)
    r = call(meta, ["--model", source, "--filter", words], tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))   # the calling files as ever
    assert not [f for f in os.listdir(out) if f.startswith("f_") or "filtered" in f]   # no filtered table
    two, said = chain_result(str(out / "g"), words, source, tmp_path)
    with open(out / "g_model_result.txt", "rb") as f:
        one = f.read()
    assert len(one) > 0 and one == two
    # the estimate is printed as well: the last line of the result file (`model` itself writes the file and says nothing)
    assert one.decode().splitlines()[-1].startswith("estimated ploidy level is : ") and one.decode().splitlines()[-1] in r.stdout.splitlines()


@pytest.mark.parametrize("source", ["cov", "fre"])
@pytest.mark.parametrize("case", ["hex30k", "tet60k"])
def test_model_only_with_a_filter_writes_the_chains_result_and_no_calling_file(case, source, tmp_path):
    meta = load_case(case)
    words = OPTION_SETS[0][0]
    r = call(meta, ["--model", source, "--filter", words, "--model-only"], tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    for suf in TEN:
        assert not (out / ("g_%s.txt" % suf)).exists(), suf
    two, _ = chain_result(os.path.join(meta["dir"], "expected", "g"), words, source, tmp_path)   # (the run's files are the fixture's)
    with open(out / "g_model_result.txt", "rb") as f:
        assert f.read() == two


def open_run(meta, out):
    op = meta["opts"]
    run = hostapi.Run(meta["gfa"], meta["db"], z=int(op["-z"]), M=float(op["-M"]), D=float(op["-D"]), G=float(op["-G"]))
    run.set_output_dir(str(out))
    run.set_unitig_id("g")
    return run


def test_model_only_with_a_filter_copies_no_calling_text_from_the_device(tmp_path):
    meta = load_case("tet60k")
    run = open_run(meta, tmp_path)
    kw = OPTION_SETS[0][1]
    run.set_model("fre", lo=1, hi=2, only=True)
    run.set_filter(**kw)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    assert run.text_bytes_fetched() == 0
    exp = hostapi.filter_rows("fre", read_tables(os.path.join(meta["dir"], "expected", "g")), 0.0, **kw)
    assert len(exp) > 0 and np.array_equal(run.model_values(), exp)
    run.close()


@pytest.mark.parametrize("variant", ["small_batches", "align_pieces_many"])
def test_value_array_through_the_facade(variant, tmp_path):
    """the 14 running counts over many pieces (and over two alignment ranges) against the shared rule on the files of the same run"""
    meta = load_case("tet60k")
    run = open_run(meta, tmp_path)
    if variant == "small_batches":
        run.set_batch_bubbles(5)
    else:
        run.set_batch_bubbles(8)
        run.set_align_pieces(8)
    for words, kw, _ in OPTION_SETS[:2]:
        for source, q in (("cov", 0.0), ("fre", 0.0), ("fre", 0.3)):
            run.set_model(source, q=q, lo=1, hi=1, max_iter=1)
            run.set_filter(**kw)
            run.find_superbubbles("g")
            run.ploidy_estimation("g", 5, 1000)
            got, exp = run.model_values(), hostapi.filter_rows(source, read_tables(str(tmp_path / "g")), q, **kw)
            assert got.dtype == np.float64 and len(got) == len(exp) and len(exp) > 0, (words, source, q, len(got), len(exp))
            assert np.array_equal(got, exp), (words, source, q)
            assert run.model_result()["values"] == len(exp)
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(tmp_path))
    run.close()


@pytest.mark.parametrize("tables,words,kw,cov_refused", HAND_SETS, ids=[s[0] + s[1].replace(" ", "") for s in HAND_SETS])
def test_chosen_rows_through_the_kernels(tables, words, kw, cov_refused, tmp_path):
    """`model -f <prefix> --filter ...`: the filter and the fit in one command from files, through the kernels of the one-command run"""
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND_TABLES[tables])
    for source in ("cov", "fre"):
        r = sh(["model", "-f", prefix, "--filter", words, "--source", source, "-u", "3", "-o", "one_" + source], tmp_path)
        if source == "cov" and cov_refused:
            with pytest.raises(RuntimeError) as e:
                hostapi.filter_rows(source, read_tables(prefix), 0.0, **kw)
            assert r.returncode != 0 and str(e.value) in r.stdout and "of stream _bicov" in r.stdout and "three-command chain" in r.stdout, r.stdout
            assert not (tmp_path / ("one_%s_model_result.txt" % source)).exists()
            continue
        assert r.returncode == 0, r.stdout
        run_filter(prefix, words, str(tmp_path / "f"))
        arg = ["-f", str(tmp_path / "f")] if source == "cov" else ["-g", str(tmp_path / "f_allele_frequency.txt")]
        r2 = sh(["model"] + arg + ["-u", "3", "-o", "two_" + source], tmp_path)
        assert r2.returncode == 0, r2.stdout
        with open(tmp_path / ("one_%s_model_result.txt" % source), "rb") as a, open(tmp_path / ("two_%s_model_result.txt" % source), "rb") as b:
            one, two = a.read(), b.read()
        assert len(one) > 0 and one == two, (source, one, two)


@pytest.mark.parametrize("what", ["cell", "fields", "none_kept"])
def test_refused_rows_are_named_as_the_host_names_them(what, tmp_path):
    tables = dict(HAND_TABLES["hand"])
    words, kw = "-l 5 -u 1000", dict(low=5, up=1000)
    if what == "cell":
        tables["tricov"] = tables["tricov"].replace("40.5\t", "nan\t")
    elif what == "fields":
        tables["pentacov"] += "1\t2\t3\t\n"
    else:
        words, kw = "-l 5000", dict(low=5000)
    prefix = str(tmp_path / "in")
    write_tables(prefix, tables)
    for source in ("cov", "fre"):
        with pytest.raises(RuntimeError) as e:
            hostapi.filter_rows(source, read_tables(prefix), 0.0, **kw)
        r = sh(["model", "-f", prefix, "--filter", words, "--source", source, "-o", "one"], tmp_path)
        assert r.returncode != 0 and str(e.value) in r.stdout, (str(e.value), r.stdout)
        word = {"cell": "in line 2 of stream _tricov", "fields": "line 4 did not have 10 elements (stream _pentacov)", "none_kept": R_ERROR}[what]
        assert word in r.stdout
        assert not (tmp_path / "one_model_result.txt").exists()


def test_no_kept_row_is_rs_error_after_the_calling_files_and_the_run_goes_on(tmp_path):
    meta = load_case("tet60k")
    words, kw, _ = OPTION_SETS[3]
    r = call(meta, ["--model", "fre", "--filter", words], tmp_path)
    out = tmp_path / "PloidyFrost_output"
    assert r.returncode != 0 and R_ERROR in r.stdout, r.stdout
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))
    assert not (out / "g_model_result.txt").exists()
    run = open_run(meta, tmp_path / "facade")
    for source in ("cov", "fre"):
        run.set_model(source, lo=1, hi=1, max_iter=1)
        run.set_filter(**kw)
        run.find_superbubbles("g")
        with pytest.raises(Exception, match=R_ERROR):
            run.ploidy_estimation("g", 5, 1000)
        assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(tmp_path / "facade"))
        assert not (tmp_path / "facade" / "g_model_result.txt").exists()
    # the same run completes a pass without a filter: the values of the unfiltered text, as ever
    run.set_filter(None)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    with open(tmp_path / "facade" / "g_allele_frequency.txt", "rb") as f:
        assert np.array_equal(run.model_values(), hostapi.model_rows("fre", f.read(), 0.0))
    assert (tmp_path / "facade" / "g_model_result.txt").exists()
    run.close()


@pytest.mark.parametrize("extra,word", [
    (["--filter", "-S"], "--model"),
    (["--model", "cov", "--filter", "-S", "-f", "graph.bfg_colors"], "--filter"),
    (["--model", "cov", "--filter", "-S", "--gpus", "2"], "--gpus"),
    (["--model", "fre", "--filter", "-i x"], "-i"),
    (["--model", "fre", "--filter", "-o x"], "-o"),
    (["--model", "fre", "--filter", "-c 1"], "-c"),
    (["--model", "fre", "--filter", "-v 0.5"], "-v"),
    (["--model", "fre", "--filter", "-q 0.6"], "-q 0.6"),
])
def test_refusals_name_the_option_and_write_nothing(extra, word, tmp_path):
    meta = load_case("tet60k")
    r = subprocess.run([CLI, "-g", meta["gfa"], "-d", meta["db"], "-o", "g"] + meta["args"] + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.startswith("Error:") and word in r.stderr and "--filter" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    assert os.listdir(tmp_path) == []


def test_set_filter_is_refused_without_a_model(tmp_path):
    meta = load_case("tet60k")
    run = open_run(meta, tmp_path)
    with pytest.raises(Exception, match="model"):
        run.set_filter(simple=True)
    run.set_model("cov")
    with pytest.raises(Exception, match="0.5"):
        run.set_filter(frequency=0.6)
    run.close()


@pytest.mark.parametrize("source", ["cov", "fre"])
def test_without_a_filter_nothing_changes(source, tmp_path):
    """a pass with a filter, then set_filter(None) on the same run: the value array and the files of a run that never had one"""
    meta = load_case("tet60k")
    run = open_run(meta, tmp_path)
    run.set_model(source, lo=1, hi=2)
    run.set_filter(**OPTION_SETS[0][1])
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    filtered = run.model_values()
    run.set_filter(None)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", 5, 1000)
    pre = os.path.join(meta["dir"], "expected", "g")
    m = hostapi.Gmm()
    m.read_cov(pre, 0.0) if source == "cov" else m.read_fre(pre + "_allele_frequency.txt", 0.0)
    assert np.array_equal(run.model_values(), m.values()) and len(filtered) < len(m.values())
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(tmp_path))
    r = sh(["model"] + (["-f", pre] if source == "cov" else ["-g", pre + "_allele_frequency.txt"]) + ["-u", "2", "-o", "chain"], tmp_path)
    assert r.returncode == 0, r.stdout
    with open(tmp_path / "g_model_result.txt", "rb") as a, open(tmp_path / "chain_model_result.txt", "rb") as b:
        assert a.read() == b.read()
    run.close()
