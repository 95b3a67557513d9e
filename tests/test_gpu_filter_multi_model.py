"""The multi row filter in front of the model of a colored run (`-f ... --model ... --filter-multi "<opts>" [--model-each-color]`,
ColoredRun.set_filter_multi; kernels in ploidyfrost_amd/csrc/pf_call_model.hip, rule in csrc/pf_filter_rows.hpp): held byte for
byte to the chain `ploidyfrost -f` / `ploidyfrost filter-multi` / `ploidyfrost model`, and element for element to the shared rule
on the host."""
import os
import subprocess

import numpy as np
import pytest

from conftest import compare_outputs, load_case
from filter_multi_cases import (CLI, EACH, HAND, HAND_COLOURS, HAND_SCI, HAND_WORDS, KEPT_COL4_MIX, ONE_COLOUR, POOLED, R_ERROR, SCI_WORDS, kept_rows,
                                read_tables, run_filter_multi, with_colour, write_tables)

from ploidyfrost_amd import hostapi

pytestmark = pytest.mark.gpu
TEN = ["alignseq", "allele_frequency", "bicov", "bifre", "tricov", "trifre", "tetracov", "tetrafre", "pentacov", "pentafre"]
PLOIDY = ["--model-ploidy", "1:2"]      # keeps K-GMM short; the chain gets the same -l 1 -u 2


def sh(args, cwd, merge=True):
    return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT if merge else subprocess.PIPE, text=True)


def call(meta, extra, cwd, merge=True):
    (cwd / "dbs.txt").write_text("".join(p + "\n" for p in meta["dbs"]))
    (cwd / "cutoffs.txt").write_text("".join("%d\t%d\n" % tuple(c) for c in meta["cutoffs"]))
    return sh(["-g", meta["gfa"], "-f", meta["colors"], "-d", str(cwd / "dbs.txt"), "-C", str(cwd / "cutoffs.txt"), "-o", "g", "-t", "1"] + meta["args"] + extra,
              cwd, merge)


def chain_result(prefix, words, source, cwd, name="chain"):
    """`filter-multi -i prefix -o f <words>` then `model -g f_allele_frequency.txt` / `model -f f` with -l 1 -u 2: the result file"""
    run_filter_multi(prefix, words, str(cwd / "f"))
    arg = ["-f", str(cwd / "f")] if source == "cov" else ["-g", str(cwd / "f_allele_frequency.txt")]
    r = sh(["model"] + arg + ["-l", "1", "-u", "2", "-o", name], cwd)
    assert r.returncode == 0, r.stdout
    with open(cwd / (name + "_model_result.txt"), "rb") as f:
        return f.read()


def chain_result_in_process(prefix, words, cwd, name):
    """the same chain for many colours: `filter-multi` as a command, then the driver of `model -g ... -l 1 -u 2` (run_model behind
    hostapi.Gmm.run) in this process, which spares a process and a device context per colour"""
    run_filter_multi(prefix, words, str(cwd / "f"))
    m = hostapi.Gmm()
    m.read_fre(str(cwd / "f_allele_frequency.txt"), 0.0)
    m.run(str(cwd / name), lo=1, hi=2)
    m.close()
    with open(cwd / (name + "_model_result.txt"), "rb") as f:
        return f.read()


# ---- 1. the same bytes as the chain ----
@pytest.mark.parametrize("words,kw", [ONE_COLOUR, POOLED], ids=["one_colour", "pooled"])
@pytest.mark.parametrize("source", ["cov", "fre"])
@pytest.mark.parametrize("case", ["col3_dip", "col4_mix"])
def test_same_bytes_as_the_chain(case, source, words, kw, tmp_path):
    meta = load_case(case)
    expected = os.path.join(meta["dir"], "expected")
    assert kept_rows(os.path.join(expected, "g"), kw) > 0
    r = call(meta, ["--model", source, "--filter-multi", words] + PLOIDY, tmp_path)
    assert r.returncode == 0, r.stdout
    out = tmp_path / "PloidyFrost_output"
    assert not compare_outputs(expected, str(out))   # the twelve calling files as ever
    assert not [f for f in os.listdir(out) if f.startswith("f_") or "filtered" in f]   # no filtered table
    two = chain_result(str(out / "g"), words, source, tmp_path)
    with open(out / "g_model_result.txt", "rb") as f:
        one = f.read()
    assert len(one) > 0 and one == two
    last = one.decode().splitlines()[-1]
    assert last.startswith("estimated ploidy level is : ") and last in r.stdout.splitlines()
    # --model-only: the same result, none of the ten calling files
    only = tmp_path / "only"
    only.mkdir()
    r = call(meta, ["--model", source, "--filter-multi", words, "--model-only"] + PLOIDY, only)
    assert r.returncode == 0, r.stdout
    for suf in TEN:
        assert not (only / "PloidyFrost_output" / ("g_%s.txt" % suf)).exists(), suf
    with open(only / "PloidyFrost_output" / "g_model_result.txt", "rb") as f:
        assert f.read() == two


# ---- 2. every colour at once ----
@pytest.mark.parametrize("case", ["col3_dip", "col4_mix", "col100"])
def test_every_colour_in_one_command(case, tmp_path):
    meta = load_case(case)
    prefix = os.path.join(meta["dir"], "expected", "g")
    words, kw = EACH
    r = call(meta, ["--model", "fre", "--filter-multi", words, "--model-each-color"] + PLOIDY, tmp_path, merge=False)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = tmp_path / "PloidyFrost_output"
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))
    assert not (out / "g_model_result.txt").exists()
    fitted, said = [], [ln for ln in r.stdout.splitlines() if ln.startswith("color ")]
    for c in range(meta["n_colors"]):
        one = out / ("g_color%d_model_result.txt" % c)
        if kept_rows(prefix, dict(kw, color=c)) == 0:
            assert not one.exists()
            assert [ln for ln in r.stderr.splitlines() if ln.startswith("color %d:" % c)] == ["color %d: no row kept, no estimate" % c]
            continue
        two = chain_result_in_process(str(out / "g"), words + " -c %d" % c, tmp_path, "chain%d" % c)
        if not fitted:   # ... and once through the `model` command itself
            assert two == chain_result(str(out / "g"), words + " -c %d" % c, "fre", tmp_path, "cli%d" % c)
        with open(one, "rb") as f:
            got = f.read()
        assert len(got) > 0 and got == two, c
        fitted.append("color %d: %s" % (c, got.decode().splitlines()[-1]))
    assert said == fitted and len(fitted) == (3 if case == "col4_mix" else meta["n_colors"])   # in colour order
    if case == "col4_mix":
        assert "color 2:" in r.stderr and not (out / "g_color2_model_result.txt").exists()


# ---- 3. the value arrays through the facade ----
def open_run(meta, work, out):
    run = hostapi.ColoredRun(meta["gfa"], meta["colors"], meta["dbs"], str(work), z=int(meta["opts"]["-z"]))
    run.set_output_dir(str(out))
    run.set_unitig_id("g")
    return run


@pytest.mark.parametrize("variant", ["small_batches", "align_pieces_many"])
def test_value_arrays_through_the_facade(variant, tmp_path):
    """a colour's rows over many pieces (and over two alignment ranges) against the shared rule on the files of the same run"""
    meta = load_case("col4_mix")
    out = tmp_path / "out"
    run = open_run(meta, tmp_path, out)
    if variant == "small_batches":
        run.set_batch_bubbles(5)
    else:
        run.set_align_pieces(8)
    words, kw = EACH
    for source, q in (("cov", 0.0), ("fre", 0.0), ("fre", 0.3)):
        run.set_model(source, q=q, lo=1, hi=1, max_iter=1)
        run.set_filter_multi(each_color=True, **kw)
        run.find_superbubbles("g")
        run.ploidy_estimation("g", meta["cutoffs"])
        texts = read_tables(str(out / "g"))
        pooled = hostapi.filter_rows(source, texts, q, multi=True, **kw)
        assert len(pooled) > 0 and np.array_equal(run.model_values(), pooled), (source, q)
        assert run.model_colors() == [0, 1, 3]
        for c in range(4):
            if KEPT_COL4_MIX[c] == 0:
                with pytest.raises(RuntimeError, match=R_ERROR):
                    hostapi.filter_rows(source, texts, q, multi=True, color=c, **kw)
                with pytest.raises(KeyError):
                    run.model_values(color=c)
                continue
            got, exp = run.model_values(color=c), hostapi.filter_rows(source, texts, q, multi=True, color=c, **kw)
            assert got.dtype == np.float64 and len(got) == len(exp) and len(exp) > 0, (source, q, c, len(got), len(exp))
            assert np.array_equal(got, exp), (source, q, c)
            assert run.model_result(color=c)["values"] == len(exp)
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))
    # one colour alone, nothing fetched: the array of that colour
    run.set_model("fre", lo=1, hi=1, max_iter=1, only=True)
    run.set_filter_multi(color=3, **kw)
    assert np.array_equal(run.model_values(), pooled)   # new settings and no new pass: still what the last pass left
    run.find_superbubbles("g")
    run.ploidy_estimation("g", meta["cutoffs"])
    assert run.text_bytes_fetched() == 0
    three = hostapi.filter_rows("fre", texts, 0.0, multi=True, color=3, **kw)
    assert np.array_equal(run.model_values(), three) and run.model_colors() == []
    run.set_filter_multi(each_color=True, **kw)
    assert np.array_equal(run.model_values(), three)
    run.close()


# ---- 4. chosen rows through the kernels ----
def test_chosen_rows_through_the_kernels(tmp_path):
    """`model -f <prefix> --filter-multi ...`: tri, tetra and penta rows of A + 7 fields, the absent sum clause, Cramer's V equal to
    the threshold and a colour beyond 64 on the device"""
    prefix = str(tmp_path / "in")
    write_tables(prefix, HAND)
    sets = [HAND_WORDS] + [with_colour(*HAND_WORDS, c) for c in HAND_COLOURS]
    for words, kw in sets:
        for source in ("cov", "fre"):
            r = sh(["model", "-f", prefix, "--filter-multi", words, "--source", source, "-u", "2", "-o", "one"], tmp_path)
            if kw.get("color") == 2:
                assert r.returncode != 0 and R_ERROR in r.stdout and not (tmp_path / "one_model_result.txt").exists()
                continue
            assert r.returncode == 0, r.stdout
            run_filter_multi(prefix, words, str(tmp_path / "f"))
            arg = ["-f", str(tmp_path / "f")] if source == "cov" else ["-g", str(tmp_path / "f_allele_frequency.txt")]
            r2 = sh(["model"] + arg + ["-u", "2", "-o", "two"], tmp_path)
            assert r2.returncode == 0, r2.stdout
            with open(tmp_path / "one_model_result.txt", "rb") as a, open(tmp_path / "two_model_result.txt", "rb") as b:
                one, two = a.read(), b.read()
            assert len(one) > 0 and one == two, (words, source, one, two)
            os.remove(tmp_path / "one_model_result.txt")
    # every colour at once from the same files
    for source in ("cov", "fre"):
        r = sh(["model", "-f", prefix, "--filter-multi", HAND_WORDS[0], "--model-each-color", "--source", source, "-u", "2", "-o", "each_" + source], tmp_path, merge=False)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert [ln.split(":")[0] for ln in r.stdout.splitlines() if ln.startswith("color ")] == ["color 0", "color 1", "color 3", "color 70"]
        assert "color 2: no row kept" in r.stderr
        for c in (0, 1, 3, 70):
            run_filter_multi(prefix, HAND_WORDS[0] + " -c %d" % c, str(tmp_path / "f"))
            arg = ["-f", str(tmp_path / "f")] if source == "cov" else ["-g", str(tmp_path / "f_allele_frequency.txt")]
            assert sh(["model"] + arg + ["-u", "2", "-o", "two"], tmp_path).returncode == 0
            with open(tmp_path / ("each_%s_color%d_model_result.txt" % (source, c)), "rb") as a, open(tmp_path / "two_model_result.txt", "rb") as b:
                one, two = a.read(), b.read()
            assert len(one) > 0 and one == two, (source, c)


def test_a_colour_whose_kept_rows_hold_no_value_is_named_and_the_colours_above_it_are_fitted(tmp_path):
    """colour 5 keeps one penta row and nothing else: no value for `cov` (penta rows are counted and never read), and for `fre` none
    once the model's own test (model -q 0.3) drops its five frequencies of 0.2"""
    prefix = str(tmp_path / "in")
    write_tables(prefix, dict(HAND, pentacov=HAND["pentacov"] + "100\t100\t100\t100\t100\t5\t1\t0\t20\t1\t0.9\t30\t\n"))
    assert kept_rows(prefix, dict(HAND_WORDS[1], color=5)) == 1 and kept_rows(prefix, dict(HAND_WORDS[1], color=5), ("pentacov",)) == 1
    for source, q in (("cov", "0"), ("fre", "0.3")):
        name = "each_" + source
        r = sh(["model", "-f", prefix, "--filter-multi", HAND_WORDS[0], "--model-each-color", "--source", source, "-q", q, "-u", "2", "-o", name], tmp_path, merge=False)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert [ln for ln in r.stderr.splitlines() if ln.startswith("color 5:")] == ["color 5: the rows kept hold no value for the model, no estimate"]
        assert not (tmp_path / (name + "_color5_model_result.txt")).exists()
        fitted = [ln.split(":")[0] for ln in r.stdout.splitlines() if ln.startswith("color ")]
        assert fitted[-1] == "color 70" and "color 5" not in fitted and (tmp_path / (name + "_color70_model_result.txt")).stat().st_size > 0


@pytest.mark.parametrize("what", ["cell", "fields", "sci"])
def test_refused_rows_are_named_as_the_host_names_them(what, tmp_path):
    tables, (words, kw) = dict(HAND), HAND_WORDS
    if what == "cell":
        tables["tricov"] = tables["tricov"].replace("\t0.3\t11\t", "\t-nan\t11\t")
    elif what == "fields":
        tables["pentacov"] += "1\t2\t3\t\n"
    else:
        tables, (words, kw) = HAND_SCI, SCI_WORDS
    prefix = str(tmp_path / "in")
    write_tables(prefix, tables)
    for source in ("cov", "fre"):
        r = sh(["model", "-f", prefix, "--filter-multi", words, "--source", source, "-u", "2", "-o", "one"], tmp_path)
        if what == "sci" and source == "fre":
            assert r.returncode == 0, r.stdout
            continue
        with pytest.raises(RuntimeError) as e:
            hostapi.filter_rows(source, read_tables(prefix), 0.0, multi=True, **kw)
        assert r.returncode != 0 and str(e.value) in r.stdout, (str(e.value), r.stdout)
        word = {"cell": "in line 2 of stream _tricov", "fields": "line 4 did not have 12 elements (stream _pentacov)", "sci": "row 10 of stream _bicov"}[what]
        assert word in r.stdout
        assert not (tmp_path / "one_model_result.txt").exists()


# ---- 5. a filter that goes away ----
def test_without_the_filter_the_colored_pass_is_as_ever(tmp_path):
    meta = load_case("col3_dip")
    out = tmp_path / "out"
    run = open_run(meta, tmp_path, out)
    run.set_model("fre", lo=1, hi=2)
    run.set_filter_multi(**ONE_COLOUR[1])
    run.find_superbubbles("g")
    run.ploidy_estimation("g", meta["cutoffs"])
    assert (out / "g_model_result.txt").exists() and len(run.model_values()) > 0
    os.remove(out / "g_model_result.txt")
    run.set_filter_multi(None)
    run.set_model(None)
    run.find_superbubbles("g")
    run.ploidy_estimation("g", meta["cutoffs"])
    assert not compare_outputs(os.path.join(meta["dir"], "expected"), str(out))
    assert not (out / "g_model_result.txt").exists() and len(run.model_values()) == 0
    with pytest.raises(Exception, match="model"):
        run.set_filter_multi(cramer=0.25)
    with pytest.raises(Exception, match="set_filter_multi"):
        run.set_model("fre")
        run.set_filter(simple=True)
    run.close()
