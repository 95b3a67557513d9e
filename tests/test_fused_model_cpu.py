"""The model fed from the resident call streams, the part that needs no GPU: the shared row rule (csrc/pf_model_rows.hpp -- the code
the kernels of pf_call_model.hip run with a lane per row, exported as pfh_model_rows) against the file readers of `PloidyFrost
model` (hostapi.Gmm().read_cov / read_fre, held to the reference by test_model_cpu.py) on crafted text, and the new entry points
in both headers."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from ploidyfrost_amd import build, hipapi, hostapi


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def reader_cov(tmp_path, bi, tri, tetra, penta=b"", q=0.0):
    p = str(tmp_path / "c")
    for suf, data in (("bi", bi), ("tri", tri), ("tetra", tetra), ("penta", penta)):
        with open(p + "_%scov.txt" % suf, "wb") as f:
            f.write(data)
    m = hostapi.Gmm()
    m.read_cov(p, q)
    return m.values()


def reader_fre(tmp_path, data, q=0.0):
    p = str(tmp_path / "f.txt")
    with open(p, "wb") as f:
        f.write(data)
    m = hostapi.Gmm()
    m.read_fre(p, q)
    return m.values()


TAIL = b"0\t0\t7\t3\t12\t\n"
BI = b"".join([
    b"60.2174\t30.5\t" + TAIL,          # atoi: 60, 30
    b"1e+06\t3\t" + TAIL,               # atoi("1e+06") = 1
    b"0.000123\t9999.5\t" + TAIL,       # 0 and 9999: sum 9999 is kept ...
    b"1\t9999.5\t" + TAIL,              # ... sum 10000 is skipped
    b"12\n",                            # too few tabs
    b"5\t\n",                           # one tab only
    b"\t7\t3\t" + TAIL,                 # an empty field: atoi skips the tab and reads the next number (7, 7)
    b"40\t0\t" + TAIL,                  # one allele holds every read: 40 / 40 = 1
])
TRI = b"".join([
    b"30\t20\t10\t" + TAIL,
    b"10\t20\t5\t" + TAIL,              # neighbour pairs: lead = 5
    b"5\t20\t10\t" + TAIL,              # lead = 10, not the minimum 5
    b"7\t8\n",                          # too few tabs
    b"0\t0\t9\t" + TAIL,
])
TETRA = b"".join([
    b"40\t30\t20\t10\t" + TAIL,
    b"10\t40\t20\t30\t" + TAIL,         # 40 > 20 -> lead 20, then 30 > 20: stays 20
    b"2500\t2500\t2500\t2499\t" + TAIL,
    b"2500\t2500\t2500\t2500\t" + TAIL,  # 10000: skipped
])
PENTA = b"1\t2\t3\t4\t5\t" + TAIL * 3  # never read


@pytest.mark.parametrize("q", [0.0, 0.05, 0.2])
def test_cov_rows_match_the_file_reader(tmp_path, q):
    exp = reader_cov(tmp_path, BI, TRI, TETRA, PENTA, q)
    got = hostapi.model_rows("cov", [BI, TRI, TETRA], q)
    assert np.array_equal(got, exp)
    if q == 0.0:
        # by hand: rows of bi kept at q = 0 (the integer quotient is 0 or 1, both inside [0, 1])
        assert list(got[:6]) == [60 / 90, 30 / 90, 1 / 4, 3 / 4, 0 / 9999, 9999 / 9999]
    else:
        assert len(got) == 0   # the integer quotient is 0 or 1: no row passes a test with 0 < q < 0.5


def test_cov_last_row_without_line_feed_and_empty_streams(tmp_path):
    bi = b"3\t4\t" + TAIL + b"8\t2\t0\t"
    assert np.array_equal(hostapi.model_rows("cov", [bi, b"", b""], 0.0), reader_cov(tmp_path, bi, b"", b""))
    assert len(hostapi.model_rows("cov", [b"", b"", b""], 0.0)) == 0


def test_cov_row_summing_to_zero_is_the_readers_error(tmp_path):
    bi = b"3\t4\t" + TAIL + b"0.4\t0.9\t" + TAIL
    with pytest.raises(RuntimeError, match="sums to 0"):
        reader_cov(tmp_path, bi, b"", b"")
    with pytest.raises(RuntimeError, match=r"row 2 of stream _bicov sums to 0"):
        hostapi.model_rows("cov", [bi, b"", b""], 0.0)
    with pytest.raises(RuntimeError, match=r"row 1 of stream _tricov sums to 0"):
        hostapi.model_rows("cov", [b"3\t4\t" + TAIL, b"0\t0\t0\t" + TAIL, b""], 0.0)


FRE = b"1\n0\n1e-05\n0.333333\n0.5\n0.25\n0.75\n0.0499999\n0.05\n0.95\n0.950001\n"


@pytest.mark.parametrize("q", [0.0, 0.05, 0.3])
def test_fre_rows_match_the_file_reader(tmp_path, q):
    exp = reader_fre(tmp_path, FRE, q)
    got = hostapi.model_rows("fre", FRE, q)
    assert np.array_equal(got, exp)


def test_fre_last_token_counts_twice_when_kept_and_only_then(tmp_path):
    kept, dropped = b"0.25\n0.4\n", b"0.25\n0.01\n"
    a = hostapi.model_rows("fre", kept, 0.05)
    assert list(a) == [0.25, 0.4, 0.4] and np.array_equal(a, reader_fre(tmp_path, kept, 0.05))
    b = hostapi.model_rows("fre", dropped, 0.05)
    assert list(b) == [0.25] and np.array_equal(b, reader_fre(tmp_path, dropped, 0.05))
    # a file that does not end in white space: the last read meets the end of the file and nothing is counted again
    c = hostapi.model_rows("fre", b"0.25\n0.4", 0.05)
    assert list(c) == [0.25, 0.4] and np.array_equal(c, reader_fre(tmp_path, b"0.25\n0.4", 0.05))


@pytest.mark.parametrize("token", [b"nan", b"-nan", b"inf", b"x"])
def test_fre_token_that_is_no_number_is_the_readers_error(tmp_path, token):
    data = b"0.5\n" + token + b"\n0.25\n"
    with pytest.raises(RuntimeError, match="not a number"):
        reader_fre(tmp_path, data)
    with pytest.raises(RuntimeError, match=r"row 2 of stream _allele_frequency holds something that is not a number"):
        hostapi.model_rows("fre", data)


def test_fre_number_outside_the_exact_range_is_named_not_approximated():
    for token in (b"1e-30", b"1e+40", b"0.1234567890123456"):
        with pytest.raises(RuntimeError, match="converts exactly"):
            hostapi.model_rows("fre", b"0.5\n" + token + b"\n")


def test_g_printed_doubles_convert_bit_for_bit():
    rng = np.random.default_rng(20261017)
    # (0, 1]: uniform, and log-uniform down to 1e-12 -- six digits and that exponent stay inside the 22 decimal places one fp64
    # division converts exactly; a frequency is a ratio of coverages below 10^4 k-mer counts, so nothing smaller is ever printed,
    # and what lies beyond is refused by name (the test above), never approximated
    small = np.concatenate([rng.uniform(0.0, 1.0, 12000), 10.0 ** rng.uniform(-12.0, 0.0, 4000), [1.0, 1e-05, 0.000123, 0.333333]])
    small = small[small > 0]
    large = np.concatenate([rng.uniform(1.0, 1e4, 12000), [1.0, 9999.5, 9999.99, 1234.5]])
    for x in (small, large):
        tokens = ["%g" % v for v in x]
        exp = np.array([float(t) for t in tokens], dtype=np.float64)
        # q far below 0: every token is kept; the text does not end in a line feed, so no token counts twice
        got = hostapi.model_rows("fre", "\n".join(tokens).encode(), -1e12)
        assert len(got) == len(exp) >= 10000
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))


def test_fixture_files_give_the_readers_arrays():
    """the committed result files of two fixtures, both sources"""
    for case in ("hex30k", "tet60k"):
        pre = os.path.join(GOLDEN, case, "expected", "g")
        for q in (0.0, 0.05):
            m = hostapi.Gmm()
            m.read_cov(pre, q)
            texts = [open(pre + "_%scov.txt" % a, "rb").read() for a in ("bi", "tri", "tetra")]
            assert np.array_equal(hostapi.model_rows("cov", texts, q), m.values())
            m = hostapi.Gmm()
            m.read_fre(pre + "_allele_frequency.txt", q)
            assert np.array_equal(hostapi.model_rows("fre", open(pre + "_allele_frequency.txt", "rb").read(), q), m.values())


# ---- ABI ------------------------------------------------------------------------------------------------------------------------

def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pfh?_[a-z_0-9]+)\s*\(", text))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (pfh?_[a-z_0-9]+)$", out, flags=re.M))


def test_new_entry_points_are_declared_and_exported():
    dev = {"pf_call_model_begin", "pf_call_model_take", "pf_call_model_finish", "pf_gmm_values", "pf_call_fetched_bytes"}
    host = {"pfh_set_model", "pfh_model_values", "pfh_model_fit", "pfh_model_ploidy", "pfh_text_bytes_fetched", "pfh_model_rows"}
    assert dev <= declared("ploidyfrost_hip.h") and dev <= exported(hipapi.LIB_PATH) and dev <= set(hipapi.DECLARED_SYMBOLS)
    assert host <= declared("ploidyfrost_host.h") and host <= exported(hostapi.LIB_PATH) and host <= set(hostapi.DECLARED_SYMBOLS)
    L = hipapi.load_library()
    assert hipapi.KERNELS[-1] == "k_call_model"
    L.pf_kernel_name.restype = __import__("ctypes").c_char_p
    assert L.pf_kernel_name(len(hipapi.KERNELS) - 1) == b"k_call_model"
    for name in ("set_model", "model_values", "model_result", "text_bytes_fetched"):
        assert callable(getattr(hostapi.Run, name))


def test_cli_usage_lists_the_model_options():
    cli = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
    out = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    for opt in ("--model cov|fre", "--model-ploidy", "--model-q", "--model-m", "--model-iter", "--model-delta", "--model-only"):
        assert opt in out, opt


@pytest.mark.parametrize("extra,word", [
    (["--model", "cov", "-f", "colors.bfg_colors"], "--model"),
    (["--model", "cov", "--gpus", "2"], "--gpus"),
    (["--model", "both"], "--model both"),
    (["--model", "cov", "--model-ploidy", "0:3"], "--model-ploidy"),
    (["--model", "fre", "--model-ploidy", "1:17"], "--model-ploidy"),
    (["--model-only"], "--model"),
])
def test_cli_refuses_before_anything_is_written(tmp_path, extra, word):
    """status 1 and one line naming the option -- decided before the graph is read, so no GPU is needed to see it"""
    cli = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
    case = os.path.join(GOLDEN, "tet60k")
    r = subprocess.run([cli, "-g", os.path.join(case, "graph.gfa"), "-d", os.path.join(case, "db"), "-o", "g"] + extra,
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error:") and word in lines[0], r.stderr
    assert os.listdir(tmp_path) == []
