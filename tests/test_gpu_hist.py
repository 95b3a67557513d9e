"""K-HIST (pf_count_histogram, csrc/pf_hist.hip) against np.bincount, bit for bit; the rows of a database; the histogram / cutoffL -d /
cutoffU -d sub-commands; `--auto-cutoffs` end to end on the databases designed in test_hist_cpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare_outputs

import hist_cases as hc

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

from ploidyfrost_amd import hipapi, hostapi, synth  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
LDS_BINS = 4096          # pf::HIST_LDS_BINS
BLOCK_RECORDS = 1024     # a block's turn: 256 lanes x 4 counters
MAX_BINS = 1 << 20


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def expect(counts, lo, hi, n_bins):
    c = counts.astype(np.int64)
    c = c[(c >= lo) & (c <= hi)]
    return np.bincount(np.minimum(c, n_bins - 1), minlength=n_bins).astype(np.uint64)


def check(dev, counts, lo, hi, n_bins):
    got = dev.count_histogram(counts, lo, hi, n_bins)
    want = expect(counts, lo, hi, n_bins)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(got.sum()) == int(((counts.astype(np.int64) >= lo) & (counts.astype(np.int64) <= hi)).sum())
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, BLOCK_RECORDS - 1, BLOCK_RECORDS, BLOCK_RECORDS + 1, 3_000_001])
def test_sizes(dev, n):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 6000, size=n, dtype=np.uint32)   # both sides of the LDS range
    check(dev, counts, 0, 0xFFFFFFFF, 8192)


def test_all_equal(dev):
    n = 1 << 18
    for v in (20, LDS_BINS - 1, LDS_BINS, 70000):
        got = check(dev, np.full(n, v, dtype=np.uint32), 0, 0xFFFFFFFF, 1 << 17)
        assert got[v] == n


def test_all_distinct(dev):
    rng = np.random.default_rng(1)
    check(dev, rng.permutation(200_000).astype(np.uint32), 0, 0xFFFFFFFF, 200_000)


def test_half_one_value_half_uniform(dev):
    rng = np.random.default_rng(2)
    n = 400_001
    counts = rng.integers(0, LDS_BINS, size=n, dtype=np.uint32)
    counts[rng.permutation(n)[: n // 2]] = 1
    check(dev, counts, 0, 0xFFFFFFFF, LDS_BINS)


def test_around_the_lds_range(dev):
    rng = np.random.default_rng(3)
    counts = rng.choice(np.array([LDS_BINS - 2, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 0], dtype=np.uint32), size=100_003)
    for n_bins in (LDS_BINS + 2, LDS_BINS + 1, LDS_BINS, LDS_BINS - 1):
        check(dev, counts, 0, 0xFFFFFFFF, n_bins)


@pytest.mark.parametrize("n_bins", [1, 2, LDS_BINS, LDS_BINS + 1, MAX_BINS])
def test_bin_counts_and_the_clamp(dev, n_bins):
    rng = np.random.default_rng(n_bins)
    counts = rng.integers(0, 2 * n_bins + 2, size=70_001, dtype=np.uint32)
    counts[:9] = [n_bins - 1, n_bins, n_bins + 1, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFE, max(n_bins - 2, 0), n_bins - 1]
    got = check(dev, counts, 0, 0xFFFFFFFF, n_bins)
    assert got[n_bins - 1] == (counts >= n_bins - 1).sum()


def test_lo_and_hi(dev):
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 300, size=50_001, dtype=np.uint32)
    counts[::1000] = 0xFFFFFFFF
    check(dev, counts, 2, 250, 300)              # cut at both ends
    check(dev, counts, 2, 250, 100)              # ... with counts above the last bin clamped into it
    check(dev, counts, 7, 7, 300)
    check(dev, counts, 0xFFFFFFFF, 1 << 40, 16)  # hi beyond 32 bits
    check(dev, counts, 1 << 32, 1 << 40, 16)     # lo beyond 32 bits: nothing
    assert not check(dev, counts, 251, 250, 300).any()   # lo > hi: zeros


def test_host_and_device_pointers_and_repeats(dev):
    import torch
    rng = np.random.default_rng(6)
    counts = rng.integers(0, 9000, size=333_337, dtype=np.uint32)
    want = expect(counts, 3, 8000, 5000)
    a = dev.count_histogram(counts, 3, 8000, 5000)
    b = dev.count_histogram(counts, 3, 8000, 5000)
    assert np.array_equal(a, want) and np.array_equal(a, b)
    dc = torch.from_numpy(counts.view(np.int32)).cuda()
    c = dev.count_histogram(dc, 3, 8000, 5000)                       # device in, host out
    out = torch.full((5000,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # (torch fills on its own stream, the context counts on another)
    dev.count_histogram(dc, 3, 8000, 5000, out=out)                  # device in, device out (overwritten, not added to)
    dev.count_histogram(counts, 3, 8000, 5000, out=out)              # host in, device out
    assert np.array_equal(c, want) and np.array_equal(out.cpu().numpy().view(np.uint64), want)
    # a device pointer that is 4 but not 16 bytes aligned: the counters in front of the vector body
    for shift in (1, 2, 3):
        assert np.array_equal(dev.count_histogram(dc[shift:], 3, 8000, 5000), expect(counts[shift:], 3, 8000, 5000))


def test_bad_bin_counts_are_named(dev):
    counts = np.arange(10, dtype=np.uint32)
    for n_bins in (0, MAX_BINS + 1):
        with pytest.raises(hipapi.DeviceError) as e:
            dev.count_histogram(counts, 0, 100, n_bins)
        assert e.value.status == hipapi.PF_ERR_ARG and "pf_count_histogram" in str(e.value) and "bins" in str(e.value)


def test_kernel_is_timed_under_its_name(dev):
    assert dev.L.pf_kernel_name(hipapi.K_HIST) == b"k_hist" and hipapi.KERNELS[-1] == "k_call_model"
    dev.enable_timing(True)
    dev.reset_timing()
    dev.count_histogram(np.full(5000, 3, dtype=np.uint32), 0, 10, 16)
    ms, launches = dev.kernel_time(hipapi.K_HIST)
    dev.enable_timing(False)
    assert launches == 1 and ms > 0


# ---- the rows of a database ----

@pytest.mark.parametrize("layout,counter_size,min_count,max_count", [("kmc1", 1, 2, 200), ("kmc1", 2, 2, 3000), ("kmc1", 4, 2, 70000),
                                                                     ("kmc2", 2, 2, 3000), ("kmc1", 4, 1, 0xFFFFFFFF), ("kmc1", 2, 1, 65535)])
def test_database_rows(layout, counter_size, min_count, max_count, tmp_path):
    rng = np.random.default_rng(counter_size * 7 + min_count)
    k = 25
    kmers = np.unique(rng.integers(0, 1 << 50, size=30_000, dtype=np.uint64))
    top = (1 << (8 * counter_size)) - 1
    counts = np.minimum(rng.geometric(0.02, size=len(kmers)).astype(np.uint64) ** 2, top).astype(np.uint32)
    counts[:50] = 1                       # below min_count = 2
    counts[50:60] = min(top, 2_000_000)   # above max_count, and with 4-byte counters above the last row
    prefix = str(tmp_path / "db")
    write = synth.write_kmc1 if layout == "kmc1" else synth.write_kmc2
    write(prefix, kmers, counts, k, counter_size=counter_size, min_count=min_count, max_count=max_count)
    _, stored, meta = synth.read_kmc(prefix)
    assert (stored > min(max_count, top)).any() or max_count >= top
    mn, rows = hostapi.kmc_histogram(prefix)
    want = hc.db_rows(stored, meta, counter_size)
    assert mn == min_count and rows.dtype == np.uint64
    assert np.array_equal(rows, want)


# ---- the sub-commands ----

def run_cli(*a, cwd=None):
    return subprocess.run([CLI] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    pyoracle.build()
    d = tmp_path_factory.mktemp("auto_single")
    meta, prefix, counts = hc.make_single(d)
    lower, upper = hc.thresholds(counts)
    ref = d / "oracle"
    ref.mkdir()
    pyoracle.Oracle(meta["gfa"], prefix).run(str(ref), "g", z=int(meta["opts"]["-z"]), lower=lower, upper=upper)
    return dict(meta=meta, db=prefix, counts=counts, lower=lower, upper=upper, oracle=str(ref), dir=d)


def test_cli_histogram_feeds_the_file_forms(single, tmp_path):
    f = tmp_path / "hist.txt"
    r = run_cli("histogram", "-d", single["db"], "-o", f)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.bincount(single["counts"], minlength=65536)[1:]
    assert f.read_text() == "".join("%d\t%d\n" % (i + 1, c) for i, c in enumerate(rows))
    assert run_cli("histogram", "-d", single["db"]).stdout == f.read_text()
    for db_form, file_form in ((("cutoffL", "-d", single["db"]), ("cutoffL", f)), (("cutoffU", "-d", single["db"]), ("cutoffU", f)),
                               (("cutoffU", "-d", single["db"], "0.9"), ("cutoffU", f, "0.9"))):
        a, b = run_cli(*db_form), run_cli(*file_form)
        assert a.returncode == 0 and a.stdout == b.stdout and a.stdout, (db_form, a.stdout, b.stdout, a.stderr)
    assert run_cli("cutoffL", "-d", single["db"]).stdout == "%d\n" % single["lower"]
    assert run_cli("cutoffU", "-d", single["db"]).stdout == "%d\n" % single["upper"]
    assert run_cli("cutoffU", "-d", single["db"], "0.9").stdout == "%d" % hc.thresholds(single["counts"], 0.9)[1]
    assert "Usage:PloidyFrost cutoffU" in run_cli("cutoffU", "-d", single["db"], "1.5").stdout


# ---- --auto-cutoffs ----

def coverage_lines(text):
    return [int(x) for x in re.findall(r"(?:Minimum|Maximum) Coverage:(-?\d+)", text)]


def test_auto_cutoffs_single_sample(single, tmp_path):
    meta = single["meta"]
    base = ["-g", meta["gfa"], "-d", single["db"], "-o", "g", "-t", "1", "-z", meta["opts"]["-z"]]
    auto, explicit = tmp_path / "auto", tmp_path / "explicit"
    auto.mkdir()
    explicit.mkdir()
    a = run_cli(*base, "--auto-cutoffs", cwd=auto)
    assert a.returncode == 0, a.stdout + a.stderr
    assert coverage_lines(a.stdout) == [single["lower"], single["upper"]]
    e = run_cli(*base, "-l", single["lower"], "-u", single["upper"], cwd=explicit)
    assert e.returncode == 0, e.stdout + e.stderr
    assert not compare_outputs(single["oracle"], str(auto / "PloidyFrost_output"))
    assert not compare_outputs(str(explicit / "PloidyFrost_output"), str(auto / "PloidyFrost_output"))
    d = run_cli(*base, cwd=explicit)   # the defaults give other files: the switch did something
    assert d.returncode == 0 and compare_outputs(str(explicit / "PloidyFrost_output"), str(auto / "PloidyFrost_output"))
    # -q is the quantile, as for -h
    q = run_cli(*base, "--auto-cutoffs", "-q", "0.9", cwd=auto)
    assert q.returncode == 0 and coverage_lines(q.stdout) == list(hc.thresholds(single["counts"], 0.9))


def test_auto_cutoffs_with_model_and_filter(single, tmp_path):
    meta = single["meta"]
    base = ["-g", meta["gfa"], "-d", single["db"], "-o", "g", "-z", meta["opts"]["-z"], "--model", "fre", "--filter", "-S -n 6"]
    auto, explicit = tmp_path / "auto", tmp_path / "explicit"
    auto.mkdir()
    explicit.mkdir()
    a = run_cli(*base, "--auto-cutoffs", cwd=auto)
    e = run_cli(*base, "-l", single["lower"], "-u", single["upper"], cwd=explicit)
    assert a.returncode == e.returncode, a.stdout + a.stderr + e.stdout + e.stderr
    assert coverage_lines(a.stdout) == [single["lower"], single["upper"]]
    fa, fe = auto / "PloidyFrost_output" / "g_model_result.txt", explicit / "PloidyFrost_output" / "g_model_result.txt"
    assert fe.exists() == fa.exists() and a.returncode == 0, a.stdout + a.stderr
    assert fa.read_bytes() == fe.read_bytes() and fa.read_bytes()


def test_auto_cutoffs_colored(tmp_path):
    pyoracle.build()
    meta, prefixes, counts = hc.make_colored(tmp_path)
    pairs = [hc.thresholds(c) for c in counts]
    assert len(set(pairs)) == len(pairs)
    ref = tmp_path / "oracle"
    ref.mkdir()
    pyoracle.ColoredOracle(meta["gfa"], meta["colors_dump"], prefixes, str(tmp_path)).run(str(ref), "g", pairs, z=int(meta["opts"]["-z"]))
    lst, cfile = tmp_path / "dbs.txt", tmp_path / "cut.txt"
    lst.write_text("".join(p + "\n" for p in prefixes))
    cfile.write_text("".join("%d\t%d\n" % p for p in pairs))
    base = ["-g", meta["gfa"], "-f", meta["colors"], "-d", lst, "-o", "g", "-z", meta["opts"]["-z"]]
    auto, explicit = tmp_path / "auto", tmp_path / "explicit"
    auto.mkdir()
    explicit.mkdir()
    a = run_cli(*base, "--auto-cutoffs", cwd=auto)
    assert a.returncode == 0, a.stdout + a.stderr
    assert coverage_lines(a.stdout) == [x for p in pairs for x in p]
    e = run_cli(*base, "-C", cfile, cwd=explicit)
    assert e.returncode == 0, e.stdout + e.stderr
    assert not compare_outputs(str(ref), str(auto / "PloidyFrost_output"))
    assert not compare_outputs(str(explicit / "PloidyFrost_output"), str(auto / "PloidyFrost_output"))
    # the facade: the same pairs from the run's own databases
    run = hostapi.ColoredRun(meta["gfa"], meta["colors"], prefixes, str(tmp_path), z=int(meta["opts"]["-z"]))
    run.set_auto_cutoffs()
    assert run.cutoffs() == pairs
    run.close()


def test_auto_cutoffs_through_the_facade(single, tmp_path):
    meta = single["meta"]
    run = hostapi.Run(meta["gfa"], single["db"], z=int(meta["opts"]["-z"]))
    run.set_output_dir(str(tmp_path))
    run.set_auto_cutoffs()
    assert run.cutoffs() == (single["lower"], single["upper"])
    run.set_unitig_id("g")
    run.find_superbubbles("g")
    run.ploidy_estimation("g")   # its defaults 10 / 1000 are not what runs
    assert run.cutoffs() == (single["lower"], single["upper"])
    assert not compare_outputs(single["oracle"], str(tmp_path))
    run.set_auto_cutoffs(0.9)
    assert run.cutoffs() == hc.thresholds(single["counts"], 0.9)
    run.set_auto_cutoffs(None)
    run.close()
    assert hostapi.cutoffs_from_rows(np.bincount(single["counts"])[1:]) == (hc.ref_cutoff_l(np.bincount(single["counts"])[1:]), single["upper"])


@pytest.mark.parametrize("extra,word", [(["-h", "H"], "-h"), (["-C", "H"], "-C"), (["-l", "12"], "-l"), (["-u", "900"], "-u"), (["--gpus", "2"], "--gpus 2")])
def test_refusals(single, extra, word, tmp_path):
    hist = tmp_path / "h.txt"
    hist.write_text("1\t5\n2\t3\n3\t9\n")
    extra = [str(hist) if x == "H" else x for x in extra]
    r = run_cli("-g", single["meta"]["gfa"], "-d", single["db"], "-o", "g", "--auto-cutoffs", *extra, cwd=tmp_path)
    assert r.returncode != 0 and "--auto-cutoffs" in r.stderr and word in r.stderr
    assert not os.path.exists(tmp_path / "PloidyFrost_output")
