"""The host side of the allele-frequency density table, no device: the plain column reader behind `ploidyfrost density` (what
script/Drawfreq.R's read.table makes of its -f file), the writer of <prefix>_allele_frequency_density.txt, and every refusal the
command line makes before anything is read or written."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case

from ploidyfrost_amd import build, hipapi, hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


def test_read_column_skips_blank_and_comment_lines(tmp_path):
    f = tmp_path / "col.txt"
    f.write_text("# a comment\n0.25\n\n  \n1e-3\n.5\n  # another\n-2\t\n 7 \n0.75")
    m = hostapi.Gmm()
    m.read_column(str(f))
    assert np.array_equal(m.values(), [0.25, 1e-3, 0.5, -2.0, 7.0, 0.75])   # no frequency test, no doubled last value
    m.close()


@pytest.mark.parametrize("bad", ["0.5x", "nan", "inf", "-inf", "0.1 0.2", "0.1\t0.2", "x"])
def test_read_column_refuses_with_the_line_number(bad, tmp_path):
    f = tmp_path / "col.txt"
    f.write_text("0.25\n# c\n\n%s\n0.5\n" % bad)
    m = hostapi.Gmm()
    with pytest.raises(RuntimeError, match="line 4 of"):
        m.read_column(str(f))
    assert len(m.values()) == 0
    with pytest.raises(RuntimeError, match="open column file"):
        m.read_column(str(tmp_path / "absent.txt"))
    m.close()


def test_writer_round_trips_doubles(tmp_path):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.random(60), [0.1, 1 / 3, 1e-310, 5e-324, 1.7976931348623157e308, -0.0, 2.0 ** -1022, np.nextafter(1.0, 2.0)]])
    d = np.concatenate([rng.random(60) * 1e-300, rng.random(8) * 1e300])
    bw = float(np.nextafter(0.0123456789, 1.0))
    m = hostapi.Gmm()
    name = m.write_density(str(tmp_path / "w"), {"x": x, "density": d, "n": 12345678901, "bw": bw})
    m.close()
    assert name == str(tmp_path / "w_allele_frequency_density.txt")
    lines = open(name).read().splitlines()
    head = lines[0].split()
    assert head[:2] == ["#", "values"] and int(head[2]) == 12345678901 and head[3] == "bandwidth" and float(head[4]) == bw
    assert head[5] == "points" and int(head[6]) == len(x) == len(lines) - 1
    cols = [ln.split("\t") for ln in lines[1:]]
    assert all(len(c) == 2 for c in cols)
    gx, gd = np.array([float(c[0]) for c in cols]), np.array([float(c[1]) for c in cols])
    assert np.array_equal(gx.view(np.uint64), x.view(np.uint64)) and np.array_equal(gd.view(np.uint64), d.view(np.uint64))
    assert np.array_equal(np.loadtxt(name), np.stack([x, d], axis=1))   # the comment is skipped by a plain reader


def test_density_needs_no_device_to_refuse():
    m = hostapi.Gmm()
    m.set_values([0.5])
    with pytest.raises(RuntimeError, match="need at least 2 data points"):
        m.density()
    m.set_values([0.25, 0.5, 0.75])
    for kw in (dict(points=1), dict(points=4097), dict(adjust=0.0), dict(adjust=-1.0), dict(adjust=float("nan")), dict(adjust=float("inf"))):
        with pytest.raises(RuntimeError):
            m.density(**kw)
    m.close()


def test_new_entry_points_are_declared():
    assert "pf_gmm_density" in hipapi.DECLARED_SYMBOLS and hipapi.K_DENSITY == len(hipapi.KERNELS)
    import ctypes as C
    L = hipapi.load_library()
    L.pf_kernel_name.restype = C.c_char_p
    assert L.pf_kernel_name(hipapi.K_DENSITY) == b"k_density"
    for s in ("pfh_gmm_read_column", "pfh_gmm_density", "pfh_gmm_write_density", "pfh_set_density", "pfh_model_density", "pfh_model_color_density"):
        assert s in hostapi.DECLARED_SYMBOLS
    for name in ("set_density", "model_density"):
        assert callable(getattr(hostapi.Run, name)) and callable(getattr(hostapi.ColoredRun, name))


def one_command(extra):
    meta = load_case("tet60k")
    return ["-g", meta["gfa"], "-d", meta["db"], "-o", "g"] + meta["args"] + extra


def model_command(extra):
    meta = load_case("tet60k")
    return ["model", "-g", os.path.join(meta["dir"], "expected", "g_allele_frequency.txt"), "-o", "m"] + extra


def density_command(extra):
    meta = load_case("tet60k")
    return ["density", "-f", os.path.join(meta["dir"], "expected", "g_allele_frequency.txt"), "-o", "d"] + extra


REFUSALS = [
    (one_command, ["--density"], "--model"),
    (one_command, ["--density", "-f", "graph.bfg_colors", "--model", "fre"], "--model"),
    (one_command, ["--model", "fre", "--density-points", "64"], "--density"),
    (one_command, ["--model", "fre", "--density-adjust", "2"], "--density"),
    (one_command, ["--model", "fre", "--density", "--density-points", "1"], "--density-points 1"),
    (one_command, ["--model", "fre", "--density", "--density-points", "4097"], "--density-points 4097"),
    (one_command, ["--model", "fre", "--density", "--density-points", "12x"], "--density-points 12x"),
    (one_command, ["--model", "fre", "--density", "--density-adjust", "0"], "--density-adjust 0"),
    (one_command, ["--model", "fre", "--density", "--density-adjust", "-1"], "--density-adjust -1"),
    (one_command, ["--model", "fre", "--density", "--density-adjust", "nan"], "--density-adjust nan"),
    (one_command, ["--model", "fre", "--density", "--density-adjust", "inf"], "--density-adjust inf"),
    (model_command, ["--density-points", "64"], "--density"),
    (model_command, ["--density-adjust", "2"], "--density"),
    (model_command, ["--density", "--density-points", "1"], "--density-points 1"),
    (model_command, ["--density", "--density-points", "4097"], "--density-points 4097"),
    (model_command, ["--density", "--density-adjust", "0"], "--density-adjust 0"),
    (model_command, ["--density", "--density-adjust", "nan"], "--density-adjust nan"),
    (density_command, ["-n", "1"], "-n 1"),
    (density_command, ["-n", "4097"], "-n 4097"),
    (density_command, ["-a", "0"], "-a 0"),
    (density_command, ["-a", "-1"], "-a -1"),
    (density_command, ["-a", "nan"], "-a nan"),
]


@pytest.mark.parametrize("command,extra,word", REFUSALS, ids=["%s %s" % (c.__name__, " ".join(e)) for c, e, _ in REFUSALS])
def test_refusals_come_before_anything_is_read_or_written(command, extra, word, tmp_path):
    r = subprocess.run([CLI] + command(extra), cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0, (r.stdout, r.stderr)
    assert r.stderr.startswith("Error:") and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert os.listdir(tmp_path) == []


def test_density_subcommand_says_how_it_is_used(tmp_path):
    r = subprocess.run([CLI, "density"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "Usage: PloidyFrost density" in r.stdout and "-f" in r.stdout and "-n" in r.stdout and "-a" in r.stdout
    r = subprocess.run([CLI], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "Usage: PloidyFrost density" in r.stdout and "--density" in r.stdout and "--density-points" in r.stdout
    r = subprocess.run([CLI, "density", "-f", str(tmp_path / "absent.txt")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "absent.txt" in r.stderr and os.listdir(tmp_path) == []
    r = subprocess.run([CLI, "model"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "--density" in r.stdout
