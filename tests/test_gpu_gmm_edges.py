"""K-GMM (ploidyfrost_amd/csrc/pf_gmm.hip: k_gmm_pass, k_gmm_update, pf_gmm_fit) at its edges, against the exact-sum reference of
tests/gmm_cases.py: g up to PF_GMM_MAX_GAUSS, the DBL_MIN guards, the grid cap, the 16-pair graph boundary, refused updates,
contexts used again, empty and NaN input, and the result file where variances are DBL_MIN.

Tolerance: gmm_cases.TOL, per group 100 times the spread of the CPU evaluations among themselves (tests/test_gmm_cases_cpu.py
measures and pins it), never more than 1e-9.  Iteration counts and means are compared exactly, NaN and infinity by place."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

from ploidyfrost_amd import hostapi  # noqa: E402

import gmm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
QUANTITIES = ("weights", "vars", "loglik", "aic")


def device_fit(case, model=None):
    """the fit of a case on a context of its own (or on `model`, whose values the caller has set)"""
    m = model or hostapi.Gmm()
    try:
        if model is None:
            m.set_values(gc.values(case.input))
        return m.fit(case.g, **case.fit)
    finally:
        if model is None:
            m.close()


def oracle_fit(x, g, **fit):
    o = pyoracle.GmmOracle()
    o.set_values(x)
    return o.fit(g, **fit)


def cpu_side(case):
    return gc.reference(case.name) if case.ref == "fsum" else oracle_fit(gc.values(case.input), case.g, **case.fit)


def same_bits(a, b):
    return (a["iterations"] == b["iterations"] and np.float64(a["loglik"]).tobytes() == np.float64(b["loglik"]).tobytes()
            and np.float64(a["aic"]).tobytes() == np.float64(b["aic"]).tobytes()
            and all(a[k].tobytes() == b[k].tobytes() for k in ("weights", "means", "vars")))


def check(case, got):
    want, n = cpu_side(case), len(gc.values(case.input))
    dev = gc.deviation(got, want, n)
    print("%s: iterations %d (reference %d) deviation %s tolerance %.1e" % (
        case.name, got["iterations"], want["iterations"], " ".join("%s %.3g" % (q, dev[q]) for q in QUANTITIES), gc.TOL[case.group]))
    assert got["iterations"] == want["iterations"], (case.name, "iterations", got["iterations"], want["iterations"])
    assert np.array_equal(got["means"], want["means"]), (case.name, "means")
    for q in QUANTITIES:
        assert dev[q] <= gc.TOL[case.group], (case.name, q, dev[q], got[q], want[q])


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_fit_matches_the_reference(name):
    case = gc.BY_NAME[name]
    check(case, device_fit(case))


def test_grid_cap_of_this_device():
    """n_blocks is capped at 4 blocks per CU: with 256 CUs the `sizes` cases 1 048 576 and 1 048 577 sit on the cap; another CU
    count gets its own neighbours"""
    import torch
    cap = 4 * torch.cuda.get_device_properties(0).multi_processor_count * 1024
    for n in () if cap == 1_048_576 else (cap - 1, cap, cap + 1):
        case = gc.size_case(n)
        check(case, device_fit(case))


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.group in ("guards", "gate")])
def test_fitting_twice_gives_the_same_bits(name):
    case = gc.BY_NAME[name]
    m = hostapi.Gmm()
    m.set_values(gc.values(case.input))
    a, b = device_fit(case, m), device_fit(case, m)
    m.close()
    assert same_bits(a, b), (a, b)


def test_context_used_again_for_another_g():
    """g = 16, then 2, then 16 on one context: the columns of the partials that the narrow fit leaves stale must not count"""
    cases = [gc.BY_NAME[n] for n in ("sweep_g16", "sweep_g2", "sweep_g16")]
    m = hostapi.Gmm()
    m.set_values(gc.values("sweep"))
    again = [device_fit(c, m) for c in cases]
    m.close()
    for c, got in zip(cases, again):
        assert same_bits(got, device_fit(c)), c.name


def test_context_used_again_for_another_size():
    """1 048 577 values, then 257, then 1 048 577 on one context: the workspaces are kept, the block count is not"""
    cases = [gc.BY_NAME[n] for n in ("size1048577_g3", "size257_g3", "size1048577_g3")]
    m = hostapi.Gmm()
    again = []
    for c in cases:
        m.set_values(gc.values(c.input))
        again.append(device_fit(c, m))
    m.close()
    for c, got in zip(cases[:2], again[:2]):
        assert same_bits(got, device_fit(c)), c.name
    assert same_bits(again[0], again[2])


@pytest.mark.parametrize("g", [3, 2])
@pytest.mark.parametrize("kind", ["empty", "nan"])
def test_empty_and_nan_input(kind, g):
    """No values, or a NaN among them: the product returns what the reference computes and raises nothing.  The reference
    goes through one update that turns every weight and variance into NaN (0 / 0, or NaN sums), sees a log-likelihood
    difference of 0 or NaN, stops after that one iteration and prints the NaN parameters, a log-likelihood of 0 or NaN and an
    AIC of inf or NaN into its result file before it goes on to the next ploidy; pfh_gmm_run can print the same lines only if
    the fit hands these values back, so that is what is asserted."""
    x = np.array([]) if kind == "empty" else np.array([0.2, np.nan, 0.5])
    want = oracle_fit(x, g)
    assert want["iterations"] == 1 and np.all(np.isnan(want["weights"])) and np.all(np.isnan(want["vars"]))
    m = hostapi.Gmm()
    m.set_values(x)
    got = m.fit(g)
    m.close()
    assert got["iterations"] == 1
    assert np.all(np.isnan(got["weights"])) and np.all(np.isnan(got["vars"])) and np.array_equal(got["means"], want["means"])
    if kind == "empty":
        assert want["loglik"] == 0.0 and want["aic"] == np.inf
        assert got["loglik"] == 0.0 and got["aic"] == np.inf
    else:
        assert np.isnan(want["loglik"]) and np.isnan(want["aic"])
        assert np.isnan(got["loglik"]) and np.isnan(got["aic"])


@pytest.mark.parametrize("key, hi", [("on_means", 9), ("ratios", 5)])
def test_result_file_where_variances_are_dbl_min(key, hi, tmp_path):
    """run() end to end: ploidy 2 .. 10 over values that sit on the means (variances end at DBL_MIN, printed 2.22507e-308, and
    the winning ploidy is picked among such fits) and ploidy 2 .. 6 over exact ratios (78 iterations at most; g = 6 .. 9 take up
    to 152); the file equals the oracle's as text"""
    x = gc.values(key)
    o, m = pyoracle.GmmOracle(), hostapi.Gmm()
    o.set_values(x)
    m.set_values(x)
    o.run(str(tmp_path / "cpu"), hi=hi)
    m.run(str(tmp_path / "gpu"), hi=hi)
    m.close()
    with open(tmp_path / "gpu_model_result.txt") as got, open(tmp_path / "cpu_model_result.txt") as want:
        got, want = got.read(), want.read()
    if key == "on_means":
        assert "2.22507e-308" in want
    assert got == want
