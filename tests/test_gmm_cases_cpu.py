"""The K-GMM edge cases of tests/gmm_cases.py checked without a GPU: three CPU evaluations of every fit -- the exact-sum reference
(math.fsum), the same code with numpy's sum over the reversed array, and the oracle's sequential C++ -- have to take the same
number of iterations, the cases have to reach what they are there for (a DBL_MIN guard, a refusal of the gate, the iteration
bound), and the CPU spread, the largest relative difference between the oracle and the exact sums, has to stay within what
gmm_cases.SPREAD records per group: the device's tolerance is 100 times that, so no change of the inputs widens it unnoticed."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402

import gmm_cases as gc  # noqa: E402

_oracle_fits = {}


def oracle_fit(case):
    if case.name not in _oracle_fits:
        o = pyoracle.GmmOracle()
        o.set_values(gc.values(case.input))
        _oracle_fits[case.name] = o.fit(case.g, **case.fit)
    return _oracle_fits[case.name]


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_three_cpu_fits_agree(name):
    case = gc.BY_NAME[name]
    x, o = gc.values(case.input), oracle_fit(case)
    if case.ref == "oracle":                      # g = 16 over a million values: the oracle alone (fsum would take a minute)
        assert o["iterations"] >= 1 and np.all(np.isfinite(o["vars"])) and np.isfinite(o["loglik"])
        return
    f = gc.reference(name)
    r = gc.reference_fit_with(gc.reversed_np_sum, x, case.g, **case.fit)
    assert f["iterations"] == r["iterations"] == o["iterations"], (f["iterations"], r["iterations"], o["iterations"])
    assert np.array_equal(f["means"], o["means"])
    d, d2 = gc.deviation(o, f, len(x)), gc.deviation(r, f, len(x))
    print("%s: n %d g %d iterations %d refused %s guards %s min var %.3g spread oracle %.3g reversed %.3g" % (
        name, len(x), case.g, f["iterations"], f["refused"], f["guards"], np.min(f["vars"]), gc.spread_of(d), gc.spread_of(d2)))
    assert gc.spread_of(d) <= gc.SPREAD[case.group], d
    assert gc.spread_of(d2) <= gc.SPREAD[case.group], d2


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.guard])
def test_guard_cases_reach_a_guard(name):
    f = gc.reference(name)
    h = f["guards"]
    assert np.min(f["vars"]) <= 1e-300 or h["rows"] + h["terms"] + h["vars"] > 0, (f["vars"], h)


@pytest.mark.parametrize("name", sorted(gc.REFUSALS))
def test_gate_cases_refuse_where_stated(name):
    f, want = gc.reference(name), gc.REFUSALS[name]
    assert f["refused"] == want, f["refused"]
    if want:                                      # frozen parameters repeat the log-likelihood: the fit ends with the refusal
        assert f["iterations"] == want[0]
    if want == [1]:
        assert np.all(f["vars"] == 0.01) and np.all(f["weights"] == 1 / gc.BY_NAME[name].g)
    if name == "gate_late":
        assert want[0] >= 2 and not np.any(f["vars"] == 0.01)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.group == "pairs"])
def test_pairs_cases_run_to_the_bound(name):
    assert gc.reference(name)["iterations"] == gc.BY_NAME[name].fit["max_iter"]


def test_tolerances_follow_the_spread():
    assert set(gc.TOL) == set(gc.SPREAD) == set(gc.GROUPS)
    for group in gc.GROUPS:
        assert gc.TOL[group] <= gc.CEILING
        assert gc.TOL[group] == gc.DEVICE_TOL.get(group, min(gc.CEILING, 100 * gc.SPREAD[group]))
