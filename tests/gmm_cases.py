"""K-GMM (ploidyfrost_amd/csrc/pf_gmm.hip) edge cases and an exact-sum reference of the fit, for tests/test_gmm_cases_cpu.py and
tests/test_gpu_gmm_edges.py.  Nothing here comes from the product or from oracle/: plain numpy float64 and math.fsum.

The fit is the EM of `PloidyFrost model`: g Gaussians with FIXED means i/(g+1), weights 1/g and variances 0.01 to start with.
One pass over the values gives the log-likelihood of the current parameters and the sums of the update.  The elementwise
operations are doubles in the product's order; every sum over the values goes through `sumfn`, math.fsum (exactly rounded)
for the reference proper.  The other summation orders -- numpy's pairwise sum over the reversed array here, the oracle's
sequential sum, the device's tree -- differ from it by their rounding alone, and that is what the tolerances below measure."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308


def _fsum(a):
    return math.fsum(a.tolist())


def reversed_np_sum(a):
    """a second summation order for the CPU test: numpy's pairwise sum, over the array back to front"""
    return float(np.sum(a[::-1]))


def _one_pass(x, w, mean, var, sumfn, hits):
    """log-likelihood of (w, mean, var), and a function that takes the sums of the update from the same pass: gs[i], vs[i], total
    (the last pass of a fit needs its log-likelihood only)"""
    g = len(w)
    with np.errstate(all="ignore"):
        inv = 1 / np.sqrt(2 * np.pi * var)
        d = x[:, None] - mean[None, :]
        dd = d * d
        q = w[None, :] * (inv[None, :] * np.exp(-(dd / (2 * var)[None, :])))
        plain = np.zeros(len(x))
        for i in range(g):                       # the row sum in index order, as a loop over the Gaussians adds it
            plain = plain + q[:, i]
        zero_row = plain == 0.0
        plain = np.where(zero_row, DBL_MIN, plain)     # the log-likelihood guards the row sum only
        ll = sumfn(np.log(plain))
        zero_term = q == 0.0
        p = np.where(zero_term, DBL_MIN, q)            # the E-step guards every term
        rowsum = np.zeros(len(x))
        for i in range(g):
            rowsum = rowsum + p[:, i]
        r = p / rowsum[:, None]
    hits["rows"] += int(zero_row.sum())
    hits["terms"] += int(zero_term.sum())

    def sums():
        with np.errstate(all="ignore"):
            gs = np.array([sumfn(r[:, i]) for i in range(g)], dtype=np.float64)
            vs = np.array([sumfn(r[:, i] * dd[:, i]) for i in range(g)], dtype=np.float64)
            return gs, vs, np.float64(sumfn(r.ravel()))
    return ll, sums


def reference_fit_with(sumfn, x, g, m_thre=5, n_thre=2, max_iter=1000, max_delta=0.01):
    """the fit with every sum over the values taken by sumfn(array) -> float.  Returns weights, means, vars, loglik, aic,
    iterations, refused (the iterations, counted from 1, whose update the gate refused) and guards: how many row sums and
    terms were replaced by DBL_MIN over all passes, how many variances by the updates."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = int(g)
    mean = np.array([i / (g + 1) for i in range(1, g + 1)], dtype=np.float64)
    w = np.full(g, 1 / g, dtype=np.float64)
    var = np.full(g, 0.01, dtype=np.float64)
    hits = {"rows": 0, "terms": 0, "vars": 0}
    refused = []
    ll, sums = _one_pass(x, w, mean, var, sumfn, hits)
    delta, count = DBL_MAX, 0
    while delta > max_delta and count < max_iter:
        gs, vs, total = sums()
        with np.errstate(all="ignore"):
            nv = 1 / gs * vs
            nw = gs / total
        zero_var = nv == 0.0
        nv = np.where(zero_var, DBL_MIN, nv)
        mx = mn = nw[0]
        for i in range(1, g):
            if mx < nw[i]:
                mx = nw[i]
            if nw[i] < mn:
                mn = nw[i]
        accept = True
        if mx != nw[0] and mx != nw[g - 1]:
            if mn < 1 / g / m_thre or mn < mx / g / n_thre:
                accept = False
        if accept:
            var, w = nv, nw
            hits["vars"] += int(zero_var.sum())
        else:
            refused.append(count + 1)
        last = ll
        ll, sums = _one_pass(x, w, mean, var, sumfn, hits)
        delta = ll - last
        count += 1
    with np.errstate(all="ignore"):
        aic = float((2 * (np.float64(g) * 2 - 1) - 2 * np.float64(ll)) / np.float64(len(x)))
    return {"weights": w, "means": mean, "vars": var, "loglik": float(ll), "aic": aic, "iterations": count, "refused": refused,
            "guards": hits}


def reference_fit(x, g, m_thre=5, n_thre=2, max_iter=1000, max_delta=0.01):
    """the high-precision side: every sum over the values is math.fsum"""
    return reference_fit_with(_fsum, x, g, m_thre, n_thre, max_iter, max_delta)


def mix(seed, n, comps, sd):
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(rng.choice(np.asarray(comps, dtype=np.float64), size=n), sd), 0.0, 1.0)


# ---- the cases -------------------------------------------------------------------------------------------------------------
# name, group, a key of INPUTS, g, the fit's keyword arguments, which CPU side the device is held to ("fsum" or "oracle":
# the oracle alone where fsum would take too long), and whether the case has to reach a DBL_MIN guard
Case = namedtuple("Case", "name group input g fit ref guard")

THREE = [0.25, 0.5, 0.75]
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 262_145, 1_048_576, 1_048_577, 2_500_003)

INPUTS = {
    "sweep": lambda: mix(11, 4099, [1 / 6, 2 / 6, 3 / 6, 4 / 6, 5 / 6], 0.02),
    "half1000": lambda: np.array([0.5] * 1000),
    "quarter1000": lambda: np.array([0.25] * 1000),
    "half10": lambda: np.array([0.5] * 10),
    "on_means": lambda: np.array([0.25] * 300 + [0.5] * 500 + [0.75] * 200),
    "stray": lambda: np.array([0.25] * 1600 + [0.5] * 1600 + [0.75] * 1600 + [0.6]),
    "thirds": lambda: np.array([1 / 3, 2 / 3] * 50),
    "ends": lambda: np.array([0.0, 1.0] * 100 + [0.5] * 5),
    "single": lambda: np.array([0.37]),
    "single_on_mean": lambda: np.array([0.2]),
    "ratios": lambda: np.array([a / (a + b) for a in range(1, 40) for b in range(1, 40)]),
    "ends_mix": lambda: np.concatenate([np.zeros(50), np.ones(50), mix(12, 2000, THREE, 0.03)]),
    "ends_mix_narrow": lambda: np.concatenate([np.zeros(50), np.ones(50), mix(12, 2000, THREE, 0.01)]),
    "narrow3": lambda: mix(13, 3000, THREE, 1e-4),
    "narrow4": lambda: mix(14, 3000, [0.2, 0.4, 0.6, 0.8], 1e-6),
    "off_mean": lambda: mix(15, 3000, [0.3], 1e-5),
    "one_peak": lambda: mix(16, 3000, [0.5], 0.02),
    "pairs": lambda: mix(17, 5000, THREE, 0.04),
}
for _n in SIZES:
    INPUTS["size%d" % _n] = (lambda n: lambda: mix(18, n, THREE, 0.04))(_n)


def _late_refusal_input():
    """A strong middle peak, a weak left one (8 %) and 30 % on the right, sd 0.06.  Found by a search with reference_fit over
    left shares 2..8 %, right shares 10..30 % and sd 0.02..0.06 and kept as found: the broad start (variance 0.01) hands the
    left Gaussian more than 1 / (3 * 5) at first, two updates are accepted, and the third, with the largest weight in the
    middle and the left weight under a sixth of it, is refused."""
    rng = np.random.default_rng(21)
    centres = np.concatenate([np.full(160, 0.25), np.full(1240, 0.5), np.full(600, 0.75)])
    return np.clip(rng.normal(centres, 0.06), 0.0, 1.0)


INPUTS["gate_late"] = _late_refusal_input
LATE_REFUSED = 3                # the iteration whose update the gate refuses, after two accepted ones


@lru_cache(maxsize=None)
def values(key):
    """the input of a case; made once, never written to"""
    v = INPUTS[key]()
    v.setflags(write=False)
    return v


def _cases():
    out = []
    for g in range(1, 17):
        out.append(Case("sweep_g%d" % g, "g_sweep", "sweep", g, dict(max_iter=60), "fsum", False))
    for g in (1, 2, 5, 16):
        for k in (1, 0):
            out.append(Case("sweep_g%d_iter%d" % (g, k), "g_sweep", "sweep", g, dict(max_iter=k), "fsum", False))
    # Three inputs of the first list reach no guard: [0.5] * 1000 at g = 3 and [0.37] at g = 4 put the largest weight on an inner
    # Gaussian and the smallest under the thresholds, so the gate refuses the first update and the variances stay 0.01; with
    # sd = 0.03 the zeros and ones of the last mixture never underflow a term.  Each is replaced by one of its kind that does
    # ([0.25] * 1000: the largest weight is the first, the gate does not apply; [0.2]: one value on the first mean; sd = 0.01),
    # and the three stay in the suite: two as refusals in `gate`, one here as an input that holds exact 0.0 and 1.0.
    # `stray` is added for the guard of the row sum, which none of the listed inputs reaches: 1600 values on every mean and one
    # value on none.  A Gaussian that holds the stray value alone gets the variance d^2 / gs, so the value's own term is
    # inv * exp(-gs / 2), which underflows for gs > 1490: every term of its row ends as 0.
    for name, key, g, guard in (("quarter1000_g3", "quarter1000", 3, True), ("half10_g1", "half10", 1, True),
                                ("on_means_g3", "on_means", 3, True), ("thirds_g2", "thirds", 2, True), ("stray_g3", "stray", 3, True),
                                ("ends_g3", "ends", 3, True), ("single_on_mean_g4", "single_on_mean", 4, True),
                                ("ratios_g3", "ratios", 3, False), ("ratios_g5", "ratios", 5, False),
                                ("ends_mix_narrow_g3", "ends_mix_narrow", 3, True), ("ends_mix_g3", "ends_mix", 3, False),
                                ("narrow3_g3", "narrow3", 3, True), ("narrow4_g4", "narrow4", 4, True),
                                ("off_mean_g3", "off_mean", 3, False)):
        out.append(Case(name, "guards", key, g, {}, "fsum", guard))
    out.append(Case("gate_first_step", "gate", "one_peak", 3, {}, "fsum", False))
    out.append(Case("gate_half1000_g3", "gate", "half1000", 3, {}, "fsum", False))
    out.append(Case("gate_single_g4", "gate", "single", 4, {}, "fsum", False))
    out.append(Case("gate_late", "gate", "gate_late", 3, {}, "fsum", False))
    out.append(Case("gate_thresholds_1_1", "gate", "sweep", 5, dict(m_thre=1, n_thre=1), "fsum", False))
    out.append(Case("gate_thresholds_50_20", "gate", "sweep", 5, dict(m_thre=50, n_thre=20), "fsum", False))
    for k in (1, 15, 16, 17, 31, 32, 33, 48):
        out.append(Case("pairs_iter%d" % k, "pairs", "pairs", 3, dict(max_delta=-1.0, max_iter=k), "fsum", False))
    for n in SIZES:
        out.append(Case("size%d_g3" % n, "sizes", "size%d" % n, 3, dict(max_iter=3), "fsum", False))
    out.append(Case("size1048577_g16", "sizes", "size1048577", 16, dict(max_iter=3), "oracle", False))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# where the gate has to refuse: case -> the iterations, counted from 1 (a refusal freezes the parameters, the next pass repeats
# the log-likelihood and the fit ends, so each has one)
REFUSALS = {"gate_first_step": [1], "gate_half1000_g3": [1], "gate_single_g4": [1], "gate_late": [LATE_REFUSED],
            "gate_thresholds_1_1": [1], "gate_thresholds_50_20": []}


def size_case(n):
    """the `sizes` case of another n: the GPU test adds the neighbours of the grid cap of a device that has not 256 CUs"""
    c = Case("size%d_g3" % n, "sizes", "size%d" % n, 3, dict(max_iter=3), "fsum", False)
    INPUTS.setdefault(c.input, lambda: mix(18, n, THREE, 0.04))
    return BY_NAME.setdefault(c.name, c)


GROUPS = ("g_sweep", "guards", "gate", "pairs", "sizes")

# ---- tolerances --------------------------------------------------------------------------------------------------------------
# SPREAD: the CPU spread per group, measured by tests/test_gmm_cases_cpu.py (which asserts that it is not exceeded) and rounded
# up: the largest relative difference of weights, variances and log-likelihood between the oracle's sequential sums and the
# exactly rounded ones, one libm in two summation orders.  The device is allowed 100 times that -- a second libm and a
# tree-shaped order on top -- and never more than the 1e-9 the suite had before.
CEILING = 1e-9
SPREAD = {
    "g_sweep": 8e-14,    # measured 7.6e-14 (sweep_g14)
    "guards": 5e-14,     # measured 4.7e-14 (stray_g3: 4801 equal terms of the log-likelihood, added one by one)
    "gate": 9e-15,       # measured 8.0e-15 (gate_half1000_g3)
    "pairs": 2e-14,      # measured 1.6e-14 (pairs_iter1)
    "sizes": 2e-12,      # measured 1.7e-12 (size2500003_g3); 5e-13 at 1 048 576 and 1 048 577, 2.9e-15 up to 1025 values
}
DEVICE_TOL = {}          # a group whose tolerance the device's libm sets instead (none)
TOL = {group: DEVICE_TOL.get(group, min(CEILING, 100 * SPREAD[group])) for group in GROUPS}


def spread_of(dev):
    """the figure the tolerances are made of: the largest of a deviation()'s weights, variances and log-likelihood"""
    return max(dev["weights"], dev["vars"], dev["loglik"])


@lru_cache(maxsize=None)
def reference(name):
    """reference_fit of a case, computed once per process and shared"""
    c = BY_NAME[name]
    return reference_fit(values(c.input), c.g, **c.fit)


def deviation(got, ref, n):
    """{quantity: largest relative difference} of a fit against a reference fit: weights and variances element by element
    relative to the reference's value, loglik relative to max(1, |loglik|), aic relative to |aic| but to no less than
    2 max(1, |loglik|) / n, which is what loglik's own allowance amounts to in aic = (2 (2g - 1) - 2 loglik) / n.  Values that
    are NaN or infinite on both sides in the same places count as equal; in different places the deviation is infinite."""
    out = {}
    for key in ("weights", "vars"):
        a, b = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        worst = 0.0
        for u, v in zip(a, b):
            worst = max(worst, _rel(u, v, abs(v)))
        out[key] = worst
    ll = ref["loglik"]
    out["loglik"] = _rel(got["loglik"], ll, max(1.0, abs(ll)))
    floor = 2 * max(1.0, abs(ll)) / n if n and math.isfinite(ll) else 0.0
    out["aic"] = _rel(got["aic"], ref["aic"], max(abs(ref["aic"]), floor))
    return out


def _rel(u, v, scale):
    if math.isnan(u) or math.isnan(v):
        return 0.0 if math.isnan(u) and math.isnan(v) else math.inf
    if u == v:
        return 0.0
    if math.isinf(u) or math.isinf(v) or scale == 0.0:
        return math.inf
    return abs(u - v) / scale
