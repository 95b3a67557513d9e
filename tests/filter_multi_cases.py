"""Shared by tests/test_filter_multi_rows_cpu.py and tests/test_gpu_filter_multi_model.py: the option sets and hand-made colored
tables the multi row filter in front of the model is held to, and the chain it has to equal (`ploidyfrost filter-multi`, then the
readers of `ploidyfrost model`)."""
import subprocess

from filter_cases import CLI, R_ERROR, TABLES, chain_values, read_tables, write_tables  # noqa: F401

# words for the command line and the same as keywords for hostapi.filter_rows(multi=True) / ColoredRun.set_filter_multi
ONE_COLOUR = ("-c 0 -v 0.25 -l 5 -u 1000", dict(color=0, cramer=0.25, low=5, up=1000))
POOLED = ("-S -P -v 0.25 -q 0.1", dict(simple=True, snp=True, cramer=0.25, frequency=0.1))
EACH = ("-v 0.25 -l 5 -u 1000", dict(cramer=0.25, low=5, up=1000))
# _bicov rows of col4_mix kept under EACH, colour by colour, counted on the fixture's files with a restatement of the predicates
# (test_counts_the_fixtures_give; colours 0 and 3 keep one of the two _tricov rows each as well)
KEPT_COL4_MIX = (180, 103, 0, 170)

# ---- hand-made colored tables: CovA .. colour isStrict VarType VarId VarNum Cramer VarDis, rows end in a tab ----
BICOV = (
    "60.2174\t59.6429\t0\t1\t0\t1\t2\t0.9\t40\t\n"
    "100.36\t19.64\t0\t1\t3\t2\t1\t0.5\t25\t\n"
    "30\t30\t70\t0\t0\t3\t4\t0.26\t7\t\n"             # a colour beyond the first 64
    "40\t60\t70\t1\t0\t4\t1\t0.25\t9\t\n"             # Cramer's V equal to -v 0.25: dropped (the test is strict)
    "4.5\t70\t1\t1\t0\t5\t1\t0.8\t25\t\n"             # CovA below -l 5
    "61\t1200.5\t1\t0\t12\t6\t1\t0.8\t3\t\n"          # CovB above -u 1000
    "25\t75\t1\t1\t0\t7\t1\t0.7\t9\t\n"
    "50\t50\t2\t1\t0\t8\t1\t0.1\t9\t\n"               # colour 2 keeps nothing under -v 0.25
    "7\t93\t3\t1\t0\t9\t1\t0.6\t9\t\n"
)
TRICOV = "20\t20\t20\t0\t1\t0\t10\t1\t0.4\t30\t\n40.5\t20.25\t20.25\t70\t0\t2\t11\t3\t0.3\t11\t\n10\t20\t30\t2\t1\t0\t12\t1\t0.2\t30\t\n"
# second row: every coverage inside (5, 1000), the first four sum to 1200 >= -u 1000 -- kept here, dropped by the single-sample rule
TETRACOV = "20\t20\t20\t20\t3\t1\t0\t13\t1\t0.5\t30\t\n300\t300\t300\t300\t0\t1\t0\t14\t1\t0.5\t30\t\n"
PENTACOV = (
    "100\t100\t100\t100\t100\t0\t1\t0\t15\t1\t0.9\t30\t\n"
    "260\t260\t260\t260\t10\t70\t1\t0\t16\t1\t0.9\t30\t\n"    # the first four sum to 1040: kept here as well
    "10\t20\t30\t40\t900\t1\t1\t2\t17\t1\t0.9\t30\t\n"
)
HAND = {"bicov": BICOV, "tricov": TRICOV, "tetracov": TETRACOV, "pentacov": PENTACOV}
HAND_COLOURS = (0, 1, 2, 3, 70)     # colour 2 keeps no row
# a kept coverage of 100000 (colour 1): R writes 1e+05, refused for cov, fine for fre
HAND_SCI = dict(HAND, bicov=BICOV + "100000\t250000\t1\t1\t0\t18\t1\t0.9\t9\t\n")
HAND_WORDS = ("-v 0.25 -l 5 -u 1000", dict(cramer=0.25, low=5, up=1000))
SCI_WORDS = ("-v 0.25 -l 5 -u 1000000", dict(cramer=0.25, low=5, up=1000000))


def with_colour(words, kw, c):
    return words + " -c %d" % c, dict(kw, color=c)


def run_filter_multi(prefix, words, out):
    """`ploidyfrost filter-multi -i prefix -o out <words>`; RuntimeError with its stderr when it fails"""
    r = subprocess.run([CLI, "filter-multi", "-i", prefix, "-o", out] + words.split(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return r


def kept_rows(prefix, kw, tables=TABLES):
    """rows of the four tables (or of those named) `filter-multi` keeps: the predicates of run_filter's multi branch restated on
    the text"""
    low, up = kw.get("low", 0), kw.get("up", 10000)
    n = 0
    for a, name in enumerate(TABLES):
        if name not in tables:
            continue
        A = a + 2
        with open("%s_%s.txt" % (prefix, name)) as f:
            for line in f:
                x = [float(t) for t in line.split()]
                if not x:
                    continue
                cov, colour, strict, vtype, num, cramer, dis = x[:A], x[A], x[A + 1], x[A + 2], x[A + 4], x[A + 5], x[A + 6]
                k = all(low < c < up for c in cov) and num < kw.get("num", 10000) and dis > kw.get("distance", -1) and vtype < kw.get("size", 10000)
                k = k and cramer > kw.get("cramer", 0.0) and (kw.get("color", -1) < 0 or colour == kw["color"])
                k = k and (not kw.get("simple") or strict == 1) and (not kw.get("indel") or vtype == 0) and (not kw.get("snp") or vtype > 0)
                n += bool(k)
    return n

