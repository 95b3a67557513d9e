"""Shared by tests/test_filter_rows_cpu.py and tests/test_gpu_filter_model.py: the option sets and hand-made tables the row filter
in front of the model is held to, and the three-command chain it has to equal (`ploidyfrost filter`, then the readers of
`ploidyfrost model`)."""
import os
import subprocess

from conftest import ROOT

from ploidyfrost_amd import hostapi

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
TABLES = ("bicov", "tricov", "tetracov", "pentacov")
R_ERROR = "non-numeric argument to mathematical function"

# option sets on the golden cases: words for the command line, the same as keywords for hostapi.filter_rows / Run.set_filter, and
# the rows kept of (bi, tri, tetra) in hex30k and tet60k, counted with a restatement of the predicates
OPTION_SETS = [
    ("-S -n 2 -d 30", dict(simple=True, num=2, distance=30), {"hex30k": (245, 10, 8), "tet60k": (324, 5, 2)}),
    ("-I -l 25 -u 70", dict(indel=True, low=25, up=70), {"hex30k": (98, 4, 0), "tet60k": (116, 0, 0)}),
    ("-P -s 4", dict(snp=True, size=4), {"hex30k": (92, 0, 0), "tet60k": (72, 0, 0)}),
    ("-S -P -d 1000000", dict(simple=True, snp=True, distance=1000000), {"hex30k": (0, 0, 0), "tet60k": (0, 0, 0)}),
]
DEFAULT_SET = ("", dict(), {})

# ---- hand-made tables (the shapes of tests/test_filter_cpu.py; rows end in a tab, as the path writes them) ----
# CovA CovB isStrict VarType VarId VarNum VarDis
BICOV = (
    "60.2174\t59.6429\t1\t0\t1\t2\t40\t\n"
    "100.36\t19.64\t1\t3\t2\t1\t25\t\n"
    "30\t30\t0\t0\t3\t4\t7\t\n"
    "4.5\t70\t1\t0\t4\t1\t25\t\n"             # CovA below -l 5
    "61\t1200.5\t0\t12\t5\t1\t3\t\n"          # CovB above -u 1000
    "100000\t250000\t1\t0\t6\t1\t9\t\n"       # kept with -u above it: R writes 1e+05
    "0.0001\t50\t1\t0\t7\t1\t9\t\n"           # kept with -l 0: R writes 1e-04
    "6000\t5000\t1\t0\t8\t1\t9\t\n"           # kept with -u 20000: the sum is >= 10000, `model -f` skips the row
    "25\t75\t1\t0\t9\t1\t9\t\n"               # frequencies exactly 0.25 and 0.75: dropped by -q 0.25 (the test is strict)
    "7\t93\t1\t0\t10\t1\t9\t\n"
)
TRICOV = "20\t20\t20\t1\t0\t7\t1\t30\t\n40.5\t20.25\t20.25\t0\t2\t8\t3\t11\t\n"
TETRACOV = "20\t20\t20\t20\t1\t0\t9\t1\t30\t\n300\t300\t300\t300\t1\t0\t10\t1\t30\t\n"   # second row: dropped only by A+B+C+D < -u 1000
PENTACOV = (
    "100\t100\t100\t100\t100\t1\t0\t11\t1\t30\t\n"     # kept
    "260\t260\t260\t260\t10\t1\t0\t12\t1\t30\t\n"      # dropped only by the sum of its first four (1040)
    "10\t20\t30\t40\t900\t1\t2\t13\t1\t30\t\n"         # kept: the fifth coverage is not in that sum
)
HAND = {"bicov": BICOV, "tricov": TRICOV, "tetracov": TETRACOV, "pentacov": PENTACOV}
# only the penta table keeps rows under -S
ONLY_PENTA = {
    "bicov": "30\t30\t0\t0\t3\t4\t7\t\n",
    "tricov": "40.5\t20.25\t20.25\t0\t2\t8\t3\t11\t\n",
    "tetracov": "20\t20\t20\t20\t0\t0\t9\t1\t30\t\n",
    "pentacov": PENTACOV,
}
# (tables, words, keywords, refused for source cov: a kept coverage R prints in scientific notation)
HAND_SETS = [
    ("hand", "-l 5 -u 1000", dict(low=5, up=1000), False),
    ("hand", "-l 5 -u 20000", dict(low=5, up=20000), False),
    ("hand", "-l 0 -u 1000", dict(low=0, up=1000), True),            # keeps 0.0001
    ("hand", "-l 5 -u 1000000", dict(low=5, up=1000000), True),      # keeps 100000
    ("hand", "-l 5 -u 1000 -q 0.25", dict(low=5, up=1000, frequency=0.25), False),
    ("hand", "-l 5 -u 1000 -S -I -n 2 -d 8 -s 1", dict(low=5, up=1000, simple=True, indel=True, num=2, distance=8, size=1), False),
    ("only_penta", "-S", dict(simple=True), False),
]
HAND_TABLES = {"hand": HAND, "only_penta": ONLY_PENTA}


def write_tables(prefix, tables):
    for name in TABLES:
        with open("%s_%s.txt" % (prefix, name), "w") as f:
            f.write(tables[name])


def read_tables(prefix):
    out = []
    for name in TABLES:
        with open("%s_%s.txt" % (prefix, name), "rb") as f:
            out.append(f.read())
    return out


def run_filter(prefix, words, out):
    """`ploidyfrost filter -i prefix -o out <words>`; RuntimeError with its stderr when it fails"""
    r = subprocess.run([CLI, "filter", "-i", prefix, "-o", out] + words.split(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return r


def chain_values(filtered, source, q):
    """what `model -f <filtered>` / `model -g <filtered>_allele_frequency.txt` reads"""
    m = hostapi.Gmm()
    if source == "cov":
        m.read_cov(filtered, q)
    else:
        m.read_fre(filtered + "_allele_frequency.txt", q)
    return m.values()
