#!/usr/bin/env python3
"""Regenerate tests/golden/cli/surface.json: what the command line of the nine reads sub-commands (count, build, build-multi, mask,
smudge, qc, trim, run, run-multi) and the dispatch in main() say, byte for byte.

The tree is built as it stands (build.build_device()) and csrc/ploidyfrost runs on a fixed, enumerated list of command lines in an
empty temporary directory, with relative file names only.  Every line ends before a device context exists: it is refused while it is
parsed, by the checks behind the parse, or by the host layer's look at the inputs (a file that is not there).  The file holds
    commit   the commit that was checked out when it was recorded (the parent of the change that moved the sub-commands out of
             pf_main.cpp; a regeneration on a later commit that changes this line alone changes nothing)
    usage    every sub-command's usage block, once
    valid    per sub-command, the words of a line that parses and passes every check behind the parse (its inputs are not there)
    cases    per sub-command: [argv, why] for a refusal in the sub-command's own form -- exit status 1, nothing on stdout, `Error:
             <sub>: <why>` and the usage block on stderr -- and [argv, exit status, stdout, stderr] for every other line; the word
             "<<valid>>" in argv stands for the sub-command's valid words
It is a statement about the command line as it is: regenerate it only in a change that means to alter the command line, and review
the diff of the fixture as that change.

usage: python tests/golden/make_cli_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
OUT = os.path.join(HERE, "cli", "surface.json")
VALID = "<<valid>>"
ENV = dict(os.environ, LC_ALL="C", LANG="C")

# the words every numeric option is given: the two number grammars of the file (digit first through strtoull; strtoll within a range)
# and the reals answer them differently
WORDS = ["", "abc", "-1", "+5", " 5", "5x", "0", "4294967296", "18446744073709551616"]
KMC = ["-k", "-ci", "-cx", "-cs"]
CLIP_VALUES = ["--adapters", "--adapter-seed", "--adapter-score", "--adapter-pair-score", "--adapter-pair-min"]
CLIP_NUMERIC = {"--adapter-seed": ["--adapters", "a.fa"], "--adapter-score": ["--adapters", "a.fa"],
                "--adapter-pair-score": ["--adapters", "a.fa", "--adapter-pairs"], "--adapter-pair-min": ["--adapters", "a.fa", "--adapter-pairs"]}
STEP = "MINLEN:5"
RUN_LONG = [["--gpus", "2"], ["--gpus"], ["--filter", "-S"], ["--filter"], ["--filter-multi", "-S"], ["--filter-multi"], ["--model-each-color"],
            ["--detach-teardown"], ["--density"], ["--density-points", "64"], ["--density-points"], ["--density-adjust", "2"],
            ["--density", "--density-points", "1"], ["--model", "cov", "--density", "--density-adjust", "abc"], ["--model", "cov"], ["--model", "abc"],
            ["--model-only"], ["--model-bogus", "1"], ["--model-ploidy", "3:2", "--model", "fre"], ["--model", "cov", "--filter", "-S"],
            ["--model", "cov", "--filter", "-c 1"], ["--model", "cov", "--filter-multi", "-S", "--model-each-color"],
            ["--model", "cov", "--filter-multi", "-c 1", "--model-each-color"], ["--model", "cov", "--density"], ["--ref-threads", "2"]]
RUN_NUMERIC = KMC + ["-q", "-u", "-g", "-z", "-M", "-D", "-G", "-t", "--chunk-bytes", "--initial-slots"]
RUN_VALUES = ["-i", "-o", "-q", "-u", "-g", "-z", "-M", "-D", "-G", "-t", "--db-out", "--gfa-out", "--chunk-bytes", "--initial-slots", "--phred", "-1", "-2"]
RUN_NOT_HERE = ["-f", "-C", "-d", "-h", "-l", "-b", "--filtered-out", "--detach-teardown", "--trimlog", "-o1", "-u1", "-o2", "-u2"]
RUN_RANGES = [["-q", "1.5"], ["-q", "-0.5"], ["-z", "3"], ["-D", "3"], ["-G", "3"], ["-M", "-2"], ["-k", "2"], ["-k", "4"], ["-k", "32"], ["-g", "24"],
              ["-ci", "0"], ["-ci", "5", "-cx", "4"], ["-cs", "0"], ["-cx", "4294967296"]]
TRIM_RULES = [[STEP, "--phred", "64"], ["--phred", "64"], ["LEADING:x"], ["SLIDINGWINDOW:3"], ["BOGUS:1"], [STEP, "MINLEN"], ["--adapters", "a.fa"],
              ["--adapters", ""], ["--adapter-seed", "2"], ["--adapter-score", "2"], ["--adapter-pairs"], ["--adapter-pair-score", "2"],
              ["--adapter-pair-min", "2"], ["--adapter-keep-both"], ["--adapters", "a.fa", "--adapter-pair-score", "2"],
              ["--adapters", "a.fa", "--adapter-pair-min", "2"], ["--adapters", "a.fa", "--adapter-keep-both"], ["--adapters", "a.fa", "--adapter-pairs"],
              ["--adapters", "a.fa", "--adapter-seed", "9"], ["--adapters", "a.fa", "--adapter-score", "1001"],
              ["--adapters", "a.fa", "--adapter-pairs", "--adapter-pair-score", "0"], ["--adapters", "a.fa", "--adapter-pairs", "--adapter-pair-min", "17"]]

# Per sub-command: `valid` parses and passes the checks behind the parse (its inputs are not there); `values` take a value, `numeric`
# a number (an entry may be (option, [words it needs in front of it])); `names` are refused by name; `rules` are the lines of the checks behind
# the parse (put behind the sub-command's name as they are); `with_valid` go behind `valid`; `mistakes` are paired in both orders
SUBS = {
    "count": dict(
        valid=["-k", "25", "-i", "nowhere.fq", "-o", "db"],
        values=KMC + ["-i", "-o", "--hist", "--chunk-bytes", "--initial-slots"],
        numeric=KMC + ["--chunk-bytes", "--initial-slots"],
        names=[],
        rules=[[], ["-o", "db"], ["-i", "a.fq"], ["-i", "a.fq", "-o", "db", "-k", "2"], ["-i", "a.fq", "-o", "db", "-k", "4"], ["-i", "a.fq", "-o", "db", "-k", "32"],
               ["-i", "a.fq", "-o", "db", "-ci", "0"], ["-i", "a.fq", "-o", "db", "-ci", "5", "-cx", "4"], ["-i", "a.fq", "-o", "db", "-cs", "0"],
               ["-i", "a.fq", "-o", "db", "-cx", "4294967296"], ["-i", "a.fq", "-o", "db", "-k", "2", "-ci", "0"], ["-k", "2", "-ci", "0"]],
        with_valid=[[], ["-b"], ["-v"], ["--gz"], ["--gz-plain"], ["--gz", "--gz-plain"], ["--fasta"], ["--hist", "h.txt"], ["-k25", "-ci1", "-cs10000", "-cx5"],
                    ["-i", "other.fq"], ["-o", "nowhere.fq"], ["-kx"], ["-ci"], ["-k25x"], ["-bx"], ["-cq", "1"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "abc"], ["-k", "abc"]],
    ),
    "build": dict(
        valid=["-k", "25", "-r", "nowhere.fq", "-o", "sample"],
        values=["-k", "-g", "-t", "-r", "-o", "--chunk-bytes", "--initial-slots"],
        numeric=["-k", "-g", "-t", "--chunk-bytes", "--initial-slots"],
        names=["-s", "-c", "-y", "-f", "-a", "-m", "-n", "-b", "-B", "-l", "-w", "-e", "--gpus"],
        rules=[[], ["-o", "sample"], ["-r", "a.fq"], ["-r", "a.fq", "-o", "sample", "-k", "2"], ["-r", "a.fq", "-o", "sample", "-k", "32"],
               ["-r", "a.fq", "-o", "sample", "-g", "24"], ["-r", "a.fq", "-o", "sample", "-k", "7", "-g", "6"], ["-r", "a.fq", "-o", "sample", "-k", "32", "-g", "40"],
               ["-r", "a.fq", "-r", "a.fq", "-o", "sample"], ["-k", "2"]],
        with_valid=[[], ["-i"], ["-d"], ["-v"], ["--fasta"], ["-i", "-d", "-v", "--fasta"], ["-r", "other.fq"], ["-o", "nowhere.fq"], ["-g", "23"], ["-t", "4"],
                    ["-k25"], ["--gz"], ["--gz-plain"], ["-c"], ["--gpus", "2"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "abc"], ["-s"]],
    ),
    "mask": dict(
        valid=["-d", "db", "-i", "nowhere.fq", "-o", "out.fq", "-l", "5"],
        values=KMC + ["-d", "--db-out", "-i", "-o", "-l", "-u", "--chunk-bytes"],
        numeric=KMC + ["-l", "-u", "--chunk-bytes"],
        names=["--fasta"],
        rules=[[], ["-d", "db", "-k", "25"], ["-d", "db", "-ci", "2"], ["-d", "db", "-b"], ["-d", "db", "--db-out", "x"], ["-i", "a.fq"], ["-d", "db"],
               ["-d", "db", "-i", "a.fq"], ["-d", "db", "-i", "a.fq", "-o", "o.fq"], ["-d", "db", "-i", "a.fq", "-o", "o.fq", "-l", "5", "--auto-cutoffs"],
               ["-d", "db", "-i", "a.fq", "-o", "o.fq", "-l", "9", "-u", "5"], ["-k", "25", "-i", "a.fq", "-o", "o.fq", "-l", "5", "-ci", "0"],
               ["-k", "4", "-i", "a.fq", "-o", "o.fq", "-l", "5"], ["-k", "4", "-i", "a.fq", "-o", "o.fq", "-l", "5", "--db-out", "x"],
               ["-k", "2", "-i", "a.fq", "-o", "o.fq", "-l", "5"], ["-k", "25", "-d", "db", "-ci", "2", "--db-out", "x"], ["-ci", "2", "--db-out", "x"],
               ["--db-out", "x", "-l", "5", "--auto-cutoffs"], ["-d", "db", "-l", "9", "-u", "5", "--auto-cutoffs"], ["-d", "db", "-o", "o.fq", "-l", "9", "-u", "5"]],
        with_valid=[[], ["-v"], ["--gz-out"], ["-u", "50"], ["--chunk-bytes", "4096"], ["-i", "other.fq"], ["-o", "nowhere.fq"], ["--gz"], ["--gz-plain"],
                    ["--initial-slots", "8"], ["-l", "7"]],
        extra=[["-k", "25", "-i", "nowhere.fq", "-o", "out.fq", "--auto-cutoffs"], ["-k25", "-ci1", "-i", "nowhere.fq", "-o", "out.fq", "-l", "5", "--db-out", "x"],
               ["-d", "db", "-i", "nowhere.fq", "-o", "out.fq", "--auto-cutoffs", "-u", "9"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "0"], ["-l", "abc"]],
    ),
    "smudge": dict(
        valid=["-k", "25", "-i", "nowhere.fq", "-l", "2", "-u", "50", "-o", "out"],
        values=KMC + ["-d", "-i", "-o", "-l", "-u", "-q", "-n", "--pairs", "--chunk-bytes", "--initial-slots"],
        numeric=KMC + ["-l", "-u", "-n", "-q", "--chunk-bytes", "--initial-slots"],
        names=[],
        rules=[[], ["-d", "db", "-k", "25"], ["-o", "out"], ["-d", "db", "-ci", "2"], ["-d", "db", "-b"], ["-d", "db", "-i", "a.fq"], ["-d", "db", "--gz"],
               ["-d", "db", "--gz-plain"], ["-d", "db", "--fasta"], ["-d", "db", "--chunk-bytes", "5"], ["-d", "db", "--initial-slots", "5"], ["-k", "25"],
               ["-d", "db"], ["-d", "db", "-o", "out", "-l", "2", "--auto-cutoffs"], ["-d", "db", "-o", "out", "-u", "2", "--auto-cutoffs"],
               ["-d", "db", "-o", "out"], ["-d", "db", "-o", "out", "-l", "2"], ["-d", "db", "-o", "out", "-u", "2"], ["-d", "db", "-o", "out", "-l", "2", "-u", "9", "-q", "0.5"],
               ["-d", "db", "-o", "out", "-l", "0", "-u", "9"], ["-d", "db", "-o", "out", "-l", "9", "-u", "2"], ["-d", "db", "-o", "out", "-l", "1", "-u", "5000"],
               ["-d", "db", "-o", "out", "-l", "2", "-u", "9", "-n", "0"], ["-d", "db", "-o", "out", "--auto-cutoffs", "-n", "0"],
               ["-k", "25", "-i", "a.fq", "-o", "out", "-l", "2", "-u", "9", "-b"], ["-k", "2", "-i", "a.fq", "-o", "out", "-l", "2", "-u", "9"],
               ["-k", "25", "-i", "a.fq", "-o", "out", "-l", "2", "-u", "9", "-ci", "0"], ["-k", "25", "-i", "a.fq", "-o", "out", "-l", "2", "-u", "9", "-b", "-ci", "0"],
               ["-d", "db", "-ci", "2", "-i", "a.fq"], ["-d", "db", "-o", "out", "-l", "9", "-u", "2", "-n", "0"], ["-d", "db", "-l", "2", "-q", "0.5"],
               ["-k", "4", "-i", "a.fq", "-o", "out", "-l", "2", "-u", "9"]],
        with_valid=[[], ["-v"], ["--gz"], ["--gz-plain"], ["--fasta"], ["-n", "20"], ["--pairs", "p.tsv"], ["--pairs", "out_smudge.tsv"], ["-k25", "-ci1"], ["-i", "other.fq"],
                    ["--chunk-bytes", "4096", "--initial-slots", "64"], ["--gz-out"]],
        extra=[["-k", "25", "-i", "nowhere.fq", "--auto-cutoffs", "-q", "0.9", "-o", "out"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "0"], ["-l", "abc"]],
    ),
    "qc": dict(
        valid=["-i", "nowhere.fq", "-o", "report.tsv"],
        values=["-i", "-1", "-2", "-o", "--phred", "--chunk-bytes"],
        numeric=["--phred", "--chunk-bytes"],
        names=["--fasta"],
        rules=[[], ["-i", "a.fq", "-1", "b.fq"], ["-i", "a.fq", "-2", "b.fq"], ["-o", "r.tsv"], ["-i", "a.fq"], ["-1", "a.fq"], ["-i", "a.fq", "-1", "b.fq", "-o", "r.tsv"]],
        with_valid=[[], ["-v"], ["--gz"], ["--gz-plain"], ["--phred", "33"], ["--phred", "64"], ["--chunk-bytes", "4096"], ["-i", "other.fq"], ["-o", "nowhere.fq"],
                    ["--initial-slots", "5"], ["-k", "25"]],
        extra=[["-1", "a", "-2", "a", "-o", "report.tsv"], ["-1", "a", "-o", "report.tsv"], ["-2", "a", "-o", "report.tsv"], ["-1", "a", "-2", "b", "-1", "c", "-o", "report.tsv"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "abc"], ["--phred", "32"]],
    ),
    "trim": dict(
        valid=["-i", "nowhere.fq", "-o", "trimmed.fq", STEP],
        values=["-i", "-o", "--phred", "--trimlog", "--chunk-bytes", "--report", "-1", "-2", "-o1", "-u1", "-o2", "-u2"] + CLIP_VALUES,
        numeric=["--phred", "--chunk-bytes"] + [(o, w) for o, w in CLIP_NUMERIC.items()],
        names=["--fasta"],
        rules=[[], ["-i", "a.fq", "-o", "t.fq"], [STEP], [STEP, "-o", "t.fq"], [STEP, "-i", "a.fq"], [STEP, "-i", "a.fq", "-1", "b.fq"], [STEP, "-1", "a.fq", "-o", "t.fq"],
               [STEP, "-i", "a.fq", "-o", "t.fq", "--adapters", "a.fa", "--adapter-pairs"], [STEP, "-o1", "p1.fq"], [STEP, "-i", "a.fq", "-u2", "p1.fq"],
               [STEP, "-1", "a.fq"], [STEP, "-2", "a.fq"], [STEP, "-1", "a.fq", "-2", "b.fq"], [STEP, "-1", "a.fq", "-2", "b.fq", "-o1", "x"],
               [STEP, "-1", "a.fq", "-2", "b.fq", "-o1", "x", "-u1", "y", "-o2", "z"], [STEP, "-i", "a.fq", "-o", "t.fq", "--report", ""],
               [STEP, "-i", "a.fq", "-1", "b.fq", "-o", "t.fq"], ["-i", "a.fq", "-1", "b.fq", "-o", "t.fq"], ["LEADING:x", "--adapter-seed", "2"],
               [STEP, "-i", "a.fq", "-o", "t.fq", "-o1", "x"]] + [["-i", "a.fq", "-o", "t.fq"] + r for r in TRIM_RULES],
        with_valid=[[], ["-v"], ["--gz"], ["--gz-plain"], ["--gz-out"], ["--phred", "64"], ["--trimlog", "log.txt"], ["--report", "r.tsv"], ["--chunk-bytes", "4096"],
                    ["-i", "other.fq"], ["-o", "nowhere.fq"], ["--adapters", "a.fa"], ["LEADING:3", "TRAILING:3", "SLIDINGWINDOW:4:15"], ["--initial-slots", "5"]],
        extra=[["-1", "a", "-2", "a", "-o1", "p1", "-u1", "u1", "-o2", "p2", "-u2", "u2", STEP], ["-1", "a", "-2", "b", "-o1", "p1", "-u1", "u1", "-o2", "p2", "-u2", "p1", STEP],
               ["-1", "a", "-2", "b", "-o1", "p1", "-u1", "u1", "-o2", "p2", "-u2", "u2", "--adapters", "a.fa", "--adapter-pairs"],
               ["-i", "nowhere.fq", "-o", "trimmed.fq", "--adapters", "a.fa"]],
        mistakes=[["--bogus"], ["--chunk-bytes", "abc"], ["--phred", "32"]],
    ),
    "run": dict(
        valid=["-i", "nowhere.fq", "-o", "sample"],
        values=KMC + RUN_VALUES + ["--report", "--smudge-n", "--smudge-pairs"] + CLIP_VALUES,
        numeric=RUN_NUMERIC + ["--smudge-n", "--phred"] + [(o, w) for o, w in CLIP_NUMERIC.items()],
        names=RUN_NOT_HERE,
        rules=[[], ["-o", "sample"], ["-i", "a.fq"], ["-i", "a.fq", "-1", "b.fq", "-2", "c.fq", STEP, "-o", "sample"], ["-1", "a.fq"], ["-2", "a.fq"],
               ["-1", "a.fq", "-1", "b.fq"], ["-1", "a.fq", "-2", "b.fq", "-o", "sample"], ["-i", "a.fq", "--phred", "64", "-o", "sample"], ["-1", "a.fq", "-o", "sample"],
               ["-1", "a.fq", "-2", "b.fq", "-1", "c.fq", STEP]] +
              [["-i", "a.fq", "-o", "sample"] + r for r in RUN_RANGES + TRIM_RULES + [
                  ["--report", "r.tsv"], ["--report", ""], ["--report", "r.tsv", "--fasta", STEP], ["--smudge-n", "5"], ["--smudge-pairs", "p"], ["--smudge-pairs", ""],
                  ["--smudge", "--smudge-n", "0"], ["--fasta", "--adapters", "a.fa"], ["--fasta", STEP], ["--fasta", "--report", "r.tsv"],
                  ["-z", "3", "-q", "2"], ["-D", "3", "-G", "3"], ["-q", "2", "-k", "2"], ["-k", "2", "--report", "r.tsv"], ["--smudge-n", "5", "-ci", "0"]]] +
              [["-1", "a.fq", "-2", "b.fq", "-o", "sample", "--fasta", STEP], ["-o", "sample", "-k", "2"], ["-i", "a.fq", "-k", "2"], ["LEADING:x"], ["-i", "a.fq", "LEADING:x"]],
        with_valid=[[], ["-v"], ["--gz"], ["--gz-plain"], ["--fasta"], ["--keep-tips"], ["--keep-isolated"], ["--smudge"], ["--smudge", "--smudge-n", "20", "--smudge-pairs", "p.tsv"],
                    ["-k25", "-ci1", "-cs10000", "-cx5"], ["-u", "50"], ["-g", "23"], ["-z", "8", "-M", "2", "-D", "-1", "-G", "-3", "-t", "1"], ["--db-out", "db", "--gfa-out", "g"],
                    ["--db-out", "x", "--gfa-out", "x"], ["--gfa-out", "x", "--report", "x.gfa", STEP], ["--chunk-bytes", "4096", "--initial-slots", "64"], ["-i", "other.fq"],
                    [STEP], [STEP, "--phred", "64"], [STEP, "--report", "r.tsv"], ["--adapters", "a.fa"], ["--model", "cov", "--filter", "-S", "--density"],
                    ["--sample", "A"], ["--gz-out"]],
        long=RUN_LONG,
        extra=[["-1", "a", "-2", "a", "-o", "sample", STEP], ["-1", "a", "-2", "b", "-1", "c", "-2", "d", "-o", "sample", STEP],
               ["-1", "a", "-2", "b", "-o", "sample", "--adapters", "a.fa", "--adapter-pairs"], ["-i", "a", "-i", "a", "-o", "sample", STEP]],
        mistakes=[["--bogus"], ["-f"], ["-k", "abc"], ["--phred", "32"]],
    ),
    "run-multi": dict(
        valid=["--sample", "A", "-i", "nowhere.fq", "-o", "out"],
        values=KMC + ["--sample"] + RUN_VALUES + CLIP_VALUES,
        numeric=RUN_NUMERIC + ["--phred"] + [(o, w) for o, w in CLIP_NUMERIC.items()],
        names=RUN_NOT_HERE,
        rules=[[], ["-o", "out"], ["-i", "a.fq"], ["-1", "a.fq"], ["-2", "a.fq"], ["--sample", "A"], ["--sample", "A", "-o", "out"], ["--sample", "A", "-i", "a.fq"],
               ["--sample", "", "-i", "a.fq", "-o", "out"], ["--sample", "A", "-i", "a.fq", "--sample", "A", "-i", "b.fq", "-o", "out"],
               ["--sample", "A", "-i", "a.fq", "--sample", "B", "-i", "a.fq", "-o", "out"], ["--sample", "A", "-i", "a.fq", "--sample", "B", "-o", "out"],
               ["--sample", "A", "-i", "a.fq", "-1", "b.fq"], ["--sample", "A", "-1", "a.fq", "-2", "b.fq", "-i", "c.fq"], ["--sample", "A", "-1", "a.fq", "--sample", "B"],
               ["--sample", "A", "-1", "a.fq", "-1", "b.fq"], ["--sample", "A", "-2", "b.fq"], ["--sample", "A", "-1", "a.fq"],
               ["--sample", "A", "-1", "a.fq", "-2", "b.fq", "-o", "out"], ["--sample", "A", "-i", "a.fq", "--phred", "64", "-o", "out"],
               ["--sample", "A", "-i", "a.fq", "--report", "r.tsv", "-o", "out"], ["--sample", "A", "-i", "a.fq", "--smudge", "-o", "out"],
               ["--sample", "A", "-i", "a.fq", "-k", "2"], ["--sample", "A", "-o", "out", "-k", "2"], ["--sample", "A", "-1", "a.fq", "-o", "out", "-k", "2"]] +
              [["--sample", "A", "-i", "a.fq", "-o", "out"] + r for r in RUN_RANGES + TRIM_RULES + [
                  ["--fasta", "--adapters", "a.fa"], ["--fasta", STEP], ["-z", "3", "-q", "2"], ["-D", "3", "-G", "3"], ["-q", "2", "-k", "2"]]],
        with_valid=[[], ["-v"], ["--gz"], ["--gz-plain"], ["--fasta"], ["--keep-tips"], ["--keep-isolated"], ["-k25", "-ci1", "-cs10000", "-cx5"], ["-u", "50"], ["-g", "23"],
                    ["-z", "8", "-M", "2", "-D", "-1", "-G", "-3", "-t", "1"], ["--db-out", "db", "--gfa-out", "g"], ["--chunk-bytes", "4096", "--initial-slots", "64"],
                    ["-i", "other.fq"], ["--sample", "B", "-i", "other.fq"], [STEP], [STEP, "--phred", "64"], ["--adapters", "a.fa"],
                    ["--model", "cov", "--filter-multi", "-S", "--model-each-color", "--density"], ["--gz-out"]],
        long=RUN_LONG,
        extra=[["--sample", "A", "-1", "a", "-2", "a", "-o", "out", STEP], ["--sample", "A", "-1", "a", "-2", "b", "--sample", "B", "-i", "c", "-o", "out", STEP],
               ["--sample", "A", "-1", "a", "-2", "b", "-o", "out", "--adapters", "a.fa", "--adapter-pairs"]],
        mistakes=[["--bogus"], ["-f"], ["-k", "abc"], ["--phred", "32"]],
    ),
}
# build-multi takes what build takes: -c is its own letter, and a file is a colour
SUBS["build-multi"] = dict(SUBS["build"], names=[n for n in SUBS["build"]["names"] if n != "-c"])
# main(): the usage without a word, and the helpers of the thresholds with a wrong number of words
DISPATCH = [[], ["histogram"], ["histogram", "-d"], ["histogram", "-x", "y"], ["histogram", "-d", "db", "-o"], ["histogram", "-d", "db", "extra"], ["cutoffL"],
            ["cutoffL", "a", "b"], ["cutoffL", "a", "b", "c"], ["cutoffU"], ["cutoffU", "a", "b", "c"], ["cutoffU", "a", "b", "c", "d"], ["cutoffU", "-d", "db", "0.5", "x"],
            ["cutoffL", "nowhere.txt"], ["cutoffU", "nowhere.txt"], ["cutoffU", "nowhere.txt", "abc"], ["cutoffU", "nowhere.txt", "1.5"]]


def lines_of(sub, s):
    """the command lines of one sub-command, in a fixed order and without repeats"""
    valid = s["valid"]
    out = [[o] for o in s["values"]]                        # every value option as the last word
    for n in s["numeric"]:                                  # every numeric option with every word
        opt, front = n if isinstance(n, tuple) else (n, [])
        for w in WORDS:
            if opt == "-t" and sub.startswith("run") and w == "4294967296":
                continue                                    # (accepted, then refused with the number of this machine's processors)
            out.append(front + [opt, w])
    out += [["--bogus"]] + [[n] for n in s["names"]]
    out += s["rules"] + [valid + w for w in s["with_valid"]] + s.get("extra", [])
    out += [valid + words for words in s.get("long", [])]
    ms = s["mistakes"]
    out += [valid + a + b for a in ms for b in ms if a != b]   # two mistakes, in both orders: the first word that offends wins
    seen, uniq = set(), []
    for l in out:
        if tuple(l) not in seen:
            seen.add(tuple(l))
            uniq.append(l)
    return uniq


def run(argv, cwd):
    r = subprocess.run([CLI] + argv, cwd=cwd, env=ENV, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode("utf-8", "surrogateescape"), r.stderr.decode("utf-8", "surrogateescape")


def main():
    sys.path.insert(0, ROOT)
    from ploidyfrost_amd import build
    build.build_device()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    doc = {"commit": commit, "usage": {}, "valid": {}, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        def record(lines):
            got = list(pool.map(lambda a: run(a, tmp), lines))
            if os.listdir(tmp):
                sys.exit("a command line wrote into the working directory: " + ", ".join(os.listdir(tmp)))
            return got
        for sub, spec in SUBS.items():
            rc, so, se = run([sub, "--no-such-option"], tmp)
            head = "Error: %s: unknown option --no-such-option\n" % sub
            if rc != 1 or so or not se.startswith(head):
                sys.exit("%s: the usage block could not be taken from %r" % (sub, se))
            usage = doc["usage"][sub] = se[len(head):]
            lines = [[sub] + l for l in lines_of(sub, spec)]
            cases = []
            valid = doc["valid"][sub] = spec["valid"]
            for argv, (rc, so, se) in zip(lines, record(lines)):
                if "device context" in so + se or "cannot be greater than" in se:
                    sys.exit("this line does not end before the device, or words this machine: " + " ".join(argv))
                if argv[1:1 + len(valid)] == valid:
                    argv = [sub, VALID] + argv[1 + len(valid):]
                head = "Error: %s: " % sub
                if rc == 1 and not so and se.startswith(head) and se.endswith("\n" + usage) and "\n" not in se[len(head):len(se) - len(usage) - 1]:
                    cases.append([argv, se[len(head):len(se) - len(usage) - 1]])   # the sub-command's own refusal: why
                else:
                    cases.append([argv, rc, so, se])
            doc["cases"][sub] = cases
        doc["cases"]["main"] = [[argv, rc, so, se] for argv, (rc, so, se) in zip(DISPATCH, record(DISPATCH))]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("{\n \"commit\": %s,\n \"markers\": %s,\n \"usage\": %s,\n \"valid\": %s,\n \"cases\": {\n" % (
            json.dumps(commit), json.dumps({"valid": VALID}), json.dumps(doc["usage"], indent=1).replace("\n", "\n "),
            json.dumps(doc["valid"])))
        for n, (sub, cases) in enumerate(doc["cases"].items()):
            f.write("  %s: [\n" % json.dumps(sub))
            f.write(",\n".join("   " + json.dumps(c) for c in cases))
            f.write("\n  ]%s\n" % ("," if n + 1 < len(doc["cases"]) else ""))
        f.write(" }\n}\n")
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes;", sum(len(c) for c in doc["cases"].values()), "cases:",
          " ".join("%s %d" % (s, len(c)) for s, c in doc["cases"].items()))


if __name__ == "__main__":
    main()
