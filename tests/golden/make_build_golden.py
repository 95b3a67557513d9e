#!/usr/bin/env python3
"""Regenerate the fixtures of `ploidyfrost build` under tests/golden/build_k25 and tests/golden/build_k7.

Needs the reference's Bifrost built by ``make -f oracle/Makefile.ref`` (oracle/_ref/Bifrost).  Each folder holds
    reads.fq   seeded synthetic reads: two haplotypes that differ in SNPs, both strands, substitution errors and a few N -- at
               k = 25 about 1 % of the bases, most of them in the last `tail` bases a read was sequenced with, as qualities fall off
    none.gfa i.gfa d.gfa id.gfa   what ``Bifrost build -k <k> [-i] [-d] -r reads.fq`` 1.0.6 wrote (S and L lines as written)
    meta.json  k and the generator's settings
The fixtures are data (an input and what the binary wrote for it); no reference source is stored.

usage: python tests/golden/make_build_golden.py
"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BIFROST = os.path.join(ROOT, "oracle", "_ref", "Bifrost")
COMP = str.maketrans("ACGT", "TGCA")
FLAG_FILES = {"none": [], "i": ["-i"], "d": ["-d"], "id": ["-i", "-d"]}
CASES = {
    "build_k25": dict(k=25, seed=2511, genome=1600, snp_every=120, read_len=100, depth=24, err=0.002, tail=20, tail_err=0.042),
    "build_k7": dict(k=7, seed=711, genome=160, snp_every=40, read_len=40, depth=6, err=0.005, tail=0, tail_err=0.0),
}


def make_reads(seed, genome, snp_every, read_len, depth, err, tail, tail_err, **_):
    rng = random.Random(seed)
    h0 = [rng.choice("ACGT") for _ in range(genome)]
    h1 = list(h0)
    for at in range(snp_every // 2, genome - 30, snp_every):
        h1[at] = rng.choice([c for c in "ACGT" if c != h1[at]])
    haps = ["".join(h0), "".join(h1)]
    reads = []
    for _ in range(genome * depth // read_len):
        h = rng.choice(haps)
        a = rng.randrange(0, genome - read_len + 1)
        r = list(h[a:a + read_len])
        for j in range(read_len):
            if rng.random() < (tail_err if j >= read_len - tail else err):
                r[j] = rng.choice([c for c in "ACGT" if c != r[j]]) if rng.random() < 0.9 else "N"
        r = "".join(r)
        reads.append(r.translate(COMP)[::-1] if rng.random() < 0.5 else r)
    return reads


def main():
    if not os.path.exists(BIFROST):
        sys.exit("oracle/_ref/Bifrost is missing: make -f oracle/Makefile.ref")
    for name, spec in CASES.items():
        out = os.path.join(HERE, name)
        os.makedirs(out, exist_ok=True)
        reads = make_reads(**spec)
        fq = os.path.join(out, "reads.fq")
        with open(fq, "w") as f:
            for i, r in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
        with tempfile.TemporaryDirectory() as tmp:
            for tag, flags in FLAG_FILES.items():
                subprocess.run([BIFROST, "build", "-k", str(spec["k"]), "-r", fq, "-o", os.path.join(tmp, tag)] + flags, check=True,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                os.replace(os.path.join(tmp, tag + ".gfa"), os.path.join(out, tag + ".gfa"))
        with open(os.path.join(out, "meta.json"), "w") as f:
            json.dump(spec, f, indent=1, sort_keys=True)
            f.write("\n")
        print(name, len(reads), "reads", {t: os.path.getsize(os.path.join(out, t + ".gfa")) for t in FLAG_FILES})


if __name__ == "__main__":
    main()
