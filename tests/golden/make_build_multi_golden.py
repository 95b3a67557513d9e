#!/usr/bin/env python3
"""Regenerate the fixtures of `ploidyfrost build-multi` under tests/golden/build_mc3_k25 and tests/golden/build_mc2_k7.

Needs the reference's Bifrost and this repository's dump helper built by ``make -f oracle/Makefile.ref`` (oracle/_ref/Bifrost,
oracle/_ref/colors_dump).  Each folder holds
    s0.fq s1.fq ...  seeded synthetic reads of one sample each: every sample drawn from two haplotypes all samples share, plus SNPs of
                     its own; both strands; substitution errors (most of them in a read's last bases) that make tips
    none.gfa none.colors.txt id.gfa id.colors.txt
                     what ``Bifrost build -c -k <k> [-i -d] -r s0.fq -r s1.fq ...`` 1.0.6 wrote (the H and S lines of it), and
                     colors_dump's reading of its pair of files (the .bfg_colors itself is not kept: its slots depend on Bifrost's
                     random seeds)
    meta.json        k and the generator's settings
The fixtures are data (inputs and what the binaries wrote for them); no reference source is stored.

The seed of build_mc3_k25 is picked so that the CPU oracle (pyoracle.ColoredOracle) calls at least one site on Bifrost's own -i -d graph
with databases counted from the reads (ci = 1); main() checks that and fails otherwise.

usage: python tests/golden/make_build_multi_golden.py
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
DUMP = os.path.join(ROOT, "oracle", "_ref", "colors_dump")
COMP = str.maketrans("ACGT", "TGCA")
FLAG_FILES = {"none": [], "id": ["-i", "-d"]}
CASES = {
    "build_mc3_k25": dict(k=25, seed=3263, samples=3, genome=800, snp_every=150, private_every=400, read_len=100, depth=16, err=0.002, tail=20,
                          tail_err=0.03),
    "build_mc2_k7": dict(k=7, seed=271, samples=2, genome=140, snp_every=45, private_every=60, read_len=40, depth=6, err=0.005, tail=0, tail_err=0.0),
}
CUTOFFS = (2, 1000)   # of the oracle check: every k-mer seen twice


def make_samples(seed, samples, genome, snp_every, private_every, read_len, depth, err, tail, tail_err, **_):
    rng = random.Random(seed)
    h0 = [rng.choice("ACGT") for _ in range(genome)]
    h1 = list(h0)
    for at in range(snp_every // 2, genome - 30, snp_every):
        h1[at] = rng.choice([c for c in "ACGT" if c != h1[at]])
    out = []
    for s in range(samples):
        haps = [list(h0), list(h1)]
        for at in range(private_every // 3 + 37 * s, genome - 30, private_every):   # this sample's own SNPs, on its second haplotype
            haps[1][at] = rng.choice([c for c in "ACGT" if c != haps[1][at]])
        haps = ["".join(h) for h in haps]
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
        out.append(reads)
    return out


def oracle_calls_a_site(out, k, samples, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import count_cases as cc
    import pyoracle
    from ploidyfrost_amd import synth
    pyoracle.build()
    dbs = []
    for s in range(samples):
        with open(os.path.join(out, "s%d.fq" % s), "rb") as f:
            reads = f.read().split(b"\n")[1::4]
        kmers, counts, _ = cc.ref_count(reads, k, ci=1, cs=10000)
        dbs.append(os.path.join(tmp, "db%d" % s))
        synth.write_kmc1(dbs[-1], kmers, counts, k, counter_size=2, min_count=1, max_count=10 ** 9)
    o = pyoracle.ColoredOracle(os.path.join(out, "id.gfa"), os.path.join(out, "id.colors.txt"), dbs, tmp)
    res = o.run(os.path.join(tmp, "cpu"), "g", [CUTOFFS] * samples)
    size = os.path.getsize(os.path.join(tmp, "cpu", "g_allele_frequency.txt"))
    print("oracle on Bifrost's id graph:", res, "allele_frequency bytes", size)
    return size > 0


def main():
    if not os.path.exists(BIFROST) or not os.path.exists(DUMP):
        sys.exit("oracle/_ref/Bifrost or oracle/_ref/colors_dump is missing: make -f oracle/Makefile.ref")
    for name, spec in CASES.items():
        out = os.path.join(HERE, name)
        os.makedirs(out, exist_ok=True)
        fqs = []
        for s, reads in enumerate(make_samples(**spec)):
            fqs.append(os.path.join(out, "s%d.fq" % s))
            with open(fqs[-1], "w") as f:
                for i, r in enumerate(reads):
                    f.write("@s%dr%d\n%s\n+\n%s\n" % (s, i, r, "I" * len(r)))
        with tempfile.TemporaryDirectory() as tmp:
            for tag, flags in FLAG_FILES.items():
                cmd = [BIFROST, "build", "-c", "-k", str(spec["k"]), "-o", os.path.join(tmp, tag)] + flags
                for fq in fqs:
                    cmd += ["-r", os.path.basename(fq)]   # (run inside the folder: the colours are named s0.fq, s1.fq, ...)
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=out)
                with open(os.path.join(out, tag + ".colors.txt"), "w") as f:
                    subprocess.run([DUMP, os.path.join(tmp, tag + ".gfa"), os.path.join(tmp, tag + ".bfg_colors")], check=True, stdout=f)
                with open(os.path.join(tmp, tag + ".gfa")) as src, open(os.path.join(out, tag + ".gfa"), "w") as dst:
                    dst.writelines(ln for ln in src if ln[0] in "HS")   # (the L lines are two thirds of the file; no reader here uses them)
            if name == "build_mc3_k25" and not oracle_calls_a_site(out, spec["k"], spec["samples"], tmp):
                sys.exit("the oracle calls no site on %s: pick another seed" % name)
        with open(os.path.join(out, "meta.json"), "w") as f:
            json.dump(spec, f, indent=1, sort_keys=True)
            f.write("\n")
        sizes = {n: os.path.getsize(os.path.join(out, n)) for n in sorted(os.listdir(out))}
        assert max(sizes.values()) < 300 * 1024, sizes
        print(name, sizes)


if __name__ == "__main__":
    main()
