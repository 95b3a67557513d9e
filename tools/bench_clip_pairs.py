"""Measurements of palindrome adapter clipping (K-PALIN, `--adapter-pairs`; profiles/clip_pairs_measure.txt):
  kernel   pf_kernel_time on one chunk of each file of the pair on device pointers: pf_trim_fastq_pair with no clip, with the simple
           adapters, with the prefix pair alone and with both (PF_K_TRIM), PF_K_CLIP alone and PF_K_PALIN alone inside those calls;
           --kernel-reps alternating repetitions behind a warm-up, median and range; the counters; the host rule on one core over the
           same chunks, for scale;
  wall     `run --adapters f --adapter-pairs --adapter-keep-both -1 -2 STEP...` on the raw pair against `run -1 -2 STEP...`
           (--chain-cli: the parent commit's binary) on files clipped beforehand by the host rule, whose cost is stated separately;
           a warm-up, then --reps alternating repetitions;
  clipped  the pairs clipped by simple mode alone, by pair mode alone and by both, and the rows of allele_frequency.txt with and
           without the switch.
Inputs: the pair of tools/bench_run_trim.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded
qualities) with read-through planted in --share of the pairs: both reads keep an insert of 20 .. 99 bases (the first bases of read 1
and their reverse complement), then run into the reverse complement of the other side's prefix and the simple adapter of their file
behind it.  One seeded prefix pair of 34 bases; the three seeded simple adapters of tools/bench_clip.py.
  python tools/bench_clip_pairs.py --work <scratch directory> --genome 470000 --depth 64 [--share 0.2] [--chain-cli PATH] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_clip as bc  # noqa: E402
import bench_run_trim as brt  # noqa: E402
from ploidyfrost_amd import hipapi, hostapi  # noqa: E402

CLI = brt.CLI
STEPS = brt.STEPS
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def make_prefix_pair():
    rng = random.Random(23)
    return tuple(bytes(rng.choice(b"ACGT") for _ in range(34)) for _ in range(2))


def adapters_fa(adapters, prefix):
    return b">PrefixPE/1\n%s\n>PrefixPE/2\n%s\n" % prefix + bc.adapters_fa(adapters)


def plant(r1, r2, adapters, prefix, share, seed):
    """rewrites the two FASTQ files with read-through in `share` of the pairs; returns (pairs planted, of them with 1 .. 15 adapter bases)"""
    rng = np.random.default_rng(seed)
    a1 = [a for a, s in adapters if s == 1][0]
    a2 = [a for a, s in adapters if s == 2][0]
    tail1, tail2 = revcomp(prefix[1]) + a1, revcomp(prefix[0]) + a2
    l1, l2 = (open(p, "rb").read().split(b"\n") for p in (r1, r2))
    n_rec = min(len(l1), len(l2)) // 4
    hit = rng.random(n_rec) < share
    insert = rng.integers(20, 100, size=n_rec)
    filler = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=256))
    short = 0
    for r in np.flatnonzero(hit):
        s1, s2 = l1[4 * r + 1], l2[4 * r + 1]
        ins = s1[:insert[r]]
        l1[4 * r + 1] = (ins + tail1 + filler)[:len(s1)]
        l2[4 * r + 1] = (revcomp(ins) + tail2 + filler)[:len(s2)]
        short += len(s1) - insert[r] < 16
    open(r1, "wb").write(b"\n".join(l1))
    open(r2, "wb").write(b"\n".join(l2))
    return int(hit.sum()), int(short)


def cut_lines(text, ends):
    lines = text.split(b"\n")
    for r, e in enumerate(ends):
        lines[4 * r + 1] = lines[4 * r + 1][:e]
        lines[4 * r + 3] = lines[4 * r + 3][:e]
    return b"\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=470000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--share", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--chain-cli", default=CLI)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    adapters, prefix = bc.make_adapters(), make_prefix_pair()
    both_sets = (adapters, [prefix])
    ad_path = os.path.join(a.work, "adapters.fa")
    open(ad_path, "wb").write(adapters_fa(adapters, prefix))
    r1, r2 = brt.write_pair(a.work, a.genome, a.depth)
    planted, short = plant(r1, r2, adapters, prefix, a.share, 100)
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes; read-through planted in %d pairs (share %.2f), inserts of 20 .. 99 bases, "
        "%d of them leave 1 .. 15 adapter bases; one prefix pair of 34 bases, 3 simple adapters of 33 (/1), 41 (/2) and 58 bases" %
        (a.genome, a.depth, os.path.getsize(r1), os.path.getsize(r2), planted, a.share, short))

    # ---- kernels: the two files as one chunk each on device pointers ----
    raw = [open(p, "rb").read() for p in (r1, r2)]
    dev = hipapi.Device(0)
    t_in = [torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda() for t in raw]
    t_out = [torch.zeros(len(raw[d // 2]) + 16, dtype=torch.uint8, device="cuda") for d in range(4)]
    dev.enable_timing(True)
    modes = (("no clip", None), ("the simple adapters (pf_clip_begin)", lambda: dev.clip_begin(adapters)),
             ("the prefix pair alone (pf_clip_begin_pairs, n_adapters = 0)", lambda: dev.clip_begin_pairs([], [prefix], keep_both=True)),
             ("the simple adapters and the prefix pair", lambda: dev.clip_begin_pairs(adapters, [prefix], keep_both=True)))
    trim_ms = {m: [] for m, _ in modes}
    clip_ms = {m: [] for m, _ in modes}
    palin_ms = {m: [] for m, _ in modes}
    counters, got = {}, None
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        for m, begin in modes:
            dev.reset_timing()
            if begin:
                begin()
            got = dev.trim_fastq_pair(t_in[0], t_in[1], STEPS, outs=t_out)
            t, c, p = dev.kernel_time(hipapi.K_TRIM)[0], dev.kernel_time(hipapi.K_CLIP)[0], dev.kernel_time(hipapi.K_PALIN)[0]
            if begin:
                counters[m] = (dev.clip_stats(), dev.clip_pair_stats() if "prefix" in m else None)
                dev.clip_end()
            if rep:
                trim_ms[m].append(t)
                clip_ms[m].append(c)
                palin_ms[m].append(p)
    n_rec = got["n_records"]
    say("kernel time on one chunk of each file (%d + %d bytes, %d pairs), device pointers [ms]:" % (len(raw[0]), len(raw[1]), n_rec))
    for m, _ in modes:
        say("  pf_trim_fastq_pair with %s: %s" % (m, brt.med(trim_ms[m])))
    m_simple, m_pairs, m_both = modes[1][0], modes[2][0], modes[3][0]
    say("  PF_K_CLIP alone (both files, inside the call with the simple adapters): %s" % brt.med(clip_ms[m_simple]))
    say("  PF_K_PALIN alone (inside the call with the prefix pair alone): %s" % brt.med(palin_ms[m_pairs]))
    say("  PF_K_CLIP and PF_K_PALIN inside the call with both: %s and %s" % (brt.med(clip_ms[m_both]), brt.med(palin_ms[m_both])))
    cs, ps = counters[m_both]
    cand = n_rec * (100 - 8 + 1)
    say("  the counters of the call with both: reads_clipped %d + %d, reads_dropped %d + %d, bases_clipped %d + %d; pairs_clipped %d, pairs_dropped %d, "
        "pairs_too_long %d, candidates_scored %d of at most %d (prefix pair, I) candidates (a pair ends its search at the first passing I): the rest of "
        "PF_K_PALIN's time is staging and the seed test (the kernel has no timer of its own for its stages)" %
        (cs["reads_clipped"][0], cs["reads_clipped"][1], cs["reads_dropped"][0], cs["reads_dropped"][1], cs["bases_clipped"][0], cs["bases_clipped"][1],
         ps["pairs_clipped"], ps["pairs_dropped"], ps["pairs_too_long"], ps["candidates_scored"], cand))
    dev.close()
    t = time.perf_counter()
    host = hostapi.trim_fastq_pair_chunk_clip(raw[0], raw[1], STEPS, both_sets, keep_both=True)
    dt_both = time.perf_counter() - t
    say("  the host rule on one core over the same chunks (pfh_trim_fastq_pair_chunk_clip, both modes and the steps): %.3f s; same (begin, len) as the device: %s" %
        (dt_both, all(host["begin"][f] == got["begin"][f].tolist() and host["len"][f] == got["len"][f].tolist() for f in range(2))))

    # ---- what is clipped ----
    ends = host   # (the clip ends do not depend on the steps)
    simple = [hostapi.trim_fastq_chunk_clip(raw[f], [], adapters, side=f + 1)["len"] for f in range(2)]
    n = [[len(x) for x in raw[f].split(b"\n")[1::4]] for f in range(2)]
    by_simple = np.array([simple[0][r] != n[0][r] or simple[1][r] != n[1][r] for r in range(n_rec)])
    final = np.array([ends["clip_end"][0][r] != simple[0][r] or ends["clip_end"][1][r] != simple[1][r] for r in range(n_rec)])
    say("what is clipped, of %d pairs (the host rule; pair mode counted where it moves an end below simple mode's): by simple mode alone %d, by pair mode alone %d, "
        "by both %d; K-PALIN's own count of pairs with a passing I: %d" %
        (n_rec, int((by_simple & ~final).sum()), int((~by_simple & final).sum()), int((by_simple & final).sum()), ends["pairs"]["pairs_clipped"] + ends["pairs"]["pairs_dropped"]))

    # ---- wall ----
    c1, c2 = os.path.join(a.work, "c1.fq"), os.path.join(a.work, "c2.fq")
    open(c1, "wb").write(cut_lines(raw[0], ends["clip_end"][0]))
    open(c2, "wb").write(cut_lines(raw[1], ends["clip_end"][1]))
    say("clipping beforehand (the host rule on one core, both modes; the call above, not part of the chain's time below): %.3f s" % dt_both)
    say("chain binary: %s" % ("this tree's" if a.chain_cli == CLI else a.chain_cli))
    cd, md, sd = os.path.join(a.work, "chain"), os.path.join(a.work, "mine"), os.path.join(a.work, "simple")
    for d in (cd, md, sd):
        os.makedirs(d, exist_ok=True)
    theirs = [a.chain_cli, "run", "-1", c1, "-2", c2, "-o", "s", "-v"] + STEPS
    mine = [CLI, "run", "-1", r1, "-2", r2, "--adapters", ad_path, "--adapter-pairs", "--adapter-keep-both", "-o", "r", "-v"] + STEPS
    brt.timed(theirs, cd)   # warm-up (and the page cache)
    brt.timed(mine, md)
    wall_c, wall_m = [], []
    for _ in range(a.reps):
        dt, rc = brt.timed(theirs, cd)
        wall_c.append(dt)
        dt, rm = brt.timed(mine, md)
        wall_m.append(dt)
    od = "PloidyFrost_output"
    same = all(open(os.path.join(cd, od, "s_" + s + ".txt"), "rb").read() == open(os.path.join(md, od, "r_" + s + ".txt"), "rb").read()
               for s in ("allele_frequency", "bicov", "super_bubble", "Unitig_Id"))
    say("wall, `run -1 -2 STEP...` on the files clipped beforehand [s]: %s" % brt.med(wall_c))
    say("  " + [l for l in rc.stderr.splitlines() if l.startswith("run: count ")][-1])
    say("wall, `run --adapters f --adapter-pairs --adapter-keep-both -1 -2 STEP...` on the raw pair [s]: %s" % brt.med(wall_m))
    say("  " + [l for l in rm.stderr.splitlines() if l.startswith("run: count ")][-1])
    for word in ("clip: ", "trim: ", "run: reads "):
        say("  " + [l for l in rm.stderr.splitlines() if l.startswith(word)][-1])
    _, rs = brt.timed([CLI, "run", "-1", r1, "-2", r2, "--adapters", ad_path, "-o", "q", "-v"] + STEPS, sd)
    rows = lambda d, p: open(os.path.join(d, od, p + "_allele_frequency.txt")).read().count("\n")
    say("  same allele_frequency / bicov / super_bubble / Unitig_Id bytes on both sides: %s; rows in allele_frequency.txt: %d with the switch, %d with --adapters alone" %
        (same, rows(md, "r"), rows(sd, "q")))
    say("  without the switch: " + [l for l in rs.stderr.splitlines() if l.startswith("clip: ")][-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"trim_pair_ms": statistics.median(trim_ms[modes[0][0]]), "trim_pair_both_ms": statistics.median(trim_ms[m_both]),
                      "clip_ms": statistics.median(clip_ms[m_simple]), "palin_ms": statistics.median(palin_ms[m_pairs]),
                      "wall_clipped_files_s": statistics.median(wall_c), "wall_run_pairs_s": statistics.median(wall_m)}))


if __name__ == "__main__":
    main()
