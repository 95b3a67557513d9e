"""Measurements of adapter clipping (K-CLIP, `--adapters`; profiles/clip_measure.txt):
  kernel  pf_kernel_time on one chunk of the first file on device pointers: pf_trim_fastq with a clip open beside pf_trim_fastq
          without (PF_K_TRIM), and PF_K_CLIP alone; --kernel-reps alternating repetitions behind a warm-up, median and range; the
          clip's counters (how many candidates reached the scoring stage); the host rule on one core over the same chunk, for scale;
  wall    `run --adapters ... STEP...` on the raw pair against `run STEP...` (--chain-cli: the parent commit's binary) on files
          clipped beforehand by the host rule, whose cost is stated separately; a warm-up, then --reps alternating repetitions.
Inputs: the pair of tools/bench_run_trim.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded
qualities) with an adapter read-through planted in --share of the reads: the read keeps an insert of 20 .. 95 bases, then runs into
the adapter of its file (seeded adapters of 33 and 41 bases, named /1 and /2, and one of 58 for both files).
  python tools/bench_clip.py --work <scratch directory> --genome 470000 --depth 64 [--share 0.2] [--chain-cli PATH] [--out FILE]"""
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

import bench_run_trim as brt  # noqa: E402
from ploidyfrost_amd import hipapi, hostapi  # noqa: E402

CLI = brt.CLI
STEPS = brt.STEPS


def make_adapters():
    rng = random.Random(17)
    return [(bytes(rng.choice(b"ACGT") for _ in range(m)), side) for m, side in ((33, 1), (41, 2), (58, 0))]


def adapters_fa(adapters):
    return b"".join(b">a%d%s\n%s\n" % (i, (b"", b"/1", b"/2")[side], ad) for i, (ad, side) in enumerate(adapters))


def plant(path, adapters, side, share, seed):
    """rewrites the FASTQ file with read-through in `share` of its reads; returns the number planted"""
    rng = np.random.default_rng(seed)
    mine = [a for a, s in adapters if s in (0, side)]
    lines = open(path, "rb").read().split(b"\n")
    n_rec, planted = len(lines) // 4, 0
    hit = rng.random(n_rec) < share
    insert = rng.integers(20, 96, size=n_rec)
    which = rng.integers(0, len(mine), size=n_rec)
    filler = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=256))
    for r in np.flatnonzero(hit):
        seq = lines[4 * r + 1]
        lines[4 * r + 1] = (seq[:insert[r]] + mine[which[r]] + filler)[:len(seq)]
        planted += 1
    open(path, "wb").write(b"\n".join(lines))
    return planted


def clip_file(src, dst, adapters, side):
    """the file clipped by the host rule (one core): a dropped read keeps its record with empty lines; seconds spent in the rule"""
    text = open(src, "rb").read()
    t = time.perf_counter()
    got = hostapi.trim_fastq_chunk_clip(text, [], adapters, side=side)
    dt = time.perf_counter() - t
    lines = text.split(b"\n")
    for r, (b, ln) in enumerate(zip(got["begin"], got["len"])):
        lines[4 * r + 1] = lines[4 * r + 1][:ln]
        lines[4 * r + 3] = lines[4 * r + 3][:ln]
    open(dst, "wb").write(b"\n".join(lines))
    return dt, got["clip"]


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

    adapters = make_adapters()
    ad_path = os.path.join(a.work, "adapters.fa")
    open(ad_path, "wb").write(adapters_fa(adapters))
    r1, r2 = brt.write_pair(a.work, a.genome, a.depth)
    planted = [plant(p, adapters, f + 1, a.share, 100 + f) for f, p in enumerate((r1, r2))]
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes; read-through planted in %d + %d reads (share %.2f), inserts of 20 .. 95 bases; "
        "3 adapters of 33 (/1), 41 (/2) and 58 bases" % (a.genome, a.depth, os.path.getsize(r1), os.path.getsize(r2), planted[0], planted[1], a.share))

    # ---- kernels: one chunk of r1 on device pointers ----
    raw = open(r1, "rb").read()
    cut = raw.rfind(b"\n@r", 0, min(len(raw), 48 << 20)) + 1 if len(raw) > (48 << 20) else len(raw)
    chunk = raw[:cut]
    dev = hipapi.Device(0)
    t_in = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).cuda()
    t_out = torch.zeros(len(chunk) + 16, dtype=torch.uint8, device="cuda")
    dev.enable_timing(True)
    plain, clipped, clip_alone = [], [], []
    stats = None
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        dev.reset_timing()
        dev.trim_fastq(t_in, STEPS, out=t_out)
        ms_plain = dev.kernel_time(hipapi.K_TRIM)[0]
        dev.reset_timing()
        dev.clip_begin(adapters)
        r = dev.trim_fastq(t_in, STEPS, out=t_out)
        ms_clip, ms_k = dev.kernel_time(hipapi.K_TRIM)[0], dev.kernel_time(hipapi.K_CLIP)[0]
        stats = dev.clip_stats()
        dev.clip_end()
        if rep:
            plain.append(ms_plain)
            clipped.append(ms_clip)
            clip_alone.append(ms_k)
    n_rec = r["n_records"]
    say("kernel time on one chunk of %d bytes of r1 (%d records), device pointers [ms]:" % (len(chunk), n_rec))
    say("  pf_trim_fastq without a clip: %s" % brt.med(plain))
    say("  pf_trim_fastq with a clip open: %s" % brt.med(clipped))
    say("  PF_K_CLIP alone (inside the call above): %s" % brt.med(clip_alone))
    offsets = n_rec * sum(100 + len(ad) - 31 for ad, s in adapters if s in (0, 1))
    say("  the clip's counters: reads_clipped %d, reads_dropped %d, bases_clipped %d, candidates_scored %d of %d (adapter, offset) candidates: the rest of "
        "PF_K_CLIP's time is staging and the seed scan (the kernel has no timer of its own for the scoring stage)" %
        (stats["reads_clipped"][0], stats["reads_dropped"][0], stats["bases_clipped"][0], stats["candidates_scored"][0], offsets))
    t = time.perf_counter()
    host = hostapi.trim_fastq_chunk_clip(chunk, STEPS, adapters, side=1)
    say("  the host rule on one core over the same chunk (pfh_trim_fastq_chunk_clip, clipping and steps): %.3f s; same (begin, len) as the device: %s" %
        (time.perf_counter() - t, host["begin"] == r["begin"].tolist() and host["len"] == r["len"].tolist()))
    dev.close()

    # ---- wall ----
    c1, c2 = os.path.join(a.work, "c1.fq"), os.path.join(a.work, "c2.fq")
    cost = [clip_file(r1, c1, adapters, 1), clip_file(r2, c2, adapters, 2)]
    say("clipping beforehand (the host rule on one core, not part of the chain's time below): %.3f + %.3f s; %d + %d reads clipped, %d + %d dropped" %
        (cost[0][0], cost[1][0], cost[0][1]["reads_clipped"][0], cost[1][1]["reads_clipped"][1], cost[0][1]["reads_dropped"][0], cost[1][1]["reads_dropped"][1]))
    say("chain binary: %s" % ("this tree's" if a.chain_cli == CLI else a.chain_cli))
    cd, md = os.path.join(a.work, "chain"), os.path.join(a.work, "mine")
    os.makedirs(cd, exist_ok=True)
    os.makedirs(md, exist_ok=True)
    theirs = [a.chain_cli, "run", "-1", c1, "-2", c2, "-o", "s", "-v"] + STEPS
    mine = [CLI, "run", "-1", r1, "-2", r2, "--adapters", ad_path, "-o", "r", "-v"] + STEPS
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
    say("wall, `run STEP...` on the files clipped beforehand [s]: %s" % brt.med(wall_c))
    say("  " + [l for l in rc.stderr.splitlines() if l.startswith("run: count ")][-1])
    say("wall, `run --adapters STEP...` on the raw pair [s]: %s" % brt.med(wall_m))
    say("  " + [l for l in rm.stderr.splitlines() if l.startswith("run: count ")][-1])
    for word in ("clip: ", "trim: ", "run: reads "):
        say("  " + [l for l in rm.stderr.splitlines() if l.startswith(word)][-1])
    say("  same allele_frequency / bicov / super_bubble / Unitig_Id bytes on both sides: %s; rows in allele_frequency.txt: %d" %
        (same, open(os.path.join(md, od, "r_allele_frequency.txt")).read().count("\n")))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"trim_ms": statistics.median(plain), "trim_clip_ms": statistics.median(clipped), "clip_ms": statistics.median(clip_alone),
                      "wall_clipped_files_s": statistics.median(wall_c), "wall_run_adapters_s": statistics.median(wall_m)}))


if __name__ == "__main__":
    main()
