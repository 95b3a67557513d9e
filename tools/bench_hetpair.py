"""Measurements of the heterozygous k-mer pairs (K-HETPAIR, `smudge`, `run --smudge`; profiles/hetpair_measure.txt):
  kernel  pf_kernel_time(PF_K_HETPAIR) of pf_hetpairs on device pointers over the synth generator's tetraploid database (--genome
          bases, about 1.2 keys a base, k = 25, depth 20: every key in range), pairs wanted and not, beside K-MASK on the same table in the
          same session (reads of 150 cut from the first haplotype with 1 % substitutions, device pointers) -- both as look-ups a second;
          --kernel-reps alternating repetitions behind a warm-up, median and range;
  table   the table kernel alone (pf_hetpair_table) over --table-pairs compacted counters: all pairs in one cell against pairs uniform
          over the cells;
  wall    `smudge -d` on that database, and `run --smudge` against `run` (--chain-cli: the parent commit's binary for the side without
          the option) on the pair of tools/bench_run_trim.py; a warm-up, then --reps alternating repetitions.
  python tools/bench_hetpair.py --work <scratch directory> [--genome 16000000] [--chain-cli PATH] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_run_trim as brt  # noqa: E402
from ploidyfrost_amd import hipapi, synth  # noqa: E402

CLI = brt.CLI
K, LO, HI = 25, 10, 100


def reads_of(hap, n_reads, n, rng):
    """n_reads reads of n bases cut from a haplotype (2-bit codes) with 1 % substitutions, packed back to back as text"""
    starts = rng.integers(0, len(hap) - n, size=n_reads)
    codes = hap[starts[:, None] + np.arange(n)[None, :]]
    sub = rng.random(codes.shape) < 0.01
    codes = np.where(sub, (codes + rng.integers(1, 4, size=codes.shape)) & 3, codes).astype(np.uint8)
    text = synth.BASES[codes].reshape(-1)
    return text, (np.arange(n_reads, dtype=np.uint64) * n), np.full(n_reads, n, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=16000000)
    ap.add_argument("--mask-reads", type=int, default=1000000)
    ap.add_argument("--table-pairs", type=int, default=10000000)
    ap.add_argument("--run-genome", type=int, default=470000)
    ap.add_argument("--run-depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--chain-cli", default=CLI)
    ap.add_argument("--skip-wall", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the database ----
    haps = synth.make_haplotypes(synth.HapSpec(genome_len=a.genome, ploidy=4, seed=4))
    km, mult = synth.canonical_counts(haps, K)
    ct = synth.synth_counts(km, mult, depth=20, jitter=3)
    say("database: the synth generator's tetraploid, genome %d, k %d, depth 20: %d keys; bounds [%d, %d]" % (a.genome, K, len(km), LO, HI))
    rng = np.random.default_rng(7)
    text, off, ln = reads_of(haps[0], a.mask_reads, 150, rng)

    dev = hipapi.Device(0)
    dk = torch.from_numpy(km.view(np.int64)).cuda()
    dc = torch.from_numpy(ct.view(np.int32)).cuda()
    dev.upload_counts(dk, dc, 1, 0xFFFFFFFF, True, k=K)
    t_in = torch.from_numpy(text).cuda()
    t_out = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
    d_off, d_len = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ln.view(np.int32)).cuda()
    dev.enable_timing(True)
    ms = {k: [] for k in ("pairs", "stats_only", "mask")}
    st, windows = None, 0
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up (it allocates the workspaces)
        got = {}
        dev.reset_timing()
        st = dev.hetpairs(dk, dc, K, LO, HI)["stats"]
        got["pairs"] = dev.kernel_time(hipapi.K_HETPAIR)[0]
        dev.reset_timing()
        dev.hetpairs(dk, dc, K, LO, HI, want_pairs=False, want_table=False)
        got["stats_only"] = dev.kernel_time(hipapi.K_HETPAIR)[0]
        dev.reset_timing()
        _, mst = dev.mask_reads(t_in, d_off, d_len, 5, out=t_out)
        got["mask"] = dev.kernel_time(hipapi.K_MASK)[0]
        windows = mst["kmers"]
        if rep:
            for k, v in got.items():
                ms[k].append(v)
    first = 3 * K * st["in_range"]
    say("pf_hetpairs on device pointers [ms], statistics %s:" % json.dumps(st))
    say("  table and pairs wanted (flag, scan, write, table; the four result arrays are allocated inside): %s" % brt.med(ms["pairs"]))
    say("  statistics alone (the flag kernel): %s" % brt.med(ms["stats_only"]))
    say("  look-ups: 3k a key in range = %d, and 3k more for every key with one partner above it (between %d and %d of them)" %
        (first, st["pairs"], st["one_partner"]))
    lo_rate = (first + 3 * K * st["pairs"]) / statistics.median(ms["stats_only"]) / 1e6
    hi_rate = (first + 3 * K * st["one_partner"]) / statistics.median(ms["stats_only"]) / 1e6
    say("  rate of the flag kernel: %.1f to %.1f G look-ups/s" % (lo_rate, hi_rate))
    say("K-MASK on the same table, same session (pf_mask_reads, %d reads of 150 with 1 %% substitutions, device pointers) [ms]: %s; %d windows: %.1f G look-ups/s"
        % (a.mask_reads, brt.med(ms["mask"]), windows, windows / statistics.median(ms["mask"]) / 1e6))

    # ---- the table kernel alone ----
    n = a.table_pairs
    W = HI - LO + 1
    one = torch.full((n,), 20, dtype=torch.int32, device="cuda")
    ua = torch.from_numpy((LO + rng.integers(0, W, size=n)).astype(np.int32)).cuda()
    ub = torch.from_numpy((LO + rng.integers(0, W, size=n)).astype(np.int32)).cuda()
    tms = {"one_cell": [], "uniform": []}
    for rep in range(a.kernel_reps + 1):
        dev.reset_timing()
        t1 = dev.hetpair_table(one, one, LO, HI)
        t_one = dev.kernel_time(hipapi.K_HETPAIR)[0]
        dev.reset_timing()
        t2 = dev.hetpair_table(ua, ub, LO, HI)
        t_uni = dev.kernel_time(hipapi.K_HETPAIR)[0]
        assert int(t1[20 - LO, 20 - LO]) == n == int(t2.sum())
        if rep:
            tms["one_cell"].append(t_one)
            tms["uniform"].append(t_uni)
    say("the table kernel alone over %d compacted pairs, W = %d [ms]: all in one cell %s; uniform over the cells %s; ratio %.2f" %
        (n, W, brt.med(tms["one_cell"]), brt.med(tms["uniform"]), statistics.median(tms["one_cell"]) / statistics.median(tms["uniform"])))
    dev.close()
    del dk, dc, t_in, t_out, one, ua, ub

    # ---- wall ----
    if not a.skip_wall:
        db = os.path.join(a.work, "tetra")
        synth.write_kmc1(db, km, ct, K)
        brt.timed([CLI, "smudge", "-d", db, "-l", LO, "-u", HI, "-n", 20, "-o", "t"], a.work)
        wall = []
        r = None
        for _ in range(a.reps):
            dt, r = brt.timed([CLI, "smudge", "-d", db, "-l", LO, "-u", HI, "-n", 20, "-o", "t", "-v"], a.work)
            wall.append(dt)
        say("wall, `smudge -d` on that database [s]: %s" % brt.med(wall))
        for l in r.stderr.splitlines():
            say("  " + l)
        r1, r2 = brt.write_pair(a.work, a.run_genome, a.run_depth)
        say("the side without --smudge: %s" % ("this tree's binary" if a.chain_cli == CLI else "the parent commit's binary"))
        theirs, mine = [a.chain_cli, "run", "-i", r1, "-i", r2, "-o", "s"], [CLI, "run", "-i", r1, "-i", r2, "-o", "s", "--smudge", "--smudge-n", a.run_depth // 2]
        cd, md = os.path.join(a.work, "run_theirs"), os.path.join(a.work, "run_mine")
        os.makedirs(cd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        brt.timed(theirs, cd)
        brt.timed(mine, md)
        wall_c, wall_m = [], []
        for _ in range(a.reps):
            wall_c.append(brt.timed(theirs, cd)[0])
            dt, r = brt.timed(mine, md)
            wall_m.append(dt)
        od = "PloidyFrost_output"
        same = all(open(os.path.join(cd, od, f), "rb").read() == open(os.path.join(md, od, f), "rb").read() for f in os.listdir(os.path.join(cd, od)))
        say("wall, `run` (genome %d, depth %d, reads of 100) [s]: %s" % (a.run_genome, a.run_depth, brt.med(wall_c)))
        say("wall, `run --smudge` [s]: %s; every other file the same bytes: %s" % (brt.med(wall_m), same))
        for l in brt.timed(mine + ["-v"], md)[1].stderr.splitlines():   # the stage time, from a run of its own
            if l.startswith("smudge: "):
                say("  " + l)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({k: statistics.median(v) for k, v in list(ms.items()) + list(tms.items())}))


if __name__ == "__main__":
    main()
