"""Measurements of duplicate removal (K-DEDUP, `--dedup`; profiles/dedup_measure.txt).  Every device step runs in a child process
under its own time limit; the first one that fails ends the run.
  kernels  pf_kernel_time on one chunk of each file of the pair on device pointers: PF_K_DEDUP alone (inside pf_trim_fastq_pair),
           pf_trim_fastq_pair (PF_K_TRIM) and pf_count_fastq_pair_trimmed (PF_K_TRIMCOUNT) without and with a dedup open, a table that
           starts at 64 slots against one that never grows; --kernel-reps repetitions behind a warm-up, median and range; the host rule
           on one core over the same chunk;
  keys     pf_dedup_keys over --keys random keys against as many copies of one key (the contended case), device pointers, --kernel-reps
           repetitions behind a warm-up; with
           --big-keys N one more figure for a table that leaves the L2;
  wall     `trim -1 -2 --dedup STEP...` against `trim -1 -2 STEP...`, and `run --dedup -1 -2 STEP...` against `run -1 -2 STEP...` on
           files deduplicated beforehand by the host rule (--chain-cli: the parent commit's binary for the side without the option); a
           warm-up with a warm page cache, then --reps alternating repetitions; the rows of allele_frequency.txt on both sides.
Inputs: the pair of tools/bench_run_trim.py with a fifth of the pairs written a second time later in the stream.
  python tools/bench_dedup.py --work <scratch directory> --genome 470000 --depth 64 [--chain-cli PATH] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import bench_run_trim as brt  # noqa: E402

CLI = brt.CLI
STEPS = brt.STEPS
CHUNK = 32 << 20
LIMITS = dict(kernels=420, keys=300, wall=900)   # seconds a step may take


def records(path):
    """the records of a FASTQ file of four-line records, as bytes each"""
    lines = open(path, "rb").read().split(b"\n")
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def write_inputs(work, genome, depth):
    """d1.fq / d2.fq: the pair with a fifth of its pairs repeated later in the stream; h1.fq / h2.fq: the same deduplicated by the host
    rule (the first copy of every pair of sequences stays)"""
    r1, r2 = brt.write_pair(work, genome, depth)
    a, b = records(r1), records(r2)
    rng = np.random.default_rng(7)
    order = list(range(len(a)))
    for i in np.flatnonzero(rng.random(len(a)) < 0.2):
        order.insert(int(rng.integers(i + 1, len(order) + 1)), int(i))
    paths = [os.path.join(work, n) for n in ("d1.fq", "d2.fq", "h1.fq", "h2.fq")]
    seen, first = set(), []
    for i in order:
        first.append(i not in seen)
        seen.add(i)
    for f, recs in enumerate((a, b)):
        with open(paths[f], "wb") as out:
            out.write(b"".join(recs[i] for i in order))
        with open(paths[2 + f], "wb") as out:
            out.write(b"".join(recs[i] for i, keep in zip(order, first) if keep))
    return paths, len(order), len(a)


def chunk_of(path, n_rec):
    raw = open(path, "rb").read()
    pos = 0
    for _ in range(4 * n_rec):
        pos = raw.index(b"\n", pos) + 1
    return raw[:pos]


def step_kernels(a, say):
    import torch
    from ploidyfrost_amd import hipapi, hostapi
    d1, d2 = os.path.join(a.work, "d1.fq"), os.path.join(a.work, "d2.fq")
    n_rec = min(open(p, "rb").read(CHUNK).count(b"\n") // 4 for p in (d1, d2))
    c1, c2 = chunk_of(d1, n_rec), chunk_of(d2, n_rec)
    dev = hipapi.Device(0)
    t1, t2 = (torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda() for c in (c1, c2))
    outs = [torch.zeros(len(c) + 16, dtype=torch.uint8, device="cuda") for c in (c1, c1, c2, c2)]
    dev.enable_timing(True)
    ms = {k: [] for k in ("trim", "trim_dd", "dedup", "dedup64", "trim_dd64", "count", "count_dd", "count_dedup")}
    stats, kept = None, None
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        got = {}
        dev.reset_timing()
        dev.trim_fastq_pair(t1, t2, STEPS, outs=outs)
        got["trim"] = dev.kernel_time(hipapi.K_TRIM)[0]
        for slots, tag in ((0, ""), (64, "64")):
            dev.dedup_begin(0, slots)
            dev.reset_timing()
            kept = dev.trim_fastq_pair(t1, t2, STEPS, outs=outs)["stats"]
            got["trim_dd" + tag], got["dedup" + tag] = dev.kernel_time(hipapi.K_TRIM)[0], dev.kernel_time(hipapi.K_DEDUP)[0]
            stats = dev.dedup_stats()
            dev.dedup_end()
        for name, on in (("count", False), ("count_dd", True)):
            dev.count_begin(25)
            if on:
                dev.dedup_begin()
            dev.reset_timing()
            dev.count_fastq_pair_trimmed(t1, t2, STEPS)
            got[name] = dev.kernel_time(hipapi.K_TRIMCOUNT)[0]
            if on:
                got["count_dedup"] = dev.kernel_time(hipapi.K_DEDUP)[0]
                dev.dedup_end()
            dev.count_abort()
        if rep:
            for k, v in got.items():
                ms[k].append(v)
    say("kernel time on one chunk of each file (%d + %d bytes, %d pairs), device pointers [ms]:" % (len(c1), len(c2), n_rec))
    say("  PF_K_DEDUP alone, inside pf_trim_fastq_pair (insert and verdict, a table that never grows): %s" % brt.med(ms["dedup"]))
    say("  PF_K_DEDUP with a table that starts at 64 slots (its growths inside it): %s; growths %d" % (brt.med(ms["dedup64"]), stats["growths"]))
    say("  pf_trim_fastq_pair without a dedup: %s" % brt.med(ms["trim"]))
    say("  pf_trim_fastq_pair with a dedup open: %s; from 64 slots: %s" % (brt.med(ms["trim_dd"]), brt.med(ms["trim_dd64"])))
    say("  pf_count_fastq_pair_trimmed without a dedup: %s" % brt.med(ms["count"]))
    say("  pf_count_fastq_pair_trimmed with a dedup open: %s; PF_K_DEDUP inside it: %s" % (brt.med(ms["count_dd"]), brt.med(ms["count_dedup"])))
    say("  the chunk: units %d unique %d duplicates %d max_copies %d; pairs kept whole %d" % (stats["units"], stats["unique"], stats["duplicates"],
                                                                                           stats["max_copies"], kept[0]["both"]))
    t = time.perf_counter()
    host = hostapi.trim_fastq_chunk_dedup(c1, STEPS, text2=c2)
    say("  the host rule on one core over the same chunk (index, trim, key, decision, copy): %.3f s; the same statistics: %s" %
        (time.perf_counter() - t, host["stats"] == kept))
    dev.close()
    return {k: statistics.median(v) for k, v in ms.items()}


def step_keys(a, say):
    import torch
    from ploidyfrost_amd import hipapi
    dev = hipapi.Device(0)
    dev.enable_timing(True)
    res = {}
    sizes = [a.keys] + ([a.big_keys] if a.big_keys else [])
    for n in sizes:
        g = torch.Generator(device="cuda").manual_seed(11)
        rnd = torch.randint(1, 1 << 62, (n, 2), dtype=torch.int64, device="cuda", generator=g)
        one = torch.ones((n, 2), dtype=torch.int64, device="cuda") * 0x123456789
        keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
        for name, keys in (("random", rnd), ("one key", one)):
            if n != a.keys and name == "one key":
                continue
            t = []
            for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
                dev.dedup_begin(0, 4 * n)   # never grows
                dev.reset_timing()
                dev.dedup_keys(keys, keep)
                if rep:
                    t.append(dev.kernel_time(hipapi.K_DEDUP)[0])
                st = dev.dedup_stats()
                dev.dedup_end()
            say("  pf_dedup_keys, %d keys, %s, a table of %d slots (%.1f MB), %d repetitions: %s ms; %.1f M keys/s; kept %d, unique %d, max_copies %d" %
                (n, name, st["slots"], st["slots"] * 32 / 1e6, len(t), brt.med(t), n / 1e3 / statistics.median(t), int(keep.sum()), st["unique"], st["max_copies"]))
            res["%s_%d" % (name.split()[0], n)] = statistics.median(t)
        del rnd, one, keep
    dev.close()
    return res


def step_wall(a, say):
    d1, d2, h1, h2 = (os.path.join(a.work, n) for n in ("d1.fq", "d2.fq", "h1.fq", "h2.fq"))
    say("the side without --dedup: %s" % ("this tree's binary" if a.chain_cli == CLI else "the parent commit's binary (%s)" % a.chain_cli))
    outs = ["-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq"]
    res = {}
    for name, theirs, mine in (("trim -1 -2", [a.chain_cli, "trim", "-1", d1, "-2", d2] + outs + STEPS, [CLI, "trim", "-1", d1, "-2", d2] + outs + STEPS + ["--dedup"]),
                               ("run -1 -2", [a.chain_cli, "run", "-1", h1, "-2", h2, "-o", "s"] + STEPS, [CLI, "run", "-1", d1, "-2", d2, "-o", "s"] + STEPS + ["--dedup"])):
        cd, md = os.path.join(a.work, name.split()[0] + "_theirs"), os.path.join(a.work, name.split()[0] + "_mine")
        os.makedirs(cd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        brt.timed(theirs, cd)   # warm-up (and the page cache)
        brt.timed(mine, md)
        wall_c, wall_m, rm = [], [], None
        for _ in range(a.reps):
            wall_c.append(brt.timed(theirs, cd)[0])
            dt, rm = brt.timed(mine, md)
            wall_m.append(dt)
        say("wall, `%s STEP...`%s [s]: %s" % (name, "" if name.startswith("trim") else " on the files deduplicated by the host rule", brt.med(wall_c)))
        say("wall, `%s --dedup STEP...` [s]: %s" % (name, brt.med(wall_m)))
        for l in rm.stderr.splitlines():
            if l.startswith(("dedup: ", "trim: ")):
                say("  " + l)
        if name.startswith("run"):
            af = [open(os.path.join(d, "PloidyFrost_output", "s_allele_frequency.txt"), "rb").read() for d in (cd, md)]
            say("  allele_frequency.txt: %d rows against %d rows with --dedup; the same bytes: %s" % (af[0].count(b"\n"), af[1].count(b"\n"), af[0] == af[1]))
        res[name] = [statistics.median(wall_c), statistics.median(wall_m)]
    return res


STEPS_OF = dict(kernels=step_kernels, keys=step_keys, wall=step_wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=470000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--big-keys", type=int, default=0)
    ap.add_argument("--chain-cli", default=CLI)
    ap.add_argument("--steps", default="kernels,keys,wall")
    ap.add_argument("--step", default="")   # (a child process: this one step, its lines as JSON on the last line)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.step:
        res = STEPS_OF[a.step](a, say)
        print("RESULT " + json.dumps(dict(lines=lines, res=res)))
        return
    (d1, d2, _, _), n_pairs, n_first = write_inputs(a.work, a.genome, a.depth)
    say("inputs: genome %d, depth %d, reads of 100; %d pairs of which %d are a second copy of an earlier one; files of %d + %d bytes" %
        (a.genome, a.depth, n_pairs, n_pairs - n_first, os.path.getsize(d1), os.path.getsize(d2)))
    result = {}
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for x in sys.argv[1:] if x]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            say("step %s: ended at its time limit of %d s; nothing more is run" % (step, LIMITS[step]))
            break
        if r.returncode:
            say("step %s: failed with status %d; nothing more is run\n%s" % (step, r.returncode, r.stderr[-1500:]))
            break
        got = json.loads(r.stdout.rsplit("RESULT ", 1)[1])
        for l in got["lines"]:
            say(l)
        result[step] = got["res"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
