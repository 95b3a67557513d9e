"""Measurements of `ploidyfrost run STEP...` (profiles/run_trim_measure.txt):
  wall    the chain it replaces (`trim -1 -2 -o1 -u1 -o2 -u2 STEP...`, then `run -i o1 -i o2`) against `run -1 -2 STEP...`, warm page
          cache, a warm-up and then --reps alternating repetitions; --chain-cli names the binary that runs the chain (the parent
          commit's, to compare against it); `run -v`'s stage times of the last repetition of both;
  kernel  pf_kernel_time on one chunk on device pointers with a count open: pf_count_fastq_trimmed against pf_trim_fastq +
          pf_count_fastq, pf_maskcount_fastq_trimmed against pf_trim_fastq + pf_maskcount_fastq; --kernel-reps alternating
          repetitions behind a warm-up, median and range;
  bytes   what is no longer written, read back or carried over PCIe.
Inputs: tests/golden/make_build_golden.py's generator (build_k25) at --genome and --depth, qualities seeded (most reads flat, a quarter
with a degrading tail, a few per cent low throughout), even records to r1.fq, odd ones to r2.fq.
  python tools/bench_run_trim.py --work <scratch directory> --genome 470000 --depth 64 [--chain-cli PATH] [--out FILE]"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ploidyfrost_amd import hipapi  # noqa: E402

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
STEPS = ["LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20", "MINLEN:50"]
EVERY = dict(ci=1, cx=0xFFFFFFFF, cs=0xFFFFFFFF)


def med(xs):
    return "median %.3f (range %.3f - %.3f)" % (statistics.median(xs), min(xs), max(xs))


def timed(cmd, cwd):
    t = time.perf_counter()
    r = subprocess.run([str(x) for x in cmd], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    dt = time.perf_counter() - t
    if r.returncode:
        sys.exit("failed: %s\n%s\n%s" % (cmd, r.stdout[-1500:], r.stderr[-1500:]))
    return dt, r


def qualities(rng, n_reads, n):
    """one quality line per read: 71 % flat 'I', 25 % a tail that degrades from a random cut (2 .. 24), 4 % '#' throughout"""
    q = np.full((n_reads, n), ord("I"), dtype=np.uint8)
    kind = rng.random(n_reads)
    low = kind < 0.04
    q[low] = ord("#")
    tail = (kind >= 0.04) & (kind < 0.29)
    cut = rng.integers(30, n, size=n_reads)
    noise = (33 + rng.integers(2, 25, size=(n_reads, n))).astype(np.uint8)
    mask = tail[:, None] & (np.arange(n)[None, :] >= cut[:, None])
    q[mask] = noise[mask]
    return [bytes(row) for row in q]


def write_pair(work, genome, depth):
    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tests", "golden", "make_build_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    reads = list(gen.make_reads(**dict(gen.CASES["build_k25"], genome=genome, depth=depth)))
    qual = qualities(np.random.default_rng(2025), len(reads), len(reads[0]))
    paths = [os.path.join(work, "r1.fq"), os.path.join(work, "r2.fq")]
    for f, p in enumerate(paths):
        with open(p, "wb") as out:
            out.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, reads[i].encode(), qual[i]) for i in range(f, len(reads), 2)))
    return paths


def chain(cli, r1, r2, d):
    """the two commands; (wall seconds of each, the last `run`)"""
    os.makedirs(d, exist_ok=True)
    t_trim, _ = timed([cli, "trim", "-1", r1, "-2", r2, "-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq"] + STEPS, d)
    t_run, r = timed([cli, "run", "-i", "o1.fq", "-i", "o2.fq", "-o", "s", "-v"], d)
    return [t_trim, t_run], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=470000)
    ap.add_argument("--depth", type=int, default=64)
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

    t = time.perf_counter()
    r1, r2 = write_pair(a.work, a.genome, a.depth)
    raw_bytes = os.path.getsize(r1) + os.path.getsize(r2)
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes (generated in %.1f s)" %
        (a.genome, a.depth, os.path.getsize(r1), os.path.getsize(r2), time.perf_counter() - t))
    say("chain binary: %s" % ("this tree's" if a.chain_cli == CLI else a.chain_cli))

    # ---- wall ----
    cd, md = os.path.join(a.work, "chain"), os.path.join(a.work, "mine")
    os.makedirs(md, exist_ok=True)
    mine = [CLI, "run", "-1", r1, "-2", r2, "-o", "r", "-v"] + STEPS
    chain(a.chain_cli, r1, r2, cd)   # warm-up (and the page cache)
    timed(mine, md)
    wall_c, wall_m, parts = [], [], []
    for _ in range(a.reps):
        ts, rc = chain(a.chain_cli, r1, r2, cd)
        wall_c.append(sum(ts))
        parts.append(ts)
        dt, rm = timed(mine, md)
        wall_m.append(dt)
    od = "PloidyFrost_output"
    same = all(open(os.path.join(cd, od, "s_" + s + ".txt"), "rb").read() == open(os.path.join(md, od, "r_" + s + ".txt"), "rb").read()
               for s in ("allele_frequency", "bicov", "super_bubble", "Unitig_Id"))
    trimmed_bytes = sum(os.path.getsize(os.path.join(cd, f)) for f in ("o1.fq", "o2.fq"))
    unpaired_bytes = sum(os.path.getsize(os.path.join(cd, f)) for f in ("u1.fq", "u2.fq"))
    say("wall, chain of 2 processes (trim, run) [s]: %s" % med(wall_c))
    say("  per command (trim, run), last repetition: %s" % " ".join("%.3f" % x for x in parts[-1]))
    say("  " + [l for l in rc.stderr.splitlines() if l.startswith("run: count ")][-1])
    say("wall, run with steps [s]: %s" % med(wall_m))
    say("  " + [l for l in rm.stderr.splitlines() if l.startswith("run: count ")][-1])
    say("  " + [l for l in rm.stderr.splitlines() if l.startswith("trim: ")][-1])
    say("  " + [l for l in rm.stderr.splitlines() if l.startswith("run: reads ")][-1])
    say("  same allele_frequency / bicov / super_bubble / Unitig_Id bytes as the chain: %s; rows in allele_frequency.txt: %d" %
        (same, open(os.path.join(md, od, "r_allele_frequency.txt")).read().count("\n")))
    say("bytes: the chain writes %d bytes of trimmed reads (o1, o2) and %d of unpaired ones (u1, u2), and its `run` reads the %d back twice "
        "(two passes) and uploads them twice; `run` with steps writes none of them, and reads and uploads the %d raw bytes twice where "
        "`trim` read and uploaded them once (and downloaded the %d)" % (trimmed_bytes, unpaired_bytes, trimmed_bytes, raw_bytes, trimmed_bytes + unpaired_bytes))

    # ---- kernels: one chunk of r1 on device pointers, a count open ----
    raw = open(r1, "rb").read()
    cut = raw.rfind(b"\n@r", 0, min(len(raw), 48 << 20)) + 1 if len(raw) > (48 << 20) else len(raw)
    chunk = raw[:cut]
    dev = hipapi.Device(0)
    t_in = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).cuda()
    t_out = torch.zeros(len(chunk) + 16, dtype=torch.uint8, device="cuda")
    slots = 2 * len(chunk)
    # the table of the second pass: the trimmed reads' own counts
    dev.count_begin(25, True, slots)
    dev.count_fastq_trimmed(t_in, STEPS)
    km, ct, _ = dev.count_finish(**EVERY)
    dev.upload_counts(km, ct, 1, 0xFFFFFFFF, True, k=25)
    dev.enable_timing(True)
    res = {"count": ([], [], []), "maskcount": ([], [], [])}
    want = {}
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        for what in ("count", "maskcount"):
            masked = what == "maskcount"
            for route in ("fused", "two"):
                dev.reset_timing()
                dev.count_begin(25, True, slots)
                if route == "fused":
                    st = dev.maskcount_fastq_trimmed(t_in, STEPS, 10)[2] if masked else dev.count_fastq_trimmed(t_in, STEPS)[2]
                    ms = [dev.kernel_time(hipapi.K_TRIMCOUNT)[0]]
                    assert dev.kernel_time(hipapi.K_TRIM)[1] == 0
                else:
                    tr = dev.trim_fastq(t_in, STEPS, out=t_out)
                    st = dev.maskcount_fastq(tr["out"], 10)[1] if masked else dev.count_fastq(tr["out"])[1]
                    ms = [dev.kernel_time(hipapi.K_TRIM)[0], dev.kernel_time(hipapi.K_MASKCOUNT if masked else hipapi.K_COUNT)[0]]
                    assert dev.kernel_time(hipapi.K_TRIMCOUNT)[1] == 0
                dev.count_abort()
                assert want.setdefault(what, st) == st, (what, route)       # both routes count the same windows
                if rep:
                    if route == "fused":
                        res[what][0].append(ms[0])
                    else:
                        res[what][1].append(sum(ms))
                        res[what][2].append(ms)
    say("kernel time on one chunk of %d bytes of r1 (%d records, %d reads handed on, %d windows), device pointers, a count open [ms]:" %
        (len(chunk), chunk.count(b"\n") // 4, want["count"]["reads"], want["count"]["kmers"]))
    for what, fused, pair in (("count", "pf_count_fastq_trimmed", "pf_trim_fastq + pf_count_fastq"),
                              ("maskcount", "pf_maskcount_fastq_trimmed", "pf_trim_fastq + pf_maskcount_fastq")):
        say("  %s: %s" % (fused, med(res[what][0])))
        say("  %s: %s (last: %.3f + %.3f)" % (pair, med(res[what][1]), res[what][2][-1][0], res[what][2][-1][1]))
    dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"wall_chain_s": statistics.median(wall_c), "wall_run_steps_s": statistics.median(wall_m),
                      "count_fused_ms": statistics.median(res["count"][0]), "count_two_ms": statistics.median(res["count"][1]),
                      "maskcount_fused_ms": statistics.median(res["maskcount"][0]), "maskcount_two_ms": statistics.median(res["maskcount"][1])}))


if __name__ == "__main__":
    main()
