"""Measurements of the read quality report (K-QC, `qc`, `--report`; profiles/qc_measure.txt):
  kernel  pf_kernel_time on one chunk of the first file on device pointers: PF_K_QC alone (pf_qc_fastq: stage raw), pf_trim_fastq
          (PF_K_TRIM) and pf_count_fastq_trimmed (PF_K_TRIMCOUNT) with and without a report open, and PF_K_QC inside them (both
          stages); --kernel-reps alternating repetitions behind a warm-up, median and range; GB/s of chunk text;
  wall    `trim -1 -2 --report` against `trim -1 -2` and `run -1 -2 STEP... --report` against `run -1 -2 STEP...` (--chain-cli: the
          parent commit's binary for the side without the option); a warm-up with a warm page cache, then --reps alternating
          repetitions.
Inputs: the pair of tools/bench_run_trim.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded qualities).
  python tools/bench_qc.py --work <scratch directory> --genome 470000 --depth 64 [--chain-cli PATH] [--out FILE]"""
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
from ploidyfrost_amd import hipapi, hostapi  # noqa: E402

CLI = brt.CLI
STEPS = brt.STEPS


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

    r1, r2 = brt.write_pair(a.work, a.genome, a.depth)
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes" % (a.genome, a.depth, os.path.getsize(r1), os.path.getsize(r2)))

    # ---- kernels: one chunk of r1 on device pointers ----
    raw = open(r1, "rb").read()
    cut = raw.rfind(b"\n@r", 0, min(len(raw), 48 << 20)) + 1 if len(raw) > (48 << 20) else len(raw)
    chunk = raw[:cut]
    dev = hipapi.Device(0)
    t_in = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).cuda()
    t_out = torch.zeros(len(chunk) + 16, dtype=torch.uint8, device="cuda")
    dev.enable_timing(True)
    ms = {k: [] for k in ("qc_raw", "trim", "trim_rep", "trim_qc", "count", "count_rep", "count_qc")}
    n_rec, tables = 0, None
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        got = {}
        dev.qc_begin()
        dev.reset_timing()
        n_rec = dev.qc_fastq(t_in)[1]
        got["qc_raw"] = dev.kernel_time(hipapi.K_QC)[0]
        dev.qc_end()
        dev.reset_timing()
        dev.trim_fastq(t_in, STEPS, out=t_out)
        got["trim"] = dev.kernel_time(hipapi.K_TRIM)[0]
        dev.qc_begin()
        dev.reset_timing()
        dev.trim_fastq(t_in, STEPS, out=t_out)
        got["trim_rep"], got["trim_qc"] = dev.kernel_time(hipapi.K_TRIM)[0], dev.kernel_time(hipapi.K_QC)[0]
        tables = dev.qc_tables()
        dev.qc_end()
        for name, report in (("count", False), ("count_rep", True)):
            dev.count_begin(25)
            if report:
                dev.qc_begin()
            dev.reset_timing()
            dev.count_fastq_trimmed(t_in, STEPS)
            got[name] = dev.kernel_time(hipapi.K_TRIMCOUNT)[0]
            if report:
                got["count_qc"] = dev.kernel_time(hipapi.K_QC)[0]
                dev.qc_end()
            dev.count_abort()
        if rep:
            for k, v in got.items():
                ms[k].append(v)
    gbs = len(chunk) / 1e6 / statistics.median(ms["qc_raw"])
    say("kernel time on one chunk of %d bytes of r1 (%d records), device pointers [ms]:" % (len(chunk), n_rec))
    say("  PF_K_QC alone (pf_qc_fastq, stage raw): %s; %.1f GB/s of chunk text" % (brt.med(ms["qc_raw"]), gbs))
    say("  pf_trim_fastq without a report: %s" % brt.med(ms["trim"]))
    say("  pf_trim_fastq with a report open: %s; PF_K_QC inside it (raw and kept): %s" % (brt.med(ms["trim_rep"]), brt.med(ms["trim_qc"])))
    say("  pf_count_fastq_trimmed without a report: %s" % brt.med(ms["count"]))
    say("  pf_count_fastq_trimmed with a report open: %s; PF_K_QC inside it: %s" % (brt.med(ms["count_rep"]), brt.med(ms["count_qc"])))
    host = hostapi.qc_fastq_chunk(chunk[: chunk.rfind(b"\n@r", 0, 4 << 20) + 1], steps=STEPS)
    dev.qc_begin()
    dev.trim_fastq(chunk[: chunk.rfind(b"\n@r", 0, 4 << 20) + 1], STEPS)
    say("  the device's tables equal the host rule's on the first 4 MB of the chunk: %s; reads kept in the whole chunk: %d of %d" %
        (bool(np.array_equal(dev.qc_tables(), host["tables"])), int(tables[0][1][1]), int(tables[0][0][1])))
    dev.qc_end()
    dev.close()

    # ---- wall ----
    say("the side without --report: %s" % ("this tree's binary" if a.chain_cli == CLI else "the parent commit's binary (%s)" % a.chain_cli))
    outs = ["-o1", "o1.fq", "-u1", "u1.fq", "-o2", "o2.fq", "-u2", "u2.fq"]
    for name, theirs, mine in (("trim -1 -2", [a.chain_cli, "trim", "-1", r1, "-2", r2] + outs + STEPS, [CLI, "trim", "-1", r1, "-2", r2] + outs + STEPS + ["--report", "rep.tsv"]),
                               ("run -1 -2 STEP...", [a.chain_cli, "run", "-1", r1, "-2", r2, "-o", "s"] + STEPS,
                                [CLI, "run", "-1", r1, "-2", r2, "-o", "s"] + STEPS + ["--report", "rep.tsv"])):
        cd, md = os.path.join(a.work, name.split()[0] + "_theirs"), os.path.join(a.work, name.split()[0] + "_mine")
        os.makedirs(cd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        brt.timed(theirs, cd)   # warm-up (and the page cache)
        brt.timed(mine, md)
        wall_c, wall_m = [], []
        for _ in range(a.reps):
            wall_c.append(brt.timed(theirs, cd)[0])
            dt, rm = brt.timed(mine, md)
            wall_m.append(dt)
        same = all(open(os.path.join(cd, f), "rb").read() == open(os.path.join(md, f), "rb").read() for f in os.listdir(cd) if os.path.isfile(os.path.join(cd, f)))
        say("wall, `%s` [s]: %s" % (name, brt.med(wall_c)))
        say("wall, `%s --report` [s]: %s; every other file the same bytes: %s; report of %d bytes" % (name, brt.med(wall_m), same, os.path.getsize(os.path.join(md, "rep.tsv"))))
        for l in rm.stderr.splitlines():
            if l.startswith("qc: "):
                say("  " + l)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({k: statistics.median(v) for k, v in ms.items()}))


if __name__ == "__main__":
    main()
