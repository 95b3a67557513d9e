"""Measurements of `--fasta` (profiles/fasta_measure.txt):
  kernel   pf_kernel_time of K-FASTA (the index alone, pf_fasta_index) on the FASTA file as one chunk on a device pointer,
           --kernel-reps repetitions behind a warm-up, median and range, GB/s of chunk text;
  count    pf_count_fasta on that chunk (K-FASTA + K-COUNT's launches) against pf_count_fastq on the same records as FASTQ (K-COUNT's
           launches, the FASTQ index among them) -- the _fastq entry is the yardstick; alternating, each into a fresh count;
  command  wall time of --reps alternating repetitions behind a warm-up, warm page cache: `run --fasta` on F against `run` on Q(F).
Inputs: the reads of tests/golden/make_build_golden.py's generator at --genome and --depth (the inputs of the `run` measurements) as
one FASTQ file Q with flat qualities (about 64 MB at the defaults), and F, the same records as FASTA at width 60: Q = Q(F).
  python tools/bench_fasta.py --work <scratch directory> [--genome 470000 --depth 64] [--out FILE]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_run_trim as brt  # noqa: E402

from ploidyfrost_amd import hipapi  # noqa: E402

CLI, med, timed = brt.CLI, brt.med, brt.timed
WIDTH = 60


def write_inputs(work, genome, depth):
    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tests", "golden", "make_build_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    reads = [r.encode() for r in gen.make_reads(**dict(gen.CASES["build_k25"], genome=genome, depth=depth))]
    q = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    f = b"".join(b">r%d\n" % i + b"".join(r[a:a + WIDTH] + b"\n" for a in range(0, len(r), WIDTH)) for i, r in enumerate(reads))
    paths = [os.path.join(work, "F.fa"), os.path.join(work, "Q.fq")]
    for p, t in zip(paths, (f, q)):
        with open(p, "wb") as out:
            out.write(t)
    return paths, f, q, len(reads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=470000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.perf_counter()
    (fa, fq), f_text, q_text, n_reads = write_inputs(a.work, a.genome, a.depth)
    say("inputs: genome %d, depth %d, %d reads of 100; Q (FASTQ, flat qualities) %d bytes, F (FASTA, width %d) %d bytes = %.2f of Q "
        "(made in %.1f s)" % (a.genome, a.depth, n_reads, len(q_text), WIDTH, len(f_text), len(f_text) / len(q_text), time.perf_counter() - t))

    # ---- kernel and count: one chunk each, device pointers ----
    dev = hipapi.Device(0)
    d_f = torch.frombuffer(bytearray(f_text), dtype=torch.uint8).cuda()
    d_q = torch.frombuffer(bytearray(q_text), dtype=torch.uint8).cuda()
    dev.enable_timing(True)
    t_index, t_fa, t_fa_index, t_fq = [], [], [], []
    stats = {}
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        dev.reset_timing()
        used = dev.fasta_index_resident(d_f)
        ms_index = dev.kernel_time(hipapi.K_FASTA)[0]
        assert used["bytes_used"] == len(f_text) and used["records"] == n_reads
        per = {}
        for name, text, call in (("fasta", d_f, dev.count_fasta), ("fastq", d_q, dev.count_fastq)):
            dev.count_begin(25, True)
            dev.reset_timing()
            _, st = call(text)
            per[name] = (dev.kernel_time(hipapi.K_FASTA)[0], dev.kernel_time(hipapi.K_COUNT)[0])
            dev.count_abort()
            stats[name] = st
        if rep:
            t_index.append(ms_index)
            t_fa.append(per["fasta"][0] + per["fasta"][1])
            t_fa_index.append(per["fasta"][0])
            t_fq.append(per["fastq"][1])
    assert stats["fasta"] == stats["fastq"], (stats["fasta"], stats["fastq"])
    gbs = lambda n, ms: n / (ms * 1e-3) / 1e9   # noqa: E731
    say("kernel, F as one chunk on a device pointer [ms]:")
    say("  K-FASTA alone (pf_fasta_index: newlines, lines, words, scans, compact, table; two host waits inside): %s = %.2f GB/s of chunk text "
        "at the median" % (med(t_index), gbs(len(f_text), statistics.median(t_index))))
    say("count of one chunk, %d records, %d windows, the same statistics from both [ms]:" % (stats["fasta"]["reads"], stats["fasta"]["kmers"]))
    say("  pf_count_fasta on F (K-FASTA + K-COUNT's launches): %s (of it K-FASTA: median %.3f)" % (med(t_fa), statistics.median(t_fa_index)))
    say("  pf_count_fastq on Q(F) (K-COUNT's launches, the FASTQ index among them): %s" % med(t_fq))
    say("  per record: %.2f ns against %.2f ns" % (statistics.median(t_fa) * 1e6 / n_reads, statistics.median(t_fq) * 1e6 / n_reads))
    dev.close()

    # ---- command ----
    da, dq = (os.path.join(a.work, x) for x in ("run_fa", "run_fq"))
    for d in (da, dq):
        os.makedirs(d, exist_ok=True)
    run_fa = [CLI, "run", "--fasta", "-i", fa, "-o", "r", "-v"]
    run_fq = [CLI, "run", "-i", fq, "-o", "r", "-v"]
    timed(run_fa, da)
    timed(run_fq, dq)
    w_fa, w_fq = [], []
    for _ in range(a.reps):
        dt, r_fa = timed(run_fa, da)
        w_fa.append(dt)
        dt, r_fq = timed(run_fq, dq)
        w_fq.append(dt)
    od = "PloidyFrost_output"
    same = all(open(os.path.join(da, od, f), "rb").read() == open(os.path.join(dq, od, f), "rb").read() for f in sorted(os.listdir(os.path.join(dq, od))))
    stage = lambda r: [l for l in r.stderr.splitlines() if l.startswith("run: count ")][-1]   # noqa: E731
    say("wall, run --fasta on F [s]: %s" % med(w_fa))
    say("  " + stage(r_fa))
    say("wall, run on Q(F) [s]: %s" % med(w_fq))
    say("  " + stage(r_fq))
    say("  every file of PloidyFrost_output identical: %s" % same)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"fasta_index_ms": statistics.median(t_index), "fasta_index_gbs": gbs(len(f_text), statistics.median(t_index)),
                      "count_fasta_ms": statistics.median(t_fa), "count_fastq_ms": statistics.median(t_fq),
                      "wall_run_fasta_s": statistics.median(w_fa), "wall_run_fastq_s": statistics.median(w_fq)}))


if __name__ == "__main__":
    main()
