"""Measurements of `ploidyfrost run-multi` (profiles/run_multi_*.txt):
  wall    run-multi against the chain it replaces (C x `mask -k --auto-cutoffs --db-out`, `build-multi -i -d`, the coloured calling
          run), warm page cache, a warm-up and then --reps alternating repetitions; --chain-cli names the binary that runs the chain
          (the parent commit's, to compare against it);
  kernel  pf_kernel_time of K-UNION at C = 3 (the samples' k-mers) and C = 8 (the k-mers of eight pieces of the masked files) against
          concatenate + rocprim::radix_sort_keys + rocprim::unique on the same device arrays (tools/exp/union_rocprim.hip), and of
          K-COLORSET against pf_color_fastq (pf_color_stats::mark_ms) over the masked text of the same sample; nine alternating
          repetitions, median and range.
Inputs: three samples of tests/golden/make_build_multi_golden.py's generator (build_mc3_k25) at --genome and --depth.
  python tools/bench_run_multi.py --work <scratch directory> --genome 300000 --depth 48 [--chain-cli PATH] [--out FILE]"""
import argparse
import ctypes as C
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
import torch  # noqa: E402,F401

from ploidyfrost_amd import hipapi  # noqa: E402

CLI = os.path.join(ROOT, "ploidyfrost_amd", "csrc", "ploidyfrost")
NAMES = ["alpha", "beta", "gamma"]


def med(xs):
    return "median %.3f (range %.3f - %.3f)" % (statistics.median(xs), min(xs), max(xs))


def timed(cmd, cwd):
    t = time.perf_counter()
    r = subprocess.run([str(x) for x in cmd], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    dt = time.perf_counter() - t
    if r.returncode:
        sys.exit("failed: %s\n%s\n%s" % (cmd, r.stdout[-1500:], r.stderr[-1500:]))
    return dt, r


def chain(cli, files, d):
    """the C + 2 commands; (wall seconds of each command, in order)"""
    os.makedirs(d, exist_ok=True)
    ts = []
    for c, n in enumerate(NAMES):
        ts.append(timed([cli, "mask", "-k", 25, "-ci", 1, "-cs", 10000, "-i", files[c], "-o", n, "--auto-cutoffs", "--db-out", "db%d" % c], d)[0])
    ts.append(timed([cli, "build-multi", "-i", "-d", "-k", 25] + [x for n in NAMES for x in ("-r", n)] + ["-o", "s"], d)[0])
    with open(os.path.join(d, "dbs.txt"), "w") as f:
        f.write("".join("%s\n" % os.path.join(d, "db%d" % c) for c in range(len(NAMES))))
    ts.append(timed([cli, "-g", "s.gfa", "-f", "s.bfg_colors", "-d", "dbs.txt", "--auto-cutoffs", "-o", "s"], d)[0])
    return ts


def kmers_of(dev, data):
    dev.count_begin(25, True)
    at = 0
    while at < len(data):
        used, _ = dev.count_fastq(data[at:at + (64 << 20)], final=at + (64 << 20) >= len(data))
        at += used
    return dev.count_finish(ci=1, cx=0xFFFFFFFF, cs=0xFFFFFFFF)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=300000)
    ap.add_argument("--depth", type=int, default=48)
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

    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tests", "golden", "make_build_multi_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    t = time.perf_counter()
    files = []
    for c, reads in enumerate(gen.make_samples(**dict(gen.CASES["build_mc3_k25"], genome=a.genome, depth=a.depth))):
        p = os.path.join(a.work, "s%d.fq" % c)
        with open(p, "w") as f:
            f.write("".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)))
        files.append(p)
    say("inputs: 3 samples, genome %d, depth %d, reads of 100: %s bytes (generated in %.1f s)" %
        (a.genome, a.depth, [os.path.getsize(p) for p in files], time.perf_counter() - t))
    say("chain binary: %s" % ("this tree's" if a.chain_cli == CLI else a.chain_cli))

    # ---- wall ----
    multi = [CLI, "run-multi"] + [x for c, n in enumerate(NAMES) for x in ("--sample", n, "-i", files[c])] + ["-o", "r", "-v"]
    chain(a.chain_cli, files, os.path.join(a.work, "chain"))   # warm-up (and the page cache)
    os.makedirs(os.path.join(a.work, "multi"), exist_ok=True)
    timed(multi, os.path.join(a.work, "multi"))
    wall_c, wall_m, parts, stage = [], [], [], ""
    for _ in range(a.reps):
        ts = chain(a.chain_cli, files, os.path.join(a.work, "chain"))
        wall_c.append(sum(ts))
        parts.append(ts)
        dt, r = timed(multi, os.path.join(a.work, "multi"))
        wall_m.append(dt)
        stage = [l for l in r.stderr.splitlines() if l.startswith("run-multi: count ")][-1]
        line = [l for l in r.stderr.splitlines() if l.startswith("run-multi: colors ")][-1]
    od = "PloidyFrost_output"
    same = all(open(os.path.join(a.work, "chain", od, "s_" + s + ".txt"), "rb").read() == open(os.path.join(a.work, "multi", od, "r_" + s + ".txt"), "rb").read()
               for s in ("allele_frequency", "bicov", "super_bubble", "Unitig_Id"))
    say("wall, chain of 5 processes [s]: %s" % med(wall_c))
    say("  per command (mask x3, build-multi, calling run), last repetition: %s" % " ".join("%.3f" % x for x in parts[-1]))
    say("wall, run-multi [s]: %s" % med(wall_m))
    say("  " + stage)
    say("  " + line)
    say("  same allele_frequency / bicov / super_bubble / Unitig_Id bytes as the chain: %s; rows in allele_frequency.txt: %d" %
        (same, open(os.path.join(a.work, "multi", od, "r_allele_frequency.txt")).read().count("\n")))

    # ---- kernels ----
    R = C.CDLL(os.path.join(ROOT, "tools", "exp", "libunion_rocprim.so"))
    R.union_rocprim_ms.restype = C.c_double
    R.union_rocprim_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p]
    dev = hipapi.Device(0)
    masked = [open(os.path.join(a.work, "chain", n), "rb").read() for n in NAMES]
    sets3 = [kmers_of(dev, m) for m in masked]
    pieces = []
    for m, cut in zip(masked, (3, 3, 2)):
        recs = m.split(b"\n")[:-1]
        per = (len(recs) // 4 + cut - 1) // cut * 4
        pieces += [b"\n".join(recs[i:i + per]) + b"\n" for i in range(0, len(recs), per)]
    sets8 = [kmers_of(dev, p) for p in pieces]
    dev.enable_timing(True)
    for tag, sets in (("C = 3", sets3), ("C = 8", sets8)):
        tens = [torch.from_numpy(s.view(np.int64).copy()).to("cuda") for s in sets]
        ns = np.array([len(s) for s in sets], dtype=np.uint64)
        ptrs = np.array([t.data_ptr() for t in tens], dtype=np.uint64)
        ours, theirs, n_r = [], [], C.c_uint64()
        want = None
        for rep in range(a.kernel_reps + 1):   # the first pair is the warm-up
            dev.reset_timing()
            got = dev.kmer_union(tens)
            ms = dev.kernel_time(hipapi.K_UNION)[0]
            first = np.zeros(4, dtype=np.uint64)
            rms = R.union_rocprim_ms(ptrs.ctypes.data, ns.ctypes.data, len(sets), C.byref(n_r), first.ctypes.data)
            assert rms >= 0 and n_r.value == len(got) and np.array_equal(first[:min(4, len(got))], got[:4])
            want = got if want is None else want
            assert np.array_equal(got, want)
            if rep:
                ours.append(ms)
                theirs.append(rms)
        say("K-UNION %s, sets of %s keys -> %d [ms]: %s" % (tag, [len(s) for s in sets], len(want), med(ours)))
        say("  concatenate + rocprim::radix_sort_keys + rocprim::unique [ms]: %s" % med(theirs))
    union = dev.kmer_union(sets3)
    keys0 = torch.from_numpy(sets3[0].view(np.int64).copy()).to("cuda")
    by_keys, by_reads = [], []
    for rep in range(a.kernel_reps + 1):
        for route in ("keys", "reads"):
            _, st = dev.unitig_build_colored(union, 25, True, True)
            try:
                dev.color_begin(3)
                dev.reset_timing()
                if route == "keys":
                    own = dev.color_kmers(0, keys0)
                else:
                    used, _ = dev.color_fastq(0, masked[0], final=True)
                    assert used == len(masked[0])
                col, got = dev.color_finish()
            finally:
                dev.unitig_release()
            if route == "keys":
                ms, runs_k = dev.kernel_time(hipapi.K_COLORSET)[0], got["runs"].copy()
                if rep:
                    by_keys.append(ms)
            else:
                assert np.array_equal(got["runs"], runs_k)
                if rep:
                    by_reads.append(col["mark_ms"])
    say("K-COLORSET, %d keys of sample 0 (%d colored, %d unplaced), graph of %d k-mers [ms]: %s" %
        (len(sets3[0]), own["kmers_colored"], own["kmers_unplaced"], len(union), med(by_keys)))
    say("  pf_color_fastq over the %d bytes of the masked text of sample 0 (classes + mark) [ms]: %s" % (len(masked[0]), med(by_reads)))
    dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"wall_chain_s": statistics.median(wall_c), "wall_run_multi_s": statistics.median(wall_m)}))


if __name__ == "__main__":
    main()
