"""Measurements of K-DEFLATE, the kernel behind blocked-gzip output (profiles/gz_out_measure.txt):
  kernel   pf_kernel_time of K-DEFLATE (pf_deflate_bgzf) on one chunk of about 32 MB of text on device pointers, --kernel-reps
           repetitions behind a warm-up, median and range, GB/s of text; beside it for the same bytes: zlib.compress at levels 1 and 6 over
           the same cuts of 65 280 bytes on one host core, the download of the plain chunk to pinned memory and the download of the packed
           members;
  ratio    K-DEFLATE's bytes against level 1's and level 6's on the same cuts, and the kinds of block it chose;
  command  wall time of --reps alternating repetitions behind a warm-up, warm page cache: `trim -1 -2 --gz-out` against `trim -1 -2`
           followed by `gzip -1` of the four files (what a user does without the flag: without it `trim` runs the code it ran before
           the flag existed); `run --gz` on the files `--gz-out` wrote against `run --gz-plain` on the files `gzip` wrote.
Input: r1 of the pair of tools/bench_gz.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded qualities).
The members are checked against Python's gzip before anything is reported.
  python tools/bench_gz_out.py --work <scratch directory> --genome 470000 --depth 64 [--out FILE]"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_run_trim as brt  # noqa: E402

from ploidyfrost_amd import hipapi  # noqa: E402

CLI, STEPS, med, timed = brt.CLI, brt.STEPS, brt.med, brt.timed
CUT = 65280
OUTS = ["o1.fq", "u1.fq", "o2.fq", "u2.fq"]


def raw_deflate(text, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return c.compress(text) + c.flush()


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

    plain = brt.write_pair(a.work, a.genome, a.depth)
    text = open(plain[0], "rb").read()
    n_members = max(1, (32 << 20) // CUT)
    chunk = text[: n_members * CUT]
    n_members = (len(chunk) + CUT - 1) // CUT
    say("input: genome %d, depth %d, reads of 100: one chunk of r1, %d bytes of text in %d cuts of %d" % (a.genome, a.depth, len(chunk), n_members, CUT))

    dev = hipapi.Device(0)
    d_text = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).cuda()
    d_out = torch.zeros(len(chunk) + 31 * n_members, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n_members + 1, dtype=torch.int64, device="cuda")
    host_plain = torch.zeros(len(chunk), dtype=torch.uint8).pin_memory()
    dev.enable_timing(True)
    t_def, t_down_plain, t_down_comp = [], [], []
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        dev.reset_timing()
        data, _, stats = dev.deflate_bgzf(d_text, out=d_out, member_off=d_off)
        ms_def = dev.kernel_time(hipapi.K_DEFLATE)[0]
        host_comp = torch.zeros(len(data), dtype=torch.uint8).pin_memory()
        downs = []
        for src, dst in ((d_text, host_plain), (data, host_comp)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            downs.append((time.perf_counter() - t0) * 1e3)
        if rep:
            t_def.append(ms_def)
            t_down_plain.append(downs[0])
            t_down_comp.append(downs[1])
    packed = bytes(host_comp.numpy())
    assert gzip.decompress(packed) == chunk
    dev.close()

    cuts = [chunk[i:i + CUT] for i in range(0, len(chunk), CUT)]
    sizes, t_zlib = {}, {}
    for level in (1, 6):
        t_zlib[level] = []
        for _ in range(3):
            t0 = time.perf_counter()
            sizes[level] = sum(len(raw_deflate(c, level)) for c in cuts)
            t_zlib[level].append((time.perf_counter() - t0) * 1e3)
    gbs = lambda ms: len(chunk) / (ms * 1e-3) / 1e9   # noqa: E731
    say("kernel, device pointers [ms]:")
    say("  K-DEFLATE (pf_deflate_bgzf: deflate with the CRC, scan of the sizes, pack; one block a member): %s = %.2f GB/s of text at the median" %
        (med(t_def), gbs(statistics.median(t_def))))
    for level in (1, 6):
        say("  zlib.compress(level=%d) over the same cuts, one host core: %s = %.3f GB/s" % (level, med(t_zlib[level]), gbs(statistics.median(t_zlib[level]))))
    say("  download of the plain chunk to pinned memory (what blocked-gzip output need not make): %s = %.2f GB/s; of the packed members: %s" %
        (med(t_down_plain), gbs(statistics.median(t_down_plain)), med(t_down_comp)))
    n_payload = len(packed) - 26 * n_members
    say("ratio: K-DEFLATE %d bytes (%d with the members' headers and trailers; %d dynamic, %d fixed, %d stored blocks; %d literals, %d matches) = %.2f times "
        "smaller than the text; level 1: %d bytes (K-DEFLATE is %.3f of it); level 6: %d bytes (K-DEFLATE is %.3f of it)" %
        (n_payload, len(packed), stats["blocks_dynamic"], stats["blocks_fixed"], stats["blocks_stored"], stats["literals"], stats["matches"],
         len(chunk) / len(packed), sizes[1], n_payload / sizes[1], sizes[6], n_payload / sizes[6]))
    # ---- command ----
    gd, pd = os.path.join(a.work, "gz_out"), os.path.join(a.work, "plain_gzip")
    for d in (gd, pd):
        os.makedirs(d, exist_ok=True)
    pair_outs = ["-o1", OUTS[0], "-u1", OUTS[1], "-o2", OUTS[2], "-u2", OUTS[3]]
    trim_gz = [CLI, "trim", "-1", plain[0], "-2", plain[1]] + pair_outs + STEPS + ["--gz-out"]
    trim_plain = [CLI, "trim", "-1", plain[0], "-2", plain[1]] + pair_outs + STEPS
    gzip_exe = shutil.which("gzip")

    def trim_then_gzip():
        dt, _ = timed(trim_plain, pd)
        t0 = time.perf_counter()
        for o in OUTS:
            if gzip_exe:
                subprocess.run([gzip_exe, "-1", "-f", "-k", o], cwd=pd, check=True)
            else:
                with open(os.path.join(pd, o), "rb") as f, gzip.open(os.path.join(pd, o + ".gz"), "wb", compresslevel=1) as g:
                    shutil.copyfileobj(f, g, 1 << 22)
        return dt, time.perf_counter() - t0

    run_gz = [CLI, "run", "--gz"] + [x for o in OUTS[:3] for x in ("-i", o)] + ["-o", "s", "-v"]
    run_gzip = [CLI, "run", "--gz-plain"] + [x for o in OUTS[:3] for x in ("-i", o + ".gz")] + ["-o", "s", "-v"]
    timed(trim_gz, gd)
    trim_then_gzip()
    timed(run_gz, gd)
    timed(run_gzip, pd)
    w_tgz, w_chain, parts, w_rgz, w_rgzip = [], [], [], [], []
    for _ in range(a.reps):
        w_tgz.append(timed(trim_gz, gd)[0])
        tt, tg = trim_then_gzip()
        w_chain.append(tt + tg)
        parts.append((tt, tg))
        w_rgz.append(timed(run_gz, gd)[0])
        w_rgzip.append(timed(run_gzip, pd)[0])
    sizes_gz = [os.path.getsize(os.path.join(gd, o)) for o in OUTS]
    sizes_gzip = [os.path.getsize(os.path.join(pd, o + ".gz")) for o in OUTS]
    sizes_plain = [os.path.getsize(os.path.join(pd, o)) for o in OUTS]
    same_text = all(gzip.decompress(open(os.path.join(gd, o), "rb").read()) == open(os.path.join(pd, o), "rb").read() for o in OUTS)
    od = "PloidyFrost_output"
    same_run = all(open(os.path.join(gd, od, f), "rb").read() == open(os.path.join(pd, od, f), "rb").read() for f in sorted(os.listdir(os.path.join(pd, od))))
    say("wall, trim -1 -2 --gz-out on the plain pair of %d + %d bytes [s]: %s" % (os.path.getsize(plain[0]), os.path.getsize(plain[1]), med(w_tgz)))
    say("wall, trim -1 -2, then %s of the four files [s]: %s (last: trim %.3f + gzip %.3f)" %
        ("gzip -1" if gzip_exe else "Python's gzip at level 1", med(w_chain), parts[-1][0], parts[-1][1]))
    say("  the four outputs: %d bytes of text; --gz-out writes %d bytes, gzip -1 %d; every --gz-out file inflates to the plain run's: %s" %
        (sum(sizes_plain), sum(sizes_gz), sum(sizes_gzip), same_text))
    say("wall, run --gz -i o1 -i o2 -i u1 on the files --gz-out wrote [s]: %s" % med(w_rgz))
    say("wall, run --gz-plain on the files gzip wrote [s]: %s; every file of PloidyFrost_output identical: %s" % (med(w_rgzip), same_run))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"deflate_ms": statistics.median(t_def), "deflate_gbs": gbs(statistics.median(t_def)), "zlib1_ms": statistics.median(t_zlib[1]),
                      "zlib6_ms": statistics.median(t_zlib[6]), "download_plain_ms": statistics.median(t_down_plain),
                      "download_packed_ms": statistics.median(t_down_comp), "bytes": len(packed), "zlib1_bytes": sizes[1], "zlib6_bytes": sizes[6],
                      "wall_trim_gz_out_s": statistics.median(w_tgz), "wall_trim_gzip_s": statistics.median(w_chain),
                      "wall_run_gz_s": statistics.median(w_rgz), "wall_run_gz_plain_s": statistics.median(w_rgzip)}))


if __name__ == "__main__":
    main()
