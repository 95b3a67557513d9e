"""Measurements of `--gz-plain` (profiles/gz_plain_measure.txt):
  kernel   pf_kernel_time of K-GUNZIP (pf_inflate_gzip) on the deflate stream of one file (about 32 MB of text, one gzip member as
           `gzip -6` writes it) on device pointers, --kernel-reps repetitions behind a warm-up, median and range, GB/s of inflated text;
           the stages' own times (find, count, decode, window, resolve), live and dead pieces and markers; beside it on the same text:
           K-INFLATE on the file as blocked gzip, and zlib.decompress of the stream on one host core;
  command  wall time of --reps alternating repetitions behind a warm-up, warm page cache: `run --gz-plain -1 -2 STEP...` on the gzip
           pair, against Python's gzip to files followed by `run -1 -2 STEP...` with --parent-cli (the binary of the commit before
           this one; default: this one, whose `run` without the flag is the same code).
Inputs: the pair of tools/bench_gz.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded qualities), each
file one gzip member at zlib level 6.
  python tools/bench_gz_plain.py --work <scratch directory> --genome 470000 --depth 64 [--parent-cli PATH] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_gz  # noqa: E402
import bench_run_trim as brt  # noqa: E402

from ploidyfrost_amd import hipapi  # noqa: E402

CLI, STEPS, med, timed = brt.CLI, brt.STEPS, brt.med, brt.timed
HEADER = b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"


def deflate(text):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    return c.compress(text) + c.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--genome", type=int, default=470000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--piece-bytes", type=int, default=0)
    ap.add_argument("--parent-cli", default=CLI)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.perf_counter()
    plain = brt.write_pair(a.work, a.genome, a.depth)
    texts = [open(p, "rb").read() for p in plain]
    streams = [deflate(x) for x in texts]
    comp = [p + ".gz" for p in plain]
    for p, s, x in zip(comp, streams, texts):
        with open(p, "wb") as f:
            f.write(HEADER + s + struct.pack("<II", zlib.crc32(x), len(x) & 0xFFFFFFFF))
    n_plain, n_comp = sum(len(x) for x in texts), sum(os.path.getsize(p) for p in comp)
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes; gzip (zlib level 6, one member each): %d + %d bytes, "
        "%.2f times smaller (made in %.1f s)" % (a.genome, a.depth, len(texts[0]), len(texts[1]), os.path.getsize(comp[0]), os.path.getsize(comp[1]),
                                                 n_plain / n_comp, time.perf_counter() - t))

    # ---- kernel: the stream of r1 ----
    text, stream = texts[0], streams[0]
    dev = hipapi.Device(0)
    d_comp = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    d_out = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
    d_win = torch.zeros(32768, dtype=torch.uint8, device="cuda")
    members = bench_gz.bgzf_members(text)
    d_bgzf = torch.frombuffer(bytearray(b"".join(members)), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(m) for m in members]).astype(np.int64)).cuda()
    dev.enable_timing(True)
    t_gun, t_inf, stages = [], [], {s: [] for s in hipapi.GUNZIP_STAGES}
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        dev.reset_timing()
        out, res, st, _ = dev.inflate_gzip(d_comp, 0, None, a.piece_bytes, out=d_out, out_cap=len(text), new_window=d_win)
        ms_gun = dev.kernel_time(hipapi.K_GUNZIP)[0]
        dev.reset_timing()
        dev.inflate_bgzf(d_bgzf, d_off, out=d_out, out_cap=len(text))
        ms_inf = dev.kernel_time(hipapi.K_INFLATE)[0]
        if rep:
            t_gun.append(ms_gun)
            t_inf.append(ms_inf)
            for s in stages:
                stages[s].append(st["stage_ms"][s])
    out, res, st, _ = dev.inflate_gzip(d_comp, 0, None, a.piece_bytes, out=d_out, out_cap=len(text), new_window=d_win)
    assert bytes(d_out[: len(text)].cpu().numpy()) == text and res["final"] == 1
    t_zlib = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = len(zlib.decompress(stream, -15))
        t_zlib.append((time.perf_counter() - t0) * 1e3)
    assert n == len(text)
    gbs = lambda ms: len(text) / (ms * 1e-3) / 1e9   # noqa: E731
    say("kernel, the stream of r1: %d compressed bytes -> %d bytes of text (%d dynamic, %d fixed, %d stored blocks), piece stride %d bytes, "
        "device pointers [ms]:" % (len(stream), len(text), st["blocks_dynamic"], st["blocks_fixed"], st["blocks_stored"], a.piece_bytes or 16384))
    say("  K-GUNZIP (pf_inflate_gzip: find, count, chain, decode, window, resolve with the CRC): %s = %.2f GB/s of text at the median" %
        (med(t_gun), gbs(statistics.median(t_gun))))
    say("  its stages (events inside the call, medians): " + ", ".join("%s %.3f" % (s, statistics.median(stages[s])) for s in hipapi.GUNZIP_STAGES))
    say("  pieces: %d found, %d live, %d dead; %d of %d symbols were markers" % (st["pieces_found"], st["pieces_live"], st["pieces_dead"], st["markers"], len(text)))
    say("  K-INFLATE on the same text as blocked gzip (%d members): %s = %.2f GB/s" % (len(members), med(t_inf), gbs(statistics.median(t_inf))))
    say("  zlib.decompress of the stream, one host core: %s = %.2f GB/s" % (med(t_zlib), gbs(statistics.median(t_zlib))))
    dev.close()

    # ---- command ----
    gd, ud = (os.path.join(a.work, x) for x in ("gzplain", "gunzip"))
    for d in (gd, ud):
        os.makedirs(d, exist_ok=True)
    run_gz = [CLI, "run", "--gz-plain", "-1", comp[0], "-2", comp[1], "-o", "r", "-v"] + STEPS

    def gunzip_then_run():
        t0 = time.perf_counter()
        outs = []
        for p in comp:
            o = os.path.join(ud, os.path.basename(p)[:-3])
            with gzip.open(p, "rb") as f, open(o, "wb") as g:
                while True:
                    b = f.read(1 << 22)
                    if not b:
                        break
                    g.write(b)
            outs.append(o)
        t_unzip = time.perf_counter() - t0
        dt, r = timed([a.parent_cli, "run", "-1", outs[0], "-2", outs[1], "-o", "r", "-v"] + STEPS, ud)
        return t_unzip, dt, r

    timed(run_gz, gd)
    gunzip_then_run()
    w_gz, w_chain, parts = [], [], []
    for _ in range(a.reps):
        dt, r_gz = timed(run_gz, gd)
        w_gz.append(dt)
        tu, tr, r_chain = gunzip_then_run()
        w_chain.append(tu + tr)
        parts.append((tu, tr))
    od = "PloidyFrost_output"
    same = all(open(os.path.join(gd, od, f), "rb").read() == open(os.path.join(ud, od, f), "rb").read() for f in sorted(os.listdir(os.path.join(ud, od))))
    stage = lambda r: [l for l in r.stderr.splitlines() if l.startswith("run: count ")][-1]   # noqa: E731
    say("wall, run --gz-plain -1 -2 STEP... on the gzip pair [s]: %s" % med(w_gz))
    say("  " + stage(r_gz))
    say("wall, Python gzip to files, then run -1 -2 STEP... on them with %s [s]: %s (last: gzip %.3f + run %.3f)" %
        ("this binary" if a.parent_cli == CLI else "the parent commit's binary", med(w_chain), parts[-1][0], parts[-1][1]))
    say("  " + stage(r_chain))
    say("  every file of PloidyFrost_output identical: %s" % same)
    say("bytes: run --gz-plain reads %d bytes from disk twice (two passes), uploads them twice and inflates %d bytes twice on the device; nothing "
        "is written before the results.  Decompressing first writes %d bytes to disk once, and run reads and uploads them twice." % (n_comp, n_plain, n_plain))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"gunzip_ms": statistics.median(t_gun), "gunzip_gbs": gbs(statistics.median(t_gun)), "inflate_ms": statistics.median(t_inf),
                      "zlib_ms": statistics.median(t_zlib), "stage_ms": {s: statistics.median(stages[s]) for s in stages},
                      "wall_gz_plain_s": statistics.median(w_gz), "wall_gunzip_run_s": statistics.median(w_chain)}))


if __name__ == "__main__":
    main()
