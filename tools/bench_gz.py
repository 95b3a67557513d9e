"""Measurements of `--gz` (profiles/gz_measure.txt):
  kernel   pf_kernel_time of K-INFLATE (pf_inflate_bgzf) on one chunk of about 32 MB of text on device pointers, --kernel-reps
           repetitions behind a warm-up, median and range, GB/s of inflated text; beside it for the same bytes: the upload of the plain
           chunk, pf_count_fastq_trimmed, and zlib.decompress over the same members on one host core;
  command  wall time of --reps alternating repetitions behind a warm-up, warm page cache: `run --gz -1 -2 STEP...` on the compressed
           pair; Python's gzip to files followed by `run -1 -2 STEP...` on the plain pair (what a user does today); the plain `run`
           alone (the floor); `run -v`'s stage times with and without --gz;
  bytes    over PCIe and to disk, each way.
Inputs: the pair of tools/bench_run_trim.py (tests/golden/make_build_golden.py's generator at --genome and --depth, seeded qualities),
compressed at level 6 into members of 65 280 bytes of text as bgzip cuts them, with the end-of-file marker.
  python tools/bench_gz.py --work <scratch directory> --genome 470000 --depth 64 [--out FILE]"""
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

import bench_run_trim as brt  # noqa: E402

from ploidyfrost_amd import hipapi  # noqa: E402

CLI, STEPS, med, timed = brt.CLI, brt.STEPS, brt.med, brt.timed
CUT = 65536 - 256
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(text):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    raw = c.compress(text) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw +
            struct.pack("<II", zlib.crc32(text), len(text)))


def bgzf_members(text):
    return [member(text[i:i + CUT]) for i in range(0, len(text), CUT)]


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
    plain = brt.write_pair(a.work, a.genome, a.depth)
    texts = [open(p, "rb").read() for p in plain]
    members = [bgzf_members(x) for x in texts]
    comp = [p + ".gz" for p in plain]
    for p, ms in zip(comp, members):
        with open(p, "wb") as f:
            f.write(b"".join(ms) + EOF_MARKER)
    n_plain, n_comp = sum(len(x) for x in texts), sum(os.path.getsize(p) for p in comp)
    say("inputs: genome %d, depth %d, reads of 100, a pair of files of %d + %d bytes; blocked gzip (level 6, members of %d bytes of text): %d + %d "
        "bytes in %d + %d members and a marker each, %.2f times smaller (made in %.1f s)" %
        (a.genome, a.depth, len(texts[0]), len(texts[1]), CUT, os.path.getsize(comp[0]), os.path.getsize(comp[1]), len(members[0]), len(members[1]),
         n_plain / n_comp, time.perf_counter() - t))

    # ---- kernel: one chunk of r1 ----
    ms1 = members[0][: max(1, (32 << 20) // CUT)]
    chunk_text = texts[0][: len(ms1) * CUT]
    data = b"".join(ms1)
    off = np.cumsum([0] + [len(m) for m in ms1]).astype(np.int64)
    dev = hipapi.Device(0)
    d_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_out = torch.zeros(len(chunk_text) + 16, dtype=torch.uint8, device="cuda")
    host_plain = torch.frombuffer(bytearray(chunk_text), dtype=torch.uint8).pin_memory()
    host_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
    d_up = torch.zeros(len(chunk_text), dtype=torch.uint8, device="cuda")
    dev.enable_timing(True)
    t_inf, t_cnt, t_up_plain, t_up_comp = [], [], [], []
    for rep in range(a.kernel_reps + 1):   # the first round is the warm-up
        dev.reset_timing()
        out, stats = dev.inflate_bgzf(d_comp, d_off, out=d_out, out_cap=len(chunk_text))
        ms_inf = dev.kernel_time(hipapi.K_INFLATE)[0]
        dev.reset_timing()
        dev.count_begin(25, True, 2 * len(chunk_text))
        dev.count_fastq_trimmed(d_out[: len(chunk_text)], STEPS, final=False)
        ms_cnt = dev.kernel_time(hipapi.K_TRIMCOUNT)[0]
        dev.count_abort()
        ups = []
        for src, dst in ((host_plain, d_up), (host_comp, d_up[: len(data)])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            ups.append((time.perf_counter() - t0) * 1e3)
        if rep:
            t_inf.append(ms_inf)
            t_cnt.append(ms_cnt)
            t_up_plain.append(ups[0])
            t_up_comp.append(ups[1])
    assert bytes(d_out[: len(chunk_text)].cpu().numpy()) == chunk_text
    t_zlib = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = sum(len(zlib.decompress(m[18:-8], -15)) for m in ms1)
        t_zlib.append((time.perf_counter() - t0) * 1e3)
    assert n == len(chunk_text)
    gbs = lambda ms: len(chunk_text) / (ms * 1e-3) / 1e9   # noqa: E731
    say("kernel, one chunk of r1: %d members, %d compressed bytes -> %d bytes of text (%d dynamic, %d fixed, %d stored blocks), device pointers [ms]:" %
        (len(ms1), len(data), len(chunk_text), stats["blocks_dynamic"], stats["blocks_fixed"], stats["blocks_stored"]))
    say("  K-INFLATE (pf_inflate_bgzf: headers, scan, inflate with the CRC; text assembled in LDS): %s = %.2f GB/s of text at the median" %
        (med(t_inf), gbs(statistics.median(t_inf))))
    say("  (the form that writes the text to global memory as it is produced was not built: no second figure)")
    say("  upload of the plain chunk from pinned memory: %s = %.2f GB/s; of the compressed chunk: %s" %
        (med(t_up_plain), gbs(statistics.median(t_up_plain)), med(t_up_comp)))
    say("  pf_count_fastq_trimmed on the same text: %s" % med(t_cnt))
    say("  zlib.decompress over the same members, one host core: %s = %.2f GB/s" % (med(t_zlib), gbs(statistics.median(t_zlib))))
    dev.close()

    # ---- command ----
    gd, pd, ud = (os.path.join(a.work, x) for x in ("gz", "plain", "gunzip"))
    for d in (gd, pd, ud):
        os.makedirs(d, exist_ok=True)
    run_gz = [CLI, "run", "--gz", "-1", comp[0], "-2", comp[1], "-o", "r", "-v"] + STEPS
    run_plain = [CLI, "run", "-1", plain[0], "-2", plain[1], "-o", "r", "-v"] + STEPS

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
        dt, r = timed([CLI, "run", "-1", outs[0], "-2", outs[1], "-o", "r", "-v"] + STEPS, ud)
        return t_unzip, dt, r

    timed(run_gz, gd)
    timed(run_plain, pd)
    gunzip_then_run()
    w_gz, w_plain, w_chain, parts = [], [], [], []
    for _ in range(a.reps):
        dt, r_gz = timed(run_gz, gd)
        w_gz.append(dt)
        tu, tr, _ = gunzip_then_run()
        w_chain.append(tu + tr)
        parts.append((tu, tr))
        dt, r_plain = timed(run_plain, pd)
        w_plain.append(dt)
    od = "PloidyFrost_output"
    same = all(open(os.path.join(gd, od, f), "rb").read() == open(os.path.join(pd, od, f), "rb").read() for f in sorted(os.listdir(os.path.join(pd, od))))
    stage = lambda r: [l for l in r.stderr.splitlines() if l.startswith("run: count ")][-1]   # noqa: E731
    say("wall, run --gz -1 -2 STEP... on the compressed pair [s]: %s" % med(w_gz))
    say("  " + stage(r_gz))
    say("wall, Python gzip to files, then run -1 -2 STEP... on them [s]: %s (last: gzip %.3f + run %.3f)" % (med(w_chain), parts[-1][0], parts[-1][1]))
    say("wall, run -1 -2 STEP... on the plain pair alone (the floor) [s]: %s" % med(w_plain))
    say("  " + stage(r_plain))
    say("  every file of PloidyFrost_output identical with and without --gz: %s" % same)
    say("bytes: run --gz reads %d bytes from disk twice (two passes), uploads them twice, and inflates %d bytes twice on the device, where only the "
        "carried record ends move again (device to device); nothing is written before the results.  Decompressing first writes %d bytes "
        "to disk once, and run reads and uploads them twice.  The plain run reads and uploads %d bytes twice." % (n_comp, n_plain, n_plain, n_plain))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"inflate_ms": statistics.median(t_inf), "inflate_gbs": gbs(statistics.median(t_inf)), "upload_plain_ms": statistics.median(t_up_plain),
                      "count_trimmed_ms": statistics.median(t_cnt), "zlib_ms": statistics.median(t_zlib), "wall_gz_s": statistics.median(w_gz),
                      "wall_gunzip_run_s": statistics.median(w_chain), "wall_plain_s": statistics.median(w_plain)}))


if __name__ == "__main__":
    main()
