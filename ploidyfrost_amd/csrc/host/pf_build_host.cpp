#include "pf_build_host.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

constexpr uint64_t FETCH_BLOCK_BYTES = 64ull << 20;   // text a download

bool write_all(int fd, const void *p, uint64_t n) {
    const char *c = static_cast<const char *>(p);
    for (uint64_t done = 0; done < n;) {
        const ssize_t put = write(fd, c + done, (size_t)(n - done));
        if (put < 0 && errno == EINTR) continue;
        if (put < 0) return false;
        done += (uint64_t)put;
    }
    return true;
}

}  // namespace

std::string build_options_refusal(const BuildOptions &opt) {
    if (!pf_count::k_ok(opt.k)) return pf_count::cut_text(pf_count::CUT_K);
    if (opt.g != BuildOptions::G_DEFAULT && !pf_unitig::g_ok(opt.g, (int)opt.k)) return pf_unitig::g_text((int)opt.k);
    return "";
}

int build_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const BuildOptions &opt, int device, pf_count_stats &counted,
                pf_unitig_stats &stats, BuildTimes *times, std::string &err) {
    counted = pf_count_stats{};
    stats = pf_unitig_stats{};
    BuildTimes tm;
    // ---- refusals that need no device ----
    if (inputs.empty()) { err = "build: no input"; return 1; }
    if (out_prefix.empty()) { err = "build: no output prefix"; return 1; }
    { const std::string why = build_options_refusal(opt); if (!why.empty()) { err = "build: " + why; return 1; } }
    const std::string out_path = out_prefix + ".gfa";
    uint64_t largest = 0;
    if (fastq_preflight("build", "read", inputs, {out_path}, largest, err)) return 1;

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("build: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); the graph is built on the GPU only";
        return 1;
    }
    struct CtxGuard { pf_ctx *c; ~CtxGuard() { pf_destroy(c); } } ctx_guard{ctx};
    // ---- count: every k-mer of the reads, both strands ----
    CountOptions copt;
    copt.k = opt.k;
    copt.ci = 1;
    copt.cx = pf_count::COUNTER_MAX;
    copt.cs = pf_count::COUNTER_MAX;
    copt.both_strands = true;
    copt.chunk_bytes = opt.chunk_bytes;
    copt.initial_slots = opt.initial_slots;
    Counted db;
    CountTimes ctm;
    if (count_stream(ctx, "build", inputs, copt, largest, db, counted, ctm, err)) return 1;
    struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
    tm.stream_s = ctm.stream_s;
    tm.finish_s = ctm.finish_s;
    pf_device_free(ctx, db.counts);   // the graph asks for the k-mers alone
    db.counts = nullptr;
    if (db.n >= pf_unitig::MAX_KMERS) { err = std::string("build: ") + pf_unitig::TOO_MANY_TEXT + " (" + std::to_string(db.n) + ")"; return 1; }
    // ---- graph ----
    const auto t_graph = clk::now();
    const uint32_t g = opt.g == BuildOptions::G_DEFAULT ? PF_UNITIG_G_DEFAULT : (uint32_t)opt.g;
    if (pf_unitig_build(ctx, db.kmers, db.n, opt.k, g, opt.clip_tips ? 1 : 0, opt.del_isolated ? 1 : 0, &stats) != PF_OK) {
        err = std::string("build: ") + pf_last_error(ctx);
        return 1;
    }
    tm.graph_s = since(t_graph);
    // ---- write: block by block through a pinned buffer ----
    const auto t_write = clk::now();
    const std::string tmp = out_path + ".tmp." + std::to_string((long)getpid());
    auto fail = [&](const std::string &m) {
        err = m;
        unlink(tmp.c_str());
        return 1;
    };
    const uint64_t block = std::max<uint64_t>(1, std::min<uint64_t>(stats.bytes, FETCH_BLOCK_BYTES));
    ChunkBuf buf;
    if (!buf.alloc(ctx, (size_t)block)) return fail("build: no memory for the text buffer");
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail("build: cannot write " + tmp + " (" + strerror(errno) + ")");
    for (uint64_t at = 0; at < stats.bytes; at += block) {
        const uint64_t nb = std::min<uint64_t>(block, stats.bytes - at);
        if (pf_unitig_fetch(ctx, at, nb, buf.p) != PF_OK) { close(fd); return fail(std::string("build: ") + pf_last_error(ctx)); }
        if (!write_all(fd, buf.p, nb)) { const int e = errno; close(fd); return fail("build: writing " + tmp + " (" + strerror(e) + ")"); }
    }
    if (close(fd) != 0) return fail("build: closing " + tmp + " (" + strerror(errno) + ")");
    if (rename(tmp.c_str(), out_path.c_str()) != 0) return fail("build: renaming " + tmp + " to " + out_path + " (" + strerror(errno) + ")");
    pf_unitig_release(ctx);
    tm.write_s = since(t_write);
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
