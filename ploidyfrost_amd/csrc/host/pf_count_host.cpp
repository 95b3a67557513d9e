#include "pf_count_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>

#include "pf_cutoffs.hpp"
#include "pf_host_graph.hpp"
#include "pf_host_util.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

constexpr uint64_t WRITE_BLOCK_BYTES = 64ull << 20;   // encoded records a download

}  // namespace

int count_options_clause(const CountOptions &opt, bool writes) {
    if (!pf_count::k_ok(opt.k)) return pf_count::CUT_K;
    if (writes && !pf_count::lut_prefix_len((int)opt.k)) return pf_count::CUT_K_LAYOUT;
    return pf_count::cut_clause(opt.ci, opt.cx, opt.cs);
}

int count_stream(pf_ctx *ctx, const char *who_c, const std::vector<ReadsInput> &inputs, const CountOptions &opt, Counted &out, pf_count_stats &stats,
                 CountTimes &tm, std::string &err) {
    return count_stream_with(ctx, who_c, opt, [&](std::string &e) {
        StreamTimes stm;
        return stream_fastq(ctx, who_c, inputs, opt.chunk_bytes, -1, "",
                            [&](const Chunk &c, Taken &t) {
                                pf_count_stats st = {};
                                const int rc = c.fasta ? pf_count_fasta(ctx, c.text, c.n, c.final ? 1 : 0, &t.used, &st, &t.bad)
                                                       : pf_count_fastq(ctx, c.text, c.n, c.final ? 1 : 0, &t.used, &st, &t.bad);
                                t.reads = st.reads;
                                return rc;
                            },
                            stm, e);
    }, out, stats, tm, err);
}

int count_stream_with(pf_ctx *ctx, const char *who_c, const CountOptions &opt, const std::function<int(std::string &)> &pass, Counted &out,
                      pf_count_stats &stats, CountTimes &tm, std::string &err) {
    const std::string who = who_c;
    out = Counted{};
    stats = pf_count_stats{};
    const auto t_stream = clk::now();
    if (pf_count_begin(ctx, opt.k, opt.both_strands ? 1 : 0, opt.initial_slots) != PF_OK) { err = who + ": " + pf_last_error(ctx); return 1; }
    if (pass(err)) {
        pf_count_abort(ctx);
        return 1;
    }
    tm.stream_s = since(t_stream);
    const auto t_finish = clk::now();
    if (pf_count_finish(ctx, opt.ci, opt.cx, opt.cs, &out.kmers, &out.counts, &out.n, &stats) != PF_OK) {
        err = who + ": " + pf_last_error(ctx);
        pf_count_abort(ctx);   // (a refusal of the cut-offs leaves the count open)
        return 1;
    }
    tm.finish_s = since(t_finish);
    return 0;
}

int counted_rows(pf_ctx *ctx, const Counted &db, const CountOptions &opt, std::vector<uint64_t> &rows) {
    KmcRecords head;   // the header fields the written database would carry: the rows are kmc_rows' of it
    head.k = opt.k;
    head.counter_size = pf_count::counter_bytes(opt.cx, opt.cs);
    head.min_count = opt.ci;
    head.max_count = opt.cx;
    head.total = db.n;
    head.both_strands = opt.both_strands;
    return kmc_rows_of_counts(ctx, head, db.counts, rows);
}

int write_counted(pf_ctx *ctx, const char *who_c, const std::string &prefix, const Counted &db, const CountOptions &opt, std::string &err) {
    const std::string who = who_c;
    const int k = (int)opt.k, p = pf_count::lut_prefix_len(k);
    if (!p) { err = who + ": " + pf_count::cut_text(pf_count::CUT_K_LAYOUT); return 1; }
    const uint32_t cb = pf_count::counter_bytes(opt.cx, opt.cs), rb = pf_count::suffix_bytes(k, p) + cb;
    const std::string pre_path = prefix + ".kmc_pre", suf_path = prefix + ".kmc_suf";
    const std::string tail = ".tmp." + std::to_string((long)getpid());
    const std::string pre_tmp = pre_path + tail, suf_tmp = suf_path + tail;
    auto fail = [&](const std::string &m) {
        err = m;
        unlink(pre_tmp.c_str());
        unlink(suf_tmp.c_str());
        return 1;
    };
    // the record area, block by block through a pinned buffer
    const uint64_t per_block = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(db.n, 1), WRITE_BLOCK_BYTES / rb));
    ChunkBuf buf;
    if (!buf.alloc(ctx, (size_t)(per_block * rb))) return fail(who + ": no memory for the record buffer");
    int fd = open(suf_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(who + ": cannot write " + suf_tmp + " (" + strerror(errno) + ")");
    bool ok = write_all(fd, "KMCS", 4);
    for (uint64_t at = 0; ok && at < db.n; at += per_block) {
        const uint64_t nb = std::min<uint64_t>(per_block, db.n - at);
        if (pf_kmc_encode(ctx, db.kmers + at, db.counts + at, nb, opt.k, (uint32_t)p, cb, reinterpret_cast<uint8_t *>(buf.p), nullptr) != PF_OK) {
            close(fd);
            return fail(who + ": " + pf_last_error(ctx));
        }
        ok = write_all(fd, buf.p, nb * rb);
    }
    ok = ok && write_all(fd, "KMCS", 4);
    if (!ok) { const int e = errno; close(fd); return fail(who + ": writing " + suf_tmp + " (" + strerror(e) + ")"); }
    if (close(fd) != 0) return fail(who + ": closing " + suf_tmp + " (" + strerror(errno) + ")");
    // the prefix table and the header
    const uint64_t n_lut = 1ull << (2 * p);
    std::vector<uint64_t> lut((size_t)n_lut + 1);
    if (pf_kmc_encode(ctx, db.kmers, db.counts, db.n, opt.k, (uint32_t)p, cb, nullptr, lut.data()) != PF_OK) return fail(who + ": " + pf_last_error(ctx));
    const std::vector<uint8_t> pre = pf_count::kmc1_pre_bytes(lut.data(), n_lut, db.n, k, p, cb, opt.ci, opt.cx, opt.both_strands);
    fd = open(pre_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(who + ": cannot write " + pre_tmp + " (" + strerror(errno) + ")");
    ok = write_all(fd, pre.data(), pre.size());
    if (!ok) { const int e = errno; close(fd); return fail(who + ": writing " + pre_tmp + " (" + strerror(e) + ")"); }
    if (close(fd) != 0) return fail(who + ": closing " + pre_tmp + " (" + strerror(errno) + ")");
    if (rename(suf_tmp.c_str(), suf_path.c_str()) != 0) return fail(who + ": renaming " + suf_tmp + " to " + suf_path + " (" + strerror(errno) + ")");
    if (rename(pre_tmp.c_str(), pre_path.c_str()) != 0) {
        const int e = errno;
        unlink(suf_path.c_str());
        return fail(who + ": renaming " + pre_tmp + " to " + pre_path + " (" + strerror(e) + ")");
    }
    return 0;
}

int count_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const CountOptions &opt, int device, pf_count_stats &stats,
                CountTimes *times, std::string &err) {
    stats = pf_count_stats{};
    CountTimes tm;
    // ---- refusals that need no device ----
    if (inputs.empty()) { err = "count: no input"; return 1; }
    if (out_prefix.empty()) { err = "count: no output prefix"; return 1; }
    { const int c = count_options_clause(opt, true); if (c) { err = std::string("count: ") + pf_count::cut_text(c); return 1; } }
    std::vector<std::string> outputs = {out_prefix + ".kmc_pre", out_prefix + ".kmc_suf"};
    if (!opt.hist.empty()) outputs.push_back(opt.hist);
    std::vector<ReadsInput> reads;
    if (fastq_preflight("count", "counted", inputs, outputs, ReadsOptions{opt.gz, opt.fasta}, reads, err)) return 1;

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("count: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); k-mers are counted on the GPU only";
        return 1;
    }
    CtxGuard ctx_guard{ctx};
    // ---- stream and finish ----
    Counted db;
    if (count_stream(ctx, "count", reads, opt, db, stats, tm, err)) return 1;
    struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
    const auto t_finish = clk::now();
    if (!opt.hist.empty()) {   // from the finished counters before they leave the device
        std::vector<uint64_t> rows;
        if (counted_rows(ctx, db, opt, rows) != PF_OK) { err = std::string("count: histogram of the counters: ") + pf_last_error(ctx); return 1; }
        const std::string text = histogram_text(opt.ci, rows);
        const std::string tmp = opt.hist + ".tmp." + std::to_string((long)getpid());
        const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        const bool ok = fd >= 0 && write_all(fd, text.data(), text.size());
        if (fd >= 0) close(fd);
        if (!ok || rename(tmp.c_str(), opt.hist.c_str()) != 0) {
            err = "count: cannot write " + opt.hist + " (" + strerror(errno) + ")";
            unlink(tmp.c_str());
            return 1;
        }
    }
    tm.finish_s += since(t_finish);
    // ---- write ----
    const auto t_write = clk::now();
    if (write_counted(ctx, "count", out_prefix, db, opt, err)) {
        if (!opt.hist.empty()) unlink(opt.hist.c_str());
        return 1;
    }
    tm.write_s = since(t_write);
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
