#include "pf_mask_host.hpp"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <memory>

#include "../pf_mask_rule.hpp"
#include "pf_count_host.hpp"
#include "pf_cutoffs.hpp"
#include "pf_host_graph.hpp"
#include "pf_host_util.hpp"
#include "pf_gz_out_host.hpp"
#include "pf_reads_stream.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

// the table is resident: the inputs through K-MASK into out_path
int mask_stream(pf_ctx *ctx, const std::vector<ReadsInput> &inputs, const std::string &out_path, uint32_t low, uint32_t up, uint64_t chunk_bytes,
                bool gz_out, pf_mask_stats &stats, MaskTimes &tm, std::string &err) {
    const auto t_stream = clk::now();
    OutFiles outs("mask");
    if (outs.open_all({out_path}, err)) return 1;
    StreamTimes st_tm;
    std::unique_ptr<GzOutFile> gzo;   // --gz-out: the output stays on the device until it is deflated, and the stream writes nothing itself
    if (gz_out) {
        gzo.reset(new GzOutFile(ctx));
        gzo->start(outs.f[0].fd, "mask", outs.f[0].tmp);
    }
    stream_fastq(ctx, "mask", inputs, chunk_bytes, gzo ? -1 : outs.f[0].fd, outs.f[0].tmp,
                 [&](const Chunk &c, Taken &t) {
                     pf_mask_stats st = {};
                     char *out = c.out;
                     if (gzo && !(out = gzo->place(c.n + 1, err))) return (int)PF_ERR_HIP;   // (err is worded)
                     const int rc = pf_mask_fastq(ctx, c.text, c.n, c.final ? 1 : 0, low, up, out, &t.used, &st, &t.bad);
                     if (rc != PF_OK) return rc;
                     if (gzo && !gzo->take(t.used, false, err)) return (int)PF_ERR_HIP;
                     t.out_len = t.used;
                     t.reads = st.reads;
                     stats.reads += st.reads;
                     stats.reads_changed += st.reads_changed;
                     stats.bases += st.bases;
                     stats.bases_masked += st.bases_masked;
                     stats.kmers += st.kmers;
                     stats.kmers_bad += st.kmers_bad;
                     return (int)PF_OK;
                 },
                 st_tm, err);
    if (gzo) {
        if (err.empty()) gzo->finish(err);
        gzo->stop();
        if (err.empty()) err = gzo->wr.err;
        st_tm.write_s = gzo->wr.write_s;
    }
    if (!err.empty() || outs.commit(err)) return 1;
    tm.stream_s = since(t_stream);
    tm.device_s = st_tm.device_s;
    tm.read_s = st_tm.read_s;
    tm.write_s = st_tm.write_s;
    return 0;
}

// the thresholds once the rows of the histogram are known
int mask_auto_lower(const std::vector<uint64_t> &rows, uint32_t &low, uint32_t up, uint32_t &lower_used, std::string &err) {
    int lo = 0, hi = 0;
    (void)cutoffs_from_rows(rows, 0.998, lo, hi);
    lower_used = low = (uint32_t)std::max(10, lo);
    if (low > up) { err = "mask: the derived lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }
    return 0;
}

int mask_create(int device, pf_ctx **ctx, std::string &err) {
    if (pf_create(device, ctx) == PF_OK) return 0;
    err = std::string("mask: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are masked on the GPU only";
    return 1;
}

}  // namespace

int mask_fastq(const std::string &db_prefix, const std::vector<std::string> &inputs, const std::string &out_path, uint32_t low, uint32_t up,
               bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used, MaskTimes *times, std::string &err, bool gz_out) {
    stats = pf_mask_stats{};
    lower_used = low;
    MaskTimes tm;
    // ---- refusals that need no device: every input is looked at before anything is written ----
    if (inputs.empty()) { err = "mask: no input"; return 1; }
    if (out_path.empty()) { err = "mask: no output path"; return 1; }
    std::vector<ReadsInput> reads;
    if (fastq_preflight("mask", "masked", inputs, {out_path}, ReadsOptions{}, reads, err)) return 1;
    if (!auto_lower && low > up) { err = "mask: the lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }

    // ---- load: the database once -- decode (K-KMC), with auto_lower its histogram (K-HIST), the table ----
    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (mask_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    {
        KmcRecords db;
        std::string e;
        if (!db.load(db_prefix, e)) { err = "Open kmc database " + db_prefix + " error (" + e + ")"; return 1; }
        uint64_t *dk = nullptr;
        uint32_t *dc = nullptr;
        int st = pf_kmc_decode(ctx, db.records, db.total, db.suffix_bytes, db.counter_size, db.lut.data(), db.n_lut(), db.lut_prefix_len, db.k, &dk, &dc);
        std::vector<uint64_t> rows;
        if (st == PF_OK && auto_lower) st = kmc_rows_of_counts(ctx, db, dc, rows);
        if (st == PF_OK) st = pf_upload_counts(ctx, dk, dc, db.total, db.k, db.min_count, db.max_count, db.both_strands);
        pf_device_free(ctx, dk);
        pf_device_free(ctx, dc);
        if (st != PF_OK) { err = "mask: count table of " + db_prefix + ": " + pf_last_error(ctx); return 1; }
        if (auto_lower && mask_auto_lower(rows, low, up, lower_used, err)) return 1;
    }
    tm.load_s = since(t_load);
    if (mask_stream(ctx, reads, out_path, low, up, chunk_bytes, gz_out, stats, tm, err)) return 1;
    if (times) *times = tm;
    return 0;
}

int mask_fastq_counted(const CountOptions &count, const std::string &db_out, const std::vector<std::string> &inputs, const std::string &out_path,
                       uint32_t low, uint32_t up, bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used,
                       MaskTimes *times, std::string &err, bool gz_out) {
    stats = pf_mask_stats{};
    lower_used = low;
    MaskTimes tm;
    if (inputs.empty()) { err = "mask: no input"; return 1; }
    if (out_path.empty()) { err = "mask: no output path"; return 1; }
    std::vector<std::string> outputs = {out_path};
    if (!db_out.empty()) { outputs.push_back(db_out + ".kmc_pre"); outputs.push_back(db_out + ".kmc_suf"); }
    std::vector<ReadsInput> reads;
    if (fastq_preflight("mask", "masked", inputs, outputs, ReadsOptions{}, reads, err)) return 1;
    if (!auto_lower && low > up) { err = "mask: the lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }
    { const int c = count_options_clause(count, !db_out.empty()); if (c) { err = std::string("mask: ") + pf_count::cut_text(c); return 1; } }

    // ---- load: the inputs counted (K-COUNT), with auto_lower the histogram of the finished counters (K-HIST), the table ----
    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (mask_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    {
        CountOptions opt = count;
        opt.chunk_bytes = chunk_bytes;
        Counted db;
        pf_count_stats cst = {};
        CountTimes ctm;
        if (count_stream(ctx, "mask", reads, opt, db, cst, ctm, err)) return 1;
        struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
        std::vector<uint64_t> rows;
        int st = auto_lower ? counted_rows(ctx, db, opt, rows) : (int)PF_OK;
        if (st == PF_OK) st = pf_upload_counts(ctx, db.kmers, db.counts, db.n, opt.k, opt.ci, opt.cx, opt.both_strands ? 1 : 0);
        if (st != PF_OK) { err = std::string("mask: count table of the inputs: ") + pf_last_error(ctx); return 1; }
        if (auto_lower && mask_auto_lower(rows, low, up, lower_used, err)) return 1;
        if (!db_out.empty() && write_counted(ctx, "mask", db_out, db, opt, err)) return 1;
    }
    tm.load_s = since(t_load);
    if (mask_stream(ctx, reads, out_path, low, up, chunk_bytes, gz_out, stats, tm, err)) {
        if (!db_out.empty()) { unlink((db_out + ".kmc_pre").c_str()); unlink((db_out + ".kmc_suf").c_str()); }   // nothing is left after a refusal
        return 1;
    }
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
