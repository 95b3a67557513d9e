#include "pf_hetpair_host.hpp"

#include <algorithm>
#include <chrono>

#include "pf_count_host.hpp"
#include "pf_cutoffs.hpp"
#include "pf_host_graph.hpp"
#include "pf_host_util.hpp"
#include "pf_reads_stream.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

pf_hetpair::Stats rule_stats(const pf_hetpair_stats &s) {
    pf_hetpair::Stats r;
    r.kmers = s.kmers;
    r.in_range = s.in_range;
    r.one_partner = s.one_partner;
    r.many_partners = s.many_partners;
    r.pairs = s.pairs;
    return r;
}

int smudge_create(int device, pf_ctx **ctx, std::string &err) {
    if (pf_create(device, ctx) == PF_OK) return 0;
    err = std::string("smudge: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); k-mer pairs are found on the GPU only";
    return 1;
}

// the refusals of the outputs that need no device
int smudge_outputs(const SmudgeOptions &opt, const std::string &out, std::vector<std::string> &outputs, std::string &err) {
    if (out.empty()) { err = "smudge: no output prefix"; return 1; }
    outputs = {smudge_report_path(out)};
    if (!opt.pairs.empty()) {
        if (same_file(opt.pairs, outputs[0]) || opt.pairs == outputs[0]) { err = "smudge: --pairs " + opt.pairs + " is the report itself"; return 1; }
        outputs.push_back(opt.pairs);
    }
    return 0;
}

// lo and hi from the rows of the histogram, as cutoffL -d / cutoffU -d [q] print them
int smudge_auto_bounds(const std::vector<uint64_t> &rows, double quantile, SmudgeResult &res, std::string &err) {
    int lo = 0, hi = 0;
    if (cutoffs_from_rows(rows, quantile, lo, hi)) { err = "smudge: the histogram of the counters has fewer than two rows: no thresholds can be derived"; return 1; }
    res.lo = (uint32_t)std::max(10, lo);
    res.hi = (uint32_t)std::max(0, hi);
    if (res.lo > res.hi) { err = "smudge: the derived lower threshold " + std::to_string(res.lo) + " is above the derived upper threshold " + std::to_string(res.hi); return 1; }
    if (res.hi - res.lo + 1 > pf_hetpair::MAX_W) { res.hi = res.lo + pf_hetpair::MAX_W - 1; res.clamped = true; }
    return 0;
}

}  // namespace

std::string smudge_report(const uint64_t *table, const pf_hetpair_stats &stats, uint32_t k, uint32_t lo, uint32_t hi, uint64_t n) {
    return pf_hetpair::report_text(table, rule_stats(stats), (int)k, lo, hi, n);
}

std::string smudge_bounds_refusal(const SmudgeOptions &opt) {
    const int c = pf_hetpair::arg_clause(pf_hetpair::MIN_K, opt.lo, opt.hi);
    return c ? std::string(pf_hetpair::arg_text(c)) : std::string();
}

int smudge_resident(pf_ctx *ctx, const char *who_c, const uint64_t *kmers_dev, const uint32_t *counts_dev, uint64_t n_keys, uint32_t k, uint32_t lo,
                    uint32_t hi, uint64_t n_hap, int pairs_fd, const std::string &pairs_name, SmudgeResult &res, std::string &report, std::string &err) {
    const std::string who = who_c;
    { const int c = pf_hetpair::arg_clause((int64_t)k, lo, hi); if (c) { err = who + ": " + pf_hetpair::arg_text(c); return 1; } }
    res.k = k;
    res.lo = lo;
    res.hi = hi;
    const auto t_pairs = clk::now();
    const uint32_t W = hi - lo + 1;
    std::vector<uint64_t> table((size_t)W * W);
    uint64_t *px = nullptr, *py = nullptr, n_pairs = 0;
    uint32_t *cx = nullptr, *cy = nullptr;
    const bool want = pairs_fd >= 0;
    struct Free { pf_ctx *c; uint64_t *&a, *&b; uint32_t *&d, *&e; ~Free() { pf_device_free(c, a); pf_device_free(c, b); pf_device_free(c, d); pf_device_free(c, e); } } free_pairs{ctx, px, py, cx, cy};
    if (pf_hetpairs(ctx, kmers_dev, counts_dev, n_keys, k, lo, hi, table.data(), want ? &px : nullptr, want ? &py : nullptr, want ? &cx : nullptr,
                    want ? &cy : nullptr, &n_pairs, &res.stats) != PF_OK) {
        err = who + ": " + pf_last_error(ctx);
        return 1;
    }
    res.times.pairs_s = since(t_pairs);
    if (n_hap) res.summary = pf_hetpair::summarize(table.data(), lo, hi, n_hap);
    const auto t_write = clk::now();
    report = smudge_report(table.data(), res.stats, k, lo, hi, n_hap);
    if (want) {
        std::vector<uint64_t> hx((size_t)n_pairs), hy((size_t)n_pairs);
        std::vector<uint32_t> hcx((size_t)n_pairs), hcy((size_t)n_pairs);
        if (n_pairs && (pf_copy_to_host(ctx, hx.data(), px, (size_t)n_pairs * 8) != PF_OK || pf_copy_to_host(ctx, hy.data(), py, (size_t)n_pairs * 8) != PF_OK ||
                        pf_copy_to_host(ctx, hcx.data(), cx, (size_t)n_pairs * 4) != PF_OK || pf_copy_to_host(ctx, hcy.data(), cy, (size_t)n_pairs * 4) != PF_OK)) {
            err = who + ": " + pf_last_error(ctx);
            return 1;
        }
        std::string block;
        for (uint64_t i = 0; i < n_pairs; ++i) {
            block += pf_hetpair::pair_line(hx[(size_t)i], hy[(size_t)i], hcx[(size_t)i], hcy[(size_t)i], (int)k);
            if (block.size() >= (1u << 22) || i + 1 == n_pairs) {
                if (!write_all(pairs_fd, block.data(), block.size(), who, pairs_name, err)) return 1;
                block.clear();
            }
        }
    }
    res.times.write_s = since(t_write);
    return 0;
}

// pf_hetpairs over the resident table, then the outputs under temporary names, renamed together
static int smudge_write(pf_ctx *ctx, const uint64_t *kmers_dev, const uint32_t *counts_dev, uint64_t n_keys, uint32_t k, const SmudgeOptions &opt,
                        const std::vector<std::string> &outputs, SmudgeResult &res, std::string &err) {
    OutFiles outs("smudge");
    if (outs.open_all(outputs, err)) return 1;
    std::string report;
    const bool want = outputs.size() > 1;
    if (smudge_resident(ctx, "smudge", kmers_dev, counts_dev, n_keys, k, res.lo, res.hi, opt.n, want ? outs.f[1].fd : -1, want ? outs.f[1].tmp : "", res, report, err))
        return 1;
    const auto t_write = clk::now();
    if (!write_all(outs.f[0].fd, report.data(), report.size(), "smudge", outs.f[0].tmp, err)) return 1;
    if (outs.commit(err)) return 1;
    res.times.write_s += since(t_write);
    return 0;
}

int smudge_db(const std::string &db_prefix, const SmudgeOptions &opt, const std::string &out, int device, SmudgeResult &res, std::string &err) {
    res = SmudgeResult();
    err.clear();   // (the caller's string may hold an earlier call's refusal: OutFiles::commit renames only while it is empty)
    // ---- refusals that need no device ----
    if (db_prefix.empty()) { err = "smudge: no database"; return 1; }
    std::vector<std::string> outputs;
    if (smudge_outputs(opt, out, outputs, err)) return 1;
    if (!opt.auto_cutoffs) { const std::string why = smudge_bounds_refusal(opt); if (!why.empty()) { err = "smudge: " + why; return 1; } }
    for (const std::string &o : outputs)
        for (const char *ext : {".kmc_pre", ".kmc_suf"})
            if (o == db_prefix + ext || same_file(o, db_prefix + ext)) { err = "smudge: the output " + o + " is a file of the database"; return 1; }
    KmcRecords db;
    { std::string e; if (!db.load(db_prefix, e)) { err = "Open kmc database " + db_prefix + " error (" + e + ")"; return 1; } }
    if (!db.both_strands) { err = "smudge: " + db_prefix + " was counted with -b: smudge needs canonical counts"; return 1; }
    if (!pf_count::k_ok(db.k)) { err = std::string("smudge: ") + pf_hetpair::arg_text(pf_hetpair::ARG_K); return 1; }

    // ---- load: decode (K-KMC), with auto_cutoffs the histogram (K-HIST), the table ----
    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (smudge_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    uint64_t *dk = nullptr;
    uint32_t *dc = nullptr;
    struct Free { pf_ctx *c; uint64_t *&k; uint32_t *&n; ~Free() { pf_device_free(c, k); pf_device_free(c, n); } } free_db{ctx, dk, dc};
    int st = pf_kmc_decode(ctx, db.records, db.total, db.suffix_bytes, db.counter_size, db.lut.data(), db.n_lut(), db.lut_prefix_len, db.k, &dk, &dc);
    std::vector<uint64_t> rows;
    if (st == PF_OK && opt.auto_cutoffs) st = kmc_rows_of_counts(ctx, db, dc, rows);
    if (st == PF_OK) st = pf_upload_counts(ctx, dk, dc, db.total, db.k, db.min_count, db.max_count, 1);
    if (st != PF_OK) { err = "smudge: count table of " + db_prefix + ": " + pf_last_error(ctx); return 1; }
    res.lo = opt.lo;
    res.hi = opt.hi;
    if (opt.auto_cutoffs && smudge_auto_bounds(rows, opt.quantile, res, err)) return 1;
    const bool clamped = res.clamped;
    const double load_s = since(t_load);
    if (smudge_write(ctx, dk, dc, db.total, db.k, opt, outputs, res, err)) return 1;
    res.clamped = clamped;
    res.times.load_s = load_s;
    return 0;
}

int smudge_counted(const CountOptions &count, const std::vector<std::string> &inputs, const SmudgeOptions &opt, const std::string &out, int device,
                   SmudgeResult &res, std::string &err) {
    res = SmudgeResult();
    err.clear();
    if (inputs.empty()) { err = "smudge: no input"; return 1; }
    std::vector<std::string> outputs;
    if (smudge_outputs(opt, out, outputs, err)) return 1;
    if (!opt.auto_cutoffs) { const std::string why = smudge_bounds_refusal(opt); if (!why.empty()) { err = "smudge: " + why; return 1; } }
    { const int c = count_options_clause(count, false); if (c) { err = std::string("smudge: ") + pf_count::cut_text(c); return 1; } }
    if (!count.both_strands) { err = "smudge: -b: smudge needs canonical counts"; return 1; }
    std::vector<ReadsInput> reads;
    if (fastq_preflight("smudge", "counted", inputs, outputs, ReadsOptions{count.gz, count.fasta}, reads, err)) return 1;

    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (smudge_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    Counted db;
    pf_count_stats cst = {};
    CountTimes ctm;
    if (count_stream(ctx, "smudge", reads, count, db, cst, ctm, err)) return 1;
    struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
    std::vector<uint64_t> rows;
    int st = opt.auto_cutoffs ? counted_rows(ctx, db, count, rows) : (int)PF_OK;
    if (st == PF_OK) st = pf_upload_counts(ctx, db.kmers, db.counts, db.n, count.k, count.ci, count.cx, 1);
    if (st != PF_OK) { err = std::string("smudge: count table of the inputs: ") + pf_last_error(ctx); return 1; }
    res.lo = opt.lo;
    res.hi = opt.hi;
    if (opt.auto_cutoffs && smudge_auto_bounds(rows, opt.quantile, res, err)) return 1;
    const bool clamped = res.clamped;
    const double load_s = since(t_load);
    if (smudge_write(ctx, db.kmers, db.counts, db.n, count.k, opt, outputs, res, err)) return 1;
    res.clamped = clamped;
    res.times.load_s = load_s;
    return 0;
}

}  // namespace pfh
