#include "pf_cutoffs.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace pfh {

int cutoffs_from_rows(const std::vector<uint64_t> &rows, double quantile, int &lower_raw, int &upper) {
    // src/Main.cpp:226-234
    size_t peak;
    for (peak = 1; peak < rows.size(); peak++)
        if (rows[peak - 1] < rows[peak]) break;
    lower_raw = int(round(1.25 * ((double)peak - 1)));
    // src/Main.cpp:245-276
    std::vector<size_t> v;
    v.reserve(rows.size() + 1);
    v.emplace_back(0);
    for (uint64_t r : rows) v.emplace_back((size_t)r + v.back());
    if (v.size() <= 2) return 1;
    const size_t cf = (size_t)(quantile * (double)(v.back() - v[1]) + (double)v[1]);
    for (peak = 2; peak < v.size(); peak++)
        if (v[peak] > cf) break;
    upper = (int)peak;
    return 0;
}

uint64_t kmc_rows_top(const KmcRecords &db) {
    const uint64_t counter_max = db.counter_size >= 4 ? 0xFFFFFFFFull : (1ull << (8 * db.counter_size)) - 1;
    return std::min<uint64_t>({db.max_count, counter_max, (uint64_t)PF_HIST_MAX_BINS - 1});
}

int kmc_rows_of_counts(pf_ctx *ctx, const KmcRecords &db, const uint32_t *counts_dev, std::vector<uint64_t> &rows) {
    rows.clear();
    const uint64_t top = kmc_rows_top(db);
    if (top < db.min_count) return PF_OK;   // no count can be stored: no row
    std::vector<uint64_t> hist((size_t)top + 1);
    const int st = pf_count_histogram(ctx, counts_dev, db.total, db.min_count, db.max_count, (uint32_t)(top + 1), hist.data());
    if (st != PF_OK) return st;
    rows.assign(hist.begin() + (size_t)db.min_count, hist.end());
    return PF_OK;
}

int kmc_rows(pf_ctx *ctx, const std::string &prefix, std::vector<uint64_t> &rows, uint64_t &min_count, std::string &err) {
    KmcRecords db;
    std::string e;
    if (!db.load(prefix, e)) { err = "Open kmc database " + prefix + " error (" + e + ")"; return 1; }
    min_count = db.min_count;
    uint64_t *dk = nullptr;
    uint32_t *dc = nullptr;
    int st = pf_kmc_decode(ctx, db.records, db.total, db.suffix_bytes, db.counter_size, db.lut.data(), db.n_lut(), db.lut_prefix_len, db.k, &dk, &dc);
    if (st == PF_OK) st = kmc_rows_of_counts(ctx, db, dc, rows);
    pf_device_free(ctx, dk);
    pf_device_free(ctx, dc);
    if (st != PF_OK) { err = std::string("k-mer histogram of ") + prefix + ": " + pf_last_error(ctx); return 1; }
    return 0;
}

int kmc_histogram(const std::string &prefix, int device, std::vector<uint64_t> &rows, uint64_t &min_count, std::string &err) {
    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("k-mer histogram: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); the counters are counted on the GPU only";
        return 1;
    }
    const int rc = kmc_rows(ctx, prefix, rows, min_count, err);
    pf_destroy(ctx);
    return rc;
}

std::string histogram_text(uint64_t min_count, const std::vector<uint64_t> &rows) {
    std::string text;
    char line[64];
    for (size_t r = 0; r < rows.size(); ++r) {
        const int n = snprintf(line, sizeof line, "%llu\t%llu\n", (unsigned long long)(min_count + r), (unsigned long long)rows[r]);
        text.append(line, (size_t)n);
    }
    return text;
}

}  // namespace pfh
