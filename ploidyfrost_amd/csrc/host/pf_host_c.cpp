#include <chrono>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "pf_bfs_host.hpp"
#include "pf_cdbg.hpp"
#include "pf_cutoffs.hpp"
#include "pf_mask_host.hpp"
#include "pf_hetpair_host.hpp"
#include "pf_count_host.hpp"
#include "pf_build_host.hpp"
#include "pf_run_host.hpp"
#include "pf_runmulti_host.hpp"
#include "../pf_runmulti_rule.hpp"
#include "../pf_run_rule.hpp"
#include "pf_bfg_write.hpp"
#include "../pf_mask_rule.hpp"
#include "../pf_trim_rule.hpp"
#include "../pf_trimrun_rule.hpp"
#include "../pf_deflate_rule.hpp"
#include "../pf_inflate_rule.hpp"
#include "../pf_gunzip_rule.hpp"
#include "../pf_fasta_rule.hpp"
#include "pf_trim_host.hpp"
#include "pf_trace.hpp"
#include "../pf_model_rows.hpp"
#include "../pf_filter_rows.hpp"
#include "pf_filter.hpp"
#include "pf_gmm_model.hpp"
#include "pf_host_colors.hpp"
#include "pf_host_minz.hpp"
#include "pf_replay_par.hpp"
#include "ploidyfrost_host.h"

struct pfh_run {
    pfh::UnitigSet graph;
    std::unique_ptr<pfh::ColoredUnitigSet> cgraph;  // colored runs: graph + colour sets (then `graph` stays empty)
    std::unique_ptr<pfh::CDBG> cdbg;
    pfh::CCDBG *ccdbg = nullptr;                     // == cdbg.get() for colored runs
    const pfh::UnitigSet &g() const { return cgraph ? cgraph->graph : graph; }
    double z_M = 2, z_D = -1, z_G = -3;
    size_t z = 8;
    double load_s = 0, upload_s = 0;
    std::string err;
    // pfh_set_auto_cutoffs: the database prefix (colored runs: the list file), the thresholds derived from it, and those the last
    // estimation used
    std::string kmc;
    bool auto_cutoffs = false;
    std::vector<std::pair<int, int>> auto_cut, used_cut;
};

static std::string g_open_err;

// no C++ exception may cross the C boundary
template <class F>
static int guarded(pfh_run *r, F &&f) {
    r->err.clear();   // (a message of an earlier call must not outlive it: pfh_last_error prefers this string)
    try {
        return f();
    } catch (const std::exception &e) {
        r->err = std::string("ploidyfrost host layer: ") + e.what();
        return PF_ERR_ARG;
    } catch (...) {
        r->err = "ploidyfrost host layer: unknown exception";
        return PF_ERR_ARG;
    }
}


struct pfh_gmm {
    pfh::GmmModel model;
    std::string err;
    explicit pfh_gmm(int device) : model(device) {}
};
template <class F>
static int gmm_guard(pfh_gmm *m, F &&fn) {
    if (!m) return 1;
    m->err.clear();
    try {
        return fn();
    } catch (const std::exception &e) {
        m->err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}

extern "C" {

pfh_run *pfh_open(const char *gfa_path, const char *kmc_prefix, uint32_t complex_size, double match, double mismatch,
                  double gap, int device) {
    using clk = std::chrono::steady_clock;
    try {
    auto r = std::make_unique<pfh_run>();
    auto t0 = clk::now();
    // K-GFA: parsed and packed on the device by the CDBG constructor, where the numbering is finished as well (K-MINZ)
    static const bool host_gfa = [] { const char *e = getenv("PF_GFA"); return e && !strcmp(e, "host"); }();
    if (!(host_gfa ? r->graph.load_gfa(gfa_path, g_open_err, true) : r->graph.open_gfa(gfa_path, g_open_err))) return nullptr;
    r->load_s = std::chrono::duration<double>(clk::now() - t0).count();
    r->z = complex_size;
    r->z_M = match; r->z_D = mismatch; r->z_G = gap;
    t0 = clk::now();
    r->cdbg = std::make_unique<pfh::CDBG>(r->graph, r->z, r->z_M, r->z_D, r->z_G, kmc_prefix ? kmc_prefix : "", device, true);
    r->upload_s = std::chrono::duration<double>(clk::now() - t0).count();
    if (!r->cdbg->good()) { g_open_err = r->cdbg->error(); return nullptr; }
    r->kmc = kmc_prefix ? kmc_prefix : "";
    return r.release();
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return nullptr;
    }
}

pfh_run *pfh_open_colored(const char *gfa_path, const char *colors_path, const char *kmc_list_file, uint32_t complex_size,
                          double match, double mismatch, double gap, uint32_t threads, int device) {
    using clk = std::chrono::steady_clock;
    try {
        auto r = std::make_unique<pfh_run>();
        auto t0 = clk::now();
        r->cgraph = std::make_unique<pfh::ColoredUnitigSet>();
        if (!r->cgraph->read(gfa_path, colors_path, threads ? threads : 1, false)) { g_open_err = r->cgraph->err; return nullptr; }
        r->load_s = std::chrono::duration<double>(clk::now() - t0).count();
        r->z = complex_size;
        r->z_M = match; r->z_D = mismatch; r->z_G = gap;
        t0 = clk::now();
        auto cc = std::make_unique<pfh::CCDBG>(*r->cgraph, r->z, r->z_M, r->z_D, r->z_G, kmc_list_file ? kmc_list_file : "",
                                               (size_t)(threads ? threads : 1), device, true);
        r->upload_s = std::chrono::duration<double>(clk::now() - t0).count();
        if (!cc->good()) { g_open_err = cc->error(); return nullptr; }
        r->ccdbg = cc.get();
        r->cdbg = std::move(cc);
        r->kmc = kmc_list_file ? kmc_list_file : "";
        return r.release();
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return nullptr;
    }
}

uint32_t pfh_num_colors(const pfh_run *r) { return r->cgraph ? (uint32_t)r->cgraph->getNbColors() : 0; }

int pfh_ploidy_estimation_colored(pfh_run *r, const char *outpre, const int *lower, const int *upper, uint32_t n_colors) {
    if (!r->ccdbg) { r->err = "pfh_ploidy_estimation_colored: the run was not opened with pfh_open_colored"; return PF_ERR_ARG; }
    return guarded(r, [&] {
        std::vector<std::pair<int, int>> cut(n_colors);
        if (r->auto_cutoffs) cut = r->auto_cut;
        else for (uint32_t c = 0; c < n_colors; ++c) cut[c] = {lower[c], upper[c]};
        r->used_cut = cut;
        return r->ccdbg->ploidyEstimation_multithread_ptr(outpre, cut, 1);
    });
}

void pfh_close(pfh_run *r) { delete r; }
const char *pfh_last_error(const pfh_run *r) {
    if (!r) return g_open_err.c_str();
    return !r->err.empty() ? r->err.c_str() : r->cdbg->error().c_str();
}
void pfh_set_output_dir(pfh_run *r, const char *dir) { r->cdbg->set_output_dir(dir); }
void pfh_set_write_files(pfh_run *r, int on) { r->cdbg->set_write_files(on != 0); }
void pfh_set_threads(pfh_run *r, uint32_t threads) { r->cdbg->set_threads(threads); }
void pfh_set_overlap_output(pfh_run *r, int on) { r->cdbg->set_overlap_output(on != 0); }
void pfh_set_third_tier_on_host(pfh_run *r, int on) { r->cdbg->set_third_tier_on_host(on != 0); }
int pfh_set_reference_threads(pfh_run *r, uint32_t n) {
    return guarded(r, [&] { return r->cdbg->set_reference_threads(n); });
}
void pfh_set_batch_bubbles(pfh_run *r, uint64_t n) { r->cdbg->set_batch_bubbles((size_t)n); }
void pfh_set_align_pieces(pfh_run *r, uint64_t n) { r->cdbg->set_align_pieces((size_t)n); }
int pfh_set_unitig_id(pfh_run *r, const char *outpre) {
    return guarded(r, [&] { return r->cdbg->setUnitigId(outpre, "", 1); });
}
int pfh_find_superbubbles(pfh_run *r, const char *outpre) {
    return guarded(r, [&] { return r->cdbg->findSuperBubble_multithread_ptr(outpre, 1); });
}
int pfh_ploidy_estimation(pfh_run *r, const char *outpre, int lower, int upper) {
    return guarded(r, [&] {
        if (r->auto_cutoffs && !r->auto_cut.empty()) { lower = r->auto_cut[0].first; upper = r->auto_cut[0].second; }
        r->used_cut.assign(1, {lower, upper});
        return r->cdbg->ploidyEstimation_multithread_ptr(outpre, lower, upper, 1);
    });
}

// ---- thresholds from the database itself (K-HIST) ---------------------------------------------------
int pfh_kmc_histogram(const char *kmc_prefix, uint64_t *rows_out, uint64_t cap, uint64_t *n_rows, uint64_t *min_count) {
    if (!kmc_prefix || !n_rows) { g_open_err = "pfh_kmc_histogram: prefix and n_rows are needed"; return 1; }
    try {
        std::vector<uint64_t> rows;
        uint64_t mn = 0;
        if (pfh::kmc_histogram(kmc_prefix, 0, rows, mn, g_open_err)) return 1;
        *n_rows = rows.size();
        if (min_count) *min_count = mn;
        if (rows_out) std::copy(rows.begin(), rows.begin() + (size_t)std::min<uint64_t>(cap, rows.size()), rows_out);
        return 0;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_cutoffs_from_rows(const uint64_t *rows, uint64_t n, double quantile, int *lower, int *upper) {
    if ((n && !rows) || !lower || !upper) return 2;
    int lo = 0, up = 0;
    const int rc = pfh::cutoffs_from_rows(std::vector<uint64_t>(rows, rows + n), quantile, lo, up);
    *lower = lo;
    if (!rc) *upper = up;
    return rc;
}
int pfh_set_auto_cutoffs(pfh_run *r, double quantile) {
    return guarded(r, [&] {
        r->auto_cutoffs = false;
        r->auto_cut.clear();
        r->used_cut.clear();
        if (quantile < 0) return (int)PF_OK;
        if (quantile > 1) { r->err = "Error: frequency cutoff value should be between 0 and 1 "; return (int)PF_ERR_ARG; }
        std::vector<std::string> names;
        if (r->ccdbg) {   // one database name per line, one line per colour (src/CCDBG.cpp:13-43)
            FILE *f = fopen(r->kmc.c_str(), "r");
            if (!f) { r->err = "pfh_set_auto_cutoffs: cannot read the database list " + r->kmc; return (int)PF_ERR_ARG; }
            std::string cur;
            int ch;
            while ((ch = fgetc(f)) != EOF) {
                if (ch == '\n') { names.push_back(cur); cur.clear(); }
                else cur.push_back((char)ch);
            }
            if (!cur.empty()) names.push_back(cur);
            fclose(f);
            names.resize(r->cgraph->getNbColors());
        } else {
            if (r->kmc.empty()) { r->err = "pfh_set_auto_cutoffs: the run was opened without a database"; return (int)PF_ERR_ARG; }
            names.push_back(r->kmc);
        }
        std::vector<std::pair<int, int>> cut;
        for (const std::string &name : names) {
            std::vector<uint64_t> rows;
            uint64_t mn = 0;
            if (pfh::kmc_rows(r->cdbg->device(), name, rows, mn, r->err)) return (int)PF_ERR_ARG;
            int lo = 0, up = 0;
            if (pfh::cutoffs_from_rows(rows, quantile, lo, up)) { r->err = "Error: Histogram File is badly Formatted."; return (int)PF_ERR_ARG; }
            lo = std::max(10, lo);
            if (lo > up) { r->err = "Error: lower cutoff need be smaller than upper cutoff "; return (int)PF_ERR_ARG; }
            cut.push_back({lo, up});
        }
        r->auto_cut = cut;
        r->auto_cutoffs = true;
        return (int)PF_OK;
    });
}
uint32_t pfh_cutoffs(const pfh_run *r, int *lower, int *upper, uint32_t cap) {
    const std::vector<std::pair<int, int>> &v = !r->used_cut.empty() ? r->used_cut : r->auto_cut;
    for (uint32_t c = 0; c < cap && c < v.size(); ++c) {
        if (lower) lower[c] = v[c].first;
        if (upper) upper[c] = v[c].second;
    }
    return (uint32_t)v.size();
}
void *pfh_device_ctx(pfh_run *r) { return r->cdbg->device(); }

// ---- blocked-gzip inputs: the next reads call of this thread takes them (`--gz`) ----
static thread_local int g_reads_gz = 0;   // 0, 1 `--gz`, 2 `--gz-plain`
void pfh_reads_gz(int on) { g_reads_gz = on == 2 ? 2 : on != 0; }
static int take_reads_gz() { const int gz = g_reads_gz; g_reads_gz = 0; return gz; }
// ---- blocked-gzip output: the next trim or mask call of this thread writes it (`--gz-out`) ----
static thread_local bool g_reads_gz_out = false;
void pfh_reads_gz_out(int on) { g_reads_gz_out = on != 0; }
static bool take_reads_gz_out() { const bool g = g_reads_gz_out; g_reads_gz_out = false; return g; }
// ---- FASTA inputs: the next count, build or run call of this thread takes them (`--fasta`) ----
static thread_local bool g_reads_fasta = false;
void pfh_reads_fasta(int on) { g_reads_fasta = on != 0; }
static bool take_reads_fasta() { const bool f = g_reads_fasta; g_reads_fasta = false; return f; }
// the host rule of K-FASTA (pf_fasta::index_fasta): the compacted text and the table of one chunk.  0, or the clause; the sizes needed
// come back in n_records / n_bases whatever the capacities.
int pfh_fasta_index(const char *text, uint64_t n, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases, char *text_out,
                    uint64_t text_cap, uint64_t *read_off, uint32_t *read_len, uint64_t table_cap) {
    pf_fasta::Index ix;
    const int clause = pf_fasta::index_fasta(text, n, final != 0, ix);
    if (bytes_used) *bytes_used = ix.bytes_used;
    if (n_records) *n_records = ix.n_records;
    if (n_bases) *n_bases = ix.bases;
    if (text_out && ix.bases <= text_cap && ix.bases) memcpy(text_out, ix.text.data(), (size_t)ix.bases);
    for (uint64_t i = 0; i < table_cap && i < ix.n_records; ++i) {
        if (read_off) read_off[i] = ix.read_off[i];
        if (read_len) read_len[i] = ix.read_len[i];
    }
    return clause;
}
const char *pfh_fasta_clause_text(int clause) { return pf_fasta::clause_text(clause); }

// ---- reads masked against the database (K-MASK) ----------------------------------------------------
int pfh_mask_fastq(const char *db_prefix, const char *const *inputs, uint32_t n_inputs, const char *out_path, uint32_t low, uint32_t up,
                   int auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats *stats, uint32_t *lower_used) {
    if (!db_prefix || !out_path || (n_inputs && !inputs)) { g_open_err = "pfh_mask_fastq: database, inputs and output are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pf_mask_stats st = {};
        uint32_t lower = low;
        const int rc = pfh::mask_fastq(db_prefix, in, out_path, low, up, auto_lower != 0, chunk_bytes, device, st, lower, nullptr, g_open_err, take_reads_gz_out());
        if (stats) *stats = st;
        if (lower_used) *lower_used = lower;
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
uint64_t pfh_mask_read(const char *seq, uint64_t n, uint32_t k, const uint32_t *counters, uint32_t low, uint32_t up, char *out) {
    return pf_mask::mask_read(seq, n, k, counters, low, up, out);
}
int pfh_mask_index_fastq(const char *text, uint64_t n, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *bad_record,
                         uint64_t *read_off, uint32_t *read_len, uint64_t cap) {
    uint64_t used = 0, recs = 0, bad = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    const int clause = pf_mask::index_fastq(text, n, final != 0, used, recs, bad, &off, &len);
    if (bytes_used) *bytes_used = used;
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    for (uint64_t i = 0; i < cap && i < off.size(); ++i) {
        if (read_off) read_off[i] = off[i];
        if (read_len) read_len[i] = len[i];
    }
    return clause;
}
const char *pfh_mask_clause_text(int clause) { return pf_mask::clause_text(clause); }

// ---- adapters clipped in front of the steps (K-CLIP) ---------------------------------------------------
// `--adapters`: the switch of the next trim / run call of this thread, and what that call reported
static thread_local pfh::ClipOptions g_reads_adapters;
static thread_local pfh::ClipReport g_clip_report;
void pfh_reads_adapters(const char *path, uint32_t seed, uint32_t score) {
    g_reads_adapters = pfh::ClipOptions{};
    g_reads_adapters.adapters = path ? path : "";
    g_reads_adapters.seed = seed;
    g_reads_adapters.score = score;
}
void pfh_reads_adapter_pairs(uint32_t pair_score, uint32_t pair_min, int keep_both) {
    g_reads_adapters.pairs = true;
    g_reads_adapters.pair_score = pair_score;
    g_reads_adapters.pair_min = pair_min;
    g_reads_adapters.keep_both = keep_both != 0;
}
static pfh::ClipOptions take_reads_adapters() {
    const pfh::ClipOptions c = g_reads_adapters;
    g_reads_adapters = pfh::ClipOptions{};
    g_clip_report = pfh::ClipReport{};
    return c;
}
void pfh_reads_adapters_report(uint32_t *adapters, uint32_t *skipped, pf_clip_stats *stats) {
    if (adapters) *adapters = g_clip_report.adapters;
    if (skipped) *skipped = g_clip_report.skipped;
    if (stats) *stats = g_clip_report.stats;
}
void pfh_reads_adapters_pair_report(uint32_t *pairs, pf_clip_pair_stats *stats) {
    if (pairs) *pairs = g_clip_report.pairs;
    if (stats) *stats = g_clip_report.pair_stats;
}
int pfh_clip_parse_adapter_pairs(const char *text, uint64_t n, char *bases, uint64_t bases_cap, uint32_t *adapter_off, uint8_t *side, uint32_t *n_adapters,
                                 char *prefix_bases, uint64_t prefix_cap, uint32_t *prefix_off, uint32_t *n_pairs, uint64_t *bad_record) {
    pf_clip::Adapters A;
    uint64_t bad = 0;
    const int c = pf_clip::parse_adapters(text ? text : "", text ? (size_t)n : 0, A, &bad, true);
    if (n_adapters) *n_adapters = A.size();
    if (n_pairs) *n_pairs = A.pairs();
    if (bad_record) *bad_record = bad;
    if (c) return c;
    if (bases) memcpy(bases, A.bases.data(), std::min<uint64_t>(bases_cap, A.bases.size()));
    if (adapter_off) memcpy(adapter_off, A.off.data(), A.off.size() * 4);
    if (side && A.size()) memcpy(side, A.side.data(), A.size());
    if (prefix_bases) memcpy(prefix_bases, A.prefix_bases.data(), std::min<uint64_t>(prefix_cap, A.prefix_bases.size()));
    if (prefix_off) memcpy(prefix_off, A.prefix_off.data(), A.prefix_off.size() * 4);
    return 0;
}
int pfh_clip_parse_adapters(const char *text, uint64_t n, char *bases, uint64_t bases_cap, uint32_t *adapter_off, uint8_t *side, uint32_t *n_adapters,
                            uint32_t *skipped, uint64_t *bad_record) {
    pf_clip::Adapters A;
    uint64_t bad = 0;
    const int c = pf_clip::parse_adapters(text ? text : "", text ? (size_t)n : 0, A, &bad);
    if (n_adapters) *n_adapters = A.size();
    if (skipped) *skipped = A.skipped;
    if (bad_record) *bad_record = bad;
    if (c) return c;
    if (bases) memcpy(bases, A.bases.data(), std::min<uint64_t>(bases_cap, A.bases.size()));
    if (adapter_off) memcpy(adapter_off, A.off.data(), A.off.size() * 4);
    if (side && A.size()) memcpy(side, A.side.data(), A.size());
    return 0;
}
const char *pfh_clip_refusal_text(int refusal) { return pf_clip::refusal_text(refusal); }
static int clip_set_refused(const char *who, const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters, uint32_t file_side, uint32_t seed,
                            uint32_t score, uint32_t phred) {
    uint32_t bad = 0;
    const int c = pf_clip::set_clause(bases, off, side, n_adapters, seed, score, &bad);
    if (c) { g_open_err = std::string(who) + ": " + pf_clip::refusal_text(c); return 1; }
    if (file_side != 1 && file_side != 2) { g_open_err = std::string(who) + ": the side of a file is 1 or 2"; return 1; }
    if (phred != 33 && phred != 64) { g_open_err = std::string(who) + ": " + pf_trim::refusal_text(pf_trim::REFUSE_PHRED) + ", not " + std::to_string(phred); return 1; }
    return 0;
}
int pfh_clip_read(const char *seq, const char *qual, uint64_t n, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                  uint32_t file_side, uint32_t seed, uint32_t score, uint32_t phred, uint32_t *clip_end, uint64_t *scored) {
    if (clip_set_refused("pfh_clip_read", bases, adapter_off, side, n_adapters, file_side, seed, score, phred)) return -1;
    if (n > 0x7FFFFFFFull) { g_open_err = "pfh_clip_read: a read holds fewer than 2^31 bases"; return -1; }
    uint64_t sc = 0;
    const uint32_t e = pf_clip::clip_read(seq, qual, (uint32_t)n, bases, adapter_off, side, n_adapters, file_side, seed, score, phred, &sc);
    if (clip_end) *clip_end = e;
    if (scored) *scored = sc;
    return 0;
}
static int clip_pair_set_refused(const char *who, const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters, const char *prefix_bases,
                                 const uint32_t *prefix_off, uint32_t n_pairs, uint32_t seed, uint32_t score, uint32_t pair_score, uint32_t pair_min, uint32_t phred) {
    const int c = pf_clip::pair_set_clause(bases, off, side, n_adapters, prefix_bases, prefix_off, n_pairs, seed, score, pair_score, pair_min);
    if (c) { g_open_err = std::string(who) + ": " + pf_clip::refusal_text(c); return 1; }
    if (phred != 33 && phred != 64) { g_open_err = std::string(who) + ": " + pf_trim::refusal_text(pf_trim::REFUSE_PHRED) + ", not " + std::to_string(phred); return 1; }
    return 0;
}
static pf_clip::PairSet pair_set(const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs, uint32_t pair_score, uint32_t pair_min, int keep_both) {
    pf_clip::PairSet P;
    P.prefix_bases = prefix_bases;
    P.prefix_off = prefix_off;
    P.n_pairs = n_pairs;
    P.pair_score = pair_score;
    P.pair_min = pair_min;
    P.keep_both = keep_both != 0;
    return P;
}
int pfh_clip_pair(const char *seq1, const char *qual1, uint64_t n1, const char *seq2, const char *qual2, uint64_t n2, const char *bases,
                  const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs,
                  uint32_t seed, uint32_t score, uint32_t pair_score, uint32_t pair_min, int keep_both, uint32_t phred, uint32_t clip_end[2],
                  pf_clip_stats *clip, pf_clip_pair_stats *pairs) {
    if (clip_pair_set_refused("pfh_clip_pair", bases, adapter_off, side, n_adapters, prefix_bases, prefix_off, n_pairs, seed, score, pair_score, pair_min, phred)) return -1;
    if (n1 > 0x7FFFFFFFull || n2 > 0x7FFFFFFFull) { g_open_err = "pfh_clip_pair: a read holds fewer than 2^31 bases"; return -1; }
    uint32_t end[2] = {0, 0};
    pf_clip::Stats cs = {};
    pf_clip::PairStats ps = {};
    pf_clip::clip_pair(seq1, qual1, (uint32_t)n1, seq2, qual2, (uint32_t)n2, bases, adapter_off, side, n_adapters,
                       pair_set(prefix_bases, prefix_off, n_pairs, pair_score, pair_min, keep_both), seed, score, phred, end, &cs, &ps);
    if (clip_end) { clip_end[0] = end[0]; clip_end[1] = end[1]; }
    if (clip) memcpy(clip, &cs, sizeof cs);
    if (pairs) memcpy(pairs, &ps, sizeof ps);
    return 0;
}

// ---- the read quality report (K-QC) --------------------------------------------------------------------
// `--report`: the switch of the next trim / run call of this thread
static thread_local std::string g_reads_report;
void pfh_reads_report(const char *path) { g_reads_report = path ? path : ""; }
static std::string take_reads_report() {
    std::string r;
    r.swap(g_reads_report);
    return r;
}
int pfh_qc_fastq(const char *const *inputs1, uint32_t n1, const char *const *inputs2, uint32_t n2, const char *report_path, uint32_t phred, uint64_t chunk_bytes,
                 int device) {
    const int gz = take_reads_gz();
    if ((n1 && !inputs1) || (n2 && !inputs2)) { g_open_err = "pfh_qc_fastq: inputs are needed"; return 1; }
    try {
        std::vector<std::string> in1, in2;
        for (uint32_t i = 0; i < n1; ++i) in1.push_back(inputs1[i] ? inputs1[i] : "");
        for (uint32_t i = 0; i < n2; ++i) in2.push_back(inputs2[i] ? inputs2[i] : "");
        pfh::QcOptions opt;
        opt.phred = phred;
        opt.gz = gz;
        opt.chunk_bytes = chunk_bytes;
        pfh::QcReport rep;
        return pfh::qc_fastq(in1, in2, report_path ? report_path : "", opt, device, rep, g_open_err);
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_qc_fastq_chunk(const char *text, uint64_t n, int final, uint32_t phred, uint32_t file_side, int trimmed, const pf_trim_step *steps, uint32_t n_steps,
                       int clip_open, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t seed, uint32_t score,
                       uint64_t *raw, uint64_t *kept, uint64_t *clip, uint64_t *bytes_used, uint64_t *n_records, uint64_t *bad_record) {
    auto refuse = [&](const std::string &m) { g_open_err = "pfh_qc_fastq_chunk: " + m; return -1; };
    if (!raw || (trimmed && !kept) || (trimmed && clip_open && !clip)) return refuse("the tables are needed");
    if (n && !text) return refuse("text is needed");
    if (file_side != 1 && file_side != 2) return refuse("the side of a file is 1 or 2");
    if (phred != 33 && phred != 64) return refuse(std::string(pf_trim::refusal_text(pf_trim::REFUSE_PHRED)) + ", not " + std::to_string(phred));
    pf_qc::ClipSet cs;
    if (trimmed) {
        uint32_t bad = 0;
        const int c = pf_trim::steps_clause(reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, &bad);
        if (c && !(c == pf_trim::REFUSE_NO_STEP && clip_open && n_steps == 0)) return refuse(pf_trim::refusal_text(c));
        if (clip_open) {
            const int cc = pf_clip::set_clause(bases, adapter_off, side, n_adapters, seed, score, &bad);
            if (cc) return refuse(pf_clip::refusal_text(cc));
            cs.open = true;
            cs.bases = bases;
            cs.off = adapter_off;
            cs.side = side;
            cs.n_adapters = n_adapters;
            cs.seed = seed;
            cs.score = score;
        }
    }
    uint64_t used = 0, recs = 0, bad_rec = 0;
    const int clause = pf_qc::qc_fastq_chunk(text ? text : "", n, final != 0, phred, file_side, trimmed != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, cs,
                                             raw, kept, clip, used, recs, bad_rec);
    if (bytes_used) *bytes_used = used;
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad_rec;
    return clause;
}
uint32_t pfh_qc_phred_hint(uint64_t min_byte, uint64_t reads) { return pf_qc::phred_hint(min_byte, reads); }
int pfh_qc_report_text(const uint64_t *tables, const uint64_t *clip, uint32_t phred, char *out, uint64_t cap, uint64_t *len) {
    if (!tables || !len) { g_open_err = "pfh_qc_report_text: tables and len are needed"; return -1; }
    const std::string t = pf_qc::report_text(tables, clip, phred);
    *len = t.size();
    if (out) memcpy(out, t.data(), std::min<uint64_t>(cap, t.size()));
    return 0;
}

// ---- duplicate reads dropped (K-DEDUP) ----------------------------------------------------------------
// `--dedup`: the switch of the next trim / run call of this thread, and what that call reported (over all its units)
static thread_local pfh::DedupOptions g_reads_dedup;
static thread_local pf_dedup_stats g_dedup_report = {};
void pfh_reads_dedup(int on, uint32_t bases, uint64_t initial_slots) {
    g_reads_dedup = pfh::DedupOptions{};
    g_reads_dedup.on = on != 0;
    g_reads_dedup.bases = bases;
    g_reads_dedup.initial_slots = initial_slots;
}
static pfh::DedupOptions take_reads_dedup() {
    const pfh::DedupOptions d = g_reads_dedup;
    g_reads_dedup = pfh::DedupOptions{};
    g_dedup_report = pf_dedup_stats{};
    return d;
}
static void dedup_report_add(const pf_dedup_stats &s) {
    pf_dedup_stats &r = g_dedup_report;
    r.units += s.units; r.unique += s.unique; r.duplicates += s.duplicates;
    r.max_copies = std::max(r.max_copies, s.max_copies);
    for (uint32_t l = 0; l < pf_dedup::LEVELS; ++l) r.levels[l] += s.levels[l];
    r.slots = std::max(r.slots, s.slots);
    r.growths += s.growths;
}
void pfh_reads_dedup_report(pf_dedup_stats *stats) { if (stats) *stats = g_dedup_report; }
int pfh_dedup_key(const char *seq1, uint64_t n1, const char *seq2, uint64_t n2, uint32_t bases, uint64_t key[2]) {
    auto refuse = [&](const std::string &m) { g_open_err = "pfh_dedup_key: " + m; return -1; };
    if (!key) return refuse("key is needed");
    if ((n1 && !seq1) || (n2 && !seq2)) return refuse("the reads are needed");
    if (!pf_dedup::bases_ok(bases)) return refuse("bases is 0 (the whole read) or 16 .. 4096, not " + std::to_string(bases));
    if (n1 > 0xFFFFFFFFull || n2 > 0xFFFFFFFFull) return refuse("a read holds fewer than 2^32 bases");
    pf_dedup::key_of(seq1 ? seq1 : "", (uint32_t)n1, seq2 ? seq2 : "", (uint32_t)n2, seq2 != nullptr, bases, key);
    return 0;
}
int pfh_dedup_units(const uint64_t *keys, const uint8_t *participates, uint64_t n, uint8_t *keep, pf_dedup_stats *stats) {
    if (n && !keys) { g_open_err = "pfh_dedup_units: keys are needed"; return -1; }
    pfh::DedupSeen seen;
    pfh::dedup_units(seen, keys, participates, n, keep);
    if (stats) *stats = pfh::dedup_stats_of(seen);
    return 0;
}
// what pf_trim_fastq / pf_trim_fastq_pair give for one chunk while a dedup is open, given the keys of the units that took part before
static int trim_chunk_dedup(const char *who, int n_files, const char *const *text_in, const uint64_t *n_in, int final, const pf_trim_step *steps, uint32_t n_steps,
                            uint32_t phred, uint32_t bases, const uint64_t *seen_keys, uint64_t n_seen, char *const *out, uint64_t *out_bytes,
                            uint64_t *bytes_used, uint32_t *const *rec_begin, uint32_t *const *rec_len, uint64_t *rec_keys, uint64_t cap, uint64_t *n_records,
                            pf_trim_stats *stats, uint64_t *bad_record) {
    auto refuse = [&](const std::string &m) { g_open_err = std::string(who) + ": " + m; return -1; };
    if (!pf_dedup::bases_ok(bases)) return refuse("bases is 0 (the whole read) or 16 .. 4096, not " + std::to_string(bases));
    if (n_seen && !seen_keys) return refuse("the keys seen before are needed");
    {
        pfh::TrimOptions o;
        if (steps) o.steps.assign(steps, steps + n_steps);
        o.phred = phred;
        o.dedup.on = true;
        o.dedup.bases = bases;
        if (pfh::trim_options_clause(o, g_open_err)) return -1;
    }
    pfh::DedupSeen seen;
    pfh::dedup_units(seen, seen_keys, nullptr, n_seen, nullptr);
    const int n_dest = n_files == 2 ? 4 : 1;
    std::string o[4];
    std::vector<uint32_t> rb[2], rl[2];
    std::vector<uint64_t> keys;
    uint64_t used[2] = {0, 0}, recs = 0, bad = 0;
    pf_trim::Stats st[2] = {};
    const char *text[2] = {"", ""};
    uint64_t nn[2] = {0, 0};
    for (int f = 0; f < n_files; ++f)
        if (text_in[f]) { text[f] = text_in[f]; nn[f] = n_in[f]; }
    const int clause = pfh::dedup_trim_chunk(n_files, text, nn, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, bases, seen, o, used, recs,
                                             bad, rb, rl, st, &keys);
    for (int d = 0; d < n_dest; ++d) {
        if (out_bytes) out_bytes[d] = o[d].size();
        if (out && out[d] && !o[d].empty()) memcpy(out[d], o[d].data(), o[d].size());
    }
    for (int f = 0; f < n_files; ++f) {
        if (bytes_used) bytes_used[f] = used[f];
        if (stats) memcpy(&stats[f], &st[f], sizeof st[f]);
        for (uint64_t i = 0; i < cap && i < rb[f].size(); ++i) {
            if (rec_begin && rec_begin[f]) rec_begin[f][i] = rb[f][i];
            if (rec_len && rec_len[f]) rec_len[f][i] = rl[f][i];
        }
    }
    if (rec_keys)
        for (uint64_t i = 0; i < 2 * cap && i < keys.size(); ++i) rec_keys[i] = keys[i];
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    return clause;
}
int pfh_trim_fastq_chunk_dedup(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint32_t bases,
                               const uint64_t *seen_keys, uint64_t n_seen, char *out, uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin,
                               uint32_t *rec_len, uint64_t *rec_keys, uint64_t cap, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record) {
    return trim_chunk_dedup("pfh_trim_fastq_chunk_dedup", 1, &text, &n, final, steps, n_steps, phred, bases, seen_keys, n_seen, &out, out_bytes, bytes_used,
                            &rec_begin, &rec_len, rec_keys, cap, n_records, stats, bad_record);
}
int pfh_trim_fastq_pair_chunk_dedup(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                                    uint32_t phred, uint32_t bases, const uint64_t *seen_keys, uint64_t n_seen, char *out[4], uint64_t out_bytes[4],
                                    uint64_t bytes_used[2], uint32_t *rec_begin[2], uint32_t *rec_len[2], uint64_t *rec_keys, uint64_t cap, uint64_t *n_records,
                                    pf_trim_stats stats[2], uint64_t *bad_record) {
    const char *text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    return trim_chunk_dedup("pfh_trim_fastq_pair_chunk_dedup", 2, text, n, final, steps, n_steps, phred, bases, seen_keys, n_seen, out, out_bytes, bytes_used,
                            rec_begin, rec_len, rec_keys, cap, n_records, stats, bad_record);
}

// ---- reads quality-trimmed (K-TRIM) ------------------------------------------------------------------
static pfh::TrimOptions trim_options(const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *trimlog, uint64_t chunk_bytes) {
    pfh::TrimOptions opt;
    if (steps) opt.steps.assign(steps, steps + n_steps);
    opt.phred = phred;
    opt.trimlog = trimlog ? trimlog : "";
    opt.chunk_bytes = chunk_bytes;
    opt.gz = take_reads_gz();
    opt.gz_out = take_reads_gz_out();
    return opt;
}
// (the stream calls alone take the adapters switch: the restatements below take their adapters as arguments)
static pfh::TrimOptions trim_stream_options(const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *trimlog, uint64_t chunk_bytes,
                                            const pfh::ClipOptions &clip) {
    pfh::TrimOptions opt = trim_options(steps, n_steps, phred, trimlog, chunk_bytes);
    opt.clip = clip;
    opt.report = take_reads_report();
    opt.dedup = take_reads_dedup();
    return opt;
}
int pfh_trim_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_path, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                   const char *trimlog, uint64_t chunk_bytes, int device, pf_trim_stats *stats) {
    const pfh::ClipOptions clip = take_reads_adapters();   // taken first: a refusal below does not leave the switch to the next call
    if (!out_path || (n_inputs && !inputs)) { g_open_err = "pfh_trim_fastq: inputs and output are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pf_trim_stats st = {};
        const pfh::TrimOptions topt = trim_stream_options(steps, n_steps, phred, trimlog, chunk_bytes, clip);
        const int rc = pfh::trim_fastq(in, out_path, topt, device, st, nullptr, g_open_err, &g_clip_report, nullptr, &g_dedup_report);
        if (stats) *stats = st;
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_trim_fastq_pair(const char *in1, const char *in2, const char *const *out_paths, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                        const char *trimlog, uint64_t chunk_bytes, int device, pf_trim_stats *stats) {
    const pfh::ClipOptions clip = take_reads_adapters();   // taken first: a refusal below does not leave the switch to the next call
    if (!in1 || !in2 || !out_paths || !out_paths[0] || !out_paths[1] || !out_paths[2] || !out_paths[3]) {
        g_open_err = "pfh_trim_fastq_pair: two inputs and four outputs are needed";
        return 1;
    }
    try {
        const std::string out[4] = {out_paths[0], out_paths[1], out_paths[2], out_paths[3]};
        pf_trim_stats st[2] = {};
        const pfh::TrimOptions topt = trim_stream_options(steps, n_steps, phred, trimlog, chunk_bytes, clip);
        const int rc = pfh::trim_fastq_pair(in1, in2, out, topt, device, st, nullptr, g_open_err, &g_clip_report, nullptr, &g_dedup_report);
        if (stats) { stats[0] = st[0]; stats[1] = st[1]; }
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_trim_parse_step(const char *word, pf_trim_step *step) {
    pf_trim::Step s;
    const int c = pf_trim::parse_step(word ? word : "", s);
    if (step) *step = pf_trim_step{s.kind, s.a, s.b};
    return c;
}
const char *pfh_trim_refusal_text(int refusal) { return pf_trim::refusal_text(refusal); }
int pfh_trim_read(const char *qual, uint64_t n, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint32_t *begin, uint32_t *end) {
    if (pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;
    if (n > 0xFFFFFFFFull) { g_open_err = "pfh_trim_read: a read holds fewer than 2^32 bases"; return -1; }
    uint32_t b = 0, e = 0;
    const bool kept = pf_trim::trim_read(qual, (uint32_t)n, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, b, e);
    if (begin) *begin = b;
    if (end) *end = e;
    return kept ? 1 : 0;
}
int pfh_trim_fastq_chunk(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, char *out,
                         uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t cap, uint64_t *n_records,
                         pf_trim_stats *stats, uint64_t *bad_record) {
    if (pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;
    std::string o;
    std::vector<uint32_t> rb, rl;
    uint64_t used = 0, recs = 0, bad = 0;
    pf_trim::Stats st = {};
    const int clause = pf_trim::trim_fastq(text, n, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, o, used, recs, bad, &rb, &rl, &st);
    if (out_bytes) *out_bytes = o.size();
    if (out && !o.empty()) memcpy(out, o.data(), o.size());
    if (bytes_used) *bytes_used = used;
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    if (stats) memcpy(stats, &st, sizeof st);
    for (uint64_t i = 0; i < cap && i < rb.size(); ++i) {
        if (rec_begin) rec_begin[i] = rb[i];
        if (rec_len) rec_len[i] = rl[i];
    }
    return clause;
}
int pfh_trim_fastq_pair_chunk_clip(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                                   uint32_t phred, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                                   const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs, uint32_t seed, uint32_t score, uint32_t pair_score,
                                   uint32_t pair_min, int keep_both, char *out[4], uint64_t out_bytes[4], uint64_t bytes_used[2], uint32_t *rec_begin[2],
                                   uint32_t *rec_len[2], uint32_t *clip_end[2], uint64_t cap, uint64_t *n_records, pf_trim_stats stats[2], pf_clip_stats *clip,
                                   pf_clip_pair_stats *pairs, uint64_t *bad_record) {
    const char *who = "pfh_trim_fastq_pair_chunk_clip";
    if (clip_pair_set_refused(who, bases, adapter_off, side, n_adapters, prefix_bases, prefix_off, n_pairs, seed, score, pair_score, pair_min, phred)) return -1;
    if (n_steps && pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;   // (no step beside adapters is a plan)
    std::string o[4];
    std::vector<uint32_t> rb[2], rl[2], ce[2];
    std::vector<uint32_t> *prb[2] = {&rb[0], &rb[1]}, *prl[2] = {&rl[0], &rl[1]}, *pce[2] = {&ce[0], &ce[1]};
    uint64_t used[2] = {0, 0}, recs = 0, bad = 0;
    pf_trim::Stats st[2] = {};
    pf_clip::Stats cs = {};
    pf_clip::PairStats ps = {};
    const char *text[2] = {text1 ? text1 : "", text2 ? text2 : ""};
    const uint64_t nn[2] = {text1 ? n1 : 0, text2 ? n2 : 0};
    const int clause = pf_clip::trim_fastq_pair(text, nn, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, bases, adapter_off, side, n_adapters,
                                                pair_set(prefix_bases, prefix_off, n_pairs, pair_score, pair_min, keep_both), seed, score, o, used, recs, bad, prb, prl,
                                                st, &cs, &ps, pce);
    for (int d = 0; d < 4; ++d) {
        if (out_bytes) out_bytes[d] = o[d].size();
        if (out && out[d] && !o[d].empty()) memcpy(out[d], o[d].data(), o[d].size());
    }
    for (int f = 0; f < 2; ++f) {
        if (bytes_used) bytes_used[f] = used[f];
        if (stats) memcpy(&stats[f], &st[f], sizeof st[f]);
        for (uint64_t i = 0; i < cap && i < rb[f].size(); ++i) {
            if (rec_begin && rec_begin[f]) rec_begin[f][i] = rb[f][i];
            if (rec_len && rec_len[f]) rec_len[f][i] = rl[f][i];
            if (clip_end && clip_end[f]) clip_end[f][i] = ce[f][i];
        }
    }
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    if (clip) memcpy(clip, &cs, sizeof cs);
    if (pairs) memcpy(pairs, &ps, sizeof ps);
    return clause;
}
int pfh_trim_fastq_chunk_clip(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *bases,
                              const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t file_side, uint32_t seed, uint32_t score, char *out,
                              uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t cap, uint64_t *n_records,
                              pf_trim_stats *stats, pf_clip_stats *clip, uint64_t *bad_record) {
    if (clip_set_refused("pfh_trim_fastq_chunk_clip", bases, adapter_off, side, n_adapters, file_side, seed, score, phred)) return -1;
    if (n_steps && pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;   // (no step beside adapters is a plan)
    std::string o;
    std::vector<uint32_t> rb, rl;
    uint64_t used = 0, recs = 0, bad = 0;
    pf_trim::Stats st = {};
    pf_clip::Stats cs = {};
    const int clause = pf_clip::trim_fastq(text, n, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, bases, adapter_off, side, n_adapters,
                                           file_side, seed, score, o, used, recs, bad, &rb, &rl, &st, &cs);
    if (out_bytes) *out_bytes = o.size();
    if (out && !o.empty()) memcpy(out, o.data(), o.size());
    if (bytes_used) *bytes_used = used;
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    if (stats) memcpy(stats, &st, sizeof st);
    if (clip) memcpy(clip, &cs, sizeof cs);
    for (uint64_t i = 0; i < cap && i < rb.size(); ++i) {
        if (rec_begin) rec_begin[i] = rb[i];
        if (rec_len) rec_len[i] = rl[i];
    }
    return clause;
}

// ---- k-mers counted from reads (K-COUNT) -----------------------------------------------------------
static pfh::CountOptions count_options(uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs, int both_strands) {
    pfh::CountOptions opt;
    opt.k = k;
    opt.ci = ci;
    opt.cx = cx;
    opt.cs = cs;
    opt.both_strands = both_strands != 0;
    return opt;
}
int pfh_count_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                    int both_strands, const char *hist, uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *stats) {
    if (!out_prefix || (n_inputs && !inputs)) { g_open_err = "pfh_count_fastq: inputs and output prefix are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pfh::CountOptions opt = count_options(k, ci, cx, cs, both_strands);
        opt.chunk_bytes = chunk_bytes;
        opt.initial_slots = initial_slots;
        opt.gz = take_reads_gz();
        opt.fasta = take_reads_fasta();
        if (hist) opt.hist = hist;
        pf_count_stats st = {};
        const int rc = pfh::count_fastq(in, out_prefix, opt, device, st, nullptr, g_open_err);
        if (stats) *stats = st;
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_mask_fastq_counted(const char *const *inputs, uint32_t n_inputs, const char *out_path, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                           int both_strands, const char *db_out, uint32_t low, uint32_t up, int auto_lower, uint64_t chunk_bytes, int device,
                           pf_mask_stats *stats, uint32_t *lower_used) {
    if (!out_path || (n_inputs && !inputs)) { g_open_err = "pfh_mask_fastq_counted: inputs and output are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pf_mask_stats st = {};
        uint32_t lower = low;
        const int rc = pfh::mask_fastq_counted(count_options(k, ci, cx, cs, both_strands), db_out ? db_out : "", in, out_path, low, up, auto_lower != 0,
                                               chunk_bytes, device, st, lower, nullptr, g_open_err, take_reads_gz_out());
        if (stats) *stats = st;
        if (lower_used) *lower_used = lower;
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
static void count_stats_c(const pf_count::Stats &s, pf_count_stats *out) {
    if (!out) return;
    *out = pf_count_stats{s.reads, s.bases, s.kmers, s.kmers_bad, s.unique, s.below_min, s.above_max, s.written};
}
int pfh_count_reads_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t k, int both_strands, uint64_t ci,
                         uint64_t cx, uint64_t cs, uint64_t *kmers_out, uint32_t *counts_out, uint64_t cap, uint64_t *n, pf_count_stats *stats) {
    if (n) *n = 0;
    if (!pf_count::k_ok(k)) return pf_count::CUT_K;
    const int clause = pf_count::cut_clause(ci, cx, cs);
    if (clause) return clause;
    pf_count::Table table;
    pf_count::Stats st;
    pf_count::count_reads_host(text, off, len, n_reads, (int)k, both_strands != 0, table, st);
    std::vector<uint64_t> kmers;
    std::vector<uint32_t> counts;
    if (!pf_count::finish_host(table, (uint32_t)ci, (uint32_t)cx, (uint32_t)cs, kmers, counts, st)) return -1;
    for (uint64_t i = 0; i < cap && i < kmers.size(); ++i) {
        if (kmers_out) kmers_out[i] = kmers[i];
        if (counts_out) counts_out[i] = counts[i];
    }
    if (n) *n = kmers.size();
    count_stats_c(st, stats);
    return 0;
}
int pfh_count_encode_kmc1(const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                          int both_strands, uint8_t *pre_out, uint64_t pre_cap, uint64_t *pre_n, uint8_t *suf_out, uint64_t suf_cap, uint64_t *suf_n) {
    if (!pf_count::k_ok(k)) return pf_count::CUT_K;
    if (!pf_count::lut_prefix_len((int)k)) return pf_count::CUT_K_LAYOUT;
    const int clause = pf_count::cut_clause(ci, cx, cs);
    if (clause) return clause;
    std::vector<uint8_t> pre, suf;
    pf_count::encode_kmc1_host(kmers, counts, n, (int)k, pf_count::lut_prefix_len((int)k), pf_count::counter_bytes(cx, cs), ci, cx, both_strands != 0, pre, suf);
    if (pre_out) memcpy(pre_out, pre.data(), (size_t)std::min<uint64_t>(pre_cap, pre.size()));
    if (suf_out) memcpy(suf_out, suf.data(), (size_t)std::min<uint64_t>(suf_cap, suf.size()));
    if (pre_n) *pre_n = pre.size();
    if (suf_n) *suf_n = suf.size();
    return 0;
}
uint32_t pfh_count_counter_bytes(uint64_t cx, uint64_t cs) { return pf_count::counter_bytes(cx, cs); }
uint32_t pfh_count_lut_prefix_len(uint32_t k) { return (uint32_t)pf_count::lut_prefix_len((int)k); }
const char *pfh_count_cut_text(int clause) { return pf_count::cut_text(clause); }

// ---- `build` (K-UNITIG) ----
static_assert(pfh::BuildOptions::G_DEFAULT == PFH_UNITIG_G_DEFAULT, "one sentinel for the default minimizer length");
int pfh_build_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, int32_t g, int clip_tips, int del_isolated,
                    uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *counted, pf_unitig_stats *stats) {
    if (!out_prefix || (n_inputs && !inputs)) { g_open_err = "pfh_build_fastq: inputs and output prefix are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pfh::BuildOptions opt;
        opt.fasta = take_reads_fasta();
        opt.k = k;
        opt.g = g;
        opt.clip_tips = clip_tips != 0;
        opt.del_isolated = del_isolated != 0;
        opt.chunk_bytes = chunk_bytes;
        opt.initial_slots = initial_slots;
        pf_count_stats cst = {};
        pf_unitig_stats st = {};
        const int rc = pfh::build_fastq(in, out_prefix, opt, device, cst, st, nullptr, g_open_err);
        if (counted) *counted = cst;
        if (stats) *stats = st;
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
// ---- `run` (K-MASKCOUNT) ----
void pfh_run_defaults(pfh_run_options *o) {
    if (!o) return;
    const pfh::RunOptions d;
    *o = pfh_run_options{};
    o->k = d.k;
    o->ci = d.ci; o->cx = d.cx; o->cs = d.cs;
    o->g = d.g;
    o->clip_tips = d.clip_tips; o->del_isolated = d.del_isolated;
    o->quantile = d.quantile;
    o->mask_up = d.mask_up;
    o->complex_size = (uint32_t)d.complex_size;
    o->match = d.match; o->mismatch = d.mismatch; o->gap = d.gap;
    o->threads = 1;
    o->model_source = -1;
}
static void run_options_from(const pfh_run_options *o, pfh::RunOptions &opt) {
    opt.k = o->k;
    opt.ci = o->ci; opt.cx = o->cx; opt.cs = o->cs;
    opt.g = o->g;
    opt.clip_tips = o->clip_tips != 0; opt.del_isolated = o->del_isolated != 0;
    opt.chunk_bytes = o->chunk_bytes; opt.initial_slots = o->initial_slots;
    opt.quantile = o->quantile;
    opt.mask_up = o->mask_up;
    opt.complex_size = o->complex_size;
    opt.match = o->match; opt.mismatch = o->mismatch; opt.gap = o->gap;
    if (o->db_out) opt.db_out = o->db_out;
    if (o->gfa_out) opt.gfa_out = o->gfa_out;
}
// the clip reports of a run's units as the one report of the call
static void clip_report_sum(const std::vector<pfh::ClipReport> &units) {
    for (const pfh::ClipReport &u : units) {
        g_clip_report.adapters = u.adapters;
        g_clip_report.skipped = u.skipped;
        g_clip_report.pairs_on = u.pairs_on;
        g_clip_report.pairs = u.pairs;
        g_clip_report.pair_stats.pairs_clipped += u.pair_stats.pairs_clipped;
        g_clip_report.pair_stats.pairs_dropped += u.pair_stats.pairs_dropped;
        g_clip_report.pair_stats.pairs_too_long += u.pair_stats.pairs_too_long;
        g_clip_report.pair_stats.candidates_scored += u.pair_stats.candidates_scored;
        for (int f = 0; f < 2; ++f) g_clip_report.pair_stats.bases_clipped[f] += u.pair_stats.bases_clipped[f];
        for (int f = 0; f < 2; ++f) {
            g_clip_report.stats.reads_clipped[f] += u.stats.reads_clipped[f];
            g_clip_report.stats.reads_dropped[f] += u.stats.reads_dropped[f];
            g_clip_report.stats.bases_clipped[f] += u.stats.bases_clipped[f];
            g_clip_report.stats.candidates_scored[f] += u.stats.candidates_scored[f];
        }
    }
}
static void trim_inputs_from(const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const pfh::ClipOptions &clip, const pfh::DedupOptions &dedup,
                             pfh::TrimInputs &t) {
    t.steps.assign(steps, steps + (steps ? n_steps : 0));
    t.phred = phred;
    t.clip = clip;
    t.dedup = dedup;
}
// `--smudge [--smudge-n N] [--smudge-pairs FILE]`: the switch of the next run call of this thread, and what that call found
struct ReadsSmudge {
    bool on = false, n_seen = false;
    uint64_t n = 0;
    std::string pairs;
};
static thread_local ReadsSmudge g_reads_smudge;
static thread_local pfh_smudge_result g_smudge_result = {};
void pfh_reads_smudge(int on, int64_t n_hap, const char *pairs_path) {
    g_reads_smudge = ReadsSmudge();
    g_reads_smudge.on = on != 0;
    g_reads_smudge.n_seen = n_hap >= 0;
    g_reads_smudge.n = n_hap >= 0 ? (uint64_t)n_hap : 0;
    g_reads_smudge.pairs = pairs_path ? pairs_path : "";
}
void pfh_reads_smudge_result(pfh_smudge_result *out) { if (out) *out = g_smudge_result; }
static ReadsSmudge take_reads_smudge() {
    ReadsSmudge r;
    std::swap(r, g_reads_smudge);
    return r;
}
static void smudge_result_c(const pfh::SmudgeResult &r, pfh_smudge_result *out) {
    if (!out) return;
    out->stats = r.stats;
    out->k = r.k;
    out->lo = r.lo;
    out->hi = r.hi;
    out->clamped = r.clamped ? 1 : 0;
    out->proposed_p = r.summary.best.p;
    out->proposed_m = r.summary.best.m;
    out->proposed_pairs = r.summary.best_pairs;
    out->all_pairs = r.summary.all_pairs;
}
static int run_fastq_c(const char *who, const char *const *inputs, uint32_t n_inputs, int paired, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                       const char *out_prefix, const pfh_run_options *o, int device, pfh_run_stats *stats, pf_trim_stats *per_unit) {
    const pfh::ClipOptions clip = take_reads_adapters();   // taken first: a refusal below does not leave the switch to the next call
    const pfh::DedupOptions dedup = take_reads_dedup();
    const ReadsSmudge smudge = take_reads_smudge();
    g_smudge_result = pfh_smudge_result{};
    if (!out_prefix || !o || (n_inputs && !inputs)) { g_open_err = std::string(who) + ": inputs, output prefix and options are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pfh::RunOptions opt;
        run_options_from(o, opt);
        opt.gz = take_reads_gz();
        opt.fasta = take_reads_fasta();
        opt.call.threads = o->threads ? o->threads : 1;
        if (o->model_source >= 0) {
            opt.call.model.on = true;
            opt.call.model.only = o->model_only != 0;
            opt.call.model.source = o->model_source;
        }
        trim_inputs_from(steps, n_steps, phred, clip, dedup, opt.trim);
        opt.report = take_reads_report();
        opt.paired = paired != 0;
        opt.smudge = smudge.on;
        opt.smudge_n = smudge.n;
        opt.smudge_n_seen = smudge.n_seen;
        opt.smudge_pairs = smudge.pairs;
        pfh::RunStats st;
        const int rc = pfh::run_fastq(in, out_prefix, opt, device, st, nullptr, g_open_err);
        if (!rc && opt.smudge) smudge_result_c(st.smudge, &g_smudge_result);
        if (stats)
            *stats = pfh_run_stats{st.counted.reads, st.counted.bases, st.counted.kmers, st.counted.kmers_bad, st.counted.unique, st.lower, st.upper,
                                   st.masked.kmers_bad, st.masked.kmers_kept, st.distinct_kept, st.graph.unitigs, st.graph.removed, st.graph.unitigs_out,
                                   st.graph.longest};
        if (per_unit) std::copy(st.trim.begin(), st.trim.end(), per_unit);
        clip_report_sum(st.clip);
        for (const pf_dedup_stats &u : st.dedup) dedup_report_add(u);
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_run_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, const pfh_run_options *o, int device, pfh_run_stats *stats) {
    return run_fastq_c("pfh_run_fastq", inputs, n_inputs, 0, nullptr, 0, 33, out_prefix, o, device, stats, nullptr);
}
int pfh_run_fastq_trimmed(const char *const *inputs, uint32_t n_inputs, int paired, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                          const char *out_prefix, const pfh_run_options *o, int device, pfh_run_stats *stats, pf_trim_stats *per_unit) {
    return run_fastq_c("pfh_run_fastq_trimmed", inputs, n_inputs, paired, steps, n_steps, phred, out_prefix, o, device, stats, per_unit);
}
// ---- `run-multi` (K-UNION, K-COLORSET) ----
static int run_multi_fastq_c(const char *who, const char *const *names, const uint32_t *n_inputs_of, const int *paired_of, uint32_t n_samples,
                             const char *const *inputs, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *out_prefix,
                             const pfh_run_options *o, const pf_filter_multi_opts *multi, int each_color, int device, pfh_run_multi_stats *stats,
                             uint64_t *per_color, pf_trim_stats *per_input) {
    const pfh::ClipOptions clip = take_reads_adapters();   // taken first: a refusal below does not leave the switch to the next call
    const pfh::DedupOptions dedup = take_reads_dedup();
    { const ReadsSmudge sm = take_reads_smudge(); if (sm.on || sm.n_seen || !sm.pairs.empty()) { g_open_err = "run-multi: --smudge is not built into run-multi (`smudge` or `run --smudge` per sample)"; return 1; } }
    if (!take_reads_report().empty()) { g_open_err = "run-multi: --report is not built into run-multi (`trim --report` or `run --report` per sample)"; return 1; }
    if (!out_prefix || !o || (n_samples && (!names || !n_inputs_of))) { g_open_err = std::string(who) + ": samples, output prefix and options are needed"; return 1; }
    try {
        std::vector<pfh::MultiSample> samples(n_samples);
        uint64_t at = 0;
        for (uint32_t c = 0; c < n_samples; ++c) {
            samples[c].name = names[c] ? names[c] : "";
            samples[c].paired = paired_of && paired_of[c];
            for (uint32_t i = 0; i < n_inputs_of[c]; ++i, ++at) samples[c].inputs.push_back(inputs && inputs[at] ? inputs[at] : "");
        }
        pfh::RunMultiOptions mopt;
        pfh::RunOptions &opt = mopt.run;
        opt.gz = take_reads_gz();
        opt.fasta = take_reads_fasta();
        run_options_from(o, opt);
        trim_inputs_from(steps, n_steps, phred, clip, dedup, opt.trim);
        mopt.call.threads = o->threads ? o->threads : 1;
        if (o->model_source >= 0) {
            if (!multi) { g_open_err = "run-multi: a model reads the coloured result streams behind the options of filter-multi: multi is needed"; return 1; }
            mopt.call.model.on = true;
            mopt.call.model.only = o->model_only != 0;
            mopt.call.model.source = o->model_source;
            mopt.call.filter_multi = multi;
            mopt.call.each_color = each_color != 0;
        }
        pfh::RunMultiStats st;
        const int rc = pfh::run_multi_fastq(samples, out_prefix, mopt, device, st, nullptr, g_open_err);
        if (stats)
            *stats = pfh_run_multi_stats{st.colors, st.reads, st.bases, st.kmers, st.bad, st.distinct, st.windows_bad, st.windows_kept, st.distinct_kept,
                                         st.graph.unitigs, st.graph.removed, st.graph.unitigs_out, st.graph.longest, st.kmers_colored, st.kmers_unplaced,
                                         st.runs, st.overflow, st.color_bytes};
        if (per_color)
            for (size_t c = 0; c < st.color.size() && c < n_samples; ++c) {
                per_color[4 * c] = st.color[c].lower;
                per_color[4 * c + 1] = st.color[c].upper;
                per_color[4 * c + 2] = st.color[c].distinct;
                per_color[4 * c + 3] = st.color[c].kept;
            }
        for (const auto &units : st.clip) clip_report_sum(units);
        for (const auto &units : st.dedup)
            for (const pf_dedup_stats &u : units) dedup_report_add(u);
        if (per_input) {   // one entry per input file; a single-ended sample's unit stands in its first entry
            uint64_t i = 0;
            for (uint32_t c = 0; c < n_samples; i += n_inputs_of[c], ++c)
                for (size_t j = 0; j < n_inputs_of[c]; ++j) per_input[i + j] = c < st.trim.size() && j < st.trim[c].size() ? st.trim[c][j] : pf_trim_stats{};
        }
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_run_multi_fastq(const char *const *names, const uint32_t *n_inputs_of, uint32_t n_samples, const char *const *inputs, const char *out_prefix,
                        const pfh_run_options *o, const pf_filter_multi_opts *multi, int each_color, int device, pfh_run_multi_stats *stats,
                        uint64_t *per_color) {
    return run_multi_fastq_c("pfh_run_multi_fastq", names, n_inputs_of, nullptr, n_samples, inputs, nullptr, 0, 33, out_prefix, o, multi, each_color, device, stats,
                             per_color, nullptr);
}
int pfh_run_multi_fastq_trimmed(const char *const *names, const uint32_t *n_inputs_of, const int *paired_of, uint32_t n_samples, const char *const *inputs,
                                const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *out_prefix, const pfh_run_options *o,
                                const pf_filter_multi_opts *multi, int each_color, int device, pfh_run_multi_stats *stats, uint64_t *per_color,
                                pf_trim_stats *per_input) {
    return run_multi_fastq_c("pfh_run_multi_fastq_trimmed", names, n_inputs_of, paired_of, n_samples, inputs, steps, n_steps, phred, out_prefix, o, multi,
                             each_color, device, stats, per_color, per_input);
}
// ---- `run STEP...`: the table of the reads handed on, on the host (../pf_trimrun_rule.hpp) ----
int pfh_trim_table_chunk(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint64_t *read_off,
                         uint32_t *read_len, uint64_t cap, uint64_t *n_reads, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats,
                         uint64_t *bad_record) {
    if (pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint64_t used = 0, recs = 0, bad = 0;
    pf_trim::Stats st = {};
    const int clause = pf_trimrun::reads_table(text, n, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, off, len, used, recs, bad, &st);
    if (n_reads) *n_reads = off.size();
    if (bytes_used) *bytes_used = used;
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    if (stats) memcpy(stats, &st, sizeof st);
    for (uint64_t i = 0; i < cap && i < off.size(); ++i) {
        if (read_off) read_off[i] = off[i];
        if (read_len) read_len[i] = len[i];
    }
    return clause;
}
int pfh_trim_table_chunk_pair(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                              uint32_t phred, uint64_t *const read_off[2], uint32_t *const read_len[2], uint64_t cap, uint64_t *n_reads, uint64_t bytes_used[2],
                              uint64_t *n_records, pf_trim_stats stats[2], uint64_t *bad_record) {
    if (pfh::trim_options_clause(trim_options(steps, n_steps, phred, nullptr, 0), g_open_err)) return -1;
    const char *const text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> len[2];
    uint64_t used[2] = {0, 0}, recs = 0, bad = 0;
    pf_trim::Stats st[2] = {};
    const int clause = pf_trimrun::reads_table_pair(text, n, final != 0, reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, off, len, used, recs, bad, st);
    if (n_reads) *n_reads = off[0].size();
    if (n_records) *n_records = recs;
    if (bad_record) *bad_record = bad;
    for (int f = 0; f < 2; ++f) {
        if (bytes_used) bytes_used[f] = used[f];
        if (stats) memcpy(&stats[f], &st[f], sizeof st[f]);
        for (uint64_t i = 0; i < cap && i < off[f].size(); ++i) {
            if (read_off && read_off[f]) read_off[f][i] = off[f][i];
            if (read_len && read_len[f]) read_len[f][i] = len[f][i];
        }
    }
    return clause;
}
const char *pfh_trim_table_clause_text(int clause) { return pf_trimrun::clause_text(clause); }
int pfh_union_host(const uint64_t *const *sets, const uint64_t *n, uint32_t n_sets, uint64_t *out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || (n_sets && (!sets || !n))) { g_open_err = "pfh_union_host: sets, n and n_out are needed"; return 1; }
    std::vector<std::vector<uint64_t>> v(n_sets);
    for (uint32_t c = 0; c < n_sets; ++c) {
        const std::string why = pf_runmulti::set_refusal(sets[c], n[c], c);
        if (!why.empty()) { g_open_err = "pfh_union_host: " + why; return 1; }
        v[c].assign(sets[c], sets[c] + n[c]);
    }
    const std::vector<uint64_t> u = pf_runmulti::union_host(std::move(v));
    if (!u.empty() && !out) { g_open_err = "pfh_union_host: out is needed"; return 1; }
    std::copy(u.begin(), u.end(), out);
    *n_out = u.size();
    return 0;
}
int pfh_count_masked_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t k, const uint32_t *counters,
                          uint32_t low, uint32_t up, uint64_t *kmers_out, uint32_t *counts_out, uint64_t cap, uint64_t *n, uint64_t stats_out[6]) {
    if (n) *n = 0;
    if (!pf_count::k_ok(k)) return 1;
    pf_count::Table table;
    pf_run::Stats st;
    pf_run::count_masked_host(text, off, len, n_reads, (int)k, counters, low, up, table, st);
    uint64_t i = 0;
    for (const auto &kv : table) {
        if (i < cap) {
            if (kmers_out) kmers_out[i] = kv.first;
            if (counts_out) counts_out[i] = (uint32_t)std::min<uint64_t>(kv.second, pf_count::COUNTER_MAX);
        }
        ++i;
    }
    if (n) *n = i;
    if (stats_out) {
        const uint64_t s[6] = {st.reads, st.bases, st.kmers, st.kmers_invalid, st.kmers_bad, st.kmers_kept};
        memcpy(stats_out, s, sizeof s);
    }
    return 0;
}
int pfh_unitig_build_host(const uint64_t *kmers, uint64_t n, uint32_t k, int32_t g, int clip_tips, int del_isolated, char *text_out, uint64_t cap,
                          uint64_t *text_bytes, uint64_t stats_out[6]) {
    if (!pf_count::k_ok(k) || (n && !kmers)) return 1;
    const int gg = g == PFH_UNITIG_G_DEFAULT ? pf_unitig::default_g((int)k) : g;
    if (!pf_unitig::g_ok(gg, (int)k)) return 2;
    pf_unitig::Stats st;
    const std::string text = pf_unitig::build_host(std::vector<uint64_t>(kmers, kmers + n), (int)k, clip_tips != 0, del_isolated != 0, gg, &st);
    if (text_out) memcpy(text_out, text.data(), (size_t)std::min<uint64_t>(cap, text.size()));
    if (text_bytes) *text_bytes = text.size();
    if (stats_out) {
        const uint64_t v[6] = {st.distinct, st.unitigs, st.removed, st.unitigs_out, st.longest, st.bytes};
        memcpy(stats_out, v, sizeof v);
    }
    return 0;
}
const char *pfh_unitig_no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_kmers) {
    static thread_local std::string text;
    text = pf_unitig::no_room_text(need, free_bytes, n_kmers);
    return text.c_str();
}
int pfh_build_colored_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, int32_t g, int clip_tips, int del_isolated,
                            uint32_t n_seeds, uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *counted, pf_unitig_stats *stats,
                            pf_color_stats *colored, uint64_t *color_bytes, double times_out[6]) {
    if (!out_prefix || (n_inputs && !inputs)) { g_open_err = "pfh_build_colored_fastq: inputs and output prefix are needed"; return 1; }
    try {
        std::vector<std::string> in;
        for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
        pfh::BuildOptions opt;
        opt.fasta = take_reads_fasta();
        opt.k = k;
        opt.g = g;
        opt.clip_tips = clip_tips != 0;
        opt.del_isolated = del_isolated != 0;
        opt.chunk_bytes = chunk_bytes;
        opt.initial_slots = initial_slots;
        pf_count_stats cst = {};
        pf_unitig_stats st = {};
        pf_color_stats col = {};
        uint64_t nb = 0;
        pfh::ColoredTimes tm;
        const int rc = pfh::build_colored_fastq(in, out_prefix, opt, n_seeds, device, cst, st, col, nb, &tm, g_open_err);
        if (counted) *counted = cst;
        if (stats) *stats = st;
        if (colored) *colored = col;
        if (color_bytes) *color_bytes = nb;
        if (times_out) {
            const double v[6] = {tm.build.stream_s, tm.build.finish_s, tm.build.graph_s, tm.color_s, tm.serialise_s, tm.build.write_s};
            memcpy(times_out, v, sizeof v);
        }
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
int pfh_build_colored_host(const char *const *reads, const uint32_t *colour_of, uint64_t n_reads, uint32_t n_colors, const char *const *names, uint32_t k,
                           int32_t g, int clip_tips, int del_isolated, uint32_t n_seeds, char *gfa_out, uint64_t gfa_cap, uint64_t *gfa_bytes,
                           uint8_t *colors_out, uint64_t colors_cap, uint64_t *colors_bytes, uint64_t graph_stats[6], uint64_t color_stats[6]) {
    if (!pf_count::k_ok(k) || (n_reads && (!reads || !colour_of)) || !names || n_colors == 0) return 1;
    const int gg = g == PFH_UNITIG_G_DEFAULT ? pf_unitig::default_g((int)k) : g;
    if (!pf_unitig::g_ok(gg, (int)k)) return 2;
    if (n_seeds == 0) n_seeds = pf_color::DEFAULT_SEEDS;
    if (!pf_color::seeds_ok(n_seeds)) return 3;
    if (n_colors > pf_color::MAX_COLORS) return 4;
    std::vector<std::vector<std::string>> per(n_colors);
    for (uint64_t i = 0; i < n_reads; ++i) {
        if (colour_of[i] >= n_colors) return 1;
        per[colour_of[i]].push_back(reads[i] ? reads[i] : "");
    }
    std::vector<std::string> nm;
    for (uint32_t c = 0; c < n_colors; ++c) nm.push_back(names[c] ? names[c] : "");
    pf_color::Colored cg;
    pf_unitig::Stats gst;
    pf_color::Stats cst;
    const std::string text = pf_color::build_colored_host(per, (int)k, clip_tips != 0, del_isolated != 0, gg, n_seeds, cg, &gst, &cst);
    if (gst.longest && (uint64_t)n_colors * (gst.longest - k + 1) >= (1ull << 32)) return 4;
    std::vector<uint8_t> bytes;
    if (!pf_bfg::write(cg, (int)k, n_seeds, nm, bytes).empty()) return 1;
    if (gfa_out) memcpy(gfa_out, text.data(), (size_t)std::min<uint64_t>(gfa_cap, text.size()));
    if (gfa_bytes) *gfa_bytes = text.size();
    if (colors_out) memcpy(colors_out, bytes.data(), (size_t)std::min<uint64_t>(colors_cap, bytes.size()));
    if (colors_bytes) *colors_bytes = bytes.size();
    if (graph_stats) {
        const uint64_t v[6] = {gst.distinct, gst.unitigs, gst.removed, gst.unitigs_out, gst.longest, gst.bytes};
        memcpy(graph_stats, v, sizeof v);
    }
    if (color_stats) {
        const uint64_t v[6] = {cst.colors, cst.windows_colored, cst.windows_unplaced, cst.windows_bad, cst.runs, cst.overflow};
        memcpy(color_stats, v, sizeof v);
    }
    return 0;
}
int pfh_bfg_colors_bytes(const uint64_t *heads, const uint32_t *m, const uint32_t *slot, const uint64_t *run_off, const uint32_t *runs, uint64_t n_lines,
                         uint32_t k, uint32_t n_seeds, const char *const *names, uint32_t n_colors, uint8_t *out, uint64_t cap, uint64_t *bytes) {
    if (!run_off || !names || (n_lines && (!heads || !m || !slot)) || !pf_count::k_ok(k) || !pf_color::seeds_ok(n_seeds)) { g_open_err = "pfh_bfg_colors_bytes: arrays, k or n_seeds"; return 1; }
    pf_color::Colored cg;
    cg.lines.resize((size_t)n_lines);
    for (uint64_t j = 0; j < n_lines; ++j) {
        cg.lines[j].head = heads[j];
        cg.lines[j].m = m[j];
        cg.lines[j].slot = slot[j];
        if (slot[j] >= n_lines) cg.overflow += 1;
    }
    cg.run_off.assign(run_off, run_off + n_lines + 1);
    if (cg.run_off.back() && !runs) { g_open_err = "pfh_bfg_colors_bytes: runs is needed"; return 1; }
    for (uint64_t i = 0; i < cg.run_off.back(); ++i) cg.runs.emplace_back(runs[2 * i], runs[2 * i + 1]);
    std::vector<std::string> nm;
    for (uint32_t c = 0; c < n_colors; ++c) nm.push_back(names[c] ? names[c] : "");
    std::vector<uint8_t> b;
    const std::string why = pf_bfg::write(cg, (int)k, n_seeds, nm, b);
    if (!why.empty()) { g_open_err = "pfh_bfg_colors_bytes: " + why; return 1; }
    if (out) memcpy(out, b.data(), (size_t)std::min<uint64_t>(cap, b.size()));
    if (bytes) *bytes = b.size();
    return 0;
}
const char *pfh_color_no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_colors, uint64_t n_kmers) {
    static thread_local std::string text;
    text = pf_color::no_room_text(need, free_bytes, n_colors, n_kmers);
    return text.c_str();
}

// ---- one graph over several GPUs -------------------------------------------------------------------
int pfh_find_shard(pfh_run *r, uint32_t u0, uint32_t u1) {
    return guarded(r, [&] { return r->cdbg->find_shard(u0, u1); });
}
const pf_bfs_record *pfh_shard_records(const pfh_run *r, uint64_t *n) {
    if (n) *n = r->cdbg->shard_records().size();
    return r->cdbg->shard_records().data();
}
const uint32_t *pfh_shard_pool(const pfh_run *r, uint64_t *n) {
    if (n) *n = r->cdbg->shard_pool().size();
    return r->cdbg->shard_pool().data();
}
int pfh_find_replay(pfh_run *r, const char *outpre, uint32_t n_shards, const pf_bfs_record *const *records, const uint64_t *n_records,
                    const uint32_t *const *pools, int write_file, const uint64_t *pool_lens, const pf_bfs_record *const *dev_records,
                    const uint32_t *const *dev_pools) {
    return guarded(r, [&] { return r->cdbg->find_replay(outpre, n_shards, records, n_records, pools, write_file != 0, pool_lens, dev_records, dev_pools); });
}
void pfh_set_replay_threads(pfh_run *r, int threads) { r->cdbg->set_replay_threads(threads); }
void pfh_set_write_super_bubble(pfh_run *r, int on) { r->cdbg->set_write_super_bubble(on != 0); }
int pfh_ploidy_select(pfh_run *r, int lower, int upper, uint64_t *n_bubbles) {
    return guarded(r, [&] { uint64_t n = 0; const int rc = r->cdbg->ploidy_select(lower, upper, n); if (n_bubbles) *n_bubbles = n; return rc; });
}
int pfh_ploidy_select_colored(pfh_run *r, const int *lower, const int *upper, int n_cutoffs, uint64_t *n_bubbles) {
    return guarded(r, [&] {
        std::vector<std::pair<int, int>> cut;
        for (int c = 0; c < n_cutoffs; ++c) cut.push_back({lower[c], upper[c]});
        uint64_t n = 0;
        const int rc = r->cdbg->ploidy_select(cut, n);
        if (n_bubbles) *n_bubbles = n;
        return rc;
    });
}
int pfh_ploidy_align(pfh_run *r, uint64_t t0, uint64_t t1, uint64_t *n_called) {
    return guarded(r, [&] { uint64_t n = 0; const int rc = r->cdbg->ploidy_align(t0, t1, n); if (n_called) *n_called = n; return rc; });
}
int pfh_ploidy_text(pfh_run *r, uint64_t var_count_base, uint64_t sizes[10], uint64_t counters[8]) {
    return guarded(r, [&] { return r->cdbg->ploidy_text(var_count_base, sizes, counters); });
}
int pfh_ploidy_write(pfh_run *r, const char *outpre, const uint64_t offsets[10], const uint64_t totals[10], int truncate) {
    return guarded(r, [&] { return r->cdbg->ploidy_write(outpre, offsets, totals, truncate != 0); });
}

int pfh_filter(int argc, char **argv, int multi) { return pfh::filter_main(argc, argv, multi != 0); }

uint64_t pfh_r_format_double(double x, char *out, uint64_t cap) {
    const std::string s = pfh::r_format_double(x);
    if (out && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, s.size());
        memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return s.size();
}

uint64_t pfh_load_trace(char *out, uint64_t cap, int reset) {
    pfh::LoadLog &l = pfh::LoadLog::get();
    std::lock_guard<std::mutex> lk(l.mu);
    std::string text;
    char num[32];
    for (auto &st : l.steps) {
        snprintf(num, sizeof num, "\t%.6f\n", st.second);
        text += st.first;
        text += num;
    }
    if (out && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    if (reset) l.steps.clear();
    return text.size();
}

void pfh_get_times(const pfh_run *r, pfh_times *o) {
    memset(o, 0, sizeof(*o));
    const pfh::PhaseTimes &t = r->cdbg->times();
    o->load_s = r->load_s; o->upload_s = r->upload_s;
    o->bfs_device_s = t.bfs_device_s; o->replay_s = t.replay_s; o->bubble_write_s = t.bubble_write_s; o->find_total_s = t.find_total_s;
    o->cov_device_s = t.cov_device_s; o->tasks_s = t.tasks_s; o->align_s = t.align_s; o->sites_s = t.sites_s;
    o->format_s = t.format_s; o->write_s = t.write_s; o->ploidy_total_s = t.ploidy_total_s;
    o->unitigs = r->g().n(); o->kmers = r->g().n_kmers; o->candidates = t.candidates; o->superbubbles = r->cdbg->n_superbubbles();
    o->tasks = t.tasks; o->align_jobs = t.align_jobs; o->site_strings = t.site_strings; o->output_bytes = r->cdbg->output_bytes();
    for (int a = 0; a < 4; ++a) o->allele[a] = r->cdbg->allele_sites(a + 2);
    o->core_cov = r->cdbg->core_cov(); o->core_num = r->cdbg->core_num();
    o->scan_s = t.scan_s; o->scan_serial_s = t.scan_serial_s;
    o->bfs_large = t.bfs_large; o->bfs_max_seen = t.bfs_max_seen;
    o->bfs_deferred = t.bfs_deferred;
    o->host_commit_records = t.host_commit_records; o->host_walk_vertices = t.host_walk_vertices;
    o->snp_jobs = t.snp_jobs; o->pair_jobs = t.pair_jobs; o->wave_jobs = t.wave_jobs; o->stack_jobs = t.stack_jobs;
}

const char *pfh_last_allele_frequency(const pfh_run *r, uint64_t *len) {
    const std::string &s = r->cdbg->last_allele_frequency();
    if (len) *len = s.size();
    return s.data();
}

void pfh_state(const pfh_run *r, uint8_t *flags, uint32_t *plus, uint32_t *minus) {
    const size_t N = r->g().n();
    if (flags) memcpy(flags, r->cdbg->state_flags().data(), N);
    if (plus) memcpy(plus, r->cdbg->state_plus().data(), N * 4);
    if (minus) memcpy(minus, r->cdbg->state_minus().data(), N * 4);
}

// ---- the commit replay on a bare state (no device) ----
}  // extern "C"
struct pfh_replay {
    pfh::UnitigState st;
    uint32_t last = 0;
    bool any = false;
    // pfh_replay_apply_parallel
    bool par = false;
    pfh::SideComponents cc;
    pfh::ParallelReplay pr;
};
extern "C" {
pfh_replay *pfh_replay_open(uint32_t n_unitigs, uint32_t complex_size) {
    try {
        auto h = std::make_unique<pfh_replay>();
        h->st.reset(n_unitigs);
        h->st.complex_size = complex_size;
        return h.release();
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return nullptr;
    }
}
void pfh_replay_close(pfh_replay *h) { delete h; }
int pfh_replay_apply(pfh_replay *h, const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool) {
    if (!h || (n_records && (!records || !pool))) return 1;
    for (uint64_t i = 0; i < n_records; ++i) {
        const pf_bfs_record &r = records[i];
        if ((r.entrance >> 1) >= h->st.flags.size() || (h->any && r.entrance < h->last)) return 2;  // shards must arrive in order
        h->last = r.entrance;
        h->any = true;
        if (!h->st.gate_open(r.entrance)) continue;
        h->st.replay(r, pool + r.list_off);
    }
    return 0;
}
// The same shard through the parallel replay (pf_replay_par.hpp): components on the host, `threads` workers.  One handle takes
// either this call or pfh_replay_apply, not both.
int pfh_replay_apply_parallel(pfh_replay *h, const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t threads) {
    if (!h || (n_records && (!records || !pool))) return 1;
    if (h->any && !h->par) return 3;
    const uint32_t N = (uint32_t)h->st.flags.size();
    for (uint64_t i = 0; i < n_records; ++i) {
        const pf_bfs_record &r = records[i];
        if ((r.entrance >> 1) >= N || ((h->any || i) && r.entrance < h->last)) return 2;
        h->last = r.entrance;
    }
    if (!h->par) {
        h->par = true;
        h->cc.reset(N);
        h->pr.begin(N, h->st.plus.data(), h->st.minus.data(), h->st.complex_size, threads ? threads : 1);
    }
    h->any = true;
    auto list_of = [&](const pf_bfs_record &r) { return pool + r.list_off; };
    h->cc.add(records, n_records, list_of);
    std::vector<uint32_t> order, class_off;
    h->cc.order(records, n_records, pfh::kReplayClasses, order, class_off);
    pfh::ReplayStats st;
    h->pr.run(records, list_of, order.data(), class_off.data(), pfh::kReplayClasses, threads ? threads : 1, st);
    h->pr.finish(h->st.flags.data(), threads ? threads : 1);
    return 0;
}
uint64_t pfh_replay_check_footprints(const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t n_unitigs,
                                     uint32_t complex_size, uint64_t slice, uint64_t *first_bad) {
    return pfh::check_footprints(records, n_records, pool, n_unitigs, complex_size, slice, first_bad);
}
// component label of every record's entrance side after the records were added (test hook for the device's labels)
void pfh_side_components(const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t n_unitigs, uint32_t *labels) {
    pfh::SideComponents cc;
    cc.reset(n_unitigs);
    cc.add(records, n_records, [&](const pf_bfs_record &r) { return pool + r.list_off; });
    for (uint64_t i = 0; i < n_records; ++i) labels[i] = cc.label(pfh::entrance_side(records[i].entrance));
}
void pfh_replay_state(const pfh_replay *h, uint8_t *flags, uint32_t *plus, uint32_t *minus) {
    const size_t N = h->st.flags.size();
    if (flags) memcpy(flags, h->st.flags.data(), N);
    if (plus) memcpy(plus, h->st.plus.data(), N * 4);
    if (minus) memcpy(minus, h->st.minus.data(), N * 4);
}

// ---- colour sets (host only) ---------------------------------------------------------------------
}  // extern "C"

struct pfh_colors {
    pfh::UnitigSet graph;
    pfh::ColorSets sets;
};

extern "C" {

pfh_colors *pfh_colors_open(const char *gfa_path, const char *colors_path, uint32_t threads) {
    try {
        auto c = std::make_unique<pfh_colors>();
        if (!c->graph.load_gfa(gfa_path, g_open_err)) return nullptr;
        if (!c->sets.load(colors_path, c->graph, threads ? threads : 1, g_open_err)) return nullptr;
        return c.release();
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return nullptr;
    }
}

// the footprint check with the colored commits: colour sets of an opened (graph, colours) pair, CSR rows from the caller
uint64_t pfh_colors_check_footprints(const pfh_colors *c, const uint32_t *succ, const pf_bfs_record *records, uint64_t n_records,
                                     const uint32_t *pool, uint32_t complex_size, uint64_t slice, uint64_t *first_bad) {
    pfh::ColourGate g;
    g.n_colors = c->sets.n_colors;
    g.k = c->graph.k;
    g.len_bp = c->graph.len_bp.data();
    g.words = c->sets.words;
    g.full_mask = c->sets.full_mask.data();
    g.size_total = c->sets.size_total.data();
    g.n_full_enc = c->sets.n_full_enc.data();
    g.succ = succ;
    return pfh::check_footprints(records, n_records, pool, c->graph.n(), complex_size, slice, first_bad, &g);
}
void pfh_colors_close(pfh_colors *c) { delete c; }
uint32_t pfh_colors_count(const pfh_colors *c) { return c->sets.n_colors; }
uint32_t pfh_colors_unitigs(const pfh_colors *c) { return c->graph.n(); }
const char *pfh_colors_name(const pfh_colors *c, uint32_t colour) {
    return colour < c->sets.names.size() ? c->sets.names[colour].c_str() : "";
}
uint64_t pfh_colors_unitig(const pfh_colors *c, uint32_t u, uint8_t *presence, uint32_t *n_kmers, uint32_t *n_full_enc) {
    const uint32_t km = c->graph.len_km(u);
    if (n_kmers) *n_kmers = km;
    if (n_full_enc) *n_full_enc = c->sets.n_full_enc[u];
    if (presence)
        for (uint32_t ci = 0; ci < c->sets.n_colors; ++ci)
            for (uint32_t i = 0; i < km; ++i) presence[(size_t)ci * km + i] = c->sets.contains(u, ci, i, 1);
    return c->sets.size_total[u];
}
uint64_t pfh_gfa_abundant_kmers(const char *gfa_path) {
    try {
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err)) return ~0ull;
        return g.n_abundant;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return ~0ull;
    }
}
uint32_t pfh_gfa_numbering_replays(const char *gfa_path) {
    try {
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err)) return ~0u;
        return g.numbering_replays;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return ~0u;
    }
}
// (the walkers of the two test hooks below: the pool the product's paths walk through, pf_bfs_host.hpp)
static pfh::WalkerPool g_walkers;
int pfh_host_walk(const uint32_t *succ, const uint32_t *pred, uint32_t n_unitigs, uint32_t entrance, pf_bfs_record *record, uint32_t *list,
                  uint64_t list_cap) {
    if (!succ || !pred || !record || n_unitigs == 0 || (entrance >> 1) >= n_unitigs) return 1;
    try {
        static thread_local std::vector<uint32_t> l;
        g_walkers.walk(succ, pred, n_unitigs, entrance, *record, l);
        if (record->n_list > list_cap) return 2;
        if (list) std::copy(l.begin(), l.end(), list);
        return 0;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
uint64_t pfh_host_walk_range(const uint32_t *succ, const uint32_t *pred, uint32_t n_unitigs, uint32_t u0, uint32_t u1,
                             pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool, uint64_t pool_cap, uint64_t *pool_used) {
    if (!succ || !pred || u0 > u1 || u1 > n_unitigs) return ~0ull;
    try {
        std::vector<uint32_t> l;
        uint64_t n = 0, used = 0;
        bool fits = true;
        for (uint32_t ov = 2 * u0; ov < 2 * u1; ++ov) {
            int deg = 0;
            for (int b = 0; b < 4; ++b) deg += succ[(size_t)ov * 4 + b] != 0xFFFFFFFFu;
            if (deg < 2) continue;
            pf_bfs_record r;
            g_walkers.walk(succ, pred, n_unitigs, ov, r, l);
            r.list_off = used;
            if (n < rec_cap && used + r.n_list <= pool_cap && records && pool) {
                records[n] = r;
                std::copy(l.begin(), l.end(), pool + used);
            } else {
                fits = false;
            }
            ++n;
            used += r.n_list;
        }
        if (pool_used) *pool_used = used;
        return fits ? n : ~0ull;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return ~0ull;
    }
}
uint64_t pfh_gfa_minimizer_counts(const char *gfa_path, uint8_t *counters, uint64_t slots) {
    try {
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err, true)) return ~0ull;
        std::vector<uint8_t> c;
        g.finish_numbering(&c);
        if (counters && slots >= c.size()) std::copy(c.begin(), c.end(), counters);
        return c.size();
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return ~0ull;
    }
}
int pfh_gfa_write_unitig_ids(const char *gfa_path, const char *out_path) {
    try {
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err)) return 1;
        FILE *f = fopen(out_path, "w");
        if (!f) { g_open_err = std::string("cannot write ") + out_path; return 1; }
        for (uint32_t u = 0; u < g.n(); ++u) {
            const std::string_view s = g.seq(u);
            fprintf(f, "%u\t%.*s\n", u + 1, (int)s.size(), s.data());
        }
        fclose(f);
        return 0;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
// The numbering with the replay's inputs handed in, as the device layer hands them over (pf_minimizer_replay_inputs): `bump` is added to
// every counter of the host's own pass (saturating: upper bounds, as K-MINZ's are) and every unitig is flagged.  Must write the same
// file as pfh_gfa_write_unitig_ids.  [tests]
int pfh_gfa_write_unitig_ids_given_inputs(const char *gfa_path, const char *out_path, int bump) {
    try {
        std::vector<uint8_t> c;
        {
            pfh::UnitigSet probe;
            if (!probe.load_gfa(gfa_path, g_open_err, true)) return 1;
            probe.finish_numbering(&c);
        }
        for (uint8_t &x : c) x = (uint8_t)std::min<int>(255, (int)x + bump);
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err, true)) return 1;
        const std::vector<uint8_t> flags(g.n(), 1);
        g.finish_numbering(nullptr, c.empty() ? nullptr : c.data(), c.empty() ? nullptr : flags.data(), c.size());
        FILE *f = fopen(out_path, "w");
        if (!f) { g_open_err = std::string("cannot write ") + out_path; return 1; }
        for (uint32_t u = 0; u < g.n(); ++u) {
            const std::string_view s = g.seq(u);
            fprintf(f, "%u\t%.*s\n", u + 1, (int)s.size(), s.data());
        }
        fclose(f);
        return 0;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
// The numbering with the two arrays of pf_minimizer_replay_inputs themselves handed in: the counter table and one flag per unitig in
// the loader's order before the move (long unitigs in file order, then the k-length ones).  Arrays of another geometry are refused,
// never ignored: the replay must run from exactly what it was given.  [tests]
int pfh_gfa_write_unitig_ids_given_arrays(const char *gfa_path, const char *out_path, const uint8_t *counters8, uint64_t n_slots,
                                          const uint8_t *flags, uint64_t n_flags) {
    try {
        if (!counters8 || !flags) { g_open_err = "pfh_gfa_write_unitig_ids_given_arrays: counters8 and flags are both needed"; return 1; }
        pfh::UnitigSet g;
        if (!g.load_gfa(gfa_path, g_open_err, true)) return 1;
        uint64_t n_kmers = 0;
        for (uint32_t u = 0; u < g.n(); ++u) n_kmers += g.len_km(u);
        const uint64_t slots = pfh::minimizer_table_slots(n_kmers);
        if (n_slots != slots) {
            g_open_err = "pfh_gfa_write_unitig_ids_given_arrays: " + std::to_string(n_slots) + " counters handed in, the table of this graph has " + std::to_string(slots);
            return 2;
        }
        if (n_flags != g.n()) {
            g_open_err = "pfh_gfa_write_unitig_ids_given_arrays: " + std::to_string(n_flags) + " flags handed in, the graph has " + std::to_string(g.n()) + " unitigs";
            return 2;
        }
        g.finish_numbering(nullptr, counters8, flags, n_slots);
        FILE *f = fopen(out_path, "w");
        if (!f) { g_open_err = std::string("cannot write ") + out_path; return 1; }
        for (uint32_t u = 0; u < g.n(); ++u) {
            const std::string_view s = g.seq(u);
            fprintf(f, "%u\t%.*s\n", u + 1, (int)s.size(), s.data());
        }
        fclose(f);
        return 0;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}
// ---- `PloidyFrost model` ---------------------------------------------------------------------------------------------
pfh_gmm *pfh_gmm_open(int device) {
    try {
        return new pfh_gmm(device);
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return nullptr;
    }
}
void pfh_gmm_close(pfh_gmm *m) { delete m; }
const char *pfh_gmm_last_error(const pfh_gmm *m) { return m ? (m->err.empty() ? m->model.error().c_str() : m->err.c_str()) : g_open_err.c_str(); }
int pfh_gmm_read_fre(pfh_gmm *m, const char *file, double min_frequency) {
    return gmm_guard(m, [&] { return m->model.readFreFile(file, min_frequency); });
}
int pfh_gmm_read_cov(pfh_gmm *m, const char *prefix, double min_frequency) {
    return gmm_guard(m, [&] { return m->model.readCovFile(prefix, min_frequency); });
}
int pfh_gmm_set_values(pfh_gmm *m, const double *values, uint64_t n) {
    return gmm_guard(m, [&] { m->model.readData(std::vector<double>(values, values + n)); return 0; });
}
uint64_t pfh_gmm_size(const pfh_gmm *m) { return m ? m->model.values().size() : 0; }
int pfh_gmm_values(const pfh_gmm *m, double *out) {
    if (!m || !out) return 1;
    std::copy(m->model.values().begin(), m->model.values().end(), out);
    return 0;
}
int pfh_gmm_fit(pfh_gmm *m, uint32_t gauss, double m_thre, double n_thre, int32_t max_iter, double max_delta, double *weights,
                double *means, double *vars, double *loglik, double *aic, uint32_t *iterations) {
    return gmm_guard(m, [&] {
        m->model.setMThreshold(m_thre);
        m->model.setNThreshold(n_thre);
        m->model.setMaxIterNum(max_iter);
        m->model.setMaxDeltaNum(max_delta);
        m->model.resize(gauss);
        if (m->model.emIterate()) return 1;
        for (uint32_t i = 0; i < gauss; ++i) {
            if (weights) weights[i] = m->model.getWeights()[i];
            if (means) means[i] = m->model.getMeans()[i];
            if (vars) vars[i] = m->model.getVars()[i];
        }
        if (loglik) *loglik = m->model.getLogLikelihood();
        if (aic) *aic = m->model.getAIC();
        if (iterations) *iterations = m->model.iterations();
        return 0;
    });
}
int pfh_gmm_run(pfh_gmm *m, int min_gauss, int max_gauss, double m_thre, double n_thre, int32_t max_iter, double max_delta,
                const char *outprefix) {
    return gmm_guard(m, [&] {
        m->model.setMThreshold(m_thre);
        m->model.setNThreshold(n_thre);
        m->model.setMaxIterNum(max_iter);
        m->model.setMaxDeltaNum(max_delta);
        return pfh::run_model(m->model, min_gauss, max_gauss, outprefix, m->err);
    });
}
int pfh_gmm_read_column(pfh_gmm *m, const char *file) {
    return gmm_guard(m, [&] { return m->model.readColumn(file); });
}
int pfh_gmm_density(pfh_gmm *m, uint32_t points, double adjust, double *x, double *density, pf_density_info *info) {
    return gmm_guard(m, [&] {
        if (!x || !density || !info) { m->err = "pfh_gmm_density: x, density and info are needed"; return 1; }
        pfh::Density d;
        if (m->model.density(points, adjust, d)) return 1;
        std::copy(d.x.begin(), d.x.end(), x);
        std::copy(d.density.begin(), d.density.end(), density);
        *info = d.info;
        return 0;
    });
}
int pfh_gmm_write_density(pfh_gmm *m, const char *outprefix, const pf_density_info *info, uint32_t points, const double *x, const double *density) {
    return gmm_guard(m, [&] {
        if (!outprefix || !info || !x || !density) { m->err = "pfh_gmm_write_density: prefix, info, x and density are needed"; return 1; }
        pfh::Density d;
        d.x.assign(x, x + points);
        d.density.assign(density, density + points);
        d.info = *info;
        return pfh::write_density(outprefix, d, m->err);
    });
}
int pfh_gmm_kernel_time(pfh_gmm *m, int enable, double *total_ms, uint64_t *launches) {
    if (!m) return 1;
    pf_ctx *ctx = m->model.device_context();
    if (!ctx) return 1;
    if (enable >= 0) return pf_enable_timing(ctx, enable);
    return pf_kernel_time(ctx, PF_K_GMM, total_ms, launches);
}
int pfh_gmm_density_time(pfh_gmm *m, double *total_ms, uint64_t *launches) {
    if (!m) return 1;
    pf_ctx *ctx = m->model.device_context();
    if (!ctx) return 1;
    return pf_kernel_time(ctx, PF_K_DENSITY, total_ms, launches);
}

// ---- the model in the same run ---------------------------------------------------------------------------------------
int pfh_set_model(pfh_run *r, int source, double min_frequency, int lo, int hi, double m_thre, double n_thre, int32_t max_iter,
                  double max_delta, int only) {
    return guarded(r, [&] {
        pfh::CDBG::ModelOptions o;
        o.on = source >= 0;
        o.only = only != 0;
        o.source = source;
        o.q = min_frequency;
        o.lo = lo; o.hi = hi;
        o.m_thre = m_thre; o.n_thre = n_thre; o.max_iter = max_iter; o.max_delta = max_delta;
        return r->cdbg->set_model(o);
    });
}
int pfh_set_density(pfh_run *r, uint32_t points, double adjust) {
    return guarded(r, [&] { return r->cdbg->set_density(points, adjust); });
}
static int density_out(const pfh::Density *d, double *x, double *density, pf_density_info *info) {
    if (!d) return 1;
    if (x) std::copy(d->x.begin(), d->x.end(), x);
    if (density) std::copy(d->density.begin(), d->density.end(), density);
    if (info) *info = d->info;
    return 0;
}
uint32_t pfh_model_density_points(const pfh_run *r, int color) {
    if (color < 0) return r->cdbg->model_density() ? (uint32_t)r->cdbg->model_density()->x.size() : 0;
    for (const pfh::CDBG::ColorFit &cf : r->cdbg->model_color_fits())
        if (cf.color == color) return cf.has_density ? (uint32_t)cf.density.x.size() : 0;
    return 0;
}
int pfh_model_density(const pfh_run *r, double *x, double *density, pf_density_info *info) {
    return density_out(r->cdbg->model_density(), x, density, info);
}
int pfh_model_color_density(const pfh_run *r, int color, double *x, double *density, pf_density_info *info) {
    for (const pfh::CDBG::ColorFit &cf : r->cdbg->model_color_fits())
        if (cf.color == color) return density_out(cf.has_density ? &cf.density : nullptr, x, density, info);
    return 1;
}
uint64_t pfh_model_values(pfh_run *r, double *out, uint64_t cap) {
    const uint64_t n = r->cdbg->model_count();
    if (r->cdbg->model_was_each_color()) {   // the last pass was split by colour: the device array is the last colour's by now; the pooled one was copied
        const std::vector<double> &v = r->cdbg->model_pooled_values();
        if (out) std::copy(v.begin(), v.begin() + (size_t)std::min<uint64_t>(cap, v.size()), out);
        return v.size();
    }
    if (out && cap && n && pf_gmm_values(r->cdbg->device(), out, cap) != PF_OK) return 0;
    return n;
}
int pfh_model_fit(const pfh_run *r, uint32_t gauss, double *weights, double *means, double *vars, double *loglik, double *aic,
                  uint32_t *iterations) {
    for (const pfh::GmmModel::Fit &f : r->cdbg->model_fits()) {
        if (f.gauss != gauss) continue;
        for (uint32_t i = 0; i < gauss; ++i) {
            if (weights) weights[i] = f.weights[i];
            if (means) means[i] = f.means[i];
            if (vars) vars[i] = f.vars[i];
        }
        if (loglik) *loglik = f.loglik;
        if (aic) *aic = f.aic;
        if (iterations) *iterations = f.iterations;
        return 0;
    }
    return 1;
}
double pfh_model_ploidy(const pfh_run *r) { return r->cdbg->model_ploidy(); }
uint64_t pfh_text_bytes_fetched(const pfh_run *r) { return r->cdbg->text_bytes_fetched(); }

// the device kernels' steps over one stream, in order, on the host: rows end at line feeds (a last row without one ends with the
// text), the row rule, and for the frequencies readFreFile's last turn
int pfh_model_rows(int source, double min_frequency, const char *const *text, const uint64_t *len, double *out, uint64_t cap,
                   uint64_t *n, char *err, uint64_t err_cap) {
    if ((source != pf::MODEL_COV && source != pf::MODEL_FRE) || !text || !len || !n) return 1;
    static const char *name[2][3] = {{"_bicov", "_tricov", "_tetracov"}, {"_allele_frequency", "", ""}};
    uint64_t count = 0;
    auto put = [&](double v) { if (out && count < cap) out[count] = v; ++count; };
    auto say = [&](int code, int ord, uint64_t row) {
        const std::string where = "row " + std::to_string(row + 1) + " of stream " + name[source][ord];
        const std::string m = code == pf::MODEL_ROW_COV_ZERO ? "Model::readCovFile() : " + where + " sums to 0 (the reference divides by it)"
                            : code == pf::MODEL_ROW_BAD_TOKEN ? "ERROR: " + where + " holds something that is not a number"
                                                              : "ERROR: " + where + " holds a number outside what the device converts exactly (more than 15 digits or a decimal exponent beyond 22)";
        if (err && err_cap) { strncpy(err, m.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    };
    const int n_ord = source == pf::MODEL_COV ? 3 : 1;
    for (int ord = 0; ord < n_ord; ++ord) {
        const char *s = text[ord];
        const uint64_t L = len[ord];
        if (L >= 0xFFFFFFF0ull) return 1;
        double last = 0;
        bool have_last = false;
        uint64_t row = 0;
        for (uint64_t start = 0; start < L; ++row) {
            uint64_t end = start;
            while (end < L && s[end] != '\n') ++end;
            double v[4];
            int code = pf::MODEL_ROW_OK;
            const int k = source == pf::MODEL_COV ? pf::model_cov_row(s + start, (uint32_t)(end - start), ord + 2, min_frequency, v, &code)
                                                  : pf::model_fre_row(s + start, (uint32_t)(end - start), min_frequency, v, &code);
            if (code != pf::MODEL_ROW_OK) return say(code, ord, row);
            for (int i = 0; i < k; ++i) put(v[i]);
            if (source == pf::MODEL_FRE) { last = v[0]; have_last = true; }
            start = end + 1;
        }
        if (source == pf::MODEL_FRE && have_last && L && s[L - 1] == '\n' && pf::model_fre_keep(last, min_frequency)) put(last);
    }
    *n = count;
    return 0;
}

int pfh_set_filter(pfh_run *r, const pf_filter_opts *opts) {
    return guarded(r, [&] { return r->cdbg->set_filter(opts); });
}

// the filtered collection's steps on the host, in its order: every row of the four tables read (what the filter refuses while it
// reads comes first), R's error when no table keeps a row, then what the model says of the kept rows, then the array
}  // extern "C"

template <typename Opts>
static pf::FilterRule filter_rule_of(const Opts *o) {
    pf::FilterRule f = {};
    f.simple = o->simple != 0; f.indel = o->indel != 0; f.snp = o->snp != 0;
    f.low = (double)o->low; f.up = (double)o->up; f.num = (double)o->num; f.distance = (double)o->distance; f.size = (double)o->size;
    f.fq = o->frequency;
    return f;
}

static int filter_rows_by_rule(int source, double min_frequency, const pf::FilterRule &f, const char *const *text, const uint64_t *len, double *out,
                               uint64_t cap, uint64_t *n, char *err, uint64_t err_cap) {
    if ((source != pf::MODEL_COV && source != pf::MODEL_FRE) || !text || !len || !n) return 1;
    auto say = [&](const std::string &m) {
        if (err && err_cap) { strncpy(err, m.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    };
    if (!(f.fq <= 0.5)) return say("frequency should < 0.5 ");
    std::vector<double> col[pf::FILTER_COLUMNS];
    bool kept_any = false;
    std::string late;
    for (int t = 0; t < pf::FILTER_TABLES; ++t) {
        const char *s = text[t];
        const uint64_t L = len[t];
        if (L >= 0xFFFFFFF0ull) return 1;
        const int A = t + 2, base = pf::filter_column_base(t);
        uint64_t row = 0;
        for (uint64_t start = 0; start < L; ++row) {
            uint64_t end = start;
            while (end < L && s[end] != '\n') ++end;
            double v[5];
            int code = pf::MODEL_ROW_OK;
            bool kept = false;
            if (source == pf::MODEL_COV) {
                const int k = pf::filter_cov_row(s + start, (uint32_t)(end - start), A, f, min_frequency, v, &kept, &code);
                for (int i = 0; i < k; ++i) col[t].push_back(v[i]);
            } else {
                const uint32_t mask = pf::filter_fre_row(s + start, (uint32_t)(end - start), A, f, v, &kept, &code);
                for (int c = 0; c < A; ++c)
                    if ((mask >> c) & 1u) col[base + c].push_back(v[c]);
            }
            kept_any = kept_any || kept;
            if (code != pf::MODEL_ROW_OK) {
                if (!pf::filter_err_is_late(code)) return say(pf::filter_error_text(code, t, row + 1, f.multi != 0));
                if (late.empty()) late = pf::filter_error_text(code, t, row + 1, f.multi != 0);
            }
            start = end + 1;
        }
    }
    if (!kept_any) return say(pf::filter_none_kept_text());
    if (!late.empty()) return say(late);
    uint64_t count = 0;
    auto put = [&](double v) { if (out && count < cap) out[count] = v; ++count; };
    if (source == pf::MODEL_COV) {
        for (int t = 0; t < 3; ++t)
            for (double v : col[t]) put(v);
    } else {
        double last = 0;
        bool have = false;
        for (const std::vector<double> &c : col)
            for (double v : c) {
                if (pf::model_fre_keep(v, min_frequency)) put(v);
                last = v; have = true;
            }
        if (have && pf::model_fre_keep(last, min_frequency)) put(last);   // the file ends in a line feed: its last token counts twice
    }
    *n = count;
    return 0;
}

extern "C" {

int pfh_filter_rows(int source, double min_frequency, const pf_filter_opts *o, const char *const *text, const uint64_t *len, double *out,
                    uint64_t cap, uint64_t *n, char *err, uint64_t err_cap) {
    if (!o) return 1;
    return filter_rows_by_rule(source, min_frequency, filter_rule_of(o), text, len, out, cap, n, err, err_cap);
}

// ---- the multi form: the colored tables behind filter-multi's predicates ----
int pfh_filter_rows_multi(int source, double min_frequency, const pf_filter_multi_opts *o, const char *const *text, const uint64_t *len,
                          double *out, uint64_t cap, uint64_t *n, char *err, uint64_t err_cap) {
    if (!o) return 1;
    pf::FilterRule f = filter_rule_of(o);
    f.multi = 1;
    f.cramer = o->cramer;
    f.color = o->color >= 0 ? (double)o->color : -1.0;
    return filter_rows_by_rule(source, min_frequency, f, text, len, out, cap, n, err, err_cap);
}

int pfh_set_filter_multi(pfh_run *r, const pf_filter_multi_opts *opts, int each_color) {
    return guarded(r, [&] { return r->cdbg->set_filter_multi(opts, each_color != 0); });
}

static const pfh::CDBG::ColorFit *color_fit_of(const pfh_run *r, int color) {
    for (const pfh::CDBG::ColorFit &cf : r->cdbg->model_color_fits())
        if (cf.color == color) return &cf;
    return nullptr;
}
uint32_t pfh_model_color_count(const pfh_run *r) { return (uint32_t)r->cdbg->model_color_fits().size(); }
int pfh_model_color_at(const pfh_run *r, uint32_t i) {
    const auto &v = r->cdbg->model_color_fits();
    return i < v.size() ? v[i].color : -1;
}
uint64_t pfh_model_color_values(const pfh_run *r, int color, double *out, uint64_t cap) {
    const pfh::CDBG::ColorFit *cf = color_fit_of(r, color);
    if (!cf) return ~0ull;
    if (out) std::copy(cf->values.begin(), cf->values.begin() + (size_t)std::min<uint64_t>(cap, cf->values.size()), out);
    return cf->values.size();
}
int pfh_model_color_fit(const pfh_run *r, int color, uint32_t gauss, double *weights, double *means, double *vars, double *loglik, double *aic,
                        uint32_t *iterations) {
    const pfh::CDBG::ColorFit *cf = color_fit_of(r, color);
    if (!cf) return 1;
    for (const pfh::GmmModel::Fit &f : cf->fits) {
        if (f.gauss != gauss) continue;
        for (uint32_t i = 0; i < gauss; ++i) {
            if (weights) weights[i] = f.weights[i];
            if (means) means[i] = f.means[i];
            if (vars) vars[i] = f.vars[i];
        }
        if (loglik) *loglik = f.loglik;
        if (aic) *aic = f.aic;
        if (iterations) *iterations = f.iterations;
        return 0;
    }
    return 1;
}
double pfh_model_color_ploidy(const pfh_run *r, int color) {
    const pfh::CDBG::ColorFit *cf = color_fit_of(r, color);
    return cf ? cf->ploidy : 0;
}

// ---- blocked gzip: the rule without a device ----------------------------------------------------------
int pfh_inflate_parse_member(const uint8_t *bytes, uint64_t n, uint32_t fields[4]) {
    pf_inflate::Header h;
    const int c = pf_inflate::parse_member(bytes, n, &h);
    if (fields) { fields[0] = h.payload_off; fields[1] = h.member_len; fields[2] = h.crc; fields[3] = h.isize; }
    return c;
}
int pfh_inflate_member(const uint8_t *payload, uint32_t n_in, uint8_t *out, uint32_t isize, uint32_t *produced, uint32_t blocks[3]) {
    int c = 0;
    pf_inflate::Blocks b;
    uint32_t made = 0;
    pf_inflate::inflate_member(payload, n_in, out, isize, &c, &b, &made);
    if (produced) *produced = made;
    if (blocks) { blocks[0] = b.stored; blocks[1] = b.fixed; blocks[2] = b.dynamic; }
    return c;
}
int pfh_inflate_bgzf_member(const uint8_t *bytes, uint64_t n, uint8_t *out, uint32_t *out_len, uint32_t blocks[3]) {
    pf_inflate::Blocks b{0, 0, 0};
    const int c = pf_inflate::inflate_bgzf_member(bytes, n, out, out_len, &b);
    if (blocks) { blocks[0] = b.stored; blocks[1] = b.fixed; blocks[2] = b.dynamic; }
    return c;
}
uint32_t pfh_inflate_crc32(const uint8_t *bytes, uint64_t n) { return pf_inflate::crc32(bytes, n); }
uint32_t pfh_inflate_crc32_sliced(const uint8_t *bytes, uint32_t n, uint32_t n_lanes) { return pf_inflate::crc32_sliced(bytes, n, n_lanes ? n_lanes : 1); }
int pfh_inflate_file_clause(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause) {
    return pf_inflate::file_clause_gz(first, n_first, file_size, clause);
}
const char *pfh_inflate_clause_text(int clause) { return pf_inflate::clause_text(clause); }

// ---- blocked-gzip output: the rule without a device ----------------------------------------------------
int64_t pfh_deflate_member(const uint8_t *text, uint32_t n, uint8_t *out, uint64_t out_cap, uint32_t result[3]) {
    if (n > pf_deflate::MEMBER_TEXT || out_cap < (uint64_t)n + pf_deflate::MEMBER_EXTRA || !out || (n && !text)) return -1;
    std::unique_ptr<pf_deflate::HostWork> w(new pf_deflate::HostWork);
    pf_deflate::Result r;
    const uint32_t size = pf_deflate::deflate_member(text, n, out, *w, &r);
    if (result) { result[0] = r.kind; result[1] = r.literals; result[2] = r.matches; }
    return (int64_t)size;
}
uint64_t pfh_deflate_bound(uint64_t n_bytes, uint32_t member_text) { return member_text ? pf_deflate::bound(n_bytes, member_text) : 0; }

// ---- plain gzip: the rule without a device ------------------------------------------------------------
static void gunzip_stats_out(const pf_gunzip::Stats &st, uint64_t stats[9]) {
    if (!stats) return;
    const uint64_t v[9] = {st.pieces_found, st.pieces_live, st.pieces_dead, st.markers, st.blocks_stored, st.blocks_fixed, st.blocks_dynamic, st.bytes_in, st.bytes_out};
    for (int i = 0; i < 9; ++i) stats[i] = v[i];
}
int pfh_gunzip_header(const uint8_t *bytes, uint64_t n, uint64_t *len) { return pf_gunzip::gzip_header(bytes, n, len); }
int pfh_gunzip_file_kind(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause) { return pf_gunzip::file_kind(first, n_first, file_size, clause); }
int pfh_gunzip_candidate(const uint8_t *bytes, uint64_t n, uint64_t bit) { return pf_gunzip::block_candidate(bytes, n, bit) ? 1 : 0; }
int pfh_gunzip_call(const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window, uint32_t piece_bytes,
                    uint8_t *out, uint64_t out_cap, uint8_t *new_window, pf_gunzip_result *res, uint64_t stats[9]) {
    if (!res || n_bytes > 0x7fffffffull || start_bit > n_bytes * 8 || n_window > pf_gunzip::RING) return -2;
    std::vector<uint8_t> text, win(pf_gunzip::RING);
    pf_gunzip::Call r;
    pf_gunzip::Stats st;
    pf_gunzip::inflate_call(comp, n_bytes, start_bit, window, n_window, piece_bytes, text, win.data(), r, &st);
    *res = pf_gunzip_result{r.out_bytes, r.end_bit, r.final, r.clause ? n_window : r.n_window, r.crc_raw, r.clause, r.clause_bit};
    gunzip_stats_out(st, stats);
    if (r.clause) return 0;
    if (text.size() > out_cap) { res->out_bytes = text.size(); return -1; }
    if (!text.empty()) memcpy(out, text.data(), text.size());
    if (new_window && r.n_window) memcpy(new_window, win.data(), r.n_window);
    return 0;
}
int pfh_gunzip_file(const uint8_t *bytes, uint64_t n, uint32_t piece_bytes, uint64_t block_bytes, uint64_t carry_max, uint8_t *out, uint64_t out_cap,
                    uint64_t *out_len, uint64_t *member, uint64_t *byte, uint64_t stats[9]) {
    std::vector<uint8_t> text;
    pf_gunzip::Stats st;
    const int c = pf_gunzip::gunzip_file(bytes, n, piece_bytes, block_bytes, text, member, byte, &st, carry_max ? carry_max : pf_gunzip::CARRY_MAX);
    gunzip_stats_out(st, stats);
    if (out_len) *out_len = text.size();
    if (!c && text.size() <= out_cap && !text.empty()) memcpy(out, text.data(), text.size());
    return c;
}
const char *pfh_gunzip_clause_text(int clause) { return pf_gunzip::clause_text(clause); }

// ---- heterozygous k-mer pairs (K-HETPAIR, `smudge`) ----------------------------------------------------
int pfh_hetpairs_host(const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lo, uint32_t hi, uint64_t *table, uint64_t *pair_x,
                      uint64_t *pair_y, uint32_t *cov_x, uint32_t *cov_y, uint64_t cap, uint64_t *n_pairs, pf_hetpair_stats *stats) {
    if (n_pairs) *n_pairs = 0;
    const int clause = pf_hetpair::arg_clause((int64_t)k, lo, hi);
    if (clause) { g_open_err = std::string("pfh_hetpairs_host: ") + pf_hetpair::arg_text(clause); return clause; }
    if (n && (!kmers || !counts)) { g_open_err = "pfh_hetpairs_host: kmers and counts are needed"; return -1; }
    pf_hetpair::Pairs pairs;
    pf_hetpair::Stats st;
    pf_hetpair::hetpairs_host(kmers, counts, n, (int)k, lo, hi, table, pairs, st);
    if (stats) *stats = pf_hetpair_stats{st.kmers, st.in_range, st.one_partner, st.many_partners, st.pairs};
    if (n_pairs) *n_pairs = pairs.x.size();
    const size_t m = (size_t)std::min<uint64_t>(cap, pairs.x.size());
    if (pair_x && m) memcpy(pair_x, pairs.x.data(), m * 8);
    if (pair_y && m) memcpy(pair_y, pairs.y.data(), m * 8);
    if (cov_x && m) memcpy(cov_x, pairs.cov_x.data(), m * 4);
    if (cov_y && m) memcpy(cov_y, pairs.cov_y.data(), m * 4);
    return 0;
}
int pfh_smudge_report_text(const uint64_t *table, const pf_hetpair_stats *stats, uint32_t k, uint32_t lo, uint32_t hi, uint64_t n, char *out, uint64_t cap,
                           uint64_t *len) {
    if (!table || !stats || !len) { g_open_err = "pfh_smudge_report_text: table, stats and len are needed"; return -1; }
    const int clause = pf_hetpair::arg_clause((int64_t)k, lo, hi);
    if (clause) { g_open_err = std::string("pfh_smudge_report_text: ") + pf_hetpair::arg_text(clause); return clause; }
    const std::string t = pfh::smudge_report(table, *stats, k, lo, hi, n);
    *len = t.size();
    if (out) memcpy(out, t.data(), std::min<uint64_t>(cap, t.size()));
    return 0;
}
int pfh_smudge_of(uint64_t a, uint64_t b, uint64_t n, uint32_t *p, uint32_t *m) {
    if (!p || !m || a < 1 || b < a || n < 1) { g_open_err = "pfh_smudge_of: 1 <= a <= b and n >= 1"; return -1; }
    const pf_hetpair::Smudge s = pf_hetpair::smudge_of(a, b, n);
    *p = s.p;
    *m = s.m;
    return 0;
}
int pfh_smudge(const char *db_prefix, const char *const *inputs, uint32_t n_inputs, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs, uint32_t lo, uint32_t hi,
               int auto_cutoffs, double quantile, uint64_t n_hap, const char *pairs_path, const char *out, uint64_t chunk_bytes, uint64_t initial_slots,
               int device, pfh_smudge_result *result) {
    const int gz = take_reads_gz();
    const bool fasta = take_reads_fasta();
    if (!out || (n_inputs && !inputs)) { g_open_err = "pfh_smudge: inputs and output are needed"; return 1; }
    if ((db_prefix != nullptr) == (n_inputs != 0)) { g_open_err = "smudge: either a database or inputs to count are given"; return 1; }
    try {
        pfh::SmudgeOptions opt;
        opt.lo = lo;
        opt.hi = hi;
        opt.auto_cutoffs = auto_cutoffs != 0;
        opt.quantile = quantile;
        opt.n = n_hap;
        opt.pairs = pairs_path ? pairs_path : "";
        pfh::SmudgeResult res;
        int rc;
        if (db_prefix) {
            rc = pfh::smudge_db(db_prefix, opt, out, device, res, g_open_err);
        } else {
            std::vector<std::string> in;
            for (uint32_t i = 0; i < n_inputs; ++i) in.push_back(inputs[i] ? inputs[i] : "");
            pfh::CountOptions c = count_options(k, ci, cx, cs, 1);
            c.chunk_bytes = chunk_bytes;
            c.initial_slots = initial_slots;
            c.gz = gz;
            c.fasta = fasta;
            rc = pfh::smudge_counted(c, in, opt, out, device, res, g_open_err);
        }
        smudge_result_c(res, result);
        return rc;
    } catch (const std::exception &e) {
        g_open_err = std::string("ploidyfrost host layer: ") + e.what();
        return 1;
    }
}

uint64_t pfh_bifrost_kmer_hash(uint64_t left_aligned_kmer, uint64_t seed) { return pfh::bifrost_kmer_hash(left_aligned_kmer, seed); }

}  // extern "C"
