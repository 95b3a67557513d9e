// K-TRIMCOUNT: step `1.trim` of the reference's workflow folded into the two passes of `ploidyfrost run` -- one chunk of raw FASTQ, or
// one chunk of each file of a pair, trimmed and counted in one call without the trimmed text.  The rule is pf_trimrun_rule.hpp; this
// file is its device form.  One call, on the text staged once:
//
//   index      fastq_index of pf_reads_dev.hpp, asked for the extents of all four lines of a record (K-TRIM's).
//   intervals  k_trim_intervals of pf_trim_dev.hpp, the kernel of K-TRIM itself: (begin, len) per record, len 0 = dropped.
//              With a clip open, K-CLIP (pf_clip.hip) runs first and the interval starts as [0, clip end).
//              With a report open, K-QC (pf_qc.hip) follows and adds both stages to its tables.
//   table      k_trimcount_keep, one thread a record: (begin, len) of file 1 (and of file 2), the hand-on predicate
//              (pf_trimrun::handed_on: kept, and for a pair kept in both files), a keep flag of 4 bytes, the pair statistics.  One
//              exclusive scan of the flags (pf_scan.hpp).  k_trimcount_scatter, one thread a record: (seq_begin + b, e - b) per file to
//              the flag's place -- the reads table as pf_count_reads / pf_maskcount_reads take it, ascending, no overlaps.
//   count      count_core (pf_count.hip) or maskcount_core (pf_maskcount.hip) over that table: classes, (flag,) insert, unchanged.  A
//              pair runs the core once per file, each over its own text and table, into the same counters.
//   traffic    per record, beside K-TRIM's intervals (the quality line read once, 8 bytes written) and the core's own: 4 bytes of flag
//              written and read twice (scan, scatter), 4 bytes of scan result, 8 (a pair: 16) bytes of (begin, len) read twice,
//              4 (8) of the sequence line's begin, 12 (24) bytes of table written by the kept ones.  No trimmed text: K-TRIM's copy
//              (the bytes of every kept record read and written) and the second index over it are gone, and neither intervals nor
//              table cross PCIe.
//   waits      one host wait beyond pf_count_fastq's (which has the index's two): for the table's length, which sizes the core's
//              grids; the trimming statistics and the ends of the records taken come back with it.  A pair has the second file's index
//              (two more) and the second core's end (one more), as two pf_count_fastq calls would.
// Statistics are kept per lane over a grid-stride loop and summed per wavefront when a kernel ends: one integer atomic per
// wavefront (k_mask_classes gives the reason).  Writes are plain vector stores.  Everything one call launches is timed as one launch
// of PF_K_TRIMCOUNT; unit: whole records taken (of both files of a pair).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_clip_dev.hpp"
#include "pf_count_dev.hpp"
#include "pf_ctx.hpp"
#include "pf_dedup_dev.hpp"
#include "pf_qc_dev.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"
#include "pf_trim_dev.hpp"
#include "pf_trimrun_rule.hpp"

namespace pf {

// ---- table ----
// keep[r] = 1 when record r is handed on; keep[n_rec] = 0 (the scan's last entry is the table's length)
__global__ __launch_bounds__(TRIM_BLOCK) void k_trimcount_keep(const uint32_t *__restrict__ len1, const uint32_t *__restrict__ len2, uint64_t n_rec,
                                                               uint32_t *__restrict__ keep, TrimCounts *c) {
    uint64_t both = 0, only1 = 0, only2 = 0;
    const bool pair = len2 != nullptr;
    if (blockIdx.x == 0 && threadIdx.x == 0) keep[n_rec] = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * TRIM_BLOCK) {
        const bool k1 = len1[r] != 0, k2 = pair ? len2[r] != 0 : true;
        keep[r] = pf_trimrun::handed_on(k1, k2) ? 1u : 0u;
        if (pair) {
            both += k1 && k2;
            only1 += k1 && !k2;
            only2 += !k1 && k2;
        }
    }
    both = wave_sum_u64(both);
    only1 = wave_sum_u64(only1);
    only2 = wave_sum_u64(only2);
    if (lane_id() == 0) {
        if (both) atomicAdd(&c->both, (unsigned long long)both);
        if (only1) atomicAdd(&c->only1, (unsigned long long)only1);
        if (only2) atomicAdd(&c->only2, (unsigned long long)only2);
    }
}

struct TrimScatterArgs {
    const uint32_t *lines[2], *begin[2], *len[2];
    const uint32_t *keep, *pos;   // the flags and their exclusive scan
    uint64_t *off[2];
    uint32_t *rlen[2];
    uint64_t n_rec;
    int n_files;
};
__global__ __launch_bounds__(TRIM_BLOCK) void k_trimcount_scatter(const TrimScatterArgs a) {
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_BLOCK) {
        if (!a.keep[r]) continue;
        const uint32_t at = a.pos[r];   // < the number of kept records <= n_rec
        for (int f = 0; f < a.n_files; ++f) {
            a.off[f][at] = (uint64_t)a.lines[f][8 * r + 2] + a.begin[f][r];
            a.rlen[f][at] = a.len[f][r];
        }
    }
}

// ---- host side ----

struct TrimTable {   // what the table phase leaves on the device for the core
    int n_files = 1;
    const char *text[2] = {nullptr, nullptr};      // staged, 16-byte aligned
    uint64_t used[2] = {0, 0};                     // bytes of the records taken
    const uint64_t *off[2] = {nullptr, nullptr};   // n_reads entries per file
    const uint32_t *len[2] = {nullptr, nullptr};
    uint64_t n_reads = 0, n_rec = 0;               // reads handed on per file; whole records taken per file
    MaskCounts *counts = nullptr;                  // all 0, no offender
};

// nothing taken, nothing kept: what a call reports until it has run
static void trim_table_reset(int n_files, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record) {
    for (int f = 0; f < n_files; ++f) bytes_used[f] = 0;
    if (n_records) *n_records = 0;
    if (bad_record) *bad_record = 0;
    if (stats) for (int f = 0; f < n_files; ++f) stats[f] = pf_trim_stats{};
}
static bool trim_chunk_empty(int n_files, const uint64_t *n_bytes) { return n_bytes[0] == 0 && (n_files == 1 || n_bytes[1] == 0); }

// Index, intervals and table of one chunk of a file (n_files = 1) or of each file of a pair (2), not empty, inside the caller's timed
// launch.  The arguments are arrays of n_files and have been reset.
static int trim_table_core(pf_ctx *ctx, const std::string &who, int n_files, const char *const *text, const uint64_t *n_bytes, int final,
                           const pf_trim_plan *plan, TrimTable &T, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record) {
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    T = TrimTable{};
    T.n_files = n_files;
    clip_forget(ctx);

    // ---- index ----
    FastqIndex ix[2];
    for (int f = 0; f < n_files; ++f) {
        if (!n_bytes[f]) continue;   // (no record: a pair's other file decides what that means)
        { const int rc = trim_stage_text(ctx, f == 0 ? (int)WS_MASK_TEXT : (int)WS_TRIM_TEXT2, text[f], n_bytes[f], &T.text[f]); if (rc) return rc; }
        ix[f].want_lines = true;
        if (f == 1) { ix[f].ws_index = WS_TRIM_INDEX2; ix[f].ws_table = WS_TRIM_TABLE2; }
        const std::string w = n_files == 2 ? who + ": file " + std::to_string(f + 1) : who;
        uint64_t bad = 0;
        const int rc = fastq_index(ctx, w.c_str(), T.text[f], n_bytes[f], final, ix[f], &bad);   // refused before anything is trimmed or counted
        if (rc) { if (bad_record) *bad_record = n_files == 2 ? 2 * bad + (uint64_t)f : bad; return rc; }
    }
    uint64_t n = ix[0].n_rec;
    if (n_files == 2) {
        n = std::min(ix[0].n_rec, ix[1].n_rec);
        if (final && ix[0].n_rec != ix[1].n_rec) {
            if (bad_record) *bad_record = 2 * n + (ix[0].n_rec < ix[1].n_rec ? 0 : 1);
            return refuse("the final chunks hold different numbers of records (file 1: " + std::to_string(ix[0].n_rec) + ", file 2: " +
                          std::to_string(ix[1].n_rec) + ")");
        }
    }
    if (n == 0) return PF_OK;   // no whole record (of both files): everything is carried
    uint32_t end32[2] = {0, 0};
    for (int f = 0; f < n_files; ++f)   // the end of record n - 1
        if (n < ix[f].n_rec) PF_HIP(hipMemcpyAsync(&end32[f], ix[f].line_start + 4 * n, 4, hipMemcpyDeviceToHost, ctx->stream));

    // ---- intervals, flags, places, table ----
    const size_t rec_bytes = up256((size_t)n * 4), flag_bytes = up256((size_t)(n + 1) * 4), off_bytes = up256((size_t)n * 8),
                 scr_bytes = up256(scan_scratch_bytes(n + 1));
    const bool clip = clip_is_open(ctx);   // K-CLIP: two more arrays behind the counters
    char *ww = static_cast<char *>(ctx_ws(ctx, WS_TRIM_WORK, 6 * rec_bytes + 2 * flag_bytes + 2 * off_bytes + scr_bytes + 256 + (clip ? 2 * rec_bytes : 0)));
    if (!ww) return PF_ERR_HIP;
    char *at = ww;
    auto take = [&](size_t bytes) { char *p = at; at += bytes; return p; };
    uint32_t *d_begin[2], *d_len[2], *d_rlen[2];
    uint64_t *d_off[2];
    for (int f = 0; f < 2; ++f) d_off[f] = reinterpret_cast<uint64_t *>(take(off_bytes));
    for (int f = 0; f < 2; ++f) d_begin[f] = reinterpret_cast<uint32_t *>(take(rec_bytes));
    for (int f = 0; f < 2; ++f) d_len[f] = reinterpret_cast<uint32_t *>(take(rec_bytes));
    for (int f = 0; f < 2; ++f) d_rlen[f] = reinterpret_cast<uint32_t *>(take(rec_bytes));
    uint32_t *d_keep = reinterpret_cast<uint32_t *>(take(flag_bytes)), *d_pos = reinterpret_cast<uint32_t *>(take(flag_bytes));
    void *scratch = take(scr_bytes);
    TrimCounts *dc = reinterpret_cast<TrimCounts *>(take(256));
    static_assert(2 * sizeof(TrimCounts) <= 256, "the counters of both files lie in the 256 bytes behind the work arrays");
    PF_HIP(hipMemsetAsync(dc, 0, 2 * sizeof(TrimCounts), ctx->stream));
    uint32_t *d_clip[2] = {nullptr, nullptr};
    if (clip) {
        const uint32_t *lines[2] = {ix[0].lines, ix[1].lines};
        for (int f = 0; f < 2; ++f) d_clip[f] = reinterpret_cast<uint32_t *>(take(rec_bytes));
        const int rc = clip_launch(ctx, n_files, T.text, n_bytes, lines, n, plan->phred, d_clip);
        if (rc) return rc;
    }
    const TrimSteps ts = trim_steps_by_value(plan->steps, plan->n_steps, plan->phred);
    for (int f = 0; f < n_files; ++f)
        k_trim_intervals<<<ctx_grid(ctx, n * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(T.text[f], n_bytes[f], ix[f].lines, n, ts, d_begin[f],
                                                                                                     d_len[f], dc + f, d_clip[f]);
    if (dedup_is_open(ctx)) {   // K-DEDUP: a later copy of a kept unit is dropped here, so stage `kept` of a report is what is handed on
        const uint32_t *dd_lines[2] = {ix[0].lines, ix[1].lines};
        const int rc = dedup_launch(ctx, n_files, T.text, n_bytes, dd_lines, n, d_begin, d_len, dc);
        if (rc) return rc;
    }
    if (qc_is_open(ctx)) {   // K-QC: both stages from what is on the device now -- the index, the final intervals, the clip ends
        const uint32_t *qc_lines[2] = {ix[0].lines, ix[1].lines};
        const int rc = qc_launch(ctx, n_files, 0, T.text, n_bytes, qc_lines, n, d_begin, d_len, clip ? d_clip : nullptr);
        if (rc) return rc;
    }
    k_trimcount_keep<<<ctx_grid(ctx, n, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(d_len[0], n_files == 2 ? d_len[1] : nullptr, n, d_keep, dc);
    PF_HIP(scan_exclusive_u32(d_keep, d_pos, n + 1, scratch, ctx->stream));
    TrimScatterArgs sa = {};
    for (int f = 0; f < n_files; ++f) {
        sa.lines[f] = ix[f].lines;
        sa.begin[f] = d_begin[f];
        sa.len[f] = d_len[f];
        sa.off[f] = d_off[f];
        sa.rlen[f] = d_rlen[f];
    }
    sa.keep = d_keep;
    sa.pos = d_pos;
    sa.n_rec = n;
    sa.n_files = n_files;
    k_trimcount_scatter<<<ctx_grid(ctx, n, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(sa);
    {
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-TRIMCOUNT launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    uint32_t n_kept = 0;
    TrimCounts h[2] = {};
    PF_HIP(hipMemcpyAsync(&n_kept, d_pos + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));   // the one wait: the table's length
    dedup_settle(ctx);   // K-DEDUP's entries came back with it
    for (int f = 0; f < n_files; ++f) {
        bytes_used[f] = T.used[f] = n < ix[f].n_rec ? (uint64_t)end32[f] : ix[f].used;
        T.off[f] = d_off[f];
        T.len[f] = d_rlen[f];
        if (!stats) continue;
        stats[f].reads = n;
        stats[f].kept = h[f].kept;
        stats[f].dropped = n - h[f].kept;
        stats[f].bases = h[f].bases;
        stats[f].bases_kept = h[f].bases_kept;
        if (n_files == 2) {
            stats[f].both = h[0].both;
            stats[f].only1 = h[0].only1;
            stats[f].only2 = h[0].only2;
            stats[f].neither = n - h[0].both - h[0].only1 - h[0].only2;
        }
    }
    T.n_reads = n_kept;
    T.n_rec = n;
    T.counts = ix[0].counts;   // reset by the index, untouched since: all 0, no offender
    if (n_records) *n_records = n;
    ctx_units(ctx, PF_K_TRIMCOUNT, n * (uint64_t)n_files);
    return PF_OK;
}

// what every entry point refuses about its chunk arguments and its plan, by `who`
static int trim_table_args(pf_ctx *ctx, const std::string &who, int n_files, const char *const *text, const uint64_t *n_bytes, const pf_trim_plan *plan,
                           const uint64_t *bytes_used) {
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    if (!bytes_used) return refuse("bytes_used is needed");
    if (!plan) return refuse("a plan is needed");
    { const std::string why = trim_steps_refusal(plan->steps, plan->n_steps, plan->phred, clip_is_open(ctx) || dedup_is_open(ctx)); if (!why.empty()) return refuse(why); }
    for (int f = 0; f < n_files; ++f) {
        if (n_bytes[f] && !text[f]) return refuse("text is needed");
        if (n_bytes[f] > 0xFFFFFF00ull) return refuse("a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    }
    return PF_OK;
}

static int trim_table_call(pf_ctx *ctx, const char *who_c, int n_files, const char *const *text, const uint64_t *n_bytes, int final, const pf_trim_plan *plan,
                           uint64_t *const *read_off, uint32_t *const *read_len, uint64_t *n_reads, uint64_t *bytes_used, uint64_t *n_records,
                           pf_trim_stats *stats, uint64_t *bad_record) {
    const std::string who = who_c;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    { const int rc = trim_table_args(ctx, who, n_files, text, n_bytes, plan, bytes_used); if (rc) return rc; }
    if (!n_reads) return refuse("n_reads is needed");
    *n_reads = 0;
    for (int f = 0; f < n_files; ++f)
        if (n_bytes[f] && (!read_off || !read_len || !read_off[f] || !read_len[f])) return refuse("read_off and read_len are needed");
    trim_table_reset(n_files, bytes_used, n_records, stats, bad_record);
    if (trim_chunk_empty(n_files, n_bytes)) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_TRIMCOUNT);
    TrimTable T;
    { const int rc = trim_table_core(ctx, who, n_files, text, n_bytes, final, plan, T, bytes_used, n_records, stats, bad_record); if (rc) return rc; }
    if (T.n_reads) {
        for (int f = 0; f < n_files; ++f) {
            PF_HIP(hipMemcpyAsync(read_off[f], T.off[f], (size_t)T.n_reads * 8, hipMemcpyDefault, ctx->stream));
            PF_HIP(hipMemcpyAsync(read_len[f], T.len[f], (size_t)T.n_reads * 4, hipMemcpyDefault, ctx->stream));
        }
        PF_HIP(hipStreamSynchronize(ctx->stream));
    }
    *n_reads = T.n_reads;
    return PF_OK;
}

// masked = false: K-COUNT's core; true: K-MASKCOUNT's with [low, up].  Exactly one of cstats / mstats is used.
static int trim_count_call(pf_ctx *ctx, const char *who_c, bool masked, int n_files, const char *const *text, const uint64_t *n_bytes, int final,
                           const pf_trim_plan *plan, uint32_t low, uint32_t up, uint64_t *bytes_used, pf_trim_stats *tstats, pf_count_stats *cstats,
                           pf_maskcount_stats *mstats, uint64_t *bad_record) {
    const std::string who = who_c;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    { const int rc = masked ? maskcount_needs(ctx, who_c) : count_needs_begin(ctx, who_c); if (rc) return rc; }
    CountState *S = count_state(ctx);
    { const int rc = trim_table_args(ctx, who, n_files, text, n_bytes, plan, bytes_used); if (rc) return rc; }
    if (masked && low > up) return refuse("low " + std::to_string(low) + " is above up " + std::to_string(up));
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    auto stats_out = [&](uint64_t n_reads) {
        if (masked) maskcount_stats_out(mstats, S, n_reads, h); else count_stats_out(cstats, S, n_reads, h);
    };
    if (cstats) *cstats = pf_count_stats{};
    if (mstats) *mstats = pf_maskcount_stats{};
    trim_table_reset(n_files, bytes_used, nullptr, tstats, bad_record);
    if (trim_chunk_empty(n_files, n_bytes)) { stats_out(0); return PF_OK; }
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_TRIMCOUNT);
    TrimTable T;
    { const int rc = trim_table_core(ctx, who, n_files, text, n_bytes, final, plan, T, bytes_used, nullptr, tstats, bad_record); if (rc) return rc; }
    if (T.n_reads)   // a chunk that hands on no read launches nothing more and counts nothing
        for (int f = 0; f < n_files; ++f) {
            const int rc = masked ? maskcount_core(ctx, S, T.text[f], T.used[f], T.off[f], T.len[f], T.n_reads, low, up, T.counts, h)
                                  : count_core(ctx, S, T.text[f], T.used[f], T.off[f], T.len[f], T.n_reads, T.counts, h);
            if (rc) return rc;
        }
    stats_out(T.n_reads * (uint64_t)n_files);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_trim_table_fastq(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint64_t *read_off,
                                   uint32_t *read_len, uint64_t *n_reads, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats,
                                   uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    return trim_table_call(ctx, "pf_trim_table_fastq", 1, &text, &n_bytes, final, plan, &read_off, &read_len, n_reads, bytes_used, n_records, stats,
                           bad_record);
}

extern "C" int pf_trim_table_fastq_pair(pf_ctx *ctx, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_plan *plan,
                                        uint64_t *read_off[2], uint32_t *read_len[2], uint64_t *n_reads, uint64_t bytes_used[2], uint64_t *n_records,
                                        pf_trim_stats stats[2], uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    const char *text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    return trim_table_call(ctx, "pf_trim_table_fastq_pair", 2, text, n, final, plan, read_off, read_len, n_reads, bytes_used, n_records, stats, bad_record);
}

extern "C" int pf_count_fastq_trimmed(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint64_t *bytes_used,
                                      pf_trim_stats *trim_stats, pf_count_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    return trim_count_call(ctx, "pf_count_fastq_trimmed", false, 1, &text, &n_bytes, final, plan, 0, 0, bytes_used, trim_stats, stats, nullptr, bad_record);
}

extern "C" int pf_count_fastq_pair_trimmed(pf_ctx *ctx, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_plan *plan,
                                           uint64_t bytes_used[2], pf_trim_stats trim_stats[2], pf_count_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    const char *text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    return trim_count_call(ctx, "pf_count_fastq_pair_trimmed", false, 2, text, n, final, plan, 0, 0, bytes_used, trim_stats, stats, nullptr, bad_record);
}

extern "C" int pf_maskcount_fastq_trimmed(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint32_t low, uint32_t up,
                                          uint64_t *bytes_used, pf_trim_stats *trim_stats, pf_maskcount_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    return trim_count_call(ctx, "pf_maskcount_fastq_trimmed", true, 1, &text, &n_bytes, final, plan, low, up, bytes_used, trim_stats, nullptr, stats,
                           bad_record);
}

extern "C" int pf_maskcount_fastq_pair_trimmed(pf_ctx *ctx, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final,
                                               const pf_trim_plan *plan, uint32_t low, uint32_t up, uint64_t bytes_used[2], pf_trim_stats trim_stats[2],
                                               pf_maskcount_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    const char *text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    return trim_count_call(ctx, "pf_maskcount_fastq_pair_trimmed", true, 2, text, n, final, plan, low, up, bytes_used, trim_stats, nullptr, stats,
                           bad_record);
}
