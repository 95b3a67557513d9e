// K-TRIM: `trimmomatic SE|PE -phred33 ... LEADING:t TRAILING:t SLIDINGWINDOW:w:t MINLEN:l` (step `1.trim` of the reference's workflow)
// on one chunk of a FASTQ file, or one chunk of each file of a pair.  The rule is pf_trim_rule.hpp; this file is its device form.
//
//   index      fastq_index of pf_reads_dev.hpp (K-MASK's and K-COUNT's), asked for the extents of all four lines of a record.
//   intervals  k_trim_intervals (pf_trim_dev.hpp, shared with K-TRIMCOUNT): a ROW of 16 lanes per read, four reads a wavefront.  A row stages 256 bytes of the quality line (and
//              64 bytes of halo behind them) into its 320 bytes of LDS with one aligned 16-byte load a lane -- the 64 lanes of a
//              wavefront read four contiguous stretches instead of 64 byte streams -- and a lane owns 16 positions.  Per step a lane
//              builds a 16-bit mask of its positions inside [b, e) ("q >= t" for LEADING / TRAILING, nothing for SLIDINGWINDOW, whose
//              lanes slide a byte sum over their positions and stop at their first bad window: w - 1 bytes of halo come from the LDS of
//              the row), and the row reduces "first" / "last" with four xor-shuffles.  The masks depend on the bytes only, never on b.
//              A read of up to 256 - 15 bytes is staged once for all steps; a longer one loops, each step over the row steps that
//              its [b, e) touches, forwards or backwards, and stops at the first hit.  Output: (begin, len) per record, len 0 = dropped.
//              With a clip open (pf_clip_begin), K-CLIP (pf_clip.hip) runs first and the interval starts as [0, clip end).
//              With a report open (pf_qc_begin), K-QC (pf_qc.hip) follows and adds both stages to its tables.
//   sizes      k_trim_sizes, one thread a record: output bytes per destination (1 single-ended, 4 for a pair: o1 u1 o2 u2), the pair
//              statistics.
//   offsets    scan_exclusive_u32_u64 over the destinations laid end to end.
//   copy       k_trim_copy: a row of 16 lanes per kept record of a file; each of its four pieces goes to its offset with aligned
//              16-byte stores (the source read as two aligned 16-byte units and shifted when it is not congruent), bytes at the
//              ragged ends, one '\n' behind each piece.  Plain vector stores.
// Statistics are kept per lane over a grid-stride loop and summed per wavefront when a kernel ends: one integer atomic per
// wavefront (k_mask_classes gives the reason).  Everything of one call is timed as one launch of PF_K_TRIM; unit: records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_clip_dev.hpp"
#include "pf_ctx.hpp"
#include "pf_dedup_dev.hpp"
#include "pf_qc_dev.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"
#include "pf_trim_dev.hpp"
#include "pf_trim_rule.hpp"

namespace pf {

// ---- sizes ----
// destination of the record of file f of a pair whose records are kept (k1, k2): o1 u1 o2 u2 = 0 1 2 3
__device__ inline int trim_dest(int f, bool k1, bool k2) { return f == 0 ? (k2 ? 0 : 1) : (k1 ? 2 : 3); }
__device__ inline uint32_t trim_record_bytes(const uint32_t *__restrict__ lines, uint64_t r, uint32_t len) {
    return (lines[8 * r + 1] - lines[8 * r]) + (lines[8 * r + 5] - lines[8 * r + 4]) + 2 * len + 4;
}
// size[d * n_rec + r] = bytes record r writes to destination d; size[n_dest * n_rec] = 0 (the scan's last entry is the total)
__global__ __launch_bounds__(TRIM_BLOCK) void k_trim_sizes(const uint32_t *__restrict__ lines1, const uint32_t *__restrict__ len1,
                                                           const uint32_t *__restrict__ lines2, const uint32_t *__restrict__ len2, uint64_t n_rec,
                                                           uint32_t *__restrict__ size, TrimCounts *c) {
    uint64_t both = 0, only1 = 0, only2 = 0;
    const bool pair = lines2 != nullptr;
    if (blockIdx.x == 0 && threadIdx.x == 0) size[(pair ? 4 : 1) * n_rec] = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * TRIM_BLOCK) {
        const uint32_t l1 = len1[r];
        if (!pair) {
            size[r] = l1 ? trim_record_bytes(lines1, r, l1) : 0u;
            continue;
        }
        const uint32_t l2 = len2[r];
        const bool k1 = l1 != 0, k2 = l2 != 0;
        uint32_t sz[4] = {0, 0, 0, 0};
        if (k1) sz[trim_dest(0, k1, k2)] = trim_record_bytes(lines1, r, l1);
        if (k2) sz[trim_dest(1, k1, k2)] = trim_record_bytes(lines2, r, l2);
#pragma unroll
        for (int d = 0; d < 4; ++d) size[(uint64_t)d * n_rec + r] = sz[d];
        both += k1 && k2;
        only1 += k1 && !k2;
        only2 += !k1 && k2;
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

// ---- copy ----
struct TrimCopyArgs {
    const char *text[2];
    uint64_t n_text[2];
    const uint32_t *lines[2], *begin[2], *len[2];
    const uint64_t *offs;   // the scan of `size`
    char *out[4];           // 16-byte aligned
    uint64_t n_rec;
    int n_files;
};
// one piece by a row: text[src, src + len) to out[dst ..), then '\n'
__device__ inline void trim_row_copy(const char *__restrict__ text, uint64_t n_text, uint64_t src, uint32_t len, char *__restrict__ out, uint64_t dst,
                                     int rl) {
    const uint64_t end = dst + len;
    uint64_t a0 = (dst + 15) & ~15ull;                       // head bytes [dst, a0)
    if (a0 > end) a0 = end;
    const uint64_t a1 = a0 + ((end - a0) & ~15ull);          // whole units [a0, a1), tail bytes [a1, end)
    if (dst + (uint64_t)rl < a0) out[dst + rl] = text[src + rl];
    for (uint64_t u = a0 + 16ull * rl; u < a1; u += 16ull * TRIM_ROW)
        *reinterpret_cast<uint4 *>(out + u) = trim_load_shifted(text, n_text, src + (u - dst));
    if (a1 + (uint64_t)rl < end) out[a1 + rl] = text[src + (a1 + rl - dst)];
    if (rl == TRIM_ROW - 1) out[end] = '\n';
}
__global__ __launch_bounds__(TRIM_BLOCK) void k_trim_copy(const TrimCopyArgs a) {
    const int rl = (int)threadIdx.x & (TRIM_ROW - 1), row = (int)threadIdx.x / TRIM_ROW;
    const uint64_t n_items = a.n_rec * (uint64_t)a.n_files;
    for (uint64_t it = (uint64_t)blockIdx.x * TRIM_ROWS + row; it < n_items; it += (uint64_t)gridDim.x * TRIM_ROWS) {
        const uint64_t r = a.n_files == 2 ? it >> 1 : it;
        const int f = a.n_files == 2 ? (int)(it & 1) : 0;
        const uint32_t len = a.len[f][r];
        if (!len) continue;
        int d = 0;
        if (a.n_files == 2) d = trim_dest(f, a.len[0][r] != 0, a.len[1][r] != 0);
        const uint64_t at = a.offs[(uint64_t)d * a.n_rec + r] - a.offs[(uint64_t)d * a.n_rec];
        const uint32_t *ln = a.lines[f] + 8 * r;
        const uint32_t b = a.begin[f][r], hl = ln[1] - ln[0], pl = ln[5] - ln[4];
        const char *text = a.text[f];
        char *out = a.out[d];
        trim_row_copy(text, a.n_text[f], ln[0], hl, out, at, rl);
        trim_row_copy(text, a.n_text[f], (uint64_t)ln[2] + b, len, out, at + hl + 1, rl);
        trim_row_copy(text, a.n_text[f], ln[4], pl, out, at + hl + 1 + len + 1, rl);
        trim_row_copy(text, a.n_text[f], (uint64_t)ln[6] + b, len, out, at + hl + 1 + len + 1 + pl + 1, rl);
    }
}

// ---- host side ----

// one chunk of a file (n_files = 1) or of each file of a pair (2); the arguments are arrays of n_files (out, out_bytes: 1 or 4)
static int trim_core(pf_ctx *ctx, const char *who_c, int n_files, const char *const *text, const uint64_t *n_bytes, int final,
                     const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, char *const *out, uint64_t *out_bytes, uint64_t *bytes_used,
                     uint32_t *const *rec_begin, uint32_t *const *rec_len, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record) {
    const std::string who = who_c;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    const int n_dest = n_files == 2 ? 4 : 1;
    if (!out_bytes || !bytes_used || !n_records) return refuse("out_bytes, bytes_used and n_records are needed");
    for (int d = 0; d < n_dest; ++d) out_bytes[d] = 0;
    for (int f = 0; f < n_files; ++f) bytes_used[f] = 0;
    *n_records = 0;
    if (bad_record) *bad_record = 0;
    if (stats) for (int f = 0; f < n_files; ++f) stats[f] = pf_trim_stats{};
    clip_forget(ctx);
    { const std::string why = trim_steps_refusal(steps, n_steps, phred, clip_is_open(ctx) || dedup_is_open(ctx)); if (!why.empty()) return refuse(why); }
    for (int f = 0; f < n_files; ++f) {
        if (n_bytes[f] && !text[f]) return refuse("text is needed");
        if (n_bytes[f] > 0xFFFFFF00ull) return refuse("a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
        for (int d = 2 * f; d < (n_files == 2 ? 2 * f + 2 : 1); ++d) {
            if (n_bytes[f] && !out[d]) return refuse("out is needed");
            if (n_bytes[f] && out[d] == text[f]) return refuse("out may not alias text");
        }
    }
    if (n_bytes[0] == 0 && (n_files == 1 || n_bytes[1] == 0)) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_TRIM);

    // ---- index ----
    const char *dt[2] = {nullptr, nullptr};
    FastqIndex ix[2];
    for (int f = 0; f < n_files; ++f) {
        if (!n_bytes[f]) continue;   // (no record: a pair's other file decides what that means)
        { const int rc = trim_stage_text(ctx, f == 0 ? (int)WS_MASK_TEXT : (int)WS_TRIM_TEXT2, text[f], n_bytes[f], &dt[f]); if (rc) return rc; }
        ix[f].want_lines = true;
        if (f == 1) { ix[f].ws_index = WS_TRIM_INDEX2; ix[f].ws_table = WS_TRIM_TABLE2; }
        const std::string w = n_files == 2 ? who + ": file " + std::to_string(f + 1) : who;
        uint64_t bad = 0;
        const int rc = fastq_index(ctx, w.c_str(), dt[f], n_bytes[f], final, ix[f], &bad);   // refused before anything is trimmed
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

    // ---- intervals, sizes, offsets ----
    const uint64_t n_size = (uint64_t)n_dest * n + 1;
    const size_t rec_bytes = up256((size_t)n * 4), size_bytes = up256((size_t)n_size * 4), offs_bytes = up256((size_t)n_size * 8),
                 scr_bytes = up256(scan_scratch_bytes(n_size));
    const bool clip = clip_is_open(ctx);   // K-CLIP: two more arrays behind the counters
    char *ww = static_cast<char *>(ctx_ws(ctx, WS_TRIM_WORK, 4 * rec_bytes + size_bytes + offs_bytes + scr_bytes + 256 + (clip ? 2 * rec_bytes : 0)));
    if (!ww) return PF_ERR_HIP;
    uint32_t *d_begin[2] = {reinterpret_cast<uint32_t *>(ww), reinterpret_cast<uint32_t *>(ww + rec_bytes)};
    uint32_t *d_len[2] = {reinterpret_cast<uint32_t *>(ww + 2 * rec_bytes), reinterpret_cast<uint32_t *>(ww + 3 * rec_bytes)};
    uint32_t *d_size = reinterpret_cast<uint32_t *>(ww + 4 * rec_bytes);
    uint64_t *d_offs = reinterpret_cast<uint64_t *>(ww + 4 * rec_bytes + size_bytes);
    void *scratch = ww + 4 * rec_bytes + size_bytes + offs_bytes;
    TrimCounts *dc = reinterpret_cast<TrimCounts *>(ww + 4 * rec_bytes + size_bytes + offs_bytes + scr_bytes);
    PF_HIP(hipMemsetAsync(dc, 0, 2 * sizeof(TrimCounts), ctx->stream));
    uint32_t *d_clip[2] = {nullptr, nullptr};
    if (clip) {
        const uint32_t *lines[2] = {ix[0].lines, ix[1].lines};
        for (int f = 0; f < 2; ++f) d_clip[f] = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(dc) + 256 + f * rec_bytes);
        const int rc = clip_launch(ctx, n_files, dt, n_bytes, lines, n, phred, d_clip);
        if (rc) return rc;
    }
    const TrimSteps ts = trim_steps_by_value(steps, n_steps, phred);
    for (int f = 0; f < n_files; ++f)
        k_trim_intervals<<<ctx_grid(ctx, n * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(dt[f], n_bytes[f], ix[f].lines, n, ts, d_begin[f],
                                                                                                     d_len[f], dc + f, d_clip[f]);
    if (dedup_is_open(ctx)) {   // K-DEDUP: a later copy of a kept unit is dropped here, so stage `kept` of a report is what is written
        const uint32_t *dd_lines[2] = {ix[0].lines, ix[1].lines};
        const int rc = dedup_launch(ctx, n_files, dt, n_bytes, dd_lines, n, d_begin, d_len, dc);
        if (rc) return rc;
    }
    if (qc_is_open(ctx)) {   // K-QC: both stages from what is on the device now -- the index, the final intervals, the clip ends
        const uint32_t *qc_lines[2] = {ix[0].lines, ix[1].lines};
        const int rc = qc_launch(ctx, n_files, 0, dt, n_bytes, qc_lines, n, d_begin, d_len, clip ? d_clip : nullptr);
        if (rc) return rc;
    }
    k_trim_sizes<<<ctx_grid(ctx, n, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(ix[0].lines, d_len[0], n_files == 2 ? ix[1].lines : nullptr,
                                                                                  n_files == 2 ? d_len[1] : nullptr, n, d_size, dc);
    PF_HIP(scan_exclusive_u32_u64(d_size, d_offs, n_size, scratch, ctx->stream));

    // ---- copy ----
    size_t cap[4], stage_at[4], stage_bytes = 0;
    bool direct[4];
    for (int d = 0; d < n_dest; ++d) {
        cap[d] = (size_t)n_bytes[n_files == 2 ? d / 2 : 0] + 1;
        direct[d] = is_device_ptr(out[d]) && ((uintptr_t)out[d] & 15) == 0;
        stage_at[d] = stage_bytes;
        if (!direct[d]) stage_bytes += up256(cap[d] + 16);
    }
    char *stage = nullptr;
    if (stage_bytes) {
        stage = static_cast<char *>(ctx_ws(ctx, WS_TRIM_OUT, stage_bytes));
        if (!stage) return PF_ERR_HIP;
    }
    TrimCopyArgs ca = {};
    for (int f = 0; f < n_files; ++f) {
        ca.text[f] = dt[f];
        ca.n_text[f] = n_bytes[f];
        ca.lines[f] = ix[f].lines;
        ca.begin[f] = d_begin[f];
        ca.len[f] = d_len[f];
    }
    ca.offs = d_offs;
    for (int d = 0; d < n_dest; ++d) ca.out[d] = direct[d] ? out[d] : stage + stage_at[d];
    ca.n_rec = n;
    ca.n_files = n_files;
    k_trim_copy<<<ctx_grid(ctx, n * (uint64_t)n_files * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(ca);
    {
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-TRIM launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    uint64_t base[5] = {0, 0, 0, 0, 0};
    for (int d = 0; d <= n_dest; ++d) PF_HIP(hipMemcpyAsync(&base[d], d_offs + (uint64_t)d * n, 8, hipMemcpyDeviceToHost, ctx->stream));
    TrimCounts h[2] = {};
    PF_HIP(hipMemcpyAsync(h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    dedup_settle(ctx);   // K-DEDUP's entries came back with the counters
    for (int d = 0; d < n_dest; ++d) {
        out_bytes[d] = base[d + 1] - base[d];
        if (!direct[d] && out_bytes[d]) PF_HIP(hipMemcpyAsync(out[d], ca.out[d], (size_t)out_bytes[d], hipMemcpyDefault, ctx->stream));
    }
    for (int f = 0; f < n_files; ++f) {
        if (rec_begin && rec_begin[f]) PF_HIP(hipMemcpyAsync(rec_begin[f], d_begin[f], (size_t)n * 4, hipMemcpyDefault, ctx->stream));
        if (rec_len && rec_len[f]) PF_HIP(hipMemcpyAsync(rec_len[f], d_len[f], (size_t)n * 4, hipMemcpyDefault, ctx->stream));
    }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < n_files; ++f) {
        bytes_used[f] = n < ix[f].n_rec ? (uint64_t)end32[f] : ix[f].used;
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
    *n_records = n;
    ctx_units(ctx, PF_K_TRIM, n * (uint64_t)n_files);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_trim_fastq(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                             char *out, uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t *n_records,
                             pf_trim_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    return trim_core(ctx, "pf_trim_fastq", 1, &text, &n_bytes, final, steps, n_steps, phred, &out, out_bytes, bytes_used, &rec_begin, &rec_len, n_records,
                     stats, bad_record);
}

extern "C" int pf_trim_fastq_pair(pf_ctx *ctx, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps,
                                  uint32_t n_steps, uint32_t phred, char *out[4], uint64_t out_bytes[4], uint64_t bytes_used[2], uint32_t *rec_begin[2],
                                  uint32_t *rec_len[2], uint64_t *n_records, pf_trim_stats stats[2], uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    if (!out) { pf::CtxErr{ctx} = "pf_trim_fastq_pair: out is needed"; return PF_ERR_ARG; }
    const char *text[2] = {text1, text2};
    const uint64_t n[2] = {n1, n2};
    return trim_core(ctx, "pf_trim_fastq_pair", 2, text, n, final, steps, n_steps, phred, out, out_bytes, bytes_used, rec_begin, rec_len, n_records, stats,
                     bad_record);
}
