// What K-MASK (pf_mask.hip) and K-COUNT (pf_count.hip) share on the device: reads as a byte text with a table (read_off, read_len),
// the class bitmaps that map window starts to reads, the LDS tile of 2-bit codes that yields one k-mer per lane, and the FASTQ index
// of a chunk.  Kernels are `static`: each of the two files carries its own copy (no device-side calls across files).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_mask_rule.hpp"
#include "pf_scan.hpp"

namespace pf {

constexpr int MASK_BLOCK = 256;
constexpr int MASK_PER_LANE = 4;                              // window starts a lane owns in one tile
constexpr int MASK_TILE = MASK_BLOCK * MASK_PER_LANE;         // bytes (window starts) of a tile
constexpr int MASK_TILE_UNITS = MASK_TILE / 16;
constexpr int MASK_HALO_UNITS = 2;                            // 32 bytes behind the tile: k - 1 <= 30
constexpr int MASK_UNITS = MASK_TILE_UNITS + MASK_HALO_UNITS; // 16-byte units staged per tile
constexpr uint64_t MASK_NO_RECORD = ~0ull;
static_assert(pf_mask::MAX_K - 1 <= 16 * MASK_HALO_UNITS, "the halo holds the rest of a tile's last window");

struct MaskCounts {   // device side of pf_mask_stats (reads is known to the host)
    unsigned long long reads_changed, bases, bases_masked, kmers, kmers_bad;
    unsigned long long bad_entry;   // k_mask_check_table / k_fq_records: the smallest offender, MASK_NO_RECORD = none
    unsigned long long kmers_invalid, kmers_kept;   // K-MASKCOUNT only: windows holding a non-base, windows counted
};
static_assert(sizeof(MaskCounts) <= 256, "the counters lie in the 256 bytes behind a call's table or index");

// 16 bytes of the text from unit `u`: one vector load inside the text, byte by byte (0 beyond the end) at its end
__device__ inline uint4 mask_load_unit(const char *__restrict__ text, uint64_t n, uint64_t u) {
    const uint64_t base = u * 16;
    if (base + 16 <= n) return *reinterpret_cast<const uint4 *>(text + base);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; ++b)
        if (base + b < n) w[b >> 2] |= (uint32_t)(uint8_t)text[base + b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ inline uint32_t unit_byte(const uint4 &v, int b) {
    const uint32_t w = (b >> 2) == 0 ? v.x : (b >> 2) == 1 ? v.y : (b >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (b & 3))) & 0xFFu;
}
__device__ inline uint64_t bit_range(uint64_t a, uint64_t b) {   // bits a .. b - 1 of a word, 0 <= a < b <= 64
    const uint64_t len = b - a;
    return (len >= 64 ? ~0ull : ((1ull << len) - 1)) << a;
}

// ---- the tile: MASK_UNITS units of the text from tile `tile` as 2-bit codes (16 bases a word, first base most significant) and a
// 1-bit "is ACGTacgt" plane (32 bases a word, written as half words).  Threads tid < MASK_UNITS stage one unit each; the caller
// synchronises the block before (the last tile has been read) and after. ----
__device__ inline void tile_stage(const char *__restrict__ text, uint64_t n, uint64_t tile, int tid, uint32_t *s_code, uint32_t *s_valid32) {
    if (tid < MASK_UNITS) {
        const uint4 v = mask_load_unit(text, n, tile * MASK_TILE_UNITS + (uint64_t)tid);
        uint32_t code = 0, valid = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint8_t ch = (uint8_t)unit_byte(v, b);
            code |= pf_mask::base_code(ch) << (30 - 2 * b);
            valid |= (uint32_t)pf_mask::is_base(ch) << (15 - b);
        }
        s_code[tid] = code;
        reinterpret_cast<uint16_t *>(s_valid32)[tid ^ 1] = (uint16_t)valid;   // (little endian: the even unit is the high half)
    }
}
// are the k bytes from position p of the tile all bases?  all_k = (1 << k) - 1
__device__ inline bool tile_window_valid(const uint32_t *s_valid32, int p, int k, uint64_t all_k) {
    const int vi = p >> 5, vt = p & 31;
    const uint64_t vv = (((uint64_t)s_valid32[vi] << 32) | s_valid32[vi + 1]) << vt;
    return (vv >> (64 - k)) == all_k;
}
// the k-mer at position p of the tile as it reads: three LDS words and two shifts
__device__ inline uint64_t tile_kmer(const uint32_t *s_code, int p, int k) {
    const int wi = p >> 4, s = (p & 15) * 2;
    const uint64_t hi = ((uint64_t)s_code[wi] << 32) | s_code[wi + 1];
    const uint64_t x = (hi << s) | ((uint64_t)s_code[wi + 2] >> (32 - s));
    return x >> (64 - 2 * k);
}

// ---- the table: ascending, inside the text, no overlaps (explicit tables only: the FASTQ index makes its own) ----
[[maybe_unused]] static __global__ void k_mask_check_table(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint64_t n_reads, uint64_t n_bytes,
                                          MaskCounts *c) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const uint64_t o = off[i], e = o + len[i];
    const bool bad = o > n_bytes || e > n_bytes || (i + 1 < n_reads && e > off[i + 1]);
    if (bad) atomicMin(&c->bad_entry, (unsigned long long)i);
}

// ---- classes ----
[[maybe_unused]] static __global__ __launch_bounds__(MASK_BLOCK) void k_mask_classes(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                                    uint64_t n_reads, uint64_t n_words, uint32_t k, uint64_t *__restrict__ seq,
                                                                    uint64_t *__restrict__ start, MaskCounts *c) {
    // grid-stride, sums kept per lane: one atomic a wavefront when the kernel ends (one a word's wavefront was 146 000 adds to two
    // addresses at 300 MB of text -- 1.8 ms of a 14 ms call, all of it the atomics)
    uint64_t bases = 0, kmers = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * MASK_BLOCK) {
        uint64_t ms = 0, mw = 0;
        const uint64_t lo = w * 64, hi = lo + 64;
        uint64_t a = 0, b = n_reads;   // the first read whose end lies beyond lo (ends ascend: the table has no overlaps)
        while (a < b) {
            const uint64_t m = (a + b) >> 1;
            if (off[m] + len[m] > lo) b = m; else a = m + 1;
        }
        for (uint64_t r = a; r < n_reads; ++r) {
            const uint64_t o = off[r];
            if (o >= hi) break;
            const uint64_t l = len[r], e = o + l;
            const uint64_t es = l >= k ? e - k + 1 : o;   // end of the window starts
            const uint64_t x = (o > lo ? o : lo) - lo;
            const uint64_t y = (e < hi ? e : hi) - lo, ys = (es < hi ? es : hi) - lo;
            if (e > lo && y > x) ms |= bit_range(x, y);
            if (es > lo && ys > x) mw |= bit_range(x, ys);
        }
        seq[w] = ms;
        start[w] = mw;
        bases += (uint64_t)__popcll(ms);
        kmers += (uint64_t)__popcll(mw);
    }
    bases = wave_sum_u64(bases);
    kmers = wave_sum_u64(kmers);
    if (lane_id() == 0) {
        if (bases) atomicAdd(&c->bases, (unsigned long long)bases);
        if (kmers) atomicAdd(&c->kmers, (unsigned long long)kmers);
    }
}

// ---- FASTQ index ----
static __global__ __launch_bounds__(MASK_BLOCK) void k_fq_newlines(const char *__restrict__ text, uint64_t n, uint64_t n_words, uint64_t *__restrict__ nl,
                                                                   uint32_t *__restrict__ cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    uint64_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = mask_load_unit(text, n, w * 4 + q);   // (bytes beyond the end read as 0: no newline)
#pragma unroll
        for (int b = 0; b < 16; ++b) m |= (uint64_t)(unit_byte(v, b) == (uint32_t)'\n') << (16 * q + b);
    }
    nl[w] = m;
    cnt[w] = (uint32_t)__popcll(m);
}

// line_start[l] = first byte of line l; line_start[0] = 0, and one entry per newline
static __global__ __launch_bounds__(MASK_BLOCK) void k_fq_line_starts(const uint64_t *__restrict__ nl, const uint32_t *__restrict__ pre, uint64_t n_words,
                                                                      uint32_t *__restrict__ line_start) {
    const uint64_t w = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x;
    if (w == 0) line_start[0] = 0;
    if (w >= n_words) return;
    uint64_t m = nl[w];
    uint32_t r = pre[w];
    while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        line_start[++r] = (uint32_t)(w * 64 + (uint64_t)b + 1);
    }
}

// n_lines: lines of the text (n_newlines, plus one for a last line without '\n')
static __global__ __launch_bounds__(MASK_BLOCK) void k_fq_records(const char *__restrict__ text, uint64_t n, const uint32_t *__restrict__ line_start,
                                                                  uint64_t n_newlines, uint64_t n_rec, uint64_t *__restrict__ off, uint32_t *__restrict__ len,
                                                                  MaskCounts *c, uint32_t *__restrict__ lines = nullptr) {
    const uint64_t r = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x;
    if (r >= n_rec) return;
    uint64_t b[4], e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t l = 4 * r + i;
        const bool has_nl = l < n_newlines;
        b[i] = line_start[l];
        e[i] = pf_mask::line_content_end(text, b[i], has_nl ? (uint64_t)line_start[l + 1] - 1 : n, has_nl);
    }
    off[r] = b[pf_mask::LINE_SEQUENCE];
    len[r] = (uint32_t)(e[pf_mask::LINE_SEQUENCE] - b[pf_mask::LINE_SEQUENCE]);
    if (lines) {   // K-TRIM: content begin and end of all four lines, 32 bytes a record
        reinterpret_cast<uint4 *>(lines)[2 * r] = make_uint4((uint32_t)b[0], (uint32_t)e[0], (uint32_t)b[1], (uint32_t)e[1]);
        reinterpret_cast<uint4 *>(lines)[2 * r + 1] = make_uint4((uint32_t)b[2], (uint32_t)e[2], (uint32_t)b[3], (uint32_t)e[3]);
    }
    const int clause = pf_mask::record_clause(text, b[pf_mask::LINE_HEADER], e[pf_mask::LINE_HEADER], e[pf_mask::LINE_SEQUENCE] - b[pf_mask::LINE_SEQUENCE],
                                              b[pf_mask::LINE_PLUS], e[pf_mask::LINE_PLUS], e[pf_mask::LINE_QUALITY] - b[pf_mask::LINE_QUALITY]);
    if (clause) atomicMin(&c->bad_entry, (unsigned long long)((r << 3) | (uint64_t)clause));
}

// ---- host side ----
// pf_mask.hip: k_mask_flag over text[0, n) against the context's resident count table, on the context's stream -- bad[w] for every
// word of every tile from the window-start bitmap, kmers_bad added to counts.  The caller has checked that a table is resident.
void mask_flag_launch(pf_ctx *ctx, const char *text, uint64_t n, uint64_t n_tiles, const uint64_t *start, uint64_t *bad, uint32_t low, uint32_t up,
                      MaskCounts *counts);

constexpr uint64_t MASK_MAX_BYTES = 1ull << 40;   // every grid of a call stays far below 2^31 blocks

// all counters 0, no offender
static inline hipError_t mask_counts_reset(MaskCounts *dc, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(dc, 0, sizeof(MaskCounts), st);
    return e != hipSuccess ? e : hipMemsetAsync(&dc->bad_entry, 0xFF, sizeof dc->bad_entry, st);
}

// the text on the device, 16-byte aligned: the caller's own memory when it is that already, else a copy in a workspace
static inline int mask_stage_text(pf_ctx *ctx, const char *text, uint64_t n, const char **dev) {
    if (is_device_ptr(text) && ((uintptr_t)text & 15) == 0) { *dev = text; return PF_OK; }
    char *p = static_cast<char *>(ctx_ws(ctx, WS_MASK_TEXT, (size_t)n + 16));
    if (!p) return PF_ERR_HIP;
    PF_HIP(hipMemcpyAsync(p, text, (size_t)n, hipMemcpyDefault, ctx->stream));
    *dev = p;
    return PF_OK;
}

// The FASTQ index of one chunk (0 < n_bytes < 2^32, text on the device): the whole records, their sequence lines as a table on the
// device, the bytes they use, the counters reset.  A format error is refused here, by `who` and by name, before the caller has
// touched anything: PF_ERR_ARG with *bad_record = the 0-based record within the chunk.
struct FastqIndex {
    uint64_t n_rec = 0, used = 0;
    const uint64_t *off = nullptr;   // device, n_rec entries (null when n_rec = 0)
    const uint32_t *len = nullptr;
    MaskCounts *counts = nullptr;    // device: all 0, no offender
    // K-TRIM asks for more (set before the call; K-MASK and K-COUNT leave them as they are):
    bool want_lines = false;                                     // fill `lines`
    int ws_index = WS_MASK_INDEX, ws_table = WS_MASK_TABLE;      // the workspaces (a pair's second file has its own)
    const uint32_t *lines = nullptr;        // device, 8 per record: content begin and end of header, sequence, plus and quality line
    const uint32_t *line_start = nullptr;   // device: first byte of every line (n_newlines + 1 entries; null when n_rec = 0)
    uint64_t n_newlines = 0;
};
static inline int fastq_index(pf_ctx *ctx, const char *who, const char *dt, uint64_t n_bytes, int final, FastqIndex &ix, uint64_t *bad_record) {
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    MaskCounts h = {};
    // newlines: bitmap, count per word, prefix
    const uint64_t n_words = (n_bytes + 63) / 64;
    const size_t nl_bytes = up256((size_t)n_words * 8), cnt_bytes = up256((size_t)n_words * 4), scr_bytes = up256(scan_scratch_bytes(n_words));
    char *iw = static_cast<char *>(ctx_ws(ctx, ix.ws_index, nl_bytes + 2 * cnt_bytes + scr_bytes + 256));
    if (!iw) return PF_ERR_HIP;
    uint64_t *nl = reinterpret_cast<uint64_t *>(iw);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(iw + nl_bytes), *pre = reinterpret_cast<uint32_t *>(iw + nl_bytes + cnt_bytes);
    void *scratch = iw + nl_bytes + 2 * cnt_bytes;
    MaskCounts *dc = reinterpret_cast<MaskCounts *>(iw + nl_bytes + 2 * cnt_bytes + scr_bytes);
    ix.counts = dc;
    const unsigned word_grid = (unsigned)((n_words + MASK_BLOCK - 1) / MASK_BLOCK);
    k_fq_newlines<<<word_grid, MASK_BLOCK, 0, ctx->stream>>>(dt, n_bytes, n_words, nl, cnt);
    PF_HIP(scan_exclusive_u32(cnt, pre, n_words, scratch, ctx->stream));
    uint32_t last_pre = 0, last_cnt = 0;
    uint64_t last_nl = 0;
    PF_HIP(hipMemcpyAsync(&last_pre, pre + (n_words - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&last_cnt, cnt + (n_words - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&last_nl, nl + (n_words - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(mask_counts_reset(dc, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t n_newlines = (uint64_t)last_pre + last_cnt;
    const bool ends_in_newline = (last_nl >> ((n_bytes - 1) & 63)) & 1ull;
    // whole records: every line of them ends in its '\n', but for the last line of a final chunk
    const uint64_t n_lines = n_newlines + ((final && !ends_in_newline) ? 1 : 0);
    const uint64_t n_rec = n_lines / 4;
    ix.n_rec = n_rec;
    ix.n_newlines = n_newlines;
    ix.used = final ? n_bytes : 0;
    if (n_rec) {
        const size_t ls_bytes = up256((size_t)(n_newlines + 2) * 4), off_bytes = up256((size_t)n_rec * 8), len_bytes = up256((size_t)n_rec * 4);
        const size_t lines_bytes = ix.want_lines ? up256((size_t)n_rec * 32) : 0;
        char *tw = static_cast<char *>(ctx_ws(ctx, ix.ws_table, ls_bytes + off_bytes + len_bytes + lines_bytes));
        if (!tw) return PF_ERR_HIP;
        uint32_t *dlines = ix.want_lines ? reinterpret_cast<uint32_t *>(tw + ls_bytes + off_bytes + len_bytes) : nullptr;
        ix.lines = dlines;
        ix.line_start = reinterpret_cast<uint32_t *>(tw);
        uint32_t *line_start = reinterpret_cast<uint32_t *>(tw);
        uint64_t *doff = reinterpret_cast<uint64_t *>(tw + ls_bytes);
        uint32_t *dlen = reinterpret_cast<uint32_t *>(tw + ls_bytes + off_bytes);
        ix.off = doff;
        ix.len = dlen;
        k_fq_line_starts<<<word_grid, MASK_BLOCK, 0, ctx->stream>>>(nl, pre, n_words, line_start);
        k_fq_records<<<(unsigned)((n_rec + MASK_BLOCK - 1) / MASK_BLOCK), MASK_BLOCK, 0, ctx->stream>>>(dt, n_bytes, line_start, n_newlines, n_rec, doff, dlen, dc, dlines);
        uint32_t end32 = 0;
        if (!final) PF_HIP(hipMemcpyAsync(&end32, line_start + 4 * n_rec, 4, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (h.bad_entry != MASK_NO_RECORD) {   // refused on the host, before anything is done with the reads
            if (bad_record) *bad_record = h.bad_entry >> 3;
            return refuse(std::string(who) + ": record " + std::to_string(h.bad_entry >> 3) + " of the chunk: " + pf_mask::clause_text((int)(h.bad_entry & 7)));
        }
        if (!final) ix.used = end32;
    }
    if (final && n_lines % 4) {   // (n_rec = 0: record 0)
        if (bad_record) *bad_record = n_rec;
        return refuse(std::string(who) + ": record " + std::to_string(n_rec) + " of the chunk: " + pf_mask::clause_text(pf_mask::CLAUSE_LINE_COUNT));
    }
    return PF_OK;
}

}  // namespace pf
