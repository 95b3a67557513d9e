// K-MASK: `kmc_tools filter -hm <db> <reads.fq> -ci<L> [-cx<U>]` against the count table that is already in HBM -- one look-up per
// k-mer of every read (CKMCFile::GetCountersForRead, KMC/kmc_api/kmc_file.cpp:904-1090), every base of every k-mer whose counter
// lies outside [L, U] replaced by N.  The rule is pf_mask_rule.hpp; this file is its device form.
//
// The unit of work is a byte of the text (a window start), never a read: lane occupancy does not depend on read length.
//   classes   k_mask_classes, flat over 64-byte words: two bitmaps with one bit per input byte -- "is a sequence byte" and "is a
//             window start" (inside a read, i + k <= the read's end) -- from the table (read_off, read_len), which is ascending and
//             without overlaps: one binary search per word, then a walk over the reads that touch it.  This is the window -> read
//             mapping: the two phases below never see a read boundary.
//   flag      k_mask_flag: a block stages a tile of 1024 bytes plus a halo of 32 into LDS as 2-bit codes (16 bases a word, first
//             base most significant) and a 1-bit "is ACGTacgt" plane, one 16-byte load a lane.  A lane owns four window starts, 256
//             apart, so that the 64 lanes of a wavefront hold 64 neighbouring k-mers (which share minimizers, hence table lines)
//             and its 64 verdicts are one word of the bad bitmap: one ballot, one store, no atomic.  The k-mer is three LDS words
//             and two shifts; the four probes of a lane are issued before the first is consumed (count_probe_at / count_finish).
//             both_strands tables are asked for the canonical form, the others for the window as it reads: one probe either way.
//   paint     k_mask_paint, flat over 16-byte units: a byte becomes N when the bad bitmap has a bit in [j - k + 1, j] and the byte
//             is a sequence byte; 64 bits ending at the unit's last byte answer that for its 16 bytes.  16-byte loads and stores;
//             a unit under no bad window is a plain copy.  It also leaves a "changed" bitmap.
//   changed   k_mask_changed, one thread a read: reads_changed from the changed bitmap (a few words a read).
// Statistics are ballots / popcounts kept per lane over a grid-stride loop and summed per wavefront when a kernel ends: one integer
// atomic per resident wavefront (8 192 a kernel, not one per 64 words -- adds to one address cost 12 ns each); the same on every run.
//
// FASTQ index (pf_mask_fastq): newline bitmap + popcount per 64-byte word (k_fq_newlines), exclusive scan (pf_scan.hpp), line starts
// scattered from the bitmap (k_fq_line_starts), then one thread a record checks the three format clauses -- a reduction to the
// smallest offending record -- and writes (read_off, read_len) of its sequence line (k_fq_records).
// Everything of one call is timed as one launch of PF_K_MASK; unit: windows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_mask_rule.hpp"
#include "pf_scan.hpp"

#define PF_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            pf::CtxErr{ctx} = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return PF_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

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
};

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

// ---- the table: ascending, inside the text, no overlaps (pf_mask_reads only: pf_mask_fastq makes its own) ----
__global__ void k_mask_check_table(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint64_t n_reads, uint64_t n_bytes,
                                   MaskCounts *c) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const uint64_t o = off[i], e = o + len[i];
    const bool bad = o > n_bytes || e > n_bytes || (i + 1 < n_reads && e > off[i + 1]);
    if (bad) atomicMin(&c->bad_entry, (unsigned long long)i);
}

// ---- classes ----
__global__ __launch_bounds__(MASK_BLOCK) void k_mask_classes(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
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

// ---- flag ----
struct MaskFlagArgs {
    const CountLine *tab;
    uint64_t mask;
    int k;
    int exact;              // the table was not counted on both strands: the window as it reads
    const char *text;
    uint64_t n;             // bytes of the text
    uint64_t n_tiles;
    const uint64_t *start;  // window-start bitmap, MASK_TILE / 64 words a tile
    uint64_t *bad;          // out: bad-window bitmap, every word of every tile
    uint32_t low, up;
    MaskCounts *c;
};

__global__ __launch_bounds__(MASK_BLOCK) void k_mask_flag(const MaskFlagArgs a) {
    __shared__ uint32_t s_code[MASK_UNITS];        // 16 bases a word, first base most significant
    __shared__ uint32_t s_valid32[MASK_UNITS / 2 + 1];   // 32 bases a word, first base most significant, written as half words
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    const uint64_t all_k = (1ull << k) - 1;
    uint64_t n_bad = 0;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile has been read
        if (tid < MASK_UNITS) {
            const uint4 v = mask_load_unit(a.text, a.n, tile * MASK_TILE_UNITS + (uint64_t)tid);
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
        __syncthreads();
        const uint64_t word0 = tile * (MASK_TILE / 64) + (uint64_t)wave;
        CountProbe pr[MASK_PER_LANE];
        bool look[MASK_PER_LANE], is_start[MASK_PER_LANE];
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {
            const uint64_t sw = a.start[word0 + (uint64_t)j * (MASK_BLOCK / 64)];   // the same word for the whole wavefront
            is_start[j] = (sw >> lane) & 1ull;
            look[j] = false;
            if (is_start[j]) {
                const int p = j * MASK_BLOCK + tid;
                const int vi = p >> 5, vt = p & 31;
                const uint64_t vv = (((uint64_t)s_valid32[vi] << 32) | s_valid32[vi + 1]) << vt;
                look[j] = (vv >> (64 - k)) == all_k;
                if (look[j]) {
                    const int wi = p >> 4, s = (p & 15) * 2;
                    const uint64_t hi = ((uint64_t)s_code[wi] << 32) | s_code[wi + 1];
                    const uint64_t x = (hi << s) | ((uint64_t)s_code[wi + 2] >> (32 - s));
                    const uint64_t fwd = x >> (64 - 2 * k);
                    const uint64_t rc = rc_kmer(fwd, k);
                    const uint64_t key = (!a.exact && rc < fwd) ? rc : fwd;
                    count_probe_at(a.tab, key, kmer_lines(fwd, rc, k, a.mask), pr[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {
            uint32_t cnt = 0;
            if (look[j]) {
                uint32_t got;
                if (count_finish(a.tab, a.mask, pr[j], got)) cnt = got;
            }
            const unsigned long long bw = __ballot(is_start[j] && pf_mask::window_bad(cnt, a.low, a.up));
            if (lane == 0) {
                a.bad[word0 + (uint64_t)j * (MASK_BLOCK / 64)] = bw;
                n_bad += (uint64_t)__popcll(bw);
            }
        }
    }
    if (lane == 0 && n_bad) atomicAdd(&a.c->kmers_bad, (unsigned long long)n_bad);
}

// ---- paint ----
__global__ __launch_bounds__(MASK_BLOCK) void k_mask_paint(const char *__restrict__ text, char *__restrict__ out, uint64_t n, uint64_t n_units,
                                                           int k, const uint64_t *__restrict__ seq, const uint64_t *__restrict__ bad,
                                                           uint16_t *__restrict__ changed, MaskCounts *c) {
    uint64_t masked = 0;   // per lane; one atomic a wavefront when the kernel ends
    for (uint64_t u = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * MASK_BLOCK) {
        uint32_t ch_bits = 0;
        const uint64_t base = u * 16, q = base >> 6;
        const int e = (int)(base & 63) + 15;   // bit of the unit's last byte in word q
        const uint64_t wq = bad[q], wp = q ? bad[q - 1] : 0ull;
        const uint64_t win = (wq << (63 - e)) | (e < 63 ? wp >> (e + 1) : 0ull);   // bit 63 = window base + 15, bit 63 - t = window base + 15 - t
        const uint32_t seq16 = (uint32_t)(seq[q] >> (base & 63)) & 0xFFFFu;
        uint4 v = mask_load_unit(text, n, u);
        if ((win >> (64 - 15 - k)) != 0 && seq16) {   // some window of base - k + 1 .. base + 15 is bad
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const bool m = pf_mask::byte_masked(win << (15 - b), k) && ((seq16 >> b) & 1u);
                const uint32_t byte = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
                if (m) {
                    ch_bits |= (uint32_t)(byte != (uint32_t)pf_mask::MASK_BYTE) << b;
                    w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)pf_mask::MASK_BYTE << (8 * (b & 3)));
                }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (base + 16 <= n) {
            *reinterpret_cast<uint4 *>(out + base) = v;
        } else {
            for (int b = 0; base + b < n; ++b) out[base + b] = (char)unit_byte(v, b);
        }
        changed[u] = (uint16_t)ch_bits;
        masked += (uint64_t)__popc(ch_bits);
    }
    masked = wave_sum_u64(masked);
    if (lane_id() == 0 && masked) atomicAdd(&c->bases_masked, (unsigned long long)masked);
}

// ---- reads_changed ----
__global__ __launch_bounds__(MASK_BLOCK) void k_mask_changed(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint64_t n_reads,
                                                             const uint64_t *__restrict__ changed, MaskCounts *c) {
    uint64_t n_changed = 0;   // per lane; one atomic a wavefront when the kernel ends
    for (uint64_t r = (uint64_t)blockIdx.x * MASK_BLOCK + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * MASK_BLOCK) {
        if (!len[r]) continue;
        bool any = false;
        const uint64_t o = off[r], e = o + len[r];
        for (uint64_t w = o >> 6; w <= (e - 1) >> 6 && !any; ++w) {
            const uint64_t lo = w * 64;
            const uint64_t x = (o > lo ? o : lo) - lo, y = (e < lo + 64 ? e : lo + 64) - lo;
            any = (changed[w] & bit_range(x, y)) != 0;
        }
        n_changed += any;
    }
    n_changed = wave_sum_u64(n_changed);
    if (lane_id() == 0 && n_changed) atomicAdd(&c->reads_changed, (unsigned long long)n_changed);
}

// ---- FASTQ index ----
__global__ __launch_bounds__(MASK_BLOCK) void k_fq_newlines(const char *__restrict__ text, uint64_t n, uint64_t n_words, uint64_t *__restrict__ nl,
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
__global__ __launch_bounds__(MASK_BLOCK) void k_fq_line_starts(const uint64_t *__restrict__ nl, const uint32_t *__restrict__ pre, uint64_t n_words,
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
__global__ __launch_bounds__(MASK_BLOCK) void k_fq_records(const char *__restrict__ text, uint64_t n, const uint32_t *__restrict__ line_start,
                                                           uint64_t n_newlines, uint64_t n_rec, uint64_t *__restrict__ off, uint32_t *__restrict__ len,
                                                           MaskCounts *c) {
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
    const int clause = pf_mask::record_clause(text, b[pf_mask::LINE_HEADER], e[pf_mask::LINE_HEADER], e[pf_mask::LINE_SEQUENCE] - b[pf_mask::LINE_SEQUENCE],
                                              b[pf_mask::LINE_PLUS], e[pf_mask::LINE_PLUS], e[pf_mask::LINE_QUALITY] - b[pf_mask::LINE_QUALITY]);
    if (clause) atomicMin(&c->bad_entry, (unsigned long long)((r << 3) | (uint64_t)clause));
}

// ---- host side ----
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr uint64_t MASK_MAX_BYTES = 1ull << 40;   // every grid of a call stays far below 2^31 blocks

// all counters 0, no offender
static hipError_t mask_counts_reset(MaskCounts *dc, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(dc, 0, sizeof(MaskCounts), st);
    return e != hipSuccess ? e : hipMemsetAsync(&dc->bad_entry, 0xFF, sizeof dc->bad_entry, st);
}

// brackets everything one call launches as one timed launch of PF_K_MASK
struct MaskTimed {
    pf_ctx *ctx;
    explicit MaskTimed(pf_ctx *c) : ctx(c) { ctx_begin(ctx, PF_K_MASK); }
    ~MaskTimed() { ctx_end(ctx); }
};

// classes, flag, paint, changed over text[0, n) on the device with the table on the device; counts zeroed by the caller, n > 0
static int mask_core(pf_ctx *ctx, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t low,
                     uint32_t up, char *out, MaskCounts *counts) {
    const uint64_t n_tiles = (n + MASK_TILE - 1) / MASK_TILE;
    const uint64_t n_words = n_tiles * (MASK_TILE / 64);   // whole tiles: the flag phase writes every word of a tile
    const uint64_t n_units = (n + 15) / 16;
    uint64_t *bits = static_cast<uint64_t *>(ctx_ws(ctx, WS_MASK_BITS, (size_t)n_words * 8 * 4));
    if (!bits) return PF_ERR_HIP;
    uint64_t *seq = bits, *start = bits + n_words, *bad = bits + 2 * n_words, *changed = bits + 3 * n_words;
    k_mask_classes<<<ctx_grid(ctx, n_words, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(off, len, n_reads, n_words, (uint32_t)ctx->tab_k, seq,
                                                                                                      start, counts);
    MaskFlagArgs a;
    a.tab = ctx->d_tab;
    a.mask = ctx->tab_cap - 1;
    a.k = ctx->tab_k;
    a.exact = ctx->tab_exact ? 1 : 0;
    a.text = text;
    a.n = n;
    a.n_tiles = n_tiles;
    a.start = start;
    a.bad = bad;
    a.low = low;
    a.up = up;
    a.c = counts;
    k_mask_flag<<<ctx_grid(ctx, n_tiles * MASK_BLOCK, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(a);
    // (the last word of `changed` a read may touch lies inside the tiles; units beyond n_units are never read as changed bits:
    // zeroed so that the words are whole)
    PF_HIP(hipMemsetAsync(changed, 0, (size_t)n_words * 8, ctx->stream));
    k_mask_paint<<<ctx_grid(ctx, n_units, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(text, out, n, n_units, ctx->tab_k, seq, bad,
                                                                                                    reinterpret_cast<uint16_t *>(changed), counts);
    if (n_reads)
        k_mask_changed<<<ctx_grid(ctx, n_reads, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(off, len, n_reads, changed, counts);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-MASK launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    return PF_OK;
}

static int mask_needs_table(pf_ctx *ctx, const char *who) {
    if (ctx->d_tab && ctx->tab_cap && ctx->tab_k >= 3 && ctx->tab_k <= pf_mask::MAX_K) return PF_OK;
    pf::CtxErr{ctx} = std::string(who) + ": no count table is resident (pf_upload_counts comes first)";
    return PF_ERR_ARG;
}

// the text on the device, 16-byte aligned: the caller's own memory when it is that already, else a copy in a workspace
static int mask_stage_text(pf_ctx *ctx, const char *text, uint64_t n, const char **dev) {
    if (is_device_ptr(text) && ((uintptr_t)text & 15) == 0) { *dev = text; return PF_OK; }
    char *p = static_cast<char *>(ctx_ws(ctx, WS_MASK_TEXT, (size_t)n + 16));
    if (!p) return PF_ERR_HIP;
    PF_HIP(hipMemcpyAsync(p, text, (size_t)n, hipMemcpyDefault, ctx->stream));
    *dev = p;
    return PF_OK;
}

static void mask_stats_out(pf_mask_stats *stats, uint64_t n_reads, const MaskCounts &h) {
    if (!stats) return;
    stats->reads = n_reads;
    stats->reads_changed = h.reads_changed;
    stats->bases = h.bases;
    stats->bases_masked = h.bases_masked;
    stats->kmers = h.kmers;
    stats->kmers_bad = h.kmers_bad;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_mask_reads(pf_ctx *ctx, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len,
                             uint64_t n_reads, uint32_t low, uint32_t up, char *out, pf_mask_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = mask_needs_table(ctx, "pf_mask_reads"); if (rc) return rc; }
    if (n_bytes && (!text || !out)) return refuse("pf_mask_reads: text and out are needed");
    if (n_reads && (!read_off || !read_len)) return refuse("pf_mask_reads: read_off and read_len are needed");
    if (low > up) return refuse("pf_mask_reads: low " + std::to_string(low) + " is above up " + std::to_string(up));
    if (n_bytes && text == out) return refuse("pf_mask_reads: out may not alias text");
    if (((uintptr_t)read_off & 7) || ((uintptr_t)read_len & 3)) return refuse("pf_mask_reads: read_off / read_len are not aligned");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    if (n_bytes > MASK_MAX_BYTES) return refuse("pf_mask_reads: the text is longer than 2^40 bytes");
    if (n_bytes == 0 && n_reads == 0) { mask_stats_out(stats, 0, h); return PF_OK; }
    PF_HIP(hipSetDevice(ctx->device));
    MaskTimed timed(ctx);
    // the table and the counters
    const size_t off_bytes = up256((size_t)n_reads * 8), len_bytes = up256((size_t)n_reads * 4);
    char *tw = static_cast<char *>(ctx_ws(ctx, WS_MASK_TABLE, off_bytes + len_bytes + 256));
    if (!tw) return PF_ERR_HIP;
    MaskCounts *dc = reinterpret_cast<MaskCounts *>(tw + off_bytes + len_bytes);
    const uint64_t *doff = read_off;
    const uint32_t *dlen = read_len;
    if (n_reads && !is_device_ptr(read_off)) {
        PF_HIP(hipMemcpyAsync(tw, read_off, (size_t)n_reads * 8, hipMemcpyDefault, ctx->stream));
        doff = reinterpret_cast<const uint64_t *>(tw);
    }
    if (n_reads && !is_device_ptr(read_len)) {
        PF_HIP(hipMemcpyAsync(tw + off_bytes, read_len, (size_t)n_reads * 4, hipMemcpyDefault, ctx->stream));
        dlen = reinterpret_cast<const uint32_t *>(tw + off_bytes);
    }
    PF_HIP(mask_counts_reset(dc, ctx->stream));
    if (n_reads) {   // refused on the host before anything reads the text through the table
        k_mask_check_table<<<(unsigned)((n_reads + MASK_BLOCK - 1) / MASK_BLOCK), MASK_BLOCK, 0, ctx->stream>>>(doff, dlen, n_reads, n_bytes, dc);
        PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (h.bad_entry != MASK_NO_RECORD)
            return refuse("pf_mask_reads: read " + std::to_string(h.bad_entry) + " lies outside the text or overlaps the next one (the table is ascending)");
    }
    if (n_bytes == 0) { mask_stats_out(stats, n_reads, h); return PF_OK; }   // empty reads only: nothing to write
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    const bool out_direct = is_device_ptr(out) && ((uintptr_t)out & 15) == 0;
    char *dout = out;
    if (!out_direct) {
        dout = static_cast<char *>(ctx_ws(ctx, WS_MASK_OUT, (size_t)n_bytes + 16));
        if (!dout) return PF_ERR_HIP;
    }
    { const int rc = mask_core(ctx, dt, n_bytes, doff, dlen, n_reads, low, up, dout, dc); if (rc) return rc; }
    PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    if (!out_direct) PF_HIP(hipMemcpyAsync(out, dout, (size_t)n_bytes, hipMemcpyDefault, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    ctx_units(ctx, PF_K_MASK, h.kmers);
    mask_stats_out(stats, n_reads, h);
    return PF_OK;
}

extern "C" int pf_mask_fastq(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, char *out,
                             uint64_t *bytes_used, pf_mask_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = mask_needs_table(ctx, "pf_mask_fastq"); if (rc) return rc; }
    if (!bytes_used) return refuse("pf_mask_fastq: bytes_used is needed");
    if (n_bytes && (!text || !out)) return refuse("pf_mask_fastq: text and out are needed");
    if (low > up) return refuse("pf_mask_fastq: low " + std::to_string(low) + " is above up " + std::to_string(up));
    if (n_bytes && text == out) return refuse("pf_mask_fastq: out may not alias text");
    if (n_bytes > 0xFFFFFF00ull) return refuse("pf_mask_fastq: a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    *bytes_used = 0;
    if (bad_record) *bad_record = 0;
    mask_stats_out(stats, 0, h);
    if (n_bytes == 0) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    MaskTimed timed(ctx);
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    // newlines: bitmap, count per word, prefix
    const uint64_t n_words = (n_bytes + 63) / 64;
    const size_t nl_bytes = up256((size_t)n_words * 8), cnt_bytes = up256((size_t)n_words * 4), scr_bytes = up256(scan_scratch_bytes(n_words));
    char *iw = static_cast<char *>(ctx_ws(ctx, WS_MASK_INDEX, nl_bytes + 2 * cnt_bytes + scr_bytes + 256));
    if (!iw) return PF_ERR_HIP;
    uint64_t *nl = reinterpret_cast<uint64_t *>(iw);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(iw + nl_bytes), *pre = reinterpret_cast<uint32_t *>(iw + nl_bytes + cnt_bytes);
    void *scratch = iw + nl_bytes + 2 * cnt_bytes;
    MaskCounts *dc = reinterpret_cast<MaskCounts *>(iw + nl_bytes + 2 * cnt_bytes + scr_bytes);
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
    uint64_t used = final ? n_bytes : 0;
    if (n_rec) {
        const size_t ls_bytes = up256((size_t)(n_newlines + 2) * 4), off_bytes = up256((size_t)n_rec * 8), len_bytes = up256((size_t)n_rec * 4);
        char *tw = static_cast<char *>(ctx_ws(ctx, WS_MASK_TABLE, ls_bytes + off_bytes + len_bytes));
        if (!tw) return PF_ERR_HIP;
        uint32_t *line_start = reinterpret_cast<uint32_t *>(tw);
        uint64_t *doff = reinterpret_cast<uint64_t *>(tw + ls_bytes);
        uint32_t *dlen = reinterpret_cast<uint32_t *>(tw + ls_bytes + off_bytes);
        k_fq_line_starts<<<word_grid, MASK_BLOCK, 0, ctx->stream>>>(nl, pre, n_words, line_start);
        k_fq_records<<<(unsigned)((n_rec + MASK_BLOCK - 1) / MASK_BLOCK), MASK_BLOCK, 0, ctx->stream>>>(dt, n_bytes, line_start, n_newlines, n_rec, doff, dlen, dc);
        uint32_t end32 = 0;
        if (!final) PF_HIP(hipMemcpyAsync(&end32, line_start + 4 * n_rec, 4, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (h.bad_entry != MASK_NO_RECORD) {   // refused on the host, before anything is masked
            if (bad_record) *bad_record = h.bad_entry >> 3;
            return refuse(std::string("pf_mask_fastq: record ") + std::to_string(h.bad_entry >> 3) + " of the chunk: " + pf_mask::clause_text((int)(h.bad_entry & 7)));
        }
        if (!final) used = end32;
        if (final && n_lines % 4) {
            if (bad_record) *bad_record = n_rec;
            return refuse(std::string("pf_mask_fastq: record ") + std::to_string(n_rec) + " of the chunk: " + pf_mask::clause_text(pf_mask::CLAUSE_LINE_COUNT));
        }
        const bool out_direct = is_device_ptr(out) && ((uintptr_t)out & 15) == 0;
        char *dout = out;
        if (!out_direct) {
            dout = static_cast<char *>(ctx_ws(ctx, WS_MASK_OUT, (size_t)used + 16));
            if (!dout) return PF_ERR_HIP;
        }
        { const int rc = mask_core(ctx, dt, used, doff, dlen, n_rec, low, up, dout, dc); if (rc) return rc; }
        PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        if (!out_direct) PF_HIP(hipMemcpyAsync(out, dout, (size_t)used, hipMemcpyDefault, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    } else if (final && n_lines % 4) {
        if (bad_record) *bad_record = 0;
        return refuse(std::string("pf_mask_fastq: record 0 of the chunk: ") + pf_mask::clause_text(pf_mask::CLAUSE_LINE_COUNT));
    }   // (a final chunk of n_bytes > 0 holds at least one line: one of the two branches above was taken)
    *bytes_used = used;
    ctx_units(ctx, PF_K_MASK, h.kmers);
    mask_stats_out(stats, n_rec, h);
    return PF_OK;
}
