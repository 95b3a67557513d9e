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
// The class kernels, the tile and the FASTQ index are shared with K-COUNT: pf_reads_dev.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_mask_rule.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"

namespace pf {

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
        tile_stage(a.text, a.n, tile, tid, s_code, s_valid32);
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
                look[j] = tile_window_valid(s_valid32, p, k, all_k);
                if (look[j]) {
                    const uint64_t fwd = tile_kmer(s_code, p, k);
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

// ---- host side ----
// brackets everything one call launches as one timed launch of PF_K_MASK

// the flag phase alone over the resident table (K-MASKCOUNT launches it as well: pf_reads_dev.hpp)
void mask_flag_launch(pf_ctx *ctx, const char *text, uint64_t n, uint64_t n_tiles, const uint64_t *start, uint64_t *bad, uint32_t low, uint32_t up,
                      MaskCounts *counts) {
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
}

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
    mask_flag_launch(ctx, text, n, n_tiles, start, bad, low, up, counts);
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
    Timed timed(ctx, PF_K_MASK);
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
    Timed timed(ctx, PF_K_MASK);
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    FastqIndex ix;
    { const int rc = fastq_index(ctx, "pf_mask_fastq", dt, n_bytes, final, ix, bad_record); if (rc) return rc; }   // refused before anything is masked
    if (ix.n_rec) {
        const bool out_direct = is_device_ptr(out) && ((uintptr_t)out & 15) == 0;
        char *dout = out;
        if (!out_direct) {
            dout = static_cast<char *>(ctx_ws(ctx, WS_MASK_OUT, (size_t)ix.used + 16));
            if (!dout) return PF_ERR_HIP;
        }
        { const int rc = mask_core(ctx, dt, ix.used, ix.off, ix.len, ix.n_rec, low, up, dout, ix.counts); if (rc) return rc; }
        PF_HIP(hipMemcpyAsync(&h, ix.counts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        if (!out_direct) PF_HIP(hipMemcpyAsync(out, dout, (size_t)ix.used, hipMemcpyDefault, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    }   // (a final chunk of n_bytes > 0 holds at least one line: it has a record, or it was refused for its line count)
    *bytes_used = ix.used;
    ctx_units(ctx, PF_K_MASK, h.kmers);
    mask_stats_out(stats, ix.n_rec, h);
    return PF_OK;
}
