// K-MASKCOUNT: the second pass of `ploidyfrost run` over the reads -- `mask` followed by the count of `build` without the masked
// text: every window that would still hold k bases after K-MASK had painted its Ns is counted into the open count, straight from
// the unmasked text.  The rule is pf_run_rule.hpp; this file is its device form, a sibling of k_count_insert (pf_count.hip).
//
//   classes   k_mask_classes as K-MASK and K-COUNT run it: the window-start bitmap of the chunk (pf_reads_dev.hpp).
//   flag      k_mask_flag as it is (pf_mask.hip, mask_flag_launch): one look-up per window in the resident count table, one ballot
//             and one 8-byte store per 64 windows -- the bad bitmap.
//   insert    k_maskcount_insert.  K-COUNT's tile: 1024 bytes plus halo as 2-bit codes in LDS, four window starts a lane, 256
//             apart, so that a wavefront's 64 starts are one word of each bitmap.  Per group of 64 starts the wavefront reads its own
//             word of the bad bitmap and the two neighbours -- three broadcast loads, the same address in every lane -- and the
//             funnel of pf_run::clear_of_bad says whether any of the at most 61 bits around a start is set.  A survivor (a start
//             whose k bytes are bases and whose range is clear) is claimed and counted exactly as k_count_insert does it: CAS on the
//             key word, relaxed add on the count word, the same overflow and probe flags, the same load bound kept by the host.
//   traffic   per window, beside K-COUNT's byte of text and its table probe: 1/8 byte of start bitmap, 3/8 byte of bad bitmap read,
//             1/8 byte written by the flag phase, and the flag phase's own byte of text and probe of the resident table.  No paint,
//             no `changed` pass, no masked text (1 byte written and 1 byte read back per byte of the chunk), no second index.
// Statistics are ballots and popcounts kept per lane and summed per wavefront when the kernel ends: one atomic per wavefront.
// Everything one pf_maskcount_reads / pf_maskcount_fastq launches is timed as one launch of PF_K_MASKCOUNT; unit: windows.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_count_dev.hpp"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_run_rule.hpp"

namespace pf {

struct MaskCountArgs {
    CountSlot *tab;
    uint64_t mask;          // slots - 1
    int k;
    const char *text;
    uint64_t n;             // bytes of the text
    uint64_t n_tiles;
    const uint64_t *start;  // window-start bitmap, MASK_TILE / 64 words a tile
    const uint64_t *bad;    // bad-window bitmap of the flag phase, every word of every tile
    MaskCounts *c;          // kmers_invalid and kmers_kept of this call
    CountDev *d;
};

__global__ __launch_bounds__(MASK_BLOCK) void k_maskcount_insert(const MaskCountArgs a) {
    __shared__ uint32_t s_code[MASK_UNITS];
    __shared__ uint32_t s_valid32[MASK_UNITS / 2 + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    const uint64_t all_k = (1ull << k) - 1;
    const uint64_t n_words = a.n_tiles * (MASK_TILE / 64);
    uint64_t n_invalid = 0, n_kept = 0, claims = 0;
    bool overflow = false, stuck = false;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile has been read
        tile_stage(a.text, a.n, tile, tid, s_code, s_valid32);
        __syncthreads();
        const uint64_t word0 = tile * (MASK_TILE / 64) + (uint64_t)wave;
        uint64_t sw[MASK_PER_LANE], prev[MASK_PER_LANE], cur[MASK_PER_LANE], next[MASK_PER_LANE];
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {   // the same words for the whole wavefront, all asked for before the first is used
            const uint64_t w = word0 + (uint64_t)j * (MASK_BLOCK / 64);
            sw[j] = a.start[w];
            cur[j] = a.bad[w];
            prev[j] = w ? a.bad[w - 1] : 0ull;
            next[j] = w + 1 < n_words ? a.bad[w + 1] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {
            const bool is_start = (sw[j] >> lane) & 1ull;
            bool valid = false, counted = false;
            if (is_start) {
                const int p = j * MASK_BLOCK + tid;
                valid = tile_window_valid(s_valid32, p, k, all_k);
                counted = pf_run::survives(true, valid, prev[j], cur[j], next[j], lane, k);
                if (counted) {
                    const uint64_t key = pf_count::window_key(tile_kmer(s_code, p, k), k, true);
                    uint64_t slot = 0;
                    const int got = count_claim(a.tab, a.mask, key, slot);
                    if (got == 2) stuck = true;
                    else {
                        claims += (uint64_t)got;
                        if (atomicAdd(&a.tab[slot].count, 1u) == 0xFFFFFFFFu) overflow = true;
                    }
                }
            }
            const unsigned long long bi = __ballot(is_start && !valid), bk = __ballot(counted);
            if (lane == 0) {
                n_invalid += (uint64_t)__popcll(bi);
                n_kept += (uint64_t)__popcll(bk);
            }
        }
    }
    claims = wave_sum_u64(claims);
    if (lane == 0) {
        if (claims) atomicAdd(&a.d->occupied, (unsigned long long)claims);
        if (n_invalid) atomicAdd(&a.c->kmers_invalid, (unsigned long long)n_invalid);
        if (n_kept) atomicAdd(&a.c->kmers_kept, (unsigned long long)n_kept);
    }
    if (overflow) a.d->overflow = 1u;
    if (stuck) a.d->stuck = 1u;
}

// ---- host side ----

// a resident table, an open count on both strands, the same k: each missing piece by name
int maskcount_needs(pf_ctx *ctx, const char *who) {
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = std::string(who) + ": " + m; return (int)PF_ERR_ARG; };
    if (!(ctx->d_tab && ctx->tab_cap && ctx->tab_k >= 3 && ctx->tab_k <= pf_mask::MAX_K)) return refuse("no count table is resident (pf_upload_counts comes first)");
    const CountState *S = count_state(ctx);
    if (!S) return refuse("no count is open (pf_count_begin comes first)");
    if (S->k != ctx->tab_k)
        return refuse("the open count's k = " + std::to_string(S->k) + " differs from the count table's k = " + std::to_string(ctx->tab_k));
    if (!S->both_strands) return refuse("the open count is not on both strands (the k-mers of the masked reads are counted in canonical form)");
    return PF_OK;
}

// classes, flag and insert over text[0, n) on the device with the table of reads on the device; counts reset by the caller, n > 0
int maskcount_core(pf_ctx *ctx, CountState *S, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len, uint64_t n_reads,
                          uint32_t low, uint32_t up, MaskCounts *counts, MaskCounts &h) {
    { const int rc = count_reserve(ctx, S, n); if (rc) return rc; }
    const uint64_t n_tiles = (n + MASK_TILE - 1) / MASK_TILE;
    const uint64_t n_words = n_tiles * (MASK_TILE / 64);   // whole tiles: the flag phase writes every word of a tile, the insert phase reads them
    uint64_t *bits = static_cast<uint64_t *>(ctx_ws(ctx, WS_MASK_BITS, (size_t)n_words * 8 * 3));
    if (!bits) return PF_ERR_HIP;
    uint64_t *seq = bits, *start = bits + n_words, *bad = bits + 2 * n_words;
    k_mask_classes<<<ctx_grid(ctx, n_words, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(off, len, n_reads, n_words, (uint32_t)S->k, seq, start, counts);
    mask_flag_launch(ctx, text, n, n_tiles, start, bad, low, up, counts);
    MaskCountArgs a;
    a.tab = S->tab;
    a.mask = S->slots - 1;
    a.k = S->k;
    a.text = text;
    a.n = n;
    a.n_tiles = n_tiles;
    a.start = start;
    a.bad = bad;
    a.c = counts;
    a.d = S->dev;
    k_maskcount_insert<<<ctx_grid(ctx, n_tiles * MASK_BLOCK, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-MASKCOUNT launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    return count_after_insert(ctx, S, "K-MASKCOUNT", counts, h);
}

// this call's statistics, and its share of the totals pf_count_finish reports
void maskcount_stats_out(pf_maskcount_stats *stats, CountState *S, uint64_t n_reads, const MaskCounts &h) {
    pf_maskcount_stats st = {};
    st.reads = n_reads;
    st.bases = h.bases;
    st.kmers = h.kmers;
    st.kmers_invalid = h.kmers_invalid;
    st.kmers_bad = h.kmers_bad;
    st.kmers_kept = h.kmers_kept;
    if (S) {
        S->total.reads += st.reads;
        S->total.bases += st.bases;
        S->total.kmers += st.kmers;
        S->total.kmers_bad += st.kmers_invalid;
    }
    if (stats) *stats = st;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_maskcount_reads(pf_ctx *ctx, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len,
                                  uint64_t n_reads, uint32_t low, uint32_t up, pf_maskcount_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = maskcount_needs(ctx, "pf_maskcount_reads"); if (rc) return rc; }
    CountState *S = count_state(ctx);
    if (n_bytes && !text) return refuse("pf_maskcount_reads: text is needed");
    if (n_reads && (!read_off || !read_len)) return refuse("pf_maskcount_reads: read_off and read_len are needed");
    if (low > up) return refuse("pf_maskcount_reads: low " + std::to_string(low) + " is above up " + std::to_string(up));
    if (((uintptr_t)read_off & 7) || ((uintptr_t)read_len & 3)) return refuse("pf_maskcount_reads: read_off / read_len are not aligned");
    if (n_bytes > MASK_MAX_BYTES) return refuse("pf_maskcount_reads: the text is longer than 2^40 bytes");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    if (n_bytes == 0 && n_reads == 0) { maskcount_stats_out(stats, S, 0, h); return PF_OK; }
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_MASKCOUNT);
    // the table of reads and the counters
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
            return refuse("pf_maskcount_reads: read " + std::to_string(h.bad_entry) + " lies outside the text or overlaps the next one (the table is ascending)");
    }
    if (n_bytes == 0) { maskcount_stats_out(stats, S, n_reads, h); return PF_OK; }   // empty reads only
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    { const int rc = maskcount_core(ctx, S, dt, n_bytes, doff, dlen, n_reads, low, up, dc, h); if (rc) return rc; }
    ctx_units(ctx, PF_K_MASKCOUNT, h.kmers);
    maskcount_stats_out(stats, S, n_reads, h);
    return PF_OK;
}

extern "C" int pf_maskcount_fastq(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, uint64_t *bytes_used,
                                  pf_maskcount_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = maskcount_needs(ctx, "pf_maskcount_fastq"); if (rc) return rc; }
    CountState *S = count_state(ctx);
    if (!bytes_used) return refuse("pf_maskcount_fastq: bytes_used is needed");
    if (n_bytes && !text) return refuse("pf_maskcount_fastq: text is needed");
    if (low > up) return refuse("pf_maskcount_fastq: low " + std::to_string(low) + " is above up " + std::to_string(up));
    if (n_bytes > 0xFFFFFF00ull) return refuse("pf_maskcount_fastq: a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    *bytes_used = 0;
    if (bad_record) *bad_record = 0;
    if (n_bytes == 0) { maskcount_stats_out(stats, S, 0, h); return PF_OK; }
    if (stats) *stats = pf_maskcount_stats{};
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_MASKCOUNT);
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    FastqIndex ix;
    { const int rc = fastq_index(ctx, "pf_maskcount_fastq", dt, n_bytes, final, ix, bad_record); if (rc) return rc; }   // refused before anything is counted
    if (ix.n_rec) {
        const int rc = maskcount_core(ctx, S, dt, ix.used, ix.off, ix.len, ix.n_rec, low, up, ix.counts, h);
        if (rc) return rc;
    }
    *bytes_used = ix.used;
    ctx_units(ctx, PF_K_MASKCOUNT, h.kmers);
    maskcount_stats_out(stats, S, ix.n_rec, h);
    return PF_OK;
}
