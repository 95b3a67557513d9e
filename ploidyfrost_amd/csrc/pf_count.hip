// K-COUNT: `kmc -k<k> -ci<ci> -cs<cs> -cx<cx> [-b] <reads.fq>` (step `2.kmc_db` of the reference's workflow) on the device -- every
// window of every read counted into an open-addressing table in HBM, the kept counters compacted and sorted into the array pair
// (kmers, counts) that pf_kmc_decode returns.  The rule is pf_count_rule.hpp; this file is its device form.
//
//   table     one 16-byte slot { u64 key, u32 count, u32 pad }: a probe touches one sector.  A power of two of slots, the slot from
//             mix64(key), 64-bit slot indices, linear probing; cleared to key = ~0, count = 0 (~0 is no key: k <= 31).
//   insert    k_count_insert.  The unit of work is a byte of the text (a window start), as in K-MASK: class bitmaps from the read
//             table, a tile of 1024 bytes plus halo as 2-bit codes in LDS, one k-mer per lane (pf_reads_dev.hpp).  Per counted
//             window: atomicCAS ~0 -> key on the key word until the key's own slot or an empty one is found, then a relaxed
//             atomicAdd of 1 on the count word.  No fence: counts start at 0 and integer sums commute, and nobody reads a count
//             before the kernel has ended.  An add that returns 0xFFFFFFFF has wrapped the counter: it sets the overflow flag, which
//             pf_count_finish turns into the refusal (unreachable at test sizes; checked by reading).
//   invariant before each launch the host makes sure that occupied + bytes of the call <= 3/4 slots (the bytes bound the windows, the
//             windows bound the new keys), growing the table first when that does not hold: a probe always meets an empty slot.  The
//             probe loop is bounded by the slot count all the same and sets an error flag instead of spinning.
//   occupied  exact: new claims are counted per lane and summed per wavefront, one atomic per resident wavefront when the kernel ends
//             (DESIGN, K-MASK "Statistics"); kmers_bad (windows holding a non-base) by ballot and popcount the same way.
//   growth    k_count_rehash, one thread per old slot: keys are distinct, so a CAS claims the slot and a plain store of the count
//             follows.  Refused by name, with the number of distinct k-mers reached, when the new table does not fit beside the old.
//   finish    k_count_flag (one ballot per 64 slots: the kept bitmap and its popcounts), an exclusive scan (pf_scan.hpp),
//             k_count_compact (counts = min(c, cs)), rocprim::radix_sort_pairs over bits [0, 2k).  The result depends on the multiset
//             of windows only: the same bits on every run, whatever the chunking and the atomics' arrival order.
//   encode    k_kmc_encode / k_kmc_lut, the inverse of K-KMC: the record area and the prefix table of a KMC1 database.
// Everything one pf_count_reads / pf_count_fastq launches is timed as one launch of PF_K_COUNT; unit: windows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_count_dev.hpp"
#include "pf_count_rule.hpp"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"

namespace pf {

// ---- table ----
__global__ __launch_bounds__(256) void k_count_clear(CountSlot *tab, uint64_t slots) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256)
        *reinterpret_cast<uint4 *>(tab + s) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
}

// ---- insert ----
struct CountInsertArgs {
    CountSlot *tab;
    uint64_t mask;          // slots - 1
    int k;
    int both_strands;
    const char *text;
    uint64_t n;             // bytes of the text
    uint64_t n_tiles;
    const uint64_t *start;  // window-start bitmap, MASK_TILE / 64 words a tile
    MaskCounts *c;          // kmers_bad of this call
    CountDev *d;
};

__global__ __launch_bounds__(MASK_BLOCK) void k_count_insert(const CountInsertArgs a) {
    __shared__ uint32_t s_code[MASK_UNITS];
    __shared__ uint32_t s_valid32[MASK_UNITS / 2 + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    const uint64_t all_k = (1ull << k) - 1;
    uint64_t n_bad = 0, claims = 0;
    bool overflow = false, stuck = false;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile has been read
        tile_stage(a.text, a.n, tile, tid, s_code, s_valid32);
        __syncthreads();
        const uint64_t word0 = tile * (MASK_TILE / 64) + (uint64_t)wave;
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {
            const uint64_t sw = a.start[word0 + (uint64_t)j * (MASK_BLOCK / 64)];   // the same word for the whole wavefront
            const bool is_start = (sw >> lane) & 1ull;
            bool counted = false;
            if (is_start) {
                const int p = j * MASK_BLOCK + tid;
                counted = tile_window_valid(s_valid32, p, k, all_k);
                if (counted) {
                    const uint64_t key = pf_count::window_key(tile_kmer(s_code, p, k), k, a.both_strands != 0);
                    uint64_t slot = 0;
                    const int got = count_claim(a.tab, a.mask, key, slot);
                    if (got == 2) stuck = true;
                    else {
                        claims += (uint64_t)got;
                        if (atomicAdd(&a.tab[slot].count, 1u) == 0xFFFFFFFFu) overflow = true;
                    }
                }
            }
            const unsigned long long bw = __ballot(is_start && !counted);
            if (lane == 0) n_bad += (uint64_t)__popcll(bw);
        }
    }
    claims = wave_sum_u64(claims);
    if (lane == 0) {
        if (claims) atomicAdd(&a.d->occupied, (unsigned long long)claims);
        if (n_bad) atomicAdd(&a.c->kmers_bad, (unsigned long long)n_bad);
    }
    if (overflow) a.d->overflow = 1u;
    if (stuck) a.d->stuck = 1u;
}

// ---- growth ----
__global__ __launch_bounds__(256) void k_count_rehash(const CountSlot *__restrict__ old_tab, uint64_t old_slots, CountSlot *tab, uint64_t mask, CountDev *d) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(old_tab + i);
        const uint64_t key = ((uint64_t)v.y << 32) | v.x;
        if (key == pf_count::EMPTY_KEY) continue;
        uint64_t slot = 0;
        if (count_claim(tab, mask, key, slot) == 2) d->stuck = 1u;
        else tab[slot].count = v.z;   // a fresh slot of a distinct key: nobody else writes it
    }
}

// ---- finish ----
// one wavefront per 64 slots: bit l of kept[w] = slot 64 w + l holds a key whose counter lies in [ci, cx]
__global__ __launch_bounds__(256) void k_count_flag(const CountSlot *__restrict__ tab, uint64_t slots, uint32_t ci, uint32_t cx, uint64_t *__restrict__ kept,
                                                    uint32_t *__restrict__ cnt, CountDev *d) {
    const int lane = lane_id();
    uint64_t unique = 0, below = 0, above = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {   // (slots is a multiple of 64)
        const uint4 v = *reinterpret_cast<const uint4 *>(tab + s);
        const bool used = (((uint64_t)v.y << 32) | v.x) != pf_count::EMPTY_KEY;
        const unsigned long long bu = __ballot(used), bl = __ballot(used && v.z < ci), ba = __ballot(used && v.z > cx);
        if (lane == 0) {
            const unsigned long long bk = bu & ~bl & ~ba;
            kept[s >> 6] = bk;
            cnt[s >> 6] = (uint32_t)__popcll(bk);
            unique += (uint64_t)__popcll(bu);
            below += (uint64_t)__popcll(bl);
            above += (uint64_t)__popcll(ba);
        }
    }
    if (lane == 0) {
        if (unique) atomicAdd(&d->unique, (unsigned long long)unique);
        if (below) atomicAdd(&d->below, (unsigned long long)below);
        if (above) atomicAdd(&d->above, (unsigned long long)above);
    }
}

__global__ __launch_bounds__(256) void k_count_compact(const CountSlot *__restrict__ tab, uint64_t slots, uint32_t cs, const uint64_t *__restrict__ kept,
                                                       const uint64_t *__restrict__ pre, uint64_t *__restrict__ kmers, uint32_t *__restrict__ counts) {
    const int lane = lane_id();
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
        const uint64_t w = kept[s >> 6];
        if (!((w >> lane) & 1ull)) continue;
        const uint4 v = *reinterpret_cast<const uint4 *>(tab + s);
        const uint64_t at = pre[s >> 6] + (uint64_t)__popcll(w & ((1ull << lane) - 1));
        kmers[at] = ((uint64_t)v.y << 32) | v.x;
        counts[at] = pf_count::stored(v.z, cs);
    }
}

// ---- encode ----
__global__ __launch_bounds__(256) void k_kmc_encode(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ counts, uint64_t n, int k, int p,
                                                    uint32_t counter_bytes, uint8_t *__restrict__ out) {
    const uint64_t rb = pf_count::suffix_bytes(k, p) + counter_bytes;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        pf_count::encode_record(kmers[i], counts[i], k, p, counter_bytes, out + i * rb);
}
// lut[e] = the first record whose k-mer is not below the first key of entry e; lut[n_lut] = n
__global__ __launch_bounds__(256) void k_kmc_lut(const uint64_t *__restrict__ kmers, uint64_t n, int k, int p, uint64_t n_lut, uint64_t *__restrict__ lut) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e <= n_lut; e += (uint64_t)gridDim.x * 256) {
        uint64_t a = 0, b = n;
        if (e < n_lut) {
            const uint64_t first = pf_count::lut_first_key(e, k, p);
            while (a < b) {
                const uint64_t m = (a + b) >> 1;
                if (kmers[m] < first) a = m + 1; else b = m;
            }
        } else a = n;
        lut[e] = a;
    }
}

// ---- host side ----

void count_destroy(pf_ctx *ctx) {
    CountState *S = count_state(ctx);
    if (!S) return;
    (void)hipFree(S->tab);
    (void)hipFree(S->dev);
    delete S;
    ctx->count = nullptr;
}

static uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = COUNT_MIN_SLOTS;
    while (p < x) p <<= 1;
    return p;
}

static int count_alloc_table(pf_ctx *ctx, const CountState *S, uint64_t slots, CountSlot **out) {
    size_t free_b = 0, total_b = 0;
    PF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (slots > (1ull << 40) || slots * sizeof(CountSlot) > free_b) {
        pf::CtxErr{ctx} = "pf_count: the count table of " + std::to_string(slots) + " slots (" + std::to_string(slots * sizeof(CountSlot)) +
                          " bytes)" + (S->tab ? " does not fit beside the old one" : " does not fit") + " in the free device memory (" +
                          std::to_string(free_b) + " bytes) at " + std::to_string(S->occupied) + " distinct k-mers";
        return PF_ERR_OVERFLOW;
    }
    CountSlot *t = nullptr;
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&t), slots * sizeof(CountSlot)));
    k_count_clear<<<ctx_grid(ctx, slots, 256, 8), 256, 0, ctx->stream>>>(t, slots);
    *out = t;
    return PF_OK;
}

// the invariant: occupied + add <= 3/4 slots before a launch that can claim `add` slots
int count_reserve(pf_ctx *ctx, CountState *S, uint64_t add) {
    uint64_t want = S->tab ? S->slots : (S->initial_slots ? S->initial_slots : pow2_at_least(2 * add));
    while (S->occupied + add > want / 4 * 3) want <<= 1;
    if (S->tab && want == S->slots) return PF_OK;
    CountSlot *t = nullptr;
    { const int rc = count_alloc_table(ctx, S, want, &t); if (rc) return rc; }
    if (S->tab) {   // (one rehash into the size that holds the bound, not a chain of doublings)
        k_count_rehash<<<ctx_grid(ctx, S->slots, 256, 8), 256, 0, ctx->stream>>>(S->tab, S->slots, t, want - 1, S->dev);
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipFree(t); pf::CtxErr{ctx} = std::string("K-COUNT rehash: ") + hipGetErrorString(e); return PF_ERR_HIP; }
        (void)hipFree(S->tab);
    }
    S->tab = t;
    S->slots = want;
    return PF_OK;
}

// classes and insert over text[0, n) on the device with the table of reads on the device; counts reset by the caller, n > 0
int count_core(pf_ctx *ctx, CountState *S, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len, uint64_t n_reads,
                      MaskCounts *counts, MaskCounts &h) {
    { const int rc = count_reserve(ctx, S, n); if (rc) return rc; }
    const uint64_t n_tiles = (n + MASK_TILE - 1) / MASK_TILE;
    const uint64_t n_words = n_tiles * (MASK_TILE / 64);   // whole tiles: the insert phase reads every word of a tile
    uint64_t *bits = static_cast<uint64_t *>(ctx_ws(ctx, WS_MASK_BITS, (size_t)n_words * 8 * 2));
    if (!bits) return PF_ERR_HIP;
    uint64_t *seq = bits, *start = bits + n_words;
    k_mask_classes<<<ctx_grid(ctx, n_words, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(off, len, n_reads, n_words, (uint32_t)S->k, seq, start, counts);
    CountInsertArgs a;
    a.tab = S->tab;
    a.mask = S->slots - 1;
    a.k = S->k;
    a.both_strands = S->both_strands ? 1 : 0;
    a.text = text;
    a.n = n;
    a.n_tiles = n_tiles;
    a.start = start;
    a.c = counts;
    a.d = S->dev;
    k_count_insert<<<ctx_grid(ctx, n_tiles * MASK_BLOCK, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-COUNT launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    return count_after_insert(ctx, S, "K-COUNT", counts, h);
}

int count_after_insert(pf_ctx *ctx, CountState *S, const char *who, MaskCounts *counts, MaskCounts &h) {
    CountDev d = {};
    PF_HIP(hipMemcpyAsync(&h, counts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&d, S->dev, sizeof d, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    S->occupied = d.occupied;
    if (d.stuck) { pf::CtxErr{ctx} = std::string(who) + ": a probe went round the whole table (the load bound was broken)"; return PF_ERR_HIP; }
    return PF_OK;
}

void count_stats_out(pf_count_stats *stats, CountState *S, uint64_t n_reads, const MaskCounts &h) {
    pf_count_stats st = {};
    st.reads = n_reads;
    st.bases = h.bases;
    st.kmers = h.kmers;
    st.kmers_bad = h.kmers_bad;
    if (S) {
        S->total.reads += st.reads;
        S->total.bases += st.bases;
        S->total.kmers += st.kmers;
        S->total.kmers_bad += st.kmers_bad;
    }
    if (stats) *stats = st;
}

int count_needs_begin(pf_ctx *ctx, const char *who) {
    if (ctx->count) return PF_OK;
    pf::CtxErr{ctx} = std::string(who) + ": no count is open (pf_count_begin comes first)";
    return PF_ERR_ARG;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_count_begin(pf_ctx *ctx, uint32_t k, int both_strands, uint64_t initial_slots) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (ctx->count) return refuse("pf_count_begin: a count is open already (pf_count_finish or pf_count_abort comes first)");
    if (!pf_count::k_ok(k)) return refuse("pf_count_begin: k = " + std::to_string(k) + ": " + pf_count::cut_text(pf_count::CUT_K));
    if (initial_slots > (1ull << 40)) return refuse("pf_count_begin: initial_slots is above 2^40");
    PF_HIP(hipSetDevice(ctx->device));
    CountState *S = new CountState;
    S->k = (int)k;
    S->both_strands = both_strands != 0;
    S->initial_slots = initial_slots ? pow2_at_least(initial_slots) : 0;
    if (hipMalloc(reinterpret_cast<void **>(&S->dev), sizeof(CountDev)) != hipSuccess || hipMemsetAsync(S->dev, 0, sizeof(CountDev), ctx->stream) != hipSuccess) {
        (void)hipFree(S->dev);
        delete S;
        pf::CtxErr{ctx} = "pf_count_begin: hipMalloc of the counters failed";
        return PF_ERR_HIP;
    }
    ctx->count = S;
    return PF_OK;
}

extern "C" int pf_count_abort(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    count_destroy(ctx);
    return PF_OK;
}

extern "C" int pf_count_reads(pf_ctx *ctx, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len, uint64_t n_reads,
                              pf_count_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = count_needs_begin(ctx, "pf_count_reads"); if (rc) return rc; }
    CountState *S = count_state(ctx);
    if (n_bytes && !text) return refuse("pf_count_reads: text is needed");
    if (n_reads && (!read_off || !read_len)) return refuse("pf_count_reads: read_off and read_len are needed");
    if (((uintptr_t)read_off & 7) || ((uintptr_t)read_len & 3)) return refuse("pf_count_reads: read_off / read_len are not aligned");
    if (n_bytes > MASK_MAX_BYTES) return refuse("pf_count_reads: the text is longer than 2^40 bytes");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    if (n_bytes == 0 && n_reads == 0) { count_stats_out(stats, S, 0, h); return PF_OK; }
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_COUNT);
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
            return refuse("pf_count_reads: read " + std::to_string(h.bad_entry) + " lies outside the text or overlaps the next one (the table is ascending)");
    }
    if (n_bytes == 0) { count_stats_out(stats, S, n_reads, h); return PF_OK; }   // empty reads only
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    { const int rc = count_core(ctx, S, dt, n_bytes, doff, dlen, n_reads, dc, h); if (rc) return rc; }
    ctx_units(ctx, PF_K_COUNT, h.kmers);
    count_stats_out(stats, S, n_reads, h);
    return PF_OK;
}

extern "C" int pf_count_fastq(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_count_stats *stats,
                              uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = count_needs_begin(ctx, "pf_count_fastq"); if (rc) return rc; }
    CountState *S = count_state(ctx);
    if (!bytes_used) return refuse("pf_count_fastq: bytes_used is needed");
    if (n_bytes && !text) return refuse("pf_count_fastq: text is needed");
    if (n_bytes > 0xFFFFFF00ull) return refuse("pf_count_fastq: a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    MaskCounts h = {};
    h.bad_entry = MASK_NO_RECORD;
    *bytes_used = 0;
    if (bad_record) *bad_record = 0;
    if (n_bytes == 0) { count_stats_out(stats, S, 0, h); return PF_OK; }
    if (stats) *stats = pf_count_stats{};
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_COUNT);
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    FastqIndex ix;
    { const int rc = fastq_index(ctx, "pf_count_fastq", dt, n_bytes, final, ix, bad_record); if (rc) return rc; }   // refused before anything is counted
    if (ix.n_rec) {
        const int rc = count_core(ctx, S, dt, ix.used, ix.off, ix.len, ix.n_rec, ix.counts, h);
        if (rc) return rc;
    }
    *bytes_used = ix.used;
    ctx_units(ctx, PF_K_COUNT, h.kmers);
    count_stats_out(stats, S, ix.n_rec, h);
    return PF_OK;
}

extern "C" int pf_count_finish(pf_ctx *ctx, uint64_t ci, uint64_t cx, uint64_t cs, uint64_t **kmers_dev, uint32_t **counts_dev, uint64_t *n,
                               pf_count_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = count_needs_begin(ctx, "pf_count_finish"); if (rc) return rc; }
    if (!kmers_dev || !counts_dev || !n) return refuse("pf_count_finish: kmers_dev, counts_dev and n are needed");
    { const int c = pf_count::cut_clause(ci, cx, cs); if (c) return refuse(std::string("pf_count_finish: ") + pf_count::cut_text(c)); }
    CountState *S = count_state(ctx);
    *kmers_dev = nullptr;
    *counts_dev = nullptr;
    *n = 0;
    PF_HIP(hipSetDevice(ctx->device));
    struct Closer { pf_ctx *c; ~Closer() { count_destroy(c); } } closer{ctx};   // the count is closed on every path from here
    pf_count_stats st = S->total;
    CountDev d = {};
    uint64_t written = 0;
    DevTmp<uint64_t> kept, pre, k0;
    DevTmp<uint32_t> cnt, c0;
    DevTmp<uint8_t> scratch;
    if (S->tab) {
        const uint64_t n_words = S->slots / 64;
        PF_HIP(kept.alloc(n_words * 8));
        PF_HIP(pre.alloc(n_words * 8));
        PF_HIP(cnt.alloc(n_words * 4));
        PF_HIP(scratch.alloc(scan_scratch_bytes(n_words)));
        k_count_flag<<<ctx_grid(ctx, S->slots, 256, 8), 256, 0, ctx->stream>>>(S->tab, S->slots, (uint32_t)ci, (uint32_t)cx, kept.p, cnt.p, S->dev);
        PF_HIP(scan_exclusive_u32_u64(cnt.p, pre.p, n_words, scratch.p, ctx->stream));
        uint64_t last_pre = 0;
        uint32_t last_cnt = 0;
        PF_HIP(hipMemcpyAsync(&last_pre, pre.p + (n_words - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipMemcpyAsync(&last_cnt, cnt.p + (n_words - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipMemcpyAsync(&d, S->dev, sizeof d, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        written = last_pre + last_cnt;
    }
    if (d.overflow) { pf::CtxErr{ctx} = std::string("pf_count_finish: ") + pf_count::OVERFLOW_TEXT; return PF_ERR_OVERFLOW; }
    uint64_t *dk = nullptr;
    uint32_t *dcn = nullptr;
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&dk), written ? written * 8 : 8));
    if (hipMalloc(reinterpret_cast<void **>(&dcn), written ? written * 4 : 4) != hipSuccess) {
        (void)hipFree(dk);
        pf::CtxErr{ctx} = "pf_count_finish: hipMalloc of the counts failed";
        return PF_ERR_HIP;
    }
    hipError_t e = hipSuccess;
    if (written) {
        e = k0.alloc(written * 8);
        if (e == hipSuccess) e = c0.alloc(written * 4);
        if (e == hipSuccess) {
            k_count_compact<<<ctx_grid(ctx, S->slots, 256, 8), 256, 0, ctx->stream>>>(S->tab, S->slots, (uint32_t)cs, kept.p, pre.p, k0.p, c0.p);
            e = hipGetLastError();
        }
        size_t need = 0;
        DevTmp<uint8_t> sort_tmp;
        if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, need, k0.p, dk, c0.p, dcn, (size_t)written, 0, 2 * (unsigned)S->k, ctx->stream);
        if (e == hipSuccess) e = sort_tmp.alloc(need);
        if (e == hipSuccess) e = rocprim::radix_sort_pairs(sort_tmp.p, need, k0.p, dk, c0.p, dcn, (size_t)written, 0, 2 * (unsigned)S->k, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        (void)hipFree(dk);
        (void)hipFree(dcn);
        pf::CtxErr{ctx} = std::string("pf_count_finish: ") + hipGetErrorString(e);
        return PF_ERR_HIP;
    }
    st.unique = d.unique;
    st.below_min = d.below;
    st.above_max = d.above;
    st.written = written;
    if (stats) *stats = st;
    *kmers_dev = dk;
    *counts_dev = dcn;
    *n = written;
    return PF_OK;
}

extern "C" int pf_kmc_encode(pf_ctx *ctx, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lut_prefix_len,
                             uint32_t counter_bytes, uint8_t *records_out, uint64_t *lut_out) {
    if (!ctx) return PF_ERR_ARG;
    if (!pf_count::k_ok(k) || lut_prefix_len == 0 || lut_prefix_len > 15 || lut_prefix_len >= k || (k - lut_prefix_len) % 4 || counter_bytes == 0 ||
        counter_bytes > 4 || (n && (!kmers || (records_out && !counts)))) {
        pf::CtxErr{ctx} = "pf_kmc_encode: inconsistent k / lut_prefix_len / counter_bytes, or arrays missing";
        return PF_ERR_ARG;
    }
    PF_HIP(hipSetDevice(ctx->device));
    DevTmp<uint64_t> tk, tl;
    DevTmp<uint32_t> tc;
    DevTmp<uint8_t> tr;
    if (n && !is_device_ptr(kmers)) {
        PF_HIP(tk.alloc(n * 8));
        PF_HIP(hipMemcpyAsync(tk.p, kmers, n * 8, hipMemcpyDefault, ctx->stream));
        kmers = tk.p;
    }
    if (n && records_out) {
        if (!is_device_ptr(counts)) {
            PF_HIP(tc.alloc(n * 4));
            PF_HIP(hipMemcpyAsync(tc.p, counts, n * 4, hipMemcpyDefault, ctx->stream));
            counts = tc.p;
        }
        const size_t bytes = (size_t)n * (pf_count::suffix_bytes((int)k, (int)lut_prefix_len) + counter_bytes);
        uint8_t *dr = records_out;
        if (!is_device_ptr(records_out)) {
            PF_HIP(tr.alloc(bytes));
            dr = tr.p;
        }
        k_kmc_encode<<<ctx_grid(ctx, n, 256, 8), 256, 0, ctx->stream>>>(kmers, counts, n, (int)k, (int)lut_prefix_len, counter_bytes, dr);
        if (dr != records_out) PF_HIP(hipMemcpyAsync(records_out, dr, bytes, hipMemcpyDefault, ctx->stream));
    }
    if (lut_out) {
        const uint64_t n_lut = 1ull << (2 * lut_prefix_len);
        uint64_t *dl = lut_out;
        if (!is_device_ptr(lut_out)) {
            PF_HIP(tl.alloc((n_lut + 1) * 8));
            dl = tl.p;
        }
        k_kmc_lut<<<ctx_grid(ctx, n_lut + 1, 256, 8), 256, 0, ctx->stream>>>(kmers, n, (int)k, (int)lut_prefix_len, n_lut, dl);
        if (dl != lut_out) PF_HIP(hipMemcpyAsync(lut_out, dl, (n_lut + 1) * 8, hipMemcpyDefault, ctx->stream));
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-KMC-ENCODE launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}
