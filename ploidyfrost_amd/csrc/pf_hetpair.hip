// K-HETPAIR: the heterozygous k-mer pairs of a Smudgeplot-style analysis from the count table that is already in HBM -- all pairs of
// distinct canonical k-mers one substitution apart, both with a counter in [lo, hi] and neither with another such neighbour, and the
// table of their two coverages.  The rule is pf_hetpair_rule.hpp; this file is its device form.
//   flag      k_hetpair_flag.  A wavefront takes 64 neighbouring keys at a time (one coalesced load of keys and counters), a ballot
//             names the keys in range, and its four rows of 16 lanes take them four at a time: keys outside [lo, hi] -- most distinct
//             k-mers of real reads are errors below lo -- cost their load and nothing else.  The lanes of a row split the 3k
//             substitutions, three probes in flight a lane (count_probe_at / count_finish, the exact-key look-up of K-MASK), each
//             lane keeps "first partner / a different second partner" (pf_hetpair::Degree) and a butterfly over the row merges them.
//             A row that ends with exactly one partner y > x computes degree(y) the same way: the mutual test, with no second array
//             and no sorted input.  The row's verdict goes into one 64-bit word a wavefront (bit i: key 64 w + i is the x of a
//             pair), the partner and its counter to the key's place in two scratch arrays.
//   scan      the words' popcounts, exclusive, in 64 bits (pf_scan.hpp); the host reads the total and allocates the results.
//   write     k_hetpair_write, one thread a key: place = the word's offset + the popcount of the lower bits.  Count / scan / write
//             as K-UNION and K-FASTA do it: no atomic decides an order, the pairs follow the keys.
//   table     k_hetpair_table over the compacted counters.  In a diploid nearly all pairs fall into a few dozen cells around
//             (n, n): the lanes of a wavefront that hold the first active lane's cell are counted by one ballot (K-HIST's
//             combining), the others add into a block-private tile in LDS -- TABLE_SLOTS direct-mapped (cell, count) slots claimed by
//             compare-and-swap, a lane that finds its slot taken by another cell adds to HBM -- flushed with one u64 atomic a used
//             slot when the block ends.
// Statistics are kept per lane and summed per wavefront when the kernel ends: one integer atomic per statistic and resident
// wavefront.  Integer atomics only: the same bits on every call.  Everything of one call is timed as one launch of PF_K_HETPAIR;
// unit: keys in range.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_hetpair_rule.hpp"
#include "pf_scan.hpp"

namespace pf {

constexpr int HP_BLOCK = 256;
constexpr int HP_PER_CU = 3;                 // blocks a CU holds at 154 VGPRs (three wavefronts a SIMD): the grid is the resident wavefronts
constexpr int HP_ROW = 16;                 // lanes a key
constexpr int HP_ROWS = WAVE / HP_ROW;     // keys a wavefront works on at once
constexpr int HP_FLIGHT = 3;               // probes in flight a lane
constexpr uint32_t TABLE_SLOTS = 4096;     // (cell, count) slots of the table kernel's tile: 32 KB of LDS

struct HetCounts {
    unsigned long long in_range, one_partner, many_partners, pairs;
};

struct HetFlagArgs {
    const CountLine *tab;
    uint64_t mask;
    int k;
    const uint64_t *kmers;
    const uint32_t *counts;
    uint64_t n, n_words;
    uint32_t lo, hi;
    uint64_t *word;        // out: n_words pair bitmaps
    uint32_t *word_pairs;  // out: their popcounts
    uint64_t *partner;     // out, may be null: y at the place of x, pair keys only
    uint32_t *partner_cov; // out, may be null
    HetCounts *c;
};

__device__ inline uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, HP_ROW);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, HP_ROW);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, WAVE);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// degree of x over the row this lane belongs to; every lane of the wavefront calls it, rows with !on probe nothing.  All lanes of a
// row return the same degree(), and the same first partner when it is 1.
__device__ inline pf_hetpair::Degree row_degree(const HetFlagArgs &a, uint64_t x, bool on, int row_lane) {
    pf_hetpair::Degree d;
    const int n_sub = 3 * a.k;
    for (int base = 0; base < n_sub; base += HP_ROW * HP_FLIGHT) {   // wave-uniform
        CountProbe pr[HP_FLIGHT];
        uint64_t y[HP_FLIGHT];
        bool look[HP_FLIGHT];
#pragma unroll
        for (int f = 0; f < HP_FLIGHT; ++f) {
            const int j = base + f * HP_ROW + row_lane;
            look[f] = on && j < n_sub;
            y[f] = 0;
            if (look[f]) {
                const uint64_t fwd = pf_hetpair::substituted(x, a.k, j);
                const uint64_t rc = rc_kmer(fwd, a.k);
                y[f] = rc < fwd ? rc : fwd;
                look[f] = y[f] != x;
                if (look[f]) count_probe_at(a.tab, y[f], kmer_lines(fwd, rc, a.k, a.mask), pr[f]);
            }
        }
#pragma unroll
        for (int f = 0; f < HP_FLIGHT; ++f) {
            if (!look[f]) continue;
            uint32_t got = 0;
            const bool present = count_finish(a.tab, a.mask, pr[f], got);
            if (pf_hetpair::is_partner(x, y[f], present, got, a.lo, a.hi)) d.add(y[f], got);
        }
    }
#pragma unroll
    for (int m = HP_ROW / 2; m > 0; m >>= 1) {
        pf_hetpair::Degree o;
        o.first = shfl_xor_u64(d.first, m);
        o.cov = (uint32_t)__shfl_xor((int)d.cov, m, HP_ROW);
        o.many = (uint32_t)__shfl_xor((int)d.many, m, HP_ROW);
        d.merge(o);
    }
    return d;
}

__global__ __launch_bounds__(HP_BLOCK) void k_hetpair_flag(const HetFlagArgs a) {
    const int lane = lane_id(), row = lane / HP_ROW, row_lane = lane % HP_ROW;
    const uint64_t wave0 = (uint64_t)blockIdx.x * (HP_BLOCK / WAVE) + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), n_waves = (uint64_t)gridDim.x * (HP_BLOCK / WAVE);
    uint64_t n_in = 0, n_one = 0, n_many = 0, n_pairs = 0;   // per lane; summed per wavefront when the kernel ends
    for (uint64_t w = wave0; w < a.n_words; w += n_waves) {
        const uint64_t i = w * WAVE + (uint64_t)lane;
        uint64_t key = 0;
        uint32_t cnt = 0;
        if (i < a.n) { key = a.kmers[i]; cnt = a.counts[i]; }
        const bool in = i < a.n && pf_hetpair::in_range(cnt, a.lo, a.hi);
        unsigned long long todo = __ballot(in);
        n_in += in;
        unsigned long long pair_word = 0;
        while (todo) {   // wave-uniform: four keys a turn
            int src[HP_ROWS];
#pragma unroll
            for (int r = 0; r < HP_ROWS; ++r) {
                src[r] = todo ? __ffsll(todo) - 1 : -1;
                todo &= todo - 1;   // (0 stays 0)
            }
            const int mine = row == 0 ? src[0] : row == 1 ? src[1] : row == 2 ? src[2] : src[3];
            const bool on = mine >= 0;
            const uint64_t x = shfl_u64(key, on ? mine : 0);
            const pf_hetpair::Degree dx = row_degree(a, x, on, row_lane);
            const uint32_t deg_x = on ? dx.degree() : 0u;
            const bool ask = deg_x == 1 && x < dx.first;
            bool is_pair = false;
            if (__any(ask)) {
                const pf_hetpair::Degree dy = row_degree(a, dx.first, ask, row_lane);
                is_pair = ask && pf_hetpair::pair_kept(x, deg_x, dx.first, dy.degree());
            }
            if (row_lane == 0) {
                n_one += deg_x == 1;
                n_many += deg_x > 1;
                n_pairs += is_pair;
                if (is_pair) {
                    const uint64_t at = w * WAVE + (uint64_t)mine;
                    if (a.partner) a.partner[at] = dx.first;
                    if (a.partner_cov) a.partner_cov[at] = dx.cov;
                }
            }
            const unsigned long long got = __ballot(is_pair && row_lane == 0);
#pragma unroll
            for (int r = 0; r < HP_ROWS; ++r)
                if ((got >> (r * HP_ROW)) & 1ull) pair_word |= 1ull << src[r];
        }
        if (lane == 0) {
            a.word[w] = pair_word;
            a.word_pairs[w] = (uint32_t)__popcll(pair_word);
        }
    }
    n_in = wave_sum_u64(n_in);
    n_one = wave_sum_u64(n_one);
    n_many = wave_sum_u64(n_many);
    n_pairs = wave_sum_u64(n_pairs);
    if (lane == 0) {
        if (n_in) atomicAdd(&a.c->in_range, (unsigned long long)n_in);
        if (n_one) atomicAdd(&a.c->one_partner, (unsigned long long)n_one);
        if (n_many) atomicAdd(&a.c->many_partners, (unsigned long long)n_many);
        if (n_pairs) atomicAdd(&a.c->pairs, (unsigned long long)n_pairs);
    }
}

// ---- write ----
struct HetWriteArgs {
    const uint64_t *kmers;
    const uint32_t *counts;
    uint64_t n;
    const uint64_t *word, *word_off;
    const uint64_t *partner;        // null: the keys are not wanted
    const uint32_t *partner_cov;
    uint64_t *pair_x, *pair_y;      // null with partner
    uint32_t *cov_x, *cov_y;
};

__global__ __launch_bounds__(HP_BLOCK) void k_hetpair_write(const HetWriteArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * HP_BLOCK + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * HP_BLOCK) {
        const uint64_t w = i / WAVE, bits = a.word[w];
        const int b = (int)(i % WAVE);
        if (!((bits >> b) & 1ull)) continue;
        const uint64_t at = a.word_off[w] + (uint64_t)__popcll(bits & ((1ull << b) - 1));
        a.cov_x[at] = a.counts[i];
        a.cov_y[at] = a.partner_cov[i];
        if (a.partner) {
            a.pair_x[at] = a.kmers[i];
            a.pair_y[at] = a.partner[i];
        }
    }
}

// ---- table ----
struct HetTableArgs {
    const uint32_t *cov_x, *cov_y;
    uint64_t n_pairs;
    uint32_t lo, W;
    unsigned long long *table;
};

__global__ __launch_bounds__(HP_BLOCK) void k_hetpair_table(const HetTableArgs a) {
    __shared__ unsigned int s_tag[TABLE_SLOTS];   // cell + 1; 0 = free (W * W <= 2^24)
    __shared__ unsigned int s_cnt[TABLE_SLOTS];
    for (uint32_t s = threadIdx.x; s < TABLE_SLOTS; s += HP_BLOCK) { s_tag[s] = 0; s_cnt[s] = 0; }
    __syncthreads();
    const int lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * HP_BLOCK;
    // every thread of a block makes the same number of turns: the ballots see whole wavefronts
    for (uint64_t base = (uint64_t)blockIdx.x * HP_BLOCK; base < a.n_pairs; base += stride) {
        const uint64_t i = base + threadIdx.x;
        bool have = i < a.n_pairs;
        uint32_t cell = 0;
        if (have) {
            const uint32_t cx = a.cov_x[i], cy = a.cov_y[i], hi = a.lo + (a.W - 1);
            have = pf_hetpair::in_range(cx, a.lo, hi) && pf_hetpair::in_range(cy, a.lo, hi);   // (a pair of pf_hetpairs always is: no cell outside the table)
            if (have) cell = (uint32_t)pf_hetpair::table_cell(cx, cy, a.lo, a.W);
        }
        const unsigned long long act = __ballot(have);
        if (!act) continue;
        const int leader = __ffsll(act) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)cell, leader, WAVE);
        const unsigned long long same = __ballot(have && cell == c0);
        if (!have) continue;
        uint32_t add = 1;
        if (cell == c0) {
            if (lane != leader) continue;
            add = (uint32_t)__popcll(same);
        }
        const uint32_t slot = (cell ^ (cell >> 12)) & (TABLE_SLOTS - 1);
        const unsigned int old = atomicCAS(&s_tag[slot], 0u, cell + 1u);
        if (old == 0u || old == cell + 1u) atomicAdd(&s_cnt[slot], add);
        else atomicAdd(&a.table[cell], (unsigned long long)add);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < TABLE_SLOTS; s += HP_BLOCK)
        if (s_tag[s]) atomicAdd(&a.table[s_tag[s] - 1u], (unsigned long long)s_cnt[s]);
}

// the table of n_pairs compacted counters in device memory into W * W zeroed cells in device memory
static int hetpair_table_launch(pf_ctx *ctx, const uint32_t *cov_x, const uint32_t *cov_y, uint64_t n_pairs, uint32_t lo, uint32_t W,
                                unsigned long long *table) {
    HetTableArgs t;
    t.cov_x = cov_x;
    t.cov_y = cov_y;
    t.n_pairs = n_pairs;
    t.lo = lo;
    t.W = W;
    t.table = table;
    const int grid = ctx_grid(ctx, n_pairs, HP_BLOCK, 4);
    // pairs one block counts into its u32 slots: below 2^32 (with 1024 blocks: 2^42 pairs, more than HBM holds)
    if ((n_pairs + grid - 1) / (uint64_t)grid >= (1ull << 32)) {
        pf::CtxErr{ctx} = "pf_hetpairs: " + std::to_string(n_pairs) + " pairs are more than a block of this device counts in 32 bits";
        return PF_ERR_ARG;
    }
    k_hetpair_table<<<grid, HP_BLOCK, 0, ctx->stream>>>(t);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_hetpairs(pf_ctx *ctx, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lo, uint32_t hi,
                           uint64_t *table, uint64_t **pair_x_dev, uint64_t **pair_y_dev, uint32_t **cov_x_dev, uint32_t **cov_y_dev,
                           uint64_t *n_pairs, pf_hetpair_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    const int n_out = (pair_x_dev != nullptr) + (pair_y_dev != nullptr) + (cov_x_dev != nullptr) + (cov_y_dev != nullptr);
    if (n_out != 0 && n_out != 4) return refuse("pf_hetpairs: pair_x_dev, pair_y_dev, cov_x_dev and cov_y_dev are given together or not at all");
    const bool want_pairs = n_out == 4;
    if (want_pairs) *pair_x_dev = *pair_y_dev = nullptr, *cov_x_dev = *cov_y_dev = nullptr;
    if (n_pairs) *n_pairs = 0;
    if (stats) *stats = pf_hetpair_stats{0, 0, 0, 0, 0};
    { const int c = pf_hetpair::arg_clause((int64_t)k, lo, hi); if (c) return refuse(std::string("pf_hetpairs: ") + pf_hetpair::arg_text(c)); }
    if (!ctx->d_tab || !ctx->tab_cap) return refuse("pf_hetpairs: no count table is resident (pf_upload_counts comes first)");
    if (ctx->tab_k != (int)k)
        return refuse("pf_hetpairs: the resident count table has k " + std::to_string(ctx->tab_k) + ", the keys have k " + std::to_string(k));
    if (ctx->tab_exact) return refuse("pf_hetpairs: the resident count table was not counted on both strands (pairs are over canonical k-mers)");
    if (n && (!kmers || !counts)) return refuse("pf_hetpairs: kmers and counts are needed");
    if (((uintptr_t)kmers & 7) || ((uintptr_t)counts & 3)) return refuse("pf_hetpairs: kmers / counts are not aligned");
    if (want_pairs && !n_pairs) return refuse("pf_hetpairs: n_pairs is needed with the pair arrays");
    const uint32_t W = hi - lo + 1;
    const size_t table_bytes = (size_t)W * W * 8;
    PF_HIP(hipSetDevice(ctx->device));
    (void)join_finish(ctx);
    const bool table_on_dev = table && is_device_ptr(table);
    if (n == 0) {   // empty results
        if (table_on_dev) { PF_HIP(hipMemsetAsync(table, 0, table_bytes, ctx->stream)); PF_HIP(hipStreamSynchronize(ctx->stream)); }
        else if (table) memset(table, 0, table_bytes);
        return PF_OK;
    }
    Timed timed(ctx, PF_K_HETPAIR);
    const bool keys_on_dev = is_device_ptr(kmers), counts_on_dev = is_device_ptr(counts);
    const uint64_t n_words = (n + WAVE - 1) / WAVE;
    // one workspace: staged keys and counters, words, their popcounts and offsets, the partners, the scan's scratch, the counters
    const size_t b_keys = keys_on_dev ? 0 : up256((size_t)n * 8), b_counts = counts_on_dev ? 0 : up256((size_t)n * 4);
    const size_t b_word = up256((size_t)n_words * 8), b_wp = up256((size_t)n_words * 4), b_off = up256((size_t)n_words * 8);
    const size_t b_partner = want_pairs ? up256((size_t)n * 8) : 0, b_pcov = (want_pairs || table) ? up256((size_t)n * 4) : 0;
    const size_t b_scan = up256(scan_scratch_bytes(n_words));
    char *ws = static_cast<char *>(ctx_ws(ctx, WS_HETPAIR, b_keys + b_counts + b_word + b_wp + b_off + b_partner + b_pcov + b_scan + 256));
    if (!ws) return PF_ERR_HIP;
    char *at = ws;
    auto take = [&](size_t bytes) { char *p = at; at += bytes; return p; };
    uint64_t *d_keys = reinterpret_cast<uint64_t *>(take(b_keys));
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(take(b_counts));
    uint64_t *d_word = reinterpret_cast<uint64_t *>(take(b_word));
    uint32_t *d_wp = reinterpret_cast<uint32_t *>(take(b_wp));
    uint64_t *d_off = reinterpret_cast<uint64_t *>(take(b_off));
    uint64_t *d_partner = b_partner ? reinterpret_cast<uint64_t *>(take(b_partner)) : nullptr;
    uint32_t *d_pcov = b_pcov ? reinterpret_cast<uint32_t *>(take(b_pcov)) : nullptr;
    void *d_scan = take(b_scan);
    HetCounts *dc = reinterpret_cast<HetCounts *>(take(256));
    const uint64_t *pk = kmers;
    const uint32_t *pc = counts;
    if (!keys_on_dev) { PF_HIP(hipMemcpyAsync(d_keys, kmers, (size_t)n * 8, hipMemcpyDefault, ctx->stream)); pk = d_keys; }
    if (!counts_on_dev) { PF_HIP(hipMemcpyAsync(d_counts, counts, (size_t)n * 4, hipMemcpyDefault, ctx->stream)); pc = d_counts; }
    PF_HIP(hipMemsetAsync(dc, 0, sizeof(HetCounts), ctx->stream));
    HetFlagArgs f;
    f.tab = ctx->d_tab;
    f.mask = ctx->tab_cap - 1;
    f.k = (int)k;
    f.kmers = pk;
    f.counts = pc;
    f.n = n;
    f.n_words = n_words;
    f.lo = lo;
    f.hi = hi;
    f.word = d_word;
    f.word_pairs = d_wp;
    f.partner = d_partner;
    f.partner_cov = d_pcov;
    f.c = dc;
    k_hetpair_flag<<<ctx_grid(ctx, n, HP_BLOCK, HP_PER_CU), HP_BLOCK, 0, ctx->stream>>>(f);
    { const hipError_t le = hipGetLastError(); if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-HETPAIR launch: ") + hipGetErrorString(le); return PF_ERR_HIP; } }
    HetCounts h = {};
    PF_HIP(hipMemcpyAsync(&h, dc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    if (d_pcov) PF_HIP(scan_exclusive_u32_u64(d_wp, d_off, n_words, d_scan, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    ctx_units(ctx, PF_K_HETPAIR, h.in_range);
    if (stats) *stats = pf_hetpair_stats{n, h.in_range, h.one_partner, h.many_partners, h.pairs};
    if (n_pairs) *n_pairs = h.pairs;
    // the compacted pairs: the caller's arrays, or the counters alone for the table
    DevTmp<uint64_t> px_, py_;
    DevTmp<uint32_t> cx_, cy_;
    DevTmp<unsigned long long> dt_;
    if (d_pcov && h.pairs) {
        if (want_pairs) { PF_HIP(px_.alloc((size_t)h.pairs * 8)); PF_HIP(py_.alloc((size_t)h.pairs * 8)); }
        PF_HIP(cx_.alloc((size_t)h.pairs * 4));
        PF_HIP(cy_.alloc((size_t)h.pairs * 4));
        HetWriteArgs wa;
        wa.kmers = pk;
        wa.counts = pc;
        wa.n = n;
        wa.word = d_word;
        wa.word_off = d_off;
        wa.partner = d_partner;
        wa.partner_cov = d_pcov;
        wa.pair_x = px_.p;
        wa.pair_y = py_.p;
        wa.cov_x = cx_.p;
        wa.cov_y = cy_.p;
        k_hetpair_write<<<ctx_grid(ctx, n, HP_BLOCK, HP_PER_CU), HP_BLOCK, 0, ctx->stream>>>(wa);
    }
    if (table) {
        unsigned long long *pt = reinterpret_cast<unsigned long long *>(table);
        if (!table_on_dev) { PF_HIP(dt_.alloc(table_bytes)); pt = dt_.p; }
        PF_HIP(hipMemsetAsync(pt, 0, table_bytes, ctx->stream));
        if (h.pairs) { const int rc = hetpair_table_launch(ctx, cx_.p, cy_.p, h.pairs, lo, W, pt); if (rc) return rc; }
        if (!table_on_dev) PF_HIP(hipMemcpyAsync(table, pt, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    { const hipError_t le = hipGetLastError(); if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-HETPAIR launch: ") + hipGetErrorString(le); return PF_ERR_HIP; } }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    if (want_pairs) {
        *pair_x_dev = px_.p; px_.p = nullptr;
        *pair_y_dev = py_.p; py_.p = nullptr;
        *cov_x_dev = cx_.p; cx_.p = nullptr;
        *cov_y_dev = cy_.p; cy_.p = nullptr;
    }
    return PF_OK;
}

// the table kernel alone over compacted counters on the device (the bench times it; the table is [host|dev])
extern "C" int pf_hetpair_table(pf_ctx *ctx, const uint32_t *cov_x_dev, const uint32_t *cov_y_dev, uint64_t n_pairs, uint32_t lo, uint32_t hi,
                                uint64_t *table) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int c = pf_hetpair::arg_clause(pf_hetpair::MIN_K, lo, hi); if (c) return refuse(std::string("pf_hetpair_table: ") + pf_hetpair::arg_text(c)); }
    if (!table || (n_pairs && (!cov_x_dev || !cov_y_dev))) return refuse("pf_hetpair_table: the counters and the table are needed");
    if (n_pairs && (!is_device_ptr(cov_x_dev) || !is_device_ptr(cov_y_dev))) return refuse("pf_hetpair_table: the counters are device arrays");
    const uint32_t W = hi - lo + 1;
    const size_t table_bytes = (size_t)W * W * 8;
    PF_HIP(hipSetDevice(ctx->device));
    DevTmp<unsigned long long> dt_;
    const bool table_on_dev = is_device_ptr(table);
    unsigned long long *pt = reinterpret_cast<unsigned long long *>(table);
    if (!table_on_dev) { PF_HIP(dt_.alloc(table_bytes)); pt = dt_.p; }
    PF_HIP(hipMemsetAsync(pt, 0, table_bytes, ctx->stream));
    if (n_pairs) {
        Timed timed(ctx, PF_K_HETPAIR);
        const int rc = hetpair_table_launch(ctx, cov_x_dev, cov_y_dev, n_pairs, lo, W, pt);
        if (rc) return rc;
        ctx_units(ctx, PF_K_HETPAIR, n_pairs);
    }
    if (!table_on_dev) PF_HIP(hipMemcpyAsync(table, pt, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}
