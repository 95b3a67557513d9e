// K-COLOR: the second pass of `Bifrost build -c` (buildUnitigColors, bifrost/src/ColoredCDBG.tcc:805-887) on the device -- every file of
// reads streamed once more over the graph pf_unitig_build_colored left in the context, one table look-up per window, and the colour
// sets of the unitigs as runs of ids.  The rule is pf_color_rule.hpp; this file is its device form.  L live k-mers (the k-mers of the
// written graph), C colours, flat position of a k-mer = k-mers of the lines before its line + its position in the line.
//
//   stage   bytes held                                          probes / atomics per window
//   table   16 a slot {u64 key, u32 flat position, u32 pad}, a power of two of at least 2 L slots, the slot from mix64(key), linear
//           probing; one CAS per key (keys are distinct), as the index stage of K-UNITIG.  Built once, read-only afterwards.
//   planes  C bit planes of ceil(L / 32) words, colour-major (as the calling run's colour SoA), cleared once.
//   mark    k_col_mark.  The unit of work is a byte of the text (a window start), as in K-MASK and K-COUNT: class bitmaps from the read
//           table, a tile of 1024 bytes plus halo as 2-bit codes in LDS, one k-mer per lane (pf_reads_dev.hpp).  Per valid window one
//           probe of the table (a 16-byte load; further slots only behind a collision).  On a hit the plane word is loaded and an
//           atomicOr issued only when the bit is clear: at 24-fold coverage nearly every window finds its bit set already.  A stale
//           read costs one redundant atomic and nothing else (or is idempotent).  The colour is a kernel argument: it changes with the
//           file, not with the chunk.  Hits, misses and bad windows are summed per lane and per wavefront before one atomic each when the
//           kernel ends.  The probe loop is bounded by the slot count and flags at its bound.                 1 probe, <= 1 atomic
//   keys    k_col_keys (K-COLORSET, pf_color_kmers): the same marking from the distinct canonical k-mers of a colour's reads instead of
//           from the reads (pf_runmulti_rule.hpp) -- one key a lane, no text, no tile, no bitmaps.                  1 probe, <= 1 atomic a key
//   runs    k_col_runs, twice (count, scan, write).  One 16-lane row per unitig; its id space c * m + p is walked 512 ids a step, 32 ids a
//           lane, gathered from the planes of the colours the 32 ids span, so ids of adjacent colours merge by themselves.  A run begins
//           at a set id behind a clear one and ends at a set id before a clear one; begins and ends are numbered by a prefix sum over
//           the row and written as (first id, last id) pairs in graph order.  The run list and the slot table are what leave the device.
// Every loop is bounded and nothing spins.  256 threads a block, no scratch, at most 56 VGPRs (eight wavefronts a SIMD); the mark
// kernel's LDS is the tile's 408 bytes (pf_reads_dev.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_color_rule.hpp"
#include "pf_count_rule.hpp"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"
#include "pf_unitig_state.hpp"

namespace pf {

struct ColSlot {
    unsigned long long key;
    uint32_t flat, pad;
};
static_assert(sizeof(ColSlot) == 16, "one slot, one 16-byte vector access");
constexpr uint32_t COL_NONE = 0xFFFFFFFFu;
constexpr int COL_ROW = 16;   // lanes that walk one unitig's ids

struct ColDev {   // device counters of one colouring
    unsigned long long hits, misses;
    uint32_t stuck, pad;
};

struct ColorState {
    ColSlot *tab = nullptr;
    uint64_t slots = 0, words = 0;
    uint32_t *planes = nullptr;
    uint32_t n_colors = 0;
    ColDev *dev = nullptr;
    pf_color_stats total = {};
    bool finished = false;
    uint64_t *run_off = nullptr;   // n_lines + 1
    uint2 *runs = nullptr;
    uint64_t n_runs = 0;
};

// ---- table ----
__global__ __launch_bounds__(256) void k_col_clear(ColSlot *tab, uint64_t slots) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256)
        *reinterpret_cast<uint4 *>(tab + s) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, COL_NONE, 0u);
}
__global__ __launch_bounds__(256) void k_col_index(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ flat_of, uint64_t n, ColSlot *tab,
                                                   uint64_t mask, ColDev *d) {
    bool stuck = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t flat = flat_of[i];
        if (flat == COL_NONE) continue;   // removed by -i / -d: it colours nothing
        const unsigned long long key = kmers[i];
        uint64_t s = mix64(key) & mask;
        bool put = false;
        for (uint64_t step = 0; step <= mask && !put; ++step) {
            if (atomicCAS(&tab[s].key, (unsigned long long)pf_count::EMPTY_KEY, key) == pf_count::EMPTY_KEY) {
                tab[s].flat = flat;   // a fresh slot of a distinct key: nobody else writes it, nobody reads it before the kernel ends
                put = true;
            }
            s = (s + 1) & mask;
        }
        if (!put) stuck = true;
    }
    if (stuck) d->stuck = 1u;
}

// the flat position of `key`; NONE: not a k-mer of the graph (or the probe went round the table: stuck)
__device__ inline uint32_t col_find(const ColSlot *__restrict__ tab, uint64_t mask, uint64_t key, bool &stuck) {
    uint64_t s = mix64(key) & mask;
    for (uint64_t step = 0; step <= mask; ++step) {
        const uint4 v = *reinterpret_cast<const uint4 *>(tab + s);
        const uint64_t cur = ((uint64_t)v.y << 32) | v.x;
        if (cur == key) return v.z;
        if (cur == pf_count::EMPTY_KEY) return COL_NONE;
        s = (s + 1) & mask;
    }
    stuck = true;
    return COL_NONE;
}

// ---- mark ----
struct ColMarkArgs {
    const ColSlot *tab;
    uint64_t mask;          // slots - 1
    int k;
    uint32_t *plane;        // the plane of this file's colour
    const char *text;
    uint64_t n;             // bytes of the text
    uint64_t n_tiles;
    const uint64_t *start;  // window-start bitmap, MASK_TILE / 64 words a tile
    MaskCounts *c;          // kmers_bad of this call
    ColDev *d;
};

__global__ __launch_bounds__(MASK_BLOCK) void k_col_mark(const ColMarkArgs a) {
    __shared__ uint32_t s_code[MASK_UNITS];
    __shared__ uint32_t s_valid32[MASK_UNITS / 2 + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    const uint64_t all_k = (1ull << k) - 1;
    uint64_t n_bad = 0, hits = 0, misses = 0;
    bool stuck = false;
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile has been read
        tile_stage(a.text, a.n, tile, tid, s_code, s_valid32);
        __syncthreads();
        const uint64_t word0 = tile * (MASK_TILE / 64) + (uint64_t)wave;
#pragma unroll
        for (int j = 0; j < MASK_PER_LANE; ++j) {
            const uint64_t sw = a.start[word0 + (uint64_t)j * (MASK_BLOCK / 64)];   // the same word for the whole wavefront
            const bool is_start = (sw >> lane) & 1ull;
            bool valid = false;
            if (is_start) {
                const int p = j * MASK_BLOCK + tid;
                valid = tile_window_valid(s_valid32, p, k, all_k);
                if (valid) {
                    const uint64_t key = pf_count::window_key(tile_kmer(s_code, p, k), k, true);
                    const uint32_t flat = col_find(a.tab, a.mask, key, stuck);
                    if (flat == COL_NONE) misses += 1;
                    else {
                        hits += 1;
                        uint32_t *w = a.plane + (flat >> 5);
                        const uint32_t bit = 1u << (flat & 31u);
                        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
                    }
                }
            }
            const unsigned long long bw = __ballot(is_start && !valid);
            if (lane == 0) n_bad += (uint64_t)__popcll(bw);
        }
    }
    hits = wave_sum_u64(hits);
    misses = wave_sum_u64(misses);
    if (lane == 0) {
        if (hits) atomicAdd(&a.d->hits, (unsigned long long)hits);
        if (misses) atomicAdd(&a.d->misses, (unsigned long long)misses);
        if (n_bad) atomicAdd(&a.c->kmers_bad, (unsigned long long)n_bad);
    }
    if (stuck) a.d->stuck = 1u;
}

// ---- mark from keys (K-COLORSET) ----
// The distinct canonical k-mers of a colour's reads instead of the reads (pf_runmulti_rule.hpp): one key a lane, consecutive lanes
// consecutive keys (coalesced 8-byte loads), one probe of the table, the plane word loaded and the atomicOr issued only where the bit
// is clear, as k_col_mark does.  Hits and misses are summed per lane and per wavefront before one atomic each.
__global__ __launch_bounds__(256) void k_col_keys(const ColSlot *__restrict__ tab, uint64_t mask, uint32_t *plane, const uint64_t *__restrict__ keys,
                                                  uint64_t n, ColDev *d) {
    uint64_t hits = 0, misses = 0;
    bool stuck = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t flat = col_find(tab, mask, keys[i], stuck);
        if (flat == COL_NONE) misses += 1;
        else {
            hits += 1;
            uint32_t *w = plane + (flat >> 5);
            const uint32_t bit = 1u << (flat & 31u);
            if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
        }
    }
    hits = wave_sum_u64(hits);
    misses = wave_sum_u64(misses);
    if ((threadIdx.x & 63) == 0) {
        if (hits) atomicAdd(&d->hits, (unsigned long long)hits);
        if (misses) atomicAdd(&d->misses, (unsigned long long)misses);
    }
    if (stuck) d->stuck = 1u;
}

// ---- runs ----
// is id `id` of the unitig whose k-mers lie from flat position `base` set?  id = colour * m + position
__device__ inline uint32_t col_bit(const uint32_t *__restrict__ planes, uint64_t words, uint64_t base, uint32_t m, uint64_t id) {
    const uint64_t c = id / m, f = base + (id - c * m);
    return (planes[c * words + (f >> 5)] >> (f & 31u)) & 1u;
}
// ids id0 .. id0 + nv - 1 (1 <= nv <= 32) as bits 0 .. nv - 1: a piece per colour the ids span, at most nv pieces
__device__ inline uint32_t col_segment(const uint32_t *__restrict__ planes, uint64_t words, uint64_t base, uint32_t m, uint64_t id0, uint32_t nv) {
    uint64_t c = id0 / m;
    uint32_t p = (uint32_t)(id0 - c * m), seg = 0, filled = 0;
    while (filled < nv) {
        const uint32_t take = min(nv - filled, m - p);   // >= 1: p < m
        const uint64_t f = base + p;
        const uint32_t *w = planes + c * words + (f >> 5);
        const uint32_t sh = (uint32_t)(f & 31u);
        uint64_t two = w[0];
        if (sh + take > 32) two |= (uint64_t)w[1] << 32;   // (the piece's last bit lies in that word: it is below `words`)
        const uint32_t bits = (uint32_t)(two >> sh) & (take == 32 ? 0xFFFFFFFFu : (1u << take) - 1u);
        seg |= bits << filled;
        filled += take;
        p += take;
        if (p == m) { p = 0; ++c; }
    }
    return seg;
}

// WRITE = false: cnt[line] = runs of the line.  WRITE = true: the pairs from run_off[line] on, ascending.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_col_runs(const uint32_t *__restrict__ planes, uint64_t words, const uint64_t *__restrict__ km_off,
                                                  const uint32_t *__restrict__ m_of, uint64_t n_lines, uint32_t n_colors, uint32_t *__restrict__ cnt,
                                                  const uint64_t *__restrict__ run_off, uint2 *__restrict__ runs) {
    const int r = (int)threadIdx.x & (COL_ROW - 1);
    const uint64_t n_rows = (uint64_t)gridDim.x * (256 / COL_ROW);
    for (uint64_t j = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / COL_ROW; j < n_lines; j += n_rows) {   // (the same j in all lanes of a row)
        const uint32_t m = m_of[j];
        const uint64_t base = km_off[j], total = (uint64_t)n_colors * m;
        uint2 *out = WRITE ? runs + run_off[j] : nullptr;
        uint32_t begun = 0, ended = 0;   // of the steps before this one
        for (uint64_t step0 = 0; step0 < total; step0 += 32 * COL_ROW) {
            const uint64_t id0 = step0 + 32ull * (uint64_t)r;
            const uint32_t nv = id0 >= total ? 0u : total - id0 < 32 ? (uint32_t)(total - id0) : 32u;
            uint32_t seg = 0, prev = 0, next = 0;
            if (nv) {
                seg = col_segment(planes, words, base, m, id0, nv);
                prev = id0 ? col_bit(planes, words, base, m, id0 - 1) : 0u;
                next = id0 + nv < total ? col_bit(planes, words, base, m, id0 + nv) : 0u;
            }
            const uint32_t begins = seg & ~((seg << 1) | prev);
            const uint32_t ends = nv ? seg & ~((seg >> 1) | (next << (nv - 1))) : 0u;
            const uint32_t nb = (uint32_t)__popc(begins), ne = (uint32_t)__popc(ends);
            uint32_t ib = nb, ie = ne;   // inclusive sums over the row
#pragma unroll
            for (int o = 1; o < COL_ROW; o <<= 1) {
                const uint32_t tb = __shfl_up(ib, o, COL_ROW), te = __shfl_up(ie, o, COL_ROW);
                if (r >= o) { ib += tb; ie += te; }
            }
            if (WRITE) {
                uint32_t at = begun + ib - nb;
                for (uint32_t b = begins; b; b &= b - 1) out[at++].x = (uint32_t)(id0 + (uint64_t)(__ffs(b) - 1));
                at = ended + ie - ne;
                for (uint32_t b = ends; b; b &= b - 1) out[at++].y = (uint32_t)(id0 + (uint64_t)(__ffs(b) - 1));
            }
            begun += __shfl(ib, COL_ROW - 1, COL_ROW);
            ended += __shfl(ie, COL_ROW - 1, COL_ROW);
        }
        if (!WRITE && r == 0) cnt[j] = begun;
    }
}

// ---- host side ----
static UnitigState *col_graph(pf_ctx *ctx) { return static_cast<UnitigState *>(ctx->unitig); }
static ColorState *col_state(pf_ctx *ctx) { return col_graph(ctx) ? static_cast<ColorState *>(col_graph(ctx)->color) : nullptr; }

void color_destroy(UnitigState *S) {
    ColorState *C = S ? static_cast<ColorState *>(S->color) : nullptr;
    if (!C) return;
    (void)hipFree(C->tab);
    (void)hipFree(C->planes);
    (void)hipFree(C->dev);
    (void)hipFree(C->run_off);
    (void)hipFree(C->runs);
    delete C;
    S->color = nullptr;
}

struct ColEvents {   // brackets one stage for the times of pf_color_stats
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    explicit ColEvents(hipStream_t s) : st(s) {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, st) != hipSuccess) drop();
    }
    void drop() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
    double ms() {   // after the stream has been waited for
        float v = 0;
        if (!a || hipEventRecord(b, st) != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&v, a, b) != hipSuccess) v = 0;
        return (double)v;
    }
    ~ColEvents() { drop(); }
};

static int col_needs_begin(pf_ctx *ctx, const char *who, bool open) {
    ColorState *C = col_state(ctx);
    if (C && !(open && C->finished)) return PF_OK;
    pf::CtxErr{ctx} = std::string(who) + (C ? ": the colouring is finished (pf_unitig_release comes first)" : ": no colouring is open (pf_unitig_build_colored and pf_color_begin come first)");
    return PF_ERR_ARG;
}

// classes and mark over text[0, n) on the device with the table of reads on the device; counts reset by the caller, n > 0
static int color_core(pf_ctx *ctx, UnitigState *S, ColorState *C, uint32_t colour, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len,
                      uint64_t n_reads, MaskCounts *counts, MaskCounts &h, ColDev &d) {
    const uint64_t n_tiles = (n + MASK_TILE - 1) / MASK_TILE;
    const uint64_t n_words = n_tiles * (MASK_TILE / 64);   // whole tiles: the mark phase reads every word of a tile
    uint64_t *bits = static_cast<uint64_t *>(ctx_ws(ctx, WS_MASK_BITS, (size_t)n_words * 8 * 2));
    if (!bits) return PF_ERR_HIP;
    uint64_t *seq = bits, *start = bits + n_words;
    ColEvents ev(ctx->stream);
    k_mask_classes<<<ctx_grid(ctx, n_words, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(off, len, n_reads, n_words, (uint32_t)S->k, seq, start, counts);
    PF_HIP(hipMemsetAsync(C->dev, 0, sizeof(ColDev), ctx->stream));
    {
        ColMarkArgs a;
        a.tab = C->tab;
        a.mask = C->slots - 1;
        a.k = S->k;
        a.plane = C->planes + (uint64_t)colour * C->words;
        a.text = text;
        a.n = n;
        a.n_tiles = n_tiles;
        a.start = start;
        a.c = counts;
        a.d = C->dev;
        k_col_mark<<<ctx_grid(ctx, n_tiles * MASK_BLOCK, MASK_BLOCK, 8), MASK_BLOCK, 0, ctx->stream>>>(a);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-COLOR launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    PF_HIP(hipMemcpyAsync(&h, counts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&d, C->dev, sizeof d, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    C->total.mark_ms += ev.ms();
    if (d.stuck) { pf::CtxErr{ctx} = "K-COLOR: a probe went round the whole table"; return PF_ERR_HIP; }
    return PF_OK;
}

static void color_stats_out(pf_color_stats *stats, ColorState *C, uint64_t n_reads, const MaskCounts &h, const ColDev &d) {
    pf_color_stats st = {};
    st.colors = C->n_colors;
    st.reads = n_reads;
    st.windows_bad = h.kmers_bad;
    st.windows_colored = d.hits;
    st.windows_unplaced = d.misses;
    C->total.reads += st.reads;
    C->total.windows_bad += st.windows_bad;
    C->total.windows_colored += st.windows_colored;
    C->total.windows_unplaced += st.windows_unplaced;
    if (stats) *stats = st;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_color_begin(pf_ctx *ctx, uint32_t n_colors) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    UnitigState *S = col_graph(ctx);
    if (!S || !S->colored) return refuse("pf_color_begin: no coloured graph is held (pf_unitig_build_colored comes first)");
    if (S->color) return refuse("pf_color_begin: a colouring is open already (pf_unitig_release comes first)");
    if (n_colors == 0) return refuse("pf_color_begin: no colour");
    if (n_colors > pf_color::MAX_COLORS) return refuse(std::string("pf_color_begin: ") + pf_color::TOO_MANY_COLORS_TEXT);
    if ((uint64_t)n_colors * S->longest_m >= (1ull << 32))
        return refuse(std::string("pf_color_begin: ") + pf_color::TOO_LONG_TEXT + ": " + std::to_string(n_colors) + " colours, " + std::to_string(S->longest_m) + " k-mers");
    PF_HIP(hipSetDevice(ctx->device));
    uint64_t slots = 64;   // (a graph without a k-mer: an empty table, every valid window unplaced)
    while (slots < 2 * S->n_live) slots <<= 1;
    const uint64_t words = (S->n_live + 31) / 32;
    const uint64_t need = slots * sizeof(ColSlot) + (uint64_t)n_colors * words * 4;
    size_t free_b = 0, total_b = 0;
    PF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        pf::CtxErr{ctx} = "pf_color_begin: " + pf_color::no_room_text(need, free_b, n_colors, S->n_live);
        return PF_ERR_OVERFLOW;
    }
    ColorState *C = new ColorState;
    S->color = C;   // (freed with the graph on every path from here)
    C->n_colors = n_colors;
    C->slots = slots;
    C->words = words;
    C->total.colors = n_colors;
    C->total.overflow = S->overflow;
    C->total.table_slots = slots;
    C->total.plane_words = words;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&C->dev), sizeof(ColDev));
    if (e == hipSuccess) e = hipMemsetAsync(C->dev, 0, sizeof(ColDev), ctx->stream);
    if (e == hipSuccess && slots) e = hipMalloc(reinterpret_cast<void **>(&C->tab), slots * sizeof(ColSlot));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&C->planes), std::max<uint64_t>((uint64_t)n_colors * words * 4, 4));
    if (e == hipSuccess) e = hipMemsetAsync(C->planes, 0, std::max<uint64_t>((uint64_t)n_colors * words * 4, 4), ctx->stream);
    ColEvents ev(ctx->stream);
    ColDev d = {};
    if (e == hipSuccess && slots) {
        k_col_clear<<<ctx_grid(ctx, slots, 256, 8), 256, 0, ctx->stream>>>(C->tab, slots);
        if (S->n_live) k_col_index<<<ctx_grid(ctx, S->n, 256, 8), 256, 0, ctx->stream>>>(S->kmers, S->flat_of, S->n, C->tab, slots - 1, C->dev);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&d, C->dev, sizeof d, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    C->total.table_ms = ev.ms();
    if (e != hipSuccess || d.stuck) {
        color_destroy(S);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            pf::CtxErr{ctx} = "pf_color_begin: " + pf_color::no_room_text(need, free_b, n_colors, S->n_live);
            return PF_ERR_OVERFLOW;
        }
        pf::CtxErr{ctx} = e != hipSuccess ? std::string("pf_color_begin: ") + hipGetErrorString(e) : std::string("K-COLOR: a probe went round the whole table");
        return PF_ERR_HIP;
    }
    return PF_OK;
}

extern "C" int pf_color_reads(pf_ctx *ctx, uint32_t colour, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len,
                              uint64_t n_reads, pf_color_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = col_needs_begin(ctx, "pf_color_reads", true); if (rc) return rc; }
    UnitigState *S = col_graph(ctx);
    ColorState *C = col_state(ctx);
    if (colour >= C->n_colors) return refuse("pf_color_reads: colour " + std::to_string(colour) + " of " + std::to_string(C->n_colors));
    if (n_bytes && !text) return refuse("pf_color_reads: text is needed");
    if (n_reads && (!read_off || !read_len)) return refuse("pf_color_reads: read_off and read_len are needed");
    if (((uintptr_t)read_off & 7) || ((uintptr_t)read_len & 3)) return refuse("pf_color_reads: read_off / read_len are not aligned");
    if (n_bytes > MASK_MAX_BYTES) return refuse("pf_color_reads: the text is longer than 2^40 bytes");
    MaskCounts h = {};
    ColDev d = {};
    h.bad_entry = MASK_NO_RECORD;
    if (n_bytes == 0 && n_reads == 0) { color_stats_out(stats, C, 0, h, d); return PF_OK; }
    PF_HIP(hipSetDevice(ctx->device));
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
            return refuse("pf_color_reads: read " + std::to_string(h.bad_entry) + " lies outside the text or overlaps the next one (the table is ascending)");
    }
    if (n_bytes == 0) { color_stats_out(stats, C, n_reads, h, d); return PF_OK; }   // empty reads only
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    { const int rc = color_core(ctx, S, C, colour, dt, n_bytes, doff, dlen, n_reads, dc, h, d); if (rc) return rc; }
    color_stats_out(stats, C, n_reads, h, d);
    return PF_OK;
}

extern "C" int pf_color_fastq(pf_ctx *ctx, uint32_t colour, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_color_stats *stats,
                              uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = col_needs_begin(ctx, "pf_color_fastq", true); if (rc) return rc; }
    UnitigState *S = col_graph(ctx);
    ColorState *C = col_state(ctx);
    if (colour >= C->n_colors) return refuse("pf_color_fastq: colour " + std::to_string(colour) + " of " + std::to_string(C->n_colors));
    if (!bytes_used) return refuse("pf_color_fastq: bytes_used is needed");
    if (n_bytes && !text) return refuse("pf_color_fastq: text is needed");
    if (n_bytes > 0xFFFFFF00ull) return refuse("pf_color_fastq: a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    MaskCounts h = {};
    ColDev d = {};
    h.bad_entry = MASK_NO_RECORD;
    *bytes_used = 0;
    if (bad_record) *bad_record = 0;
    if (n_bytes == 0) { color_stats_out(stats, C, 0, h, d); return PF_OK; }
    if (stats) *stats = pf_color_stats{};
    PF_HIP(hipSetDevice(ctx->device));
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    FastqIndex ix;
    { const int rc = fastq_index(ctx, "pf_color_fastq", dt, n_bytes, final, ix, bad_record); if (rc) return rc; }   // refused before anything is coloured
    if (ix.n_rec) {
        const int rc = color_core(ctx, S, C, colour, dt, ix.used, ix.off, ix.len, ix.n_rec, ix.counts, h, d);
        if (rc) return rc;
    }
    *bytes_used = ix.used;
    color_stats_out(stats, C, ix.n_rec, h, d);
    return PF_OK;
}

extern "C" int pf_color_kmers(pf_ctx *ctx, uint32_t colour, const uint64_t *kmers_dev, uint64_t n, pf_color_kmers_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    { const int rc = col_needs_begin(ctx, "pf_color_kmers", true); if (rc) return rc; }
    ColorState *C = col_state(ctx);
    if (colour >= C->n_colors) return refuse("pf_color_kmers: colour " + std::to_string(colour) + " of " + std::to_string(C->n_colors));
    if (n && !kmers_dev) return refuse("pf_color_kmers: kmers_dev is needed");
    if (n && (!is_device_ptr(kmers_dev) || ((uintptr_t)kmers_dev & 7))) return refuse("pf_color_kmers: kmers_dev is not an aligned array on the device");
    if (n >= (1ull << 40)) return refuse("pf_color_kmers: more than 2^40 keys");
    pf_color_kmers_stats st = {};
    st.kmers = n;
    if (n) {
        PF_HIP(hipSetDevice(ctx->device));
        ColDev d = {};
        ctx_begin(ctx, PF_K_COLORSET);
        ColEvents ev(ctx->stream);
        PF_HIP(hipMemsetAsync(C->dev, 0, sizeof(ColDev), ctx->stream));
        k_col_keys<<<ctx_grid(ctx, n, 256, 8), 256, 0, ctx->stream>>>(C->tab, C->slots - 1, C->planes + (uint64_t)colour * C->words, kmers_dev, n, C->dev);
        const hipError_t le = hipGetLastError();
        ctx_end(ctx);
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-COLORSET launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
        PF_HIP(hipMemcpyAsync(&d, C->dev, sizeof d, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        C->total.mark_ms += ev.ms();
        ctx_units(ctx, PF_K_COLORSET, n);
        if (d.stuck) { pf::CtxErr{ctx} = "K-COLORSET: a probe went round the whole table"; return PF_ERR_HIP; }
        st.kmers_colored = d.hits;
        st.kmers_unplaced = d.misses;
    }
    if (stats) *stats = st;
    return PF_OK;
}

extern "C" int pf_color_finish(pf_ctx *ctx, pf_color_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    { const int rc = col_needs_begin(ctx, "pf_color_finish", true); if (rc) return rc; }
    UnitigState *S = col_graph(ctx);
    ColorState *C = col_state(ctx);
    PF_HIP(hipSetDevice(ctx->device));
    const uint64_t n_lines = S->n_lines;
    DevTmp<uint32_t> cnt;
    DevTmp<uint8_t> scratch;
    PF_HIP(cnt.alloc((n_lines + 1) * 4));
    PF_HIP(scratch.alloc(scan_scratch_bytes(n_lines + 1)));
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&C->run_off), (n_lines + 1) * 8));
    PF_HIP(hipMemsetAsync(cnt.p, 0, (n_lines + 1) * 4, ctx->stream));
    ColEvents ev(ctx->stream);
    const int g_rows = ctx_grid(ctx, std::max<uint64_t>(n_lines, 1) * COL_ROW, 256, 8);
    if (n_lines) k_col_runs<false><<<g_rows, 256, 0, ctx->stream>>>(C->planes, C->words, S->km_off, S->m_of, n_lines, C->n_colors, cnt.p, nullptr, nullptr);
    PF_HIP(scan_exclusive_u32_u64(cnt.p, C->run_off, n_lines + 1, scratch.p, ctx->stream));
    uint64_t n_runs = 0;
    PF_HIP(hipMemcpyAsync(&n_runs, C->run_off + n_lines, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&C->runs), std::max<uint64_t>(n_runs * sizeof(uint2), 8)));
    if (n_runs) k_col_runs<true><<<g_rows, 256, 0, ctx->stream>>>(C->planes, C->words, S->km_off, S->m_of, n_lines, C->n_colors, nullptr, C->run_off, C->runs);
    PF_HIP(hipGetLastError());
    PF_HIP(hipStreamSynchronize(ctx->stream));
    C->total.runs_ms = ev.ms();
    C->n_runs = n_runs;
    C->total.runs = n_runs;
    C->total.lines = n_lines;
    C->finished = true;
    if (stats) *stats = C->total;
    return PF_OK;
}

extern "C" int pf_color_fetch(pf_ctx *ctx, uint64_t *heads, uint32_t *m, uint32_t *slot, uint64_t *run_off, uint32_t *runs) {
    if (!ctx) return PF_ERR_ARG;
    { const int rc = col_needs_begin(ctx, "pf_color_fetch", false); if (rc) return rc; }
    UnitigState *S = col_graph(ctx);
    ColorState *C = col_state(ctx);
    if (!C->finished) { pf::CtxErr{ctx} = "pf_color_fetch: the colouring is not finished (pf_color_finish comes first)"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    const uint64_t n = S->n_lines;
    if (heads && n) PF_HIP(hipMemcpyAsync(heads, S->heads, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (m && n) PF_HIP(hipMemcpyAsync(m, S->m_of, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (slot && n) PF_HIP(hipMemcpyAsync(slot, S->slot, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (run_off) PF_HIP(hipMemcpyAsync(run_off, C->run_off, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (runs && C->n_runs) PF_HIP(hipMemcpyAsync(runs, C->runs, C->n_runs * 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}
