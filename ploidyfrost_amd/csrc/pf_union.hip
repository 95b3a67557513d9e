// K-UNION: the sorted distinct union of several sorted distinct arrays of 64-bit keys on the device -- the vertices of the coloured
// graph from the k-mers of every sample's masked reads (`ploidyfrost run-multi`; the rule is pf_runmulti_rule.hpp).  Rounds of pairwise
// merges, ceil(log2 C) of them, an odd set carried to the next round as it is.
//
// One merge of A (na keys) and B (nb keys), merged order = A before B among equal keys, na + nb positions:
//   tile    a block takes UNION_TILE positions of the merged order.  Two lanes find by a diagonal search over both inputs (at most 64
//           steps each, two 8-byte loads a step) how many keys of A lie before the tile's first and behind its last position.
//   stage   both pieces go to LDS (UNION_TILE keys, 8 KB), every lane loading consecutive keys: coalesced, each key read once.
//   merge   every lane finds its UNION_ITEMS positions by the same search in LDS (at most 11 steps) and merges them serially.
//   drop    a key equal to its predecessor in merged order is dropped (the inputs are distinct, so an equal pair is one key of A in
//           front of one key of B).  A lane's first position has its predecessor outside the lane: it is read from the inputs
//           (A[a - 1] and B[b - 1] of the lane's split), whether that lies in this tile, in the tile before or nowhere.
//   number  survivors are numbered by a prefix sum over the block; the count kernel writes the tile's total, pf_scan turns the totals
//           into tile offsets, the write kernel does the merge again, compacts the survivors in LDS and writes them coalesced.
// A call takes its count, offset and scan workspaces once, for the largest merge; every merge allocates its result alone.
// No atomics, nothing spins, every loop is bounded.  256 threads a block, 8 KB + 128 B of LDS (eight blocks a CU fit), no scratch.
// HBM traffic of a merge: both inputs twice (16 B a key) and the output once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_runmulti_rule.hpp"
#include "pf_scan.hpp"

namespace pf {

constexpr int UNION_BLOCK = 256, UNION_ITEMS = pf_runmulti::UNION_ITEMS, UNION_TILE = pf_runmulti::UNION_TILE;
static_assert(UNION_TILE == UNION_BLOCK * UNION_ITEMS, "a lane merges UNION_ITEMS positions of the tile");

// keys of A among the first d positions of the merged order (A before B among equal keys); 0 <= d <= na + nb
template <class KeysA, class KeysB>
__device__ inline uint64_t union_split(KeysA A, uint64_t na, KeysB B, uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    for (int step = 0; step < 65 && lo < hi; ++step) {   // (the interval halves: 64 steps empty any of them)
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct UnionFlags {   // what the check of one set found
    uint32_t unsorted, repeat;
};

// a set is ascending without a repeat: plain stores of 1 (every writer writes the same)
__global__ __launch_bounds__(256) void k_union_check(const uint64_t *__restrict__ keys, uint64_t n, UnionFlags *f) {
    bool unsorted = false, repeat = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t a = keys[i - 1], b = keys[i];
        unsorted |= a > b;
        repeat |= a == b;
    }
    if (unsorted) f->unsorted = 1u;
    if (repeat) f->repeat = 1u;
}

// WRITE = false: cnt[tile] = survivors of the tile.  WRITE = true: the survivors from tile_off[tile] on.
template <bool WRITE>
__global__ __launch_bounds__(UNION_BLOCK) void k_union_merge(const uint64_t *__restrict__ A, uint64_t na, const uint64_t *__restrict__ B, uint64_t nb,
                                                             uint64_t n_tiles, uint32_t *__restrict__ cnt, const uint64_t *__restrict__ tile_off,
                                                             uint64_t *__restrict__ out) {
    __shared__ uint64_t s_key[UNION_TILE];
    __shared__ uint64_t s_split[2];
    __shared__ uint32_t s_wave[UNION_BLOCK / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t n = na + nb;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t d0 = tile * UNION_TILE, d1 = d0 + UNION_TILE < n ? d0 + UNION_TILE : n;
        __syncthreads();   // the previous tile's LDS has been read
        if (tid < 2) s_split[tid] = union_split(A, na, B, nb, tid ? d1 : d0);
        __syncthreads();
        const uint64_t a0 = s_split[0], a1 = s_split[1], b0 = d0 - a0, b1 = d1 - a1;
        const uint32_t la = (uint32_t)(a1 - a0), lb = (uint32_t)(b1 - b0), len = la + lb;   // len = d1 - d0 <= UNION_TILE
        for (uint32_t i = (uint32_t)tid; i < len; i += UNION_BLOCK) s_key[i] = i < la ? A[a0 + i] : B[b0 + (i - la)];
        __syncthreads();
        // the lane's positions [p0, p1) of the tile, its split of the two pieces
        const uint32_t p0 = min((uint32_t)tid * UNION_ITEMS, len), p1 = min(p0 + UNION_ITEMS, len);
        const uint64_t *sa = s_key, *sb = s_key + la;
        uint32_t ia = (uint32_t)union_split(sa, (uint64_t)la, sb, (uint64_t)lb, (uint64_t)p0), ib = p0 - ia;
        // the predecessor of position p0 in merged order, from the inputs
        const uint64_t ga = a0 + ia, gb = b0 + ib;
        bool has_prev = ga > 0 || gb > 0;
        uint64_t prev = 0;
        if (p0 < p1) {
            if (ga > 0) prev = A[ga - 1];
            if (gb > 0) { const uint64_t pb = B[gb - 1]; if (ga == 0 || pb > prev) prev = pb; }
        }
        uint64_t item[UNION_ITEMS];   // (indexed by the unrolled j alone: registers)
        uint32_t kept = 0;            // bit j: item j survives
#pragma unroll
        for (int j = 0; j < UNION_ITEMS; ++j) {
            item[j] = 0;
            if (p0 + j < p1) {
                const bool from_a = ia < la && (ib >= lb || sa[ia] <= sb[ib]);
                const uint64_t key = from_a ? sa[ia] : sb[ib];
                if (from_a) ++ia; else ++ib;
                item[j] = key;
                if (!has_prev || key != prev) kept |= 1u << j;
                prev = key;
                has_prev = true;
            }
        }
        const uint32_t n_keep = (uint32_t)__popc(kept);
        // survivors before this lane, in the tile
        uint32_t incl = n_keep;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();   // (and every lane has read its keys from s_key)
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < UNION_BLOCK / 64; ++w) {
            const uint32_t x = s_wave[w];
            if (w < wave) before += x;
            total += x;
        }
        if (!WRITE) {
            if (tid == 0) cnt[tile] = total;
        } else {
            uint32_t at = before + incl - n_keep;
#pragma unroll
            for (int j = 0; j < UNION_ITEMS; ++j)
                if ((kept >> j) & 1u) s_key[at++] = item[j];   // at < total <= len
            __syncthreads();
            const uint64_t base = tile_off[tile];
            for (uint32_t i = (uint32_t)tid; i < total; i += UNION_BLOCK) out[base + i] = s_key[i];
        }
    }
}

// the count, offset and scan workspaces of a call's merges, taken once for the largest of them (the merges run one after the other)
struct UnionWork {
    DevTmp<uint32_t> cnt;
    DevTmp<uint64_t> off;
    DevTmp<uint8_t> scratch;
    hipError_t alloc(uint64_t n_keys) {
        const uint64_t tiles = (n_keys + UNION_TILE - 1) / UNION_TILE + 1;
        hipError_t e = cnt.alloc(tiles * 4);
        if (e == hipSuccess) e = off.alloc(tiles * 8);
        if (e == hipSuccess) e = scratch.alloc(scan_scratch_bytes(tiles));
        return e;
    }
};

// one merge: *out (hipMalloc, na + nb keys of room), *n_out
static int union_pair(pf_ctx *ctx, UnionWork &w, const uint64_t *A, uint64_t na, const uint64_t *B, uint64_t nb, uint64_t **out, uint64_t *n_out) {
    const uint64_t n = na + nb, n_tiles = (n + UNION_TILE - 1) / UNION_TILE;
    *out = nullptr;
    *n_out = 0;
    DevTmp<uint64_t> res;
    {
        const hipError_t e = res.alloc(std::max<uint64_t>(n, 1) * 8);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            pf::CtxErr{ctx} = "pf_kmer_union: " + pf_runmulti::no_room_text("the merged keys", n * 8, free_b, na, nb);
            return PF_ERR_OVERFLOW;
        }
        PF_HIP(e);
    }
    if (n_tiles) {
        PF_HIP(hipMemsetAsync(w.cnt.p + n_tiles, 0, 4, ctx->stream));
        const int grid = ctx_grid(ctx, n_tiles * UNION_BLOCK, UNION_BLOCK, 8);
        k_union_merge<false><<<grid, UNION_BLOCK, 0, ctx->stream>>>(A, na, B, nb, n_tiles, w.cnt.p, nullptr, nullptr);
        PF_HIP(hipGetLastError());
        PF_HIP(scan_exclusive_u32_u64(w.cnt.p, w.off.p, n_tiles + 1, w.scratch.p, ctx->stream));
        k_union_merge<true><<<grid, UNION_BLOCK, 0, ctx->stream>>>(A, na, B, nb, n_tiles, nullptr, w.off.p, res.p);
        PF_HIP(hipGetLastError());
        PF_HIP(hipMemcpyAsync(n_out, w.off.p + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));   // (the next merge reuses the workspaces and asks for this one's size)
    }
    *out = res.p;
    res.p = nullptr;
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_kmer_union(pf_ctx *ctx, uint32_t n_sets, const uint64_t *const *sets_dev, const uint64_t *n, uint64_t **out_dev, uint64_t *n_out) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (!out_dev || !n_out) return refuse("pf_kmer_union: out_dev and n_out are needed");
    *out_dev = nullptr;
    *n_out = 0;
    if (n_sets == 0) return refuse("pf_kmer_union: no set");
    if (n_sets > pf_runmulti::MAX_SETS) return refuse(std::string("pf_kmer_union: ") + pf_runmulti::TOO_MANY_SETS_TEXT + ": " + std::to_string(n_sets));
    if (!sets_dev || !n) return refuse("pf_kmer_union: sets_dev and n are needed");
    uint64_t sum = 0;
    for (uint32_t c = 0; c < n_sets; ++c) {
        if (n[c] >= (1ull << 40) || (sum += n[c]) >= (1ull << 40)) return refuse("pf_kmer_union: more than 2^40 keys");
        if (n[c] && !is_device_ptr(sets_dev[c])) return refuse("pf_kmer_union: set " + std::to_string(c) + " is not an array on the device");
        if (n[c] && ((uintptr_t)sets_dev[c] & 7)) return refuse("pf_kmer_union: set " + std::to_string(c) + " is not aligned");
    }
    PF_HIP(hipSetDevice(ctx->device));
    ctx_begin(ctx, PF_K_UNION);
    struct End { pf_ctx *c; ~End() { ctx_end(c); } } end{ctx};
    // ---- every set is ascending and distinct: refused before anything is merged ----
    {
        DevTmp<UnionFlags> flags;
        PF_HIP(flags.alloc(n_sets * sizeof(UnionFlags)));
        PF_HIP(hipMemsetAsync(flags.p, 0, n_sets * sizeof(UnionFlags), ctx->stream));
        for (uint32_t c = 0; c < n_sets; ++c)
            if (n[c] > 1) k_union_check<<<ctx_grid(ctx, n[c], 256, 8), 256, 0, ctx->stream>>>(sets_dev[c], n[c], flags.p + c);
        PF_HIP(hipGetLastError());
        std::vector<UnionFlags> h(n_sets);
        PF_HIP(hipMemcpyAsync(h.data(), flags.p, n_sets * sizeof(UnionFlags), hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t c = 0; c < n_sets; ++c) {
            if (h[c].unsorted) return refuse("pf_kmer_union: " + pf_runmulti::unsorted_text(c));
            if (h[c].repeat) return refuse("pf_kmer_union: " + pf_runmulti::repeat_text(c));
        }
    }
    // ---- rounds of pairwise merges; what a round made is freed when the next has read it ----
    struct Set { const uint64_t *p; uint64_t n; bool owned; };
    std::vector<Set> cur(n_sets);
    for (uint32_t c = 0; c < n_sets; ++c) cur[c] = Set{sets_dev[c], n[c], false};
    auto drop = [&](std::vector<Set> &v) { for (Set &s : v) if (s.owned) (void)hipFree(const_cast<uint64_t *>(s.p)); v.clear(); };
    const uint64_t units = sum;
    UnionWork work;   // (a merge takes at most all keys)
    PF_HIP(work.alloc(sum));
    if (n_sets == 1) {   // a copy: the result is the caller's to free, the input stays the caller's
        uint64_t *copy = nullptr;
        const int rc = union_pair(ctx, work, cur[0].p, cur[0].n, nullptr, 0, &copy, n_out);
        if (rc) return rc;
        *out_dev = copy;
        ctx_units(ctx, PF_K_UNION, units);
        return PF_OK;
    }
    for (int round = 0; round < 11 && cur.size() > 1; ++round) {   // 2^10 sets at the most
        std::vector<Set> next;
        for (size_t j = 0; j + 1 < cur.size(); j += 2) {
            uint64_t *m = nullptr, nm = 0;
            const int rc = union_pair(ctx, work, cur[j].p, cur[j].n, cur[j + 1].p, cur[j + 1].n, &m, &nm);
            if (rc) { drop(cur); drop(next); return rc; }
            next.push_back(Set{m, nm, true});
        }
        if (cur.size() & 1) { next.push_back(cur.back()); cur.pop_back(); }   // the odd set is carried
        drop(cur);
        cur.swap(next);
    }
    *out_dev = const_cast<uint64_t *>(cur[0].p);   // (made by a merge: two sets at least)
    *n_out = cur[0].n;
    ctx_units(ctx, PF_K_UNION, units);
    return PF_OK;
}
