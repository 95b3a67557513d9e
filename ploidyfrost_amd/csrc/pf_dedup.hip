// K-DEDUP: duplicate reads dropped on the device (`--dedup`).  The rule -- unit, key, decision, statistics, the table's shape -- is
// pf_dedup_rule.hpp; this file is its device form.  A dedup is state on the context (pf_dedup_begin .. pf_dedup_end): a hash table
// resident in HBM across the chunks of a stream, the number of units taken so far, the device counters.
//
//   insert     k_dedup_insert.  A ROW of 16 lanes per unit, 16 rows a block (K-TRIM's shape).  A lane reads its 16 bases of the raw
//              sequence line as one aligned 16-byte unit and a shift (trim_load_shifted), codes them into one word of 3 bits a base
//              and adds the two terms of the word to its sums; a read longer than 256 bases loops over row steps.  A pair does read
//              1, then read 2.  The row adds its sums with four xor-shuffles (a butterfly: the sums are mod 2^64, any order) and lane
//              0 of a unit that takes part closes the key and inserts it:
//                  s = home(h1);  old = CAS(&slot[s].h1, 0, h1);  when old is 0 or h1: old2 = CAS(&slot[s].h2, 0, h2);  when old2 is 0
//                  or h2 the slot is this key's, otherwise s = s + 1.
//              No lock and NO SPIN: nobody waits for anybody.  Whoever installs h2 first owns the slot; a different key with the same
//              h1 finds its own slot further on, and always the same one, because a slot that holds both words never changes and
//              nothing is deleted -- every slot a probe has passed stays passed.  Then atomicMax(&slot[s].first, ~unit) and
//              atomicAdd(&slot[s].copies, 1), and s goes to the unit's scratch word.  Every access to the table in this kernel is an
//              atomic of agent scope; no plain load decides anything.  A slot is 32 aligned bytes: a probe is one HBM sector.
//   verdict    k_dedup_verdict, a second launch (plain loads): one thread per unit.  A unit that takes part is kept when ~first of its
//              slot is its own number; otherwise its interval becomes (0, 0) in every file and it leaves the call's TrimCounts again
//              (kept, bases_kept of each file; the pair statistics are taken from the intervals afterwards, by k_trim_sizes and
//              k_trimcount_keep).  The smallest number wins whatever order the atomics arrived in.
//   growth     the host knows n (the whole records of the call) before it launches, and the number of entries came back with the last
//              call's final copy of its counters (dedup_settle: no host wait of its own).  2 * (entries + n) <= slots holds before
//              every insert; otherwise k_dedup_rehash moves every used slot, with its unit and its copies, into a table of the
//              needed size (the same protocol; the keys are distinct) and the old one is freed.  At half load a probe never goes
//              round the table; one that did would raise `stuck`, which pf_dedup_stats_get refuses by name.
//   levels     k_dedup_levels, one pass over the table for pf_dedup_stats_get: per-wavefront sums, one integer atomic per statistic
//              and wavefront.
// Everything one call launches here is timed as one launch of PF_K_DEDUP inside the call's own; unit: units that take part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_dedup_dev.hpp"
#include "pf_dedup_rule.hpp"
#include "pf_reads_dev.hpp"
#include "pf_trim_dev.hpp"

static_assert(sizeof(((pf_dedup_stats *)nullptr)->levels) / sizeof(uint64_t) == pf_dedup::LEVELS, "the rule header restates the ABI's levels");

namespace pf {

struct DedupSlot {
    unsigned long long h1, h2, first, copies;   // first = ~(number of the first unit): atomicMax keeps the smallest number
};
static_assert(sizeof(DedupSlot) == 32, "one slot, one 32-byte sector");
constexpr uint64_t DEDUP_NO_SLOT = ~0ull;

struct DedupDev {   // device counters of an open dedup; the first two come back with every call (dedup_settle)
    unsigned long long entries, units;
    unsigned long long stuck;
    unsigned long long unique, max_copies, levels[pf_dedup::LEVELS];   // k_dedup_levels
};

struct DedupState {
    DedupSlot *tab = nullptr;
    uint64_t slots = 0, growths = 0;
    uint32_t bases = 0;
    uint64_t next_unit = 0;          // units taken since the begin
    uint64_t entries = 0;            // as of the last settled launch
    uint64_t units = 0;              // the same: units that took part
    DedupDev *dev = nullptr;
    unsigned long long *h_back = nullptr;   // pinned: {entries, units} of the launch in flight
    hipEvent_t back_done = nullptr;
    bool pending = false;
};
static inline DedupState *dedup_state(pf_ctx *ctx) { return static_cast<DedupState *>(ctx->dedup); }

// ---- device ----
__device__ inline uint64_t dedup_row_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = TRIM_ROW / 2; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, TRIM_ROW), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, TRIM_ROW);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ inline uint64_t dedup_wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)v, o, WAVE), hi = __shfl_down((uint32_t)(v >> 32), o, WAVE);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// the slot of key (h1, h2), claimed when it is new: its index, or DEDUP_NO_SLOT when the probe went round the table.
// `fresh` is raised by the one caller that installed h2.
__device__ inline uint64_t dedup_claim(DedupSlot *tab, uint64_t mask, unsigned long long h1, unsigned long long h2, bool &fresh) {
    uint64_t s = pf_dedup::home(h1, mask + 1);
    for (uint64_t step = 0; step <= mask; ++step) {
        const unsigned long long old = atomicCAS(&tab[s].h1, 0ull, h1);
        if (old == 0ull || old == h1) {
            const unsigned long long old2 = atomicCAS(&tab[s].h2, 0ull, h2);
            if (old2 == 0ull || old2 == h2) { fresh = old2 == 0ull; return s; }
        }
        s = (s + 1) & mask;
    }
    return DEDUP_NO_SLOT;
}
// one unit into the table
__device__ inline uint64_t dedup_insert(DedupSlot *tab, uint64_t mask, uint64_t h1, uint64_t h2, uint64_t unit, uint64_t &fresh_n, uint64_t &stuck_n) {
    bool fresh = false;
    const uint64_t s = dedup_claim(tab, mask, h1, h2, fresh);
    if (s == DEDUP_NO_SLOT) { stuck_n += 1; return s; }
    fresh_n += fresh;
    atomicMax(&tab[s].first, (unsigned long long)~unit);
    atomicAdd(&tab[s].copies, 1ull);
    return s;
}
// a kernel's counters: per-wavefront sums, one integer atomic per counter and wavefront (every lane of the wavefront arrives)
__device__ inline void dedup_counters_out(DedupDev *dev, uint64_t fresh_n, uint64_t units_n, uint64_t stuck_n) {
    fresh_n = wave_sum_u64(fresh_n);
    units_n = wave_sum_u64(units_n);
    stuck_n = wave_sum_u64(stuck_n);
    if (lane_id() == 0) {
        if (fresh_n) atomicAdd(&dev->entries, (unsigned long long)fresh_n);
        if (units_n) atomicAdd(&dev->units, (unsigned long long)units_n);
        if (stuck_n) atomicAdd(&dev->stuck, (unsigned long long)stuck_n);
    }
}

struct DedupArgs {
    const char *text[2];
    uint64_t n_bytes[2];
    const uint32_t *lines[2];
    uint32_t *rec_begin[2], *rec_len[2];
    uint64_t n_rec, unit0;
    int n_files;
    uint32_t bases;
    DedupSlot *tab;
    uint64_t mask;
    uint64_t *slot_of;   // n_rec
    DedupDev *dev;
    TrimCounts *counts;
};

__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_insert(const DedupArgs a) {
    const int rl = (int)threadIdx.x & (TRIM_ROW - 1), row = (int)threadIdx.x / TRIM_ROW;
    uint64_t fresh_n = 0, units_n = 0, stuck_n = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_ROWS + row; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_ROWS) {
        bool takes_part = a.rec_len[0][r] != 0;
        if (a.n_files == 2) takes_part = takes_part && a.rec_len[1][r] != 0;
        uint64_t sum0 = 0, sum1 = 0;
        uint32_t cov[2] = {0, 0};
        for (int f = 0; f < a.n_files; ++f) {
            const uint32_t sb = a.lines[f][8 * r + 2], n = a.lines[f][8 * r + 3] - sb;
            const uint32_t L = takes_part ? pf_dedup::covered(n, a.bases) : 0u;
            cov[f] = L;
            for (uint64_t i0 = 16ull * (uint32_t)rl; i0 < L; i0 += TRIM_STEP_BYTES) {
                const uint32_t cnt = L - i0 < 16 ? (uint32_t)(L - i0) : 16u;
                const uint4 v = trim_load_shifted(a.text[f], a.n_bytes[f], (uint64_t)sb + i0);
                uint64_t word = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((uint32_t)k < cnt) word |= (uint64_t)pf_dedup::code((uint8_t)unit_byte(v, k)) << (pf_dedup::CODE_BITS * k);
                const uint64_t index = pf_dedup::index_of(i0 >> 4, f == 1);
                sum0 += pf_dedup::term(word, index, 0);
                sum1 += pf_dedup::term(word, index, 1);
            }
        }
        sum0 = dedup_row_sum_u64(sum0);
        sum1 = dedup_row_sum_u64(sum1);
        if (rl == 0 && takes_part) {
            const bool pair = a.n_files == 2;
            const uint64_t h1 = pf_dedup::close(sum0, cov[0], cov[1], pair, 0), h2 = pf_dedup::close(sum1, cov[0], cov[1], pair, 1);
            a.slot_of[r] = dedup_insert(a.tab, a.mask, h1, h2, a.unit0 + r, fresh_n, stuck_n);
            units_n += 1;
        }
    }
    dedup_counters_out(a.dev, fresh_n, units_n, stuck_n);
}

__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_verdict(const DedupArgs a) {
    uint64_t gone[2] = {0, 0}, gone_bases[2] = {0, 0};
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_BLOCK) {
        bool takes_part = a.rec_len[0][r] != 0;
        if (a.n_files == 2) takes_part = takes_part && a.rec_len[1][r] != 0;
        if (!takes_part) continue;
        const uint64_t s = a.slot_of[r];
        if (s == DEDUP_NO_SLOT || ~a.tab[s].first == a.unit0 + r) continue;   // the first of its key (or never placed: `stuck` says so)
        for (int f = 0; f < a.n_files; ++f) {
            gone[f] += 1;
            gone_bases[f] += a.rec_len[f][r];
            a.rec_begin[f][r] = 0;
            a.rec_len[f][r] = 0;
        }
    }
    for (int f = 0; f < a.n_files; ++f) {
        const uint64_t g = wave_sum_u64(gone[f]), b = wave_sum_u64(gone_bases[f]);
        if (lane_id() == 0 && g) {   // kept and bases_kept hold this unit since k_trim_intervals: they cannot pass below 0
            atomicAdd(&a.counts[f].kept, (unsigned long long)(0ull - g));
            atomicAdd(&a.counts[f].bases_kept, (unsigned long long)(0ull - b));
        }
    }
}

// the table by itself: key i (two words, forced non-zero) as unit unit0 + i
__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_keys(const uint64_t *__restrict__ keys, uint64_t n, uint64_t unit0, DedupSlot *tab, uint64_t mask,
                                                           uint64_t *__restrict__ slot_of, DedupDev *dev) {
    uint64_t fresh_n = 0, units_n = 0, stuck_n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TRIM_BLOCK) {
        slot_of[i] = dedup_insert(tab, mask, pf_dedup::nonzero(keys[2 * i]), pf_dedup::nonzero(keys[2 * i + 1]), unit0 + i, fresh_n, stuck_n);
        units_n += 1;
    }
    dedup_counters_out(dev, fresh_n, units_n, stuck_n);
}
__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_keys_verdict(const uint64_t *__restrict__ slot_of, uint64_t n, uint64_t unit0,
                                                                   const DedupSlot *__restrict__ tab, uint8_t *__restrict__ keep) {
    for (uint64_t i = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TRIM_BLOCK) {
        const uint64_t s = slot_of[i];
        keep[i] = (s == DEDUP_NO_SLOT || ~tab[s].first == unit0 + i) ? 1 : 0;
    }
}

// every used slot of the old table into the new one, with its unit and its copies (the keys of a table are distinct)
__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_rehash(const DedupSlot *__restrict__ old_tab, uint64_t old_slots, DedupSlot *tab, uint64_t mask,
                                                             DedupDev *dev) {
    uint64_t stuck_n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * TRIM_BLOCK) {
        const DedupSlot o = old_tab[i];
        if (o.h1 == 0ull) continue;
        bool fresh = false;
        const uint64_t s = dedup_claim(tab, mask, o.h1, o.h2, fresh);
        if (s == DEDUP_NO_SLOT) { stuck_n += 1; continue; }
        atomicMax(&tab[s].first, o.first);
        atomicAdd(&tab[s].copies, o.copies);
    }
    stuck_n = wave_sum_u64(stuck_n);
    if (lane_id() == 0 && stuck_n) atomicAdd(&dev->stuck, (unsigned long long)stuck_n);
}

__global__ __launch_bounds__(TRIM_BLOCK) void k_dedup_levels(const DedupSlot *__restrict__ tab, uint64_t slots, DedupDev *dev) {
    uint64_t unique = 0, max_copies = 0, levels[pf_dedup::LEVELS];
#pragma unroll
    for (uint32_t l = 0; l < pf_dedup::LEVELS; ++l) levels[l] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TRIM_BLOCK + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * TRIM_BLOCK) {
        const uint64_t c = tab[i].copies;
        if (c == 0) continue;
        unique += 1;
        max_copies = c > max_copies ? c : max_copies;
        const uint32_t lv = pf_dedup::level_of(c);
#pragma unroll
        for (uint32_t l = 0; l < pf_dedup::LEVELS; ++l) levels[l] += lv == l;
    }
    unique = wave_sum_u64(unique);
    max_copies = dedup_wave_max_u64(max_copies);
    if (lane_id() == 0) {
        if (unique) atomicAdd(&dev->unique, (unsigned long long)unique);
        if (max_copies) atomicMax(&dev->max_copies, (unsigned long long)max_copies);
    }
#pragma unroll
    for (uint32_t l = 0; l < pf_dedup::LEVELS; ++l) {
        const uint64_t v = wave_sum_u64(levels[l]);
        if (lane_id() == 0 && v) atomicAdd(&dev->levels[l], (unsigned long long)v);
    }
}

// ---- host side ----
static int dedup_launch_error(pf_ctx *ctx) {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-DEDUP launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    return PF_OK;
}

void dedup_settle(pf_ctx *ctx) {
    DedupState *S = dedup_state(ctx);
    if (!S || !S->pending) return;
    (void)hipEventSynchronize(S->back_done);   // behind the caller's own final wait this returns at once
    const uint64_t units = S->h_back[1];
    S->entries = S->h_back[0];
    ctx_units(ctx, PF_K_DEDUP, units - S->units);
    S->units = units;
    S->pending = false;
}

// the invariant 2 * (entries + n) <= slots before a launch that inserts n units: grows and rehashes when it does not hold
static int dedup_reserve(pf_ctx *ctx, DedupState *S, uint64_t n) {
    dedup_settle(ctx);
    const uint64_t need = pf_dedup::needed_slots(S->slots, S->entries, n);
    if (need == S->slots) return PF_OK;
    size_t free_b = 0, total_b = 0;
    PF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need == 0 || need > (1ull << 40) || need * sizeof(DedupSlot) > free_b) {
        pf::CtxErr{ctx} = "pf_dedup: the table of " + std::to_string(need) + " slots (" + std::to_string(need * sizeof(DedupSlot)) +
                          " bytes) does not fit beside the old one in the free device memory (" + std::to_string(free_b) + " bytes) at " +
                          std::to_string(S->next_unit) + " units";
        return PF_ERR_OVERFLOW;
    }
    DedupSlot *grown = nullptr;
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&grown), need * sizeof(DedupSlot)));
    struct Undo { DedupSlot *p; ~Undo() { if (p) (void)hipFree(p); } } undo{grown};
    PF_HIP(hipMemsetAsync(grown, 0, need * sizeof(DedupSlot), ctx->stream));
    k_dedup_rehash<<<ctx_grid(ctx, S->slots, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(S->tab, S->slots, grown, need - 1, S->dev);
    { const int rc = dedup_launch_error(ctx); if (rc) return rc; }
    PF_HIP(hipStreamSynchronize(ctx->stream));   // the old table is read until here (a growth is rare: the size at least doubles)
    undo.p = S->tab;   // freed
    S->tab = grown;
    S->slots = need;
    S->growths += 1;
    return PF_OK;
}

// {entries, units} of the launches so far to the pinned words, behind everything queued: the caller's final wait passes it
static int dedup_send_back(pf_ctx *ctx, DedupState *S) {
    PF_HIP(hipMemcpyAsync(S->h_back, S->dev, 16, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipEventRecord(S->back_done, ctx->stream));
    S->pending = true;
    return PF_OK;
}

int dedup_launch(pf_ctx *ctx, int n_files, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec,
                 uint32_t *const *rec_begin, uint32_t *const *rec_len, TrimCounts *counts) {
    DedupState *S = dedup_state(ctx);
    if (!S) { pf::CtxErr{ctx} = "K-DEDUP: no dedup is open"; return PF_ERR_ARG; }
    if (n_rec == 0) return PF_OK;
    size_t at = (size_t)-1;
    (void)ctx_begin_at(ctx, PF_K_DEDUP, ctx->stream, &at);
    struct End { pf_ctx *c; size_t at; ~End() { ctx_end_at(c, at, c->stream); } } end{ctx, at};
    { const int rc = dedup_reserve(ctx, S, n_rec); if (rc) return rc; }
    uint64_t *slot_of = static_cast<uint64_t *>(ctx_ws(ctx, WS_DEDUP, (size_t)n_rec * 8));
    if (!slot_of) return PF_ERR_HIP;
    DedupArgs a = {};
    for (int f = 0; f < n_files; ++f) {
        a.text[f] = text[f];
        a.n_bytes[f] = n_bytes[f];
        a.lines[f] = lines[f];
        a.rec_begin[f] = rec_begin[f];
        a.rec_len[f] = rec_len[f];
    }
    a.n_rec = n_rec;
    a.unit0 = S->next_unit;
    a.n_files = n_files;
    a.bases = S->bases;
    a.tab = S->tab;
    a.mask = S->slots - 1;
    a.slot_of = slot_of;
    a.dev = S->dev;
    a.counts = counts;
    k_dedup_insert<<<ctx_grid(ctx, n_rec * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(a);
    k_dedup_verdict<<<ctx_grid(ctx, n_rec, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(a);
    { const int rc = dedup_launch_error(ctx); if (rc) return rc; }
    S->next_unit += n_rec;
    return dedup_send_back(ctx, S);
}

void dedup_destroy(pf_ctx *ctx) {
    DedupState *S = dedup_state(ctx);
    if (!S) return;
    if (S->tab) (void)hipFree(S->tab);
    if (S->dev) (void)hipFree(S->dev);
    if (S->h_back) (void)hipHostFree(S->h_back);
    if (S->back_done) (void)hipEventDestroy(S->back_done);
    delete S;
    ctx->dedup = nullptr;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_dedup_begin(pf_ctx *ctx, uint32_t bases, uint64_t initial_slots) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_dedup_begin: " + m; return (int)PF_ERR_ARG; };
    if (ctx->dedup) return refuse("a dedup is open already");
    if (!pf_dedup::bases_ok(bases))
        return refuse("bases is 0 (the whole read) or " + std::to_string(pf_dedup::MIN_BASES) + " .. " + std::to_string(pf_dedup::MAX_BASES) + ", not " +
                      std::to_string(bases));
    if (initial_slots > (1ull << 40)) return refuse("initial_slots is at most 2^40, not " + std::to_string(initial_slots));
    PF_HIP(hipSetDevice(ctx->device));
    const uint64_t slots = pf_dedup::round_slots(initial_slots);
    size_t free_b = 0, total_b = 0;
    PF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (slots * sizeof(DedupSlot) > free_b) {
        pf::CtxErr{ctx} = "pf_dedup: the table of " + std::to_string(slots) + " slots (" + std::to_string(slots * sizeof(DedupSlot)) +
                          " bytes) does not fit in the free device memory (" + std::to_string(free_b) + " bytes) at 0 units";
        return PF_ERR_OVERFLOW;
    }
    DedupState *S = new DedupState;
    ctx->dedup = S;
    S->bases = bases;
    S->slots = slots;
    struct Undo { pf_ctx *c; bool armed; ~Undo() { if (armed) dedup_destroy(c); } } undo{ctx, true};
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->tab), slots * sizeof(DedupSlot)));
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->dev), sizeof(DedupDev)));
    PF_HIP(hipHostMalloc(reinterpret_cast<void **>(&S->h_back), 16, hipHostMallocDefault));
    PF_HIP(hipEventCreateWithFlags(&S->back_done, hipEventDisableTiming));
    PF_HIP(hipMemsetAsync(S->tab, 0, slots * sizeof(DedupSlot), ctx->stream));
    PF_HIP(hipMemsetAsync(S->dev, 0, sizeof(DedupDev), ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    undo.armed = false;
    return PF_OK;
}

extern "C" int pf_dedup_stats_get(pf_ctx *ctx, pf_dedup_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_dedup_stats_get: " + m; return (int)PF_ERR_ARG; };
    DedupState *S = dedup_state(ctx);
    if (!S) return refuse("no dedup is open");
    if (!stats) return refuse("stats is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemsetAsync(&S->dev->unique, 0, sizeof(DedupDev) - offsetof(DedupDev, unique), ctx->stream));
    k_dedup_levels<<<ctx_grid(ctx, S->slots, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(S->tab, S->slots, S->dev);
    { const int rc = dedup_launch_error(ctx); if (rc) return rc; }
    DedupDev h = {};
    PF_HIP(hipMemcpyAsync(&h, S->dev, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    dedup_settle(ctx);
    if (h.stuck) {
        pf::CtxErr{ctx} = "pf_dedup_stats_get: " + std::to_string(h.stuck) + " units found no slot: a probe went round the table of " + std::to_string(S->slots) +
                          " slots";
        return PF_ERR_OVERFLOW;
    }
    *stats = pf_dedup_stats{};
    stats->units = h.units;
    stats->unique = h.unique;
    stats->duplicates = h.units - h.unique;
    stats->max_copies = h.max_copies;
    for (uint32_t l = 0; l < pf_dedup::LEVELS; ++l) stats->levels[l] = h.levels[l];
    stats->slots = S->slots;
    stats->growths = S->growths;
    return PF_OK;
}

extern "C" int pf_dedup_keys(pf_ctx *ctx, const uint64_t *keys, uint64_t n, uint8_t *keep) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_dedup_keys: " + m; return (int)PF_ERR_ARG; };
    DedupState *S = dedup_state(ctx);
    if (!S) return refuse("no dedup is open");
    if (n == 0) return PF_OK;
    if (!keys || !keep) return refuse("keys and keep are needed");
    if (n > (1ull << 32)) return refuse("a call holds at most 2^32 keys, not " + std::to_string(n));
    PF_HIP(hipSetDevice(ctx->device));
    size_t at = (size_t)-1;
    (void)ctx_begin_at(ctx, PF_K_DEDUP, ctx->stream, &at);
    struct End { pf_ctx *c; size_t at; ~End() { ctx_end_at(c, at, c->stream); } } end{ctx, at};
    { const int rc = dedup_reserve(ctx, S, n); if (rc) return rc; }
    const bool keys_dev = is_device_ptr(keys), keep_dev = is_device_ptr(keep);
    const size_t slot_bytes = up256((size_t)n * 8), key_bytes = keys_dev ? 0 : up256((size_t)n * 16), keep_bytes = keep_dev ? 0 : up256((size_t)n);
    char *ww = static_cast<char *>(ctx_ws(ctx, WS_DEDUP, slot_bytes + key_bytes + keep_bytes));
    if (!ww) return PF_ERR_HIP;
    uint64_t *slot_of = reinterpret_cast<uint64_t *>(ww);
    const uint64_t *d_keys = keys;
    if (!keys_dev) {
        PF_HIP(hipMemcpyAsync(ww + slot_bytes, keys, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        d_keys = reinterpret_cast<const uint64_t *>(ww + slot_bytes);
    }
    uint8_t *d_keep = keep_dev ? keep : reinterpret_cast<uint8_t *>(ww + slot_bytes + key_bytes);
    k_dedup_keys<<<ctx_grid(ctx, n, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(d_keys, n, S->next_unit, S->tab, S->slots - 1, slot_of, S->dev);
    k_dedup_keys_verdict<<<ctx_grid(ctx, n, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(slot_of, n, S->next_unit, S->tab, d_keep);
    { const int rc = dedup_launch_error(ctx); if (rc) return rc; }
    S->next_unit += n;
    if (!keep_dev) PF_HIP(hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    { const int rc = dedup_send_back(ctx, S); if (rc) return rc; }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    dedup_settle(ctx);
    return PF_OK;
}

extern "C" int pf_dedup_end(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    if (!ctx->dedup) { pf::CtxErr{ctx} = "pf_dedup_end: no dedup is open"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    unsigned long long stuck = 0;   // (a dedup closed without pf_dedup_stats_get is still held to it)
    const hipError_t e = hipMemcpyAsync(&stuck, &dedup_state(ctx)->dev->stuck, 8, hipMemcpyDeviceToHost, ctx->stream);
    PF_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t slots = dedup_state(ctx)->slots;
    dedup_destroy(ctx);
    if (e == hipSuccess && stuck) {
        pf::CtxErr{ctx} = "pf_dedup_end: " + std::to_string(stuck) + " units found no slot: a probe went round the table of " + std::to_string(slots) + " slots";
        return PF_ERR_OVERFLOW;
    }
    return PF_OK;
}
