// What K-COUNT (pf_count.hip) and K-MASKCOUNT (pf_maskcount.hip) share: the open count of a context -- its table of 16-byte slots in
// HBM, the claim of a slot, the device counters -- and the host steps around a launch that inserts (the load bound, the totals).
// Device code is inline: each of the two files carries its own copy (no device-side calls across files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ploidyfrost_hip.h"
#include "pf_count_rule.hpp"
#include "pf_ctx.hpp"
#include "pf_device_common.hpp"
#include "pf_reads_dev.hpp"

namespace pf {

struct CountSlot {
    unsigned long long key;
    uint32_t count, pad;
};
static_assert(sizeof(CountSlot) == 16, "one slot, one 16-byte vector access");
constexpr uint64_t COUNT_MIN_SLOTS = 64;   // one word of the kept bitmap

struct CountDev {   // device counters of one run
    unsigned long long occupied;                  // claimed slots, exact
    unsigned long long unique, below, above;      // k_count_flag
    uint32_t overflow, stuck;                     // a counter wrapped; a probe went round the table
};

struct CountState {
    CountSlot *tab = nullptr;
    uint64_t slots = 0, occupied = 0, initial_slots = 0;
    int k = 0;
    bool both_strands = true;
    CountDev *dev = nullptr;
    pf_count_stats total = {};
};

__device__ inline uint64_t slot_key(const CountSlot *s) {
    return __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of `key`: its own, or an empty one claimed for it.  0 = found, 1 = claimed, 2 = the probe went round the table
__device__ inline int count_claim(CountSlot *tab, uint64_t mask, uint64_t key, uint64_t &slot) {
    uint64_t s = mix64(key) & mask;
    for (uint64_t step = 0; step <= mask; ++step) {
        unsigned long long cur = slot_key(tab + s);
        int claimed = 0;
        if (cur == pf_count::EMPTY_KEY) {
            cur = atomicCAS(&tab[s].key, (unsigned long long)pf_count::EMPTY_KEY, (unsigned long long)key);
            if (cur == pf_count::EMPTY_KEY) { cur = key; claimed = 1; }
        }
        if (cur == key) { slot = s; return claimed; }
        s = (s + 1) & mask;
    }
    return 2;
}

// ---- host side (pf_count.hip) ----
inline CountState *count_state(pf_ctx *ctx) { return static_cast<CountState *>(ctx->count); }
// the invariant: occupied + add <= 3/4 slots before a launch that can claim `add` slots (grows and rehashes when it does not hold)
int count_reserve(pf_ctx *ctx, CountState *S, uint64_t add);
// after a launch that inserted: the call's counters and the run's to the host, the claimed slots taken over, a probe that went round
// the table refused by name
int count_after_insert(pf_ctx *ctx, CountState *S, const char *who, MaskCounts *counts, MaskCounts &h);

// ---- what K-TRIMCOUNT (pf_trimcount.hip) runs over the table it made ----
// pf_count.hip: an open count, by `who`; classes and insert over text[0, n) on the device with the table of reads on the device
// (counts reset by the caller, n > 0; `counts` accumulates over calls, h is their state after this one); this call's statistics and
// its share of the totals pf_count_finish reports
int count_needs_begin(pf_ctx *ctx, const char *who);
int count_core(pf_ctx *ctx, CountState *S, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len, uint64_t n_reads, MaskCounts *counts,
               MaskCounts &h);
void count_stats_out(pf_count_stats *stats, CountState *S, uint64_t n_reads, const MaskCounts &h);
// pf_maskcount.hip: a resident table, an open count on both strands, the same k, each missing piece by `who`; classes, flag and
// insert; the statistics
int maskcount_needs(pf_ctx *ctx, const char *who);
int maskcount_core(pf_ctx *ctx, CountState *S, const char *text, uint64_t n, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t low,
                   uint32_t up, MaskCounts *counts, MaskCounts &h);
void maskcount_stats_out(pf_maskcount_stats *stats, CountState *S, uint64_t n_reads, const MaskCounts &h);

}  // namespace pf
