// What K-TRIM (pf_trim.hip) and K-TRIMCOUNT (pf_trimcount.hip) share on the device: the steps of a call by value, the per-file
// counters, and k_trim_intervals -- the interval [b, e) of every record of a chunk (the rule: pf_trim_rule.hpp), from [0, n) or, with
// a clip open (pf_clip_dev.hpp), from [0, clip end).  Kernels are `static`:
// each of the two files carries its own copy (no device-side calls across files), as with pf_reads_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_trim_rule.hpp"

static_assert(sizeof(pf_trim_step) == sizeof(pf_trim::Step) && sizeof(pf_trim_stats) == sizeof(pf_trim::Stats), "the rule header restates the ABI's records");
static_assert((int)PF_TRIM_LEADING == (int)pf_trim::KIND_LEADING && (int)PF_TRIM_TRAILING == (int)pf_trim::KIND_TRAILING &&
              (int)PF_TRIM_SLIDINGWINDOW == (int)pf_trim::KIND_SLIDINGWINDOW && (int)PF_TRIM_MINLEN == (int)pf_trim::KIND_MINLEN &&
              PF_TRIM_MAX_STEPS == pf_trim::MAX_STEPS, "the rule header restates the ABI's constants");

namespace pf {

constexpr int TRIM_BLOCK = 256;
constexpr int TRIM_ROW = 16;                                   // lanes of a row: one read
constexpr int TRIM_ROWS = TRIM_BLOCK / TRIM_ROW;               // rows of a block
constexpr int TRIM_STEP_BYTES = TRIM_ROW * 16;                 // bytes of a row step
constexpr int TRIM_HALO_UNITS = 4;                             // 64 bytes behind them: the rest of the last window, w - 1 <= 63
constexpr int TRIM_UNITS = TRIM_ROW + TRIM_HALO_UNITS;
constexpr uint32_t TRIM_NONE = 0xFFFFFFFFu;
static_assert(pf_trim::MAX_W - 1 <= 16 * TRIM_HALO_UNITS, "the halo holds the rest of a row step's last window");

struct TrimSteps {   // by value
    uint32_t n, phred;
    pf_trim::Step s[pf_trim::MAX_STEPS];
};
struct TrimCounts {   // device side of pf_trim_stats: [0], [1] per file; the pair fields in [0]
    unsigned long long kept, bases, bases_kept, both, only1, only2;
};

__device__ inline uint32_t row_min_u32(uint32_t v) {
#pragma unroll
    for (int o = TRIM_ROW / 2; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, TRIM_ROW));
    return v;
}
__device__ inline uint32_t row_max_u32(uint32_t v) {
#pragma unroll
    for (int o = TRIM_ROW / 2; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, TRIM_ROW));
    return v;
}
// the lanes of a row run together: its LDS is written, then read by other lanes of the same row
__device__ inline void row_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// the 16 bytes of the text from byte s: one aligned unit, or two and a shift (K-TRIM's copy, K-QC's reads)
__device__ inline uint4 trim_load_shifted(const char *__restrict__ text, uint64_t n, uint64_t s) {
    const uint4 lo = mask_load_unit(text, n, s >> 4);
    const uint32_t sh = (uint32_t)(s & 15);
    if (sh == 0) return lo;
    const uint4 hi = mask_load_unit(text, n, (s >> 4) + 1);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t d = sh >> 2, bits = (sh & 3) * 8;
    uint32_t t[5], o[4];
#pragma unroll
    for (int i = 0; i < 5; ++i) t[i] = d == 0 ? w[i] : d == 1 ? w[i + 1] : d == 2 ? w[i + 2] : w[i + 3];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (uint32_t)(((((uint64_t)t[i + 1]) << 32) | t[i]) >> bits);
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- intervals ----
[[maybe_unused]] static __global__ __launch_bounds__(TRIM_BLOCK) void k_trim_intervals(const char *__restrict__ text, uint64_t n_bytes, const uint32_t *__restrict__ lines,
                                                               uint64_t n_rec, const TrimSteps ts, uint32_t *__restrict__ rec_begin,
                                                               uint32_t *__restrict__ rec_len, TrimCounts *c,
                                                               const uint32_t *__restrict__ clip_end = nullptr) {
    __shared__ uint4 s_q[TRIM_ROWS][TRIM_UNITS];
    const int rl = (int)threadIdx.x & (TRIM_ROW - 1), row = (int)threadIdx.x / TRIM_ROW;
    uint4 *sq = s_q[row];
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(sq);
    const int x0 = 16 * rl;   // this lane's first byte of the row step
    uint64_t kept = 0, bases = 0, bases_kept = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_ROWS + row; r < n_rec; r += (uint64_t)gridDim.x * TRIM_ROWS) {
        const uint32_t qb = lines[8 * r + 6], n = lines[8 * r + 7] - qb;
        const uint64_t unit0 = qb >> 4;          // the aligned unit that holds the line's first byte
        const uint32_t mis = qb & 15u;           // position p of the read is byte mis + p from there
        uint32_t b = 0, e = clip_end ? clip_end[r] : n;   // K-CLIP (pf_clip.hip): the interval starts as [0, clip end), 0 = dropped
        bool alive = e > 0;                      // (every step keeps e > b while the read lives)
        int64_t staged = -1;
        // row step `chunk` of the line into the row's LDS; position of byte x of it: chunk * 256 + x - mis
        auto stage = [&](int64_t chunk) {
            if (staged == chunk) return;
            row_sync();   // the last row step has been read
            const uint64_t u = unit0 + (uint64_t)chunk * TRIM_ROW + (uint64_t)rl;
            sq[rl] = mask_load_unit(text, n_bytes, u);
            if (rl < TRIM_HALO_UNITS) sq[TRIM_ROW + rl] = mask_load_unit(text, n_bytes, u + TRIM_ROW);
            row_sync();
            staged = chunk;
        };
        // bits of this lane's 16 positions that lie in [lo, hi)
        auto inside = [&](int64_t base, uint32_t lo, uint32_t hi) {
            int64_t a = (int64_t)lo - base, z = (int64_t)hi - base;
            a = a < 0 ? 0 : a > 16 ? 16 : a;
            z = z < 0 ? 0 : z > 16 ? 16 : z;
            return z > a ? ((1u << z) - 1u) & ~((1u << a) - 1u) : 0u;
        };
        auto good_bits = [&](uint32_t thr) {   // byte >= t + phred, i.e. q >= t
            const uint4 v = sq[rl];
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) m |= (uint32_t)(unit_byte(v, k) >= thr) << k;
            return m;
        };
        for (uint32_t s = 0; s < ts.n && alive; ++s) {
            const pf_trim::Step st = ts.s[s];
            if (st.kind == pf_trim::KIND_LEADING) {
                uint32_t first = TRIM_NONE;
                const int64_t c1 = ((int64_t)mis + e - 1) >> 8;
                for (int64_t ch = ((int64_t)mis + b) >> 8; ch <= c1 && first == TRIM_NONE; ++ch) {
                    stage(ch);
                    const int64_t base = ch * TRIM_STEP_BYTES + x0 - (int64_t)mis;
                    const uint32_t m = good_bits(st.a + ts.phred) & inside(base, b, e);
                    first = row_min_u32(m ? (uint32_t)(base + (__ffs((int)m) - 1)) : TRIM_NONE);
                }
                if (first == TRIM_NONE) alive = false; else b = first;
            } else if (st.kind == pf_trim::KIND_TRAILING) {
                uint32_t end = 0;   // 1 + the last good position, 0 = none
                const int64_t c0 = ((int64_t)mis + b) >> 8;
                for (int64_t ch = ((int64_t)mis + e - 1) >> 8; ch >= c0 && end == 0; --ch) {
                    stage(ch);
                    const int64_t base = ch * TRIM_STEP_BYTES + x0 - (int64_t)mis;
                    const uint32_t m = good_bits(st.a + ts.phred) & inside(base, b, e);
                    end = row_max_u32(m ? (uint32_t)(base + (31 - __clz((int)m)) + 1) : 0u);
                }
                if (end == 0) alive = false; else e = end;
            } else if (st.kind == pf_trim::KIND_SLIDINGWINDOW) {
                const uint32_t w = st.a;
                if (e - b < w) { alive = false; continue; }
                const uint32_t last_start = e - w;   // windows start in [b, last_start]
                uint32_t bad = TRIM_NONE;
                const int64_t c1 = ((int64_t)mis + last_start) >> 8;
                for (int64_t ch = ((int64_t)mis + b) >> 8; ch <= c1 && bad == TRIM_NONE; ++ch) {
                    stage(ch);
                    const int64_t base = ch * TRIM_STEP_BYTES + x0 - (int64_t)mis;
                    const uint32_t in = inside(base, b, last_start + 1);
                    uint32_t mine = TRIM_NONE;
                    if (in) {
                        const int k0 = __ffs((int)in) - 1, k1 = 31 - __clz((int)in);
                        uint32_t sum = 0;
                        for (uint32_t i = 0; i < w; ++i) sum += sb[x0 + k0 + (int)i];
                        for (int k = k0;; ++k) {
                            if (pf_trim::window_bad_bytes(sum, w, st.b, ts.phred)) { mine = (uint32_t)(base + k); break; }
                            if (k == k1) break;
                            sum += (uint32_t)sb[x0 + k + (int)w] - (uint32_t)sb[x0 + k];
                        }
                    }
                    bad = row_min_u32(mine);
                }
                if (bad == b) alive = false;
                else if (bad != TRIM_NONE) e = pf_trim::sliding_end(b, bad - b, w);
            } else {   // KIND_MINLEN
                if (pf_trim::too_short(b, e, st.a)) alive = false;
            }
        }
        if (rl == 0) {
            rec_begin[r] = alive ? b : 0u;
            rec_len[r] = alive ? e - b : 0u;
            kept += alive;
            bases += n;
            bases_kept += alive ? e - b : 0u;
        }
    }
    kept = wave_sum_u64(kept);
    bases = wave_sum_u64(bases);
    bases_kept = wave_sum_u64(bases_kept);
    if (lane_id() == 0) {
        if (kept) atomicAdd(&c->kept, (unsigned long long)kept);
        if (bases) atomicAdd(&c->bases, (unsigned long long)bases);
        if (bases_kept) atomicAdd(&c->bases_kept, (unsigned long long)bases_kept);
    }
}

// ---- host side ----
// the steps and the offset of one call: "" = accepted, else the refusal as K-TRIM words it (without the caller's name)
// (clip_open: a clip is open on the context, and no step beside it is a plan as well)
static inline std::string trim_steps_refusal(const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, bool clip_open = false) {
    uint32_t bad_step = 0;
    const int c = pf_trim::steps_clause(reinterpret_cast<const pf_trim::Step *>(steps), n_steps, phred, &bad_step);
    if (!c || (c == pf_trim::REFUSE_NO_STEP && clip_open && n_steps == 0)) return "";
    if (c == pf_trim::REFUSE_PHRED) return std::string(pf_trim::refusal_text(c)) + ", not " + std::to_string(phred);
    if (c == pf_trim::REFUSE_NO_STEP || c == pf_trim::REFUSE_TOO_MANY) return pf_trim::refusal_text(c);
    return "step " + std::to_string(bad_step) + ": " + pf_trim::refusal_text(c);
}
static inline TrimSteps trim_steps_by_value(const pf_trim_step *steps, uint32_t n_steps, uint32_t phred) {
    TrimSteps ts = {};
    ts.n = n_steps;
    ts.phred = phred;
    for (uint32_t s = 0; s < n_steps; ++s) ts.s[s] = pf_trim::Step{steps[s].kind, steps[s].a, steps[s].b};
    return ts;
}

// the text of file f on the device, 16-byte aligned (mask_stage_text for a slot of the caller's choice)
static inline int trim_stage_text(pf_ctx *ctx, int slot, const char *text, uint64_t n, const char **dev) {
    if (is_device_ptr(text) && ((uintptr_t)text & 15) == 0) { *dev = text; return PF_OK; }
    char *p = static_cast<char *>(ctx_ws(ctx, slot, (size_t)n + 16));
    if (!p) return PF_ERR_HIP;
    PF_HIP(hipMemcpyAsync(p, text, (size_t)n, hipMemcpyDefault, ctx->stream));
    *dev = p;
    return PF_OK;
}

}  // namespace pf
