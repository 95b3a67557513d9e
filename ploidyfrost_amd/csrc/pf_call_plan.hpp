// The sizing plan of the resident calling pipeline: every grid, per-wavefront scratch size and first-call pool capacity that
// pf_call_align_lane asks for and pf_call_reserve_lanes takes ahead of it (pf_call.hip), in one place, so that a reserved first
// pass finds every buffer it wants.  Plain host C++ without a HIP include: tests/cpp/test_call_plan.cpp holds the numbers.
// (K-PAIR's and K-STACK's per-wavefront scratch stay with their kernels -- PairGeom<>::scratch_bytes, stack_scratch_bytes() -- and
// are multiplied by the grids below.)
#pragma once

#include <algorithm>
#include <cstdint>

namespace pf_call {

// first-pass pool sizes per bubble of a range: bytes of aligned rows, sites, group bytes, indel lengths, bytes of path text
// (learnt afterwards; a pool that turns out too small costs a repeated attempt -- at configs[4]'s parameters, k = 31 and insertions
// to 50 bp, a whole K-BUBBLE run thrown away: 334 B of rows, 2.4 sites, 8 group bytes, 1.1 indel lengths and 55 B of path text per
// bubble there; 216 B / 1.2 / 2.7 / 0.03 / 17 B at configs[2]'s)
constexpr uint32_t FIRST_ROW_TEXT = 384, FIRST_SITES = 4, FIRST_GROUPS = 12, FIRST_ILEN = 2, FIRST_PATH_TEXT = 64;

// wavefronts per CU of the kernels whose grids loop over a list.  K-PAIR is register-bound (the score row of the fill is 65 / 129
// registers): 3 / 2 wavefronts per SIMD
constexpr int paths_per_cu = 16, sites_per_cu = 16, pair_per_cu = 12, pair2_per_cu = 4, stack_per_cu = 8;

struct CallGrids {
    int paths, sites, pair, pair2, stack;   // sites, pair2: the most (call_sites_grid, call_pair2_grid)
};
inline CallGrids call_grids(int n_cu) { return {n_cu * paths_per_cu, n_cu * sites_per_cu, n_cu * pair_per_cu, n_cu * pair2_per_cu, n_cu * stack_per_cu}; }

inline uint64_t round_up(uint64_t x, uint64_t to) { return (x + to - 1) & ~(to - 1); }   // (to: a power of two)
inline uint64_t grown(uint64_t need, uint64_t slack) { return need + need / 8 + slack; }  // a pool that overflowed: what it asked for and an eighth

// ---- K-PATHS ----
// stacks sized by the complex size (a non-complex bubble has at most that many vertices)
inline uint32_t depth_cap(uint32_t complex_size) { return std::max<uint32_t>(complex_size + 4, 16); }
// per wavefront: major[depth], minor[4 depth], seg_start[depth + 1], seen[4 depth] (colored), as k_call_paths carves them; the first
// launch asks for an offset (8) and a length (4) of 256 walks on top
inline uint64_t paths_stack_bytes(uint32_t depth) { return (10ull * depth + 4) * 4; }
inline uint64_t paths_per_wave(uint32_t depth) { return round_up(256 * 8 + 256 * 4 + paths_stack_bytes(depth), 256); }
// the launch for bubbles of more than 255 walks: the stacks, then tables of max_paths walks (offset 8, length 4)
inline uint64_t paths_big_per_wave(uint32_t depth, uint32_t max_paths) { return round_up(round_up(paths_stack_bytes(depth), 8) + ((uint64_t)max_paths + 1) * 12, 256); }
inline int paths_big_grid(uint32_t n_many) { return (int)std::min<uint32_t>(n_many, 32); }
constexpr uint32_t MANY_LIST_MIN = 4096;   // entries of the list of such bubbles
inline uint32_t grown_many(uint32_t n_many) { return n_many + n_many / 8 + 64; }

// ---- K-PAIR, second tier: a wavefront per 64 bubbles of its list; fewer than this many bubbles are not worth a launch ----
inline int call_pair2_grid(uint32_t n_pair2, const CallGrids &g) { return (int)std::min<uint32_t>((n_pair2 + 63) / 64, (uint32_t)g.pair2); }
inline uint32_t pair2_min(int n_cu) { return (uint32_t)n_cu * 32u; }

// ---- K-SITES ----
inline uint32_t first_site_string(int k) { return (uint32_t)(2 * k + 64); }   // room for one site string
inline uint32_t grown_site_string(uint32_t ks_need) { return (ks_need + 63u) & ~63u; }
inline uint64_t sites_rows_cap(uint32_t max_rows) { return std::max<uint64_t>(256, round_up(max_rows, 64)); }
// per wavefront: two string tables of rows_cap x ks, per row 4 + 4 + 4 + 1 + 1 + 8 bytes; colored: two colour sets, a value per colour
// and a flag per row
inline uint64_t sites_per_wave(uint64_t rows_cap, uint64_t ks, uint32_t n_colors, uint32_t col_words) {
    return round_up(2 * rows_cap * ks + rows_cap * (4 + 4 + 4 + 1 + 1 + 8) + (n_colors ? rows_cap * (16ull * col_words + 8ull * n_colors + 1) : 0), 256);
}
// (tables for thousands of rows: fewer wavefronts, at most 2 GB of them)
inline int call_sites_grid(uint32_t n_branching, const CallGrids &g, uint64_t per_wave) {
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(n_branching, (uint32_t)g.sites), (2ull << 30) / per_wave));
}
// site values (doubles): eight per colour and branching bubble, a started chunk per wavefront
inline uint64_t site_values_cap(uint32_t n_colors, uint32_t n_branching, int sites_grid, uint64_t learnt) {
    return std::max<uint64_t>(learnt, 8ull * std::max<uint32_t>(n_colors, 1) * n_branching + 1024ull * sites_grid + 1024);
}

// ---- the pools of a range of nb bubbles ----
// capacities learnt from earlier batches (0: none yet)
struct LearntPools {
    uint64_t path_pool = 0, path_text = 0, row_text = 0, sites = 0, groups = 0, ilen = 0, walk = 0;
};
struct BatchPools {
    uint64_t path_pool;   // entries of K-PATHS' pool behind the strict region of four per bubble (a started piece per wavefront)
    uint64_t path_text;   // bytes
    uint64_t row_text, sites, groups, ilen;   // what the aligning kernels publish: bytes, entries, bytes, entries
    uint64_t walk;        // colored: entries of the walks' vertex lists, or 0
    uint64_t path_entries(uint32_t nb) const { return 4ull * nb + path_pool; }
};
inline BatchPools batch_pools(uint32_t nb, const CallGrids &g, const LearntPools &l, bool colored) {
    BatchPools p;
    p.path_pool = std::max<uint64_t>(l.path_pool, (uint64_t)nb / 2 + 128ull * g.paths + 1024);
    p.path_text = std::max<uint64_t>(l.path_text, (uint64_t)nb * FIRST_PATH_TEXT + (1u << 16));
    p.row_text = std::max<uint64_t>(l.row_text, (uint64_t)FIRST_ROW_TEXT * nb + (1u << 16));
    p.sites = std::max<uint64_t>(l.sites, (uint64_t)FIRST_SITES * nb + 64);
    p.groups = std::max<uint64_t>(l.groups, (uint64_t)FIRST_GROUPS * nb + 64);
    p.ilen = std::max<uint64_t>(l.ilen, (uint64_t)FIRST_ILEN * nb + 64);
    p.walk = colored ? std::max<uint64_t>(l.walk, (uint64_t)nb * 2 + 256ull * g.paths + 1024) : 0;
    return p;
}
// the aligned rows of the branching bubbles come on top of what K-SNP took: the room K-BUBBLE wants before it runs
inline uint64_t row_text_need(uint64_t path_text_used, uint32_t n_branching, uint32_t nb) { return 3 * path_text_used + 128ull * n_branching + 160ull * nb; }

// ---- what a reservation guesses where a first call sizes by counts it has not got yet ----
// K-BUBBLE's job index: a quarter of the bubbles go there
inline uint64_t reserve_job_index_bytes(uint32_t nb) { return (uint64_t)nb / 4 * 4 + 4096; }
// site values: a branching bubble in 32, single-sample, the whole K-SITES grid
inline uint64_t reserve_site_values(uint32_t nb, const CallGrids &g) { return (uint64_t)nb / 4 + 1024ull * g.sites + 1024; }

}  // namespace pf_call
