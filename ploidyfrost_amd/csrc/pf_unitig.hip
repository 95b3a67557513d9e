// K-UNITIG: `Bifrost build [-i] [-d] -k <k> -r reads.fq -o sample` (step `4.bifrost` of the reference's workflow) on the device -- the
// compacted de Bruijn graph of the sorted distinct canonical k-mers that pf_count_finish leaves in HBM, written as the text of
// <sample>.gfa.  The rule is pf_unitig_rule.hpp; this file is its device form.  n k-mers, oriented k-mer ("node") v = 2 i + o: k-mer i
// read as stored (o = 0) or as its reverse complement (o = 1); v ^ 1 is the same k-mer read the other way, and every chain of links
// has a mirror chain of the nodes v ^ 1 in reverse order.
//
//   stage      bytes held per k-mer                           probes / dependent gathers per k-mer
//   index      32  table {u64 key, u32 index, u32 pad}, a power of two of at least 2 n slots, key slot from mix64, linear probing;
//                  one CAS per key (keys are distinct), as k_count_rehash                      1 probe
//   adjacency  1   presence bits (4 successors, 4 predecessors of the stored reading) and
//              8   next[2i + o]: the only successor of node 2i + o as a node, else NONE        8 probes, their first loads issued together
//   link       -   next[] in place: kept when the successor has one predecessor, is another k-mer, and the node is not the stored
//                  reading of a self-complementary k-mer (rule header)                         2 gathers of a neighbour's byte
//   simplify   1   dead[]: one thread per chain start walks at most k - 1 links; at the other end removed() decides, the walk is
//                  repeated to mark.  Both ends mark (idempotent), the end with the smaller node counts.  Then adjacency and link
//                  again over live k-mers (a second presence byte: the first tells old closed cycles from new ones)   <= 2 (k - 1) gathers per short chain
//   rank       32  {pointer, distance} per node towards the chain start, two buffers, never jumped in place; one `changed` word a
//                  round read by the host, at most ceil(log2(2 n)) + 1 rounds (the table is freed first)          2 gathers a round and node
//   cycles     16  only when some node reached no chain start: those lie on closed cycles.  The smallest node of each by the same
//                  jumping with a running minimum (a third buffer), then one thread per cycle walks it once to write distances.
//                  Acceptable because closed cycles are whole plasmids or organelles, a handful per graph; chains are never walked.
//                  A node of a closed cycle never reaches a start, so it counts as moved in every round of the rank stage (unless the
//                  cycle's length is a power of two): a graph that holds one closed cycle runs all ceil(log2(2 n)) + 1 rounds there,
//                  each with its read of the `changed` word, where a graph of chains alone stops after about log2 of its longest
//                  unitig.  The distances of cycle nodes wrap 32 bits on the way; the walk writes them anew.  The rounds DESIGN.md
//                  reports are of inputs without closed cycles; the cost of the full count of rounds has not been measured.
//   emit       2+4 start flags, the line of every start; starts of the chosen readings selected (pf_scan.hpp), sorted by their first
//                  k-mer with rocprim::radix_sort_pairs over bits [0, 2k), line lengths scanned exclusively; every live node of a
//                  chosen reading writes its last base at line + prefix + k - 1 + distance, the start the prefix, its first k - 1
//                  bases and the '\n'                                                           3 gathers per node (root, line, offset)
//   placement  pf_unitig_build_colored only (pf_color_rule.hpp; `build-multi`): between the sort and the sizing of the text, n_seeds
//                  rounds of an ask kernel (atomicMin of the line into the claim of a free slot) and a grant kernel (the claim's line
//                  takes the slot; DA = the round), the lines left over numbered behind the slots by a scan, the tag's bytes added to
//                  the line lengths; emit writes the tag, and the flat position km_off[line] + distance of every live k-mer, which
//                  K-COLOR (pf_color.hip) reads with the lines' heads, k-mer counts and slots (pf_unitig_state.hpp)   1 hash a round and line
// Every loop is bounded (by k, the slot count or 2 n) and sets an error flag at its bound; nothing spins.  The kernels are gathers
// bound by latency: 256 threads a block, no LDS, no scratch, and no second argument of __launch_bounds__ that would make the compiler
// trade registers for it -- all of them compile to 24 VGPRs or fewer (eight wavefronts a SIMD) but k_uni_adj, which keeps its eight
// first slots in registers (104 VGPRs, four wavefronts a SIMD, eight misses in flight each); counters are summed per wavefront
// before one atomic.  The result depends on the set of
// k-mers only: the same bytes on every run.  Everything one pf_unitig_build launches is timed as one launch of PF_K_UNITIG; unit:
// k-mers.  The stage times of pf_unitig_stats come from events of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_color_rule.hpp"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"
#include "pf_unitig_rule.hpp"
#include "pf_unitig_state.hpp"

namespace pf {

struct UniSlot {
    unsigned long long key;
    uint32_t index, pad;
};
static_assert(sizeof(UniSlot) == 16, "one slot, one 16-byte vector access");
constexpr uint32_t UNI_NONE = 0xFFFFFFFFu;
constexpr int UNI_MAX_ROUNDS = 40;

struct UniDev {   // device counters of one build
    unsigned long long starts, removed, cycle_nodes, cycles, old_cycles, longest;
    uint32_t stuck, bad_input;
    uint32_t changed[2 * UNI_MAX_ROUNDS];   // one word a round: rank, then cycles
};

__device__ inline uint64_t node_read(const uint64_t *__restrict__ kmers, uint32_t v, int k) {
    const uint64_t x = kmers[v >> 1];
    return (v & 1u) ? pf_count::rev_comp(x, k) : x;
}
__device__ inline uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)v, o, WAVE);
        const uint32_t hi = __shfl_down((uint32_t)(v >> 32), o, WAVE);
        const uint64_t x = ((uint64_t)hi << 32) | lo;
        v = x > v ? x : v;
    }
    return v;
}
__device__ inline void add_per_wave(unsigned long long *to, uint64_t mine) {
    mine = wave_sum_u64(mine);
    if (lane_id() == 0 && mine) atomicAdd(to, (unsigned long long)mine);
}

// ---- input, index ----
__global__ __launch_bounds__(256) void k_uni_check(const uint64_t *__restrict__ kmers, uint64_t n, int k, UniDev *d) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t x = kmers[i];
        if (x > pf_unitig::kmer_mask(k) || pf_unitig::canon(x, k) != x || (i && kmers[i - 1] >= x)) bad = true;
    }
    if (bad) d->bad_input = 1u;
}

__global__ __launch_bounds__(256) void k_uni_clear(UniSlot *tab, uint64_t slots) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256)
        *reinterpret_cast<uint4 *>(tab + s) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, UNI_NONE, 0u);
}

__global__ __launch_bounds__(256) void k_uni_index(const uint64_t *__restrict__ kmers, uint64_t n, UniSlot *tab, uint64_t mask, UniDev *d) {
    bool stuck = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const unsigned long long key = kmers[i];
        uint64_t s = mix64(key) & mask;
        bool put = false;
        for (uint64_t step = 0; step <= mask && !put; ++step) {
            if (atomicCAS(&tab[s].key, (unsigned long long)pf_count::EMPTY_KEY, key) == pf_count::EMPTY_KEY) {
                tab[s].index = (uint32_t)i;   // a fresh slot of a distinct key: nobody else writes it, nobody reads it before the kernel ends
                put = true;
            }
            s = (s + 1) & mask;
        }
        if (!put) stuck = true;
    }
    if (stuck) d->stuck = 1u;
}

// ---- adjacency ----
// the rest of a probe whose first slot held another key; NONE: absent (or the probe went round the table: stuck)
__device__ inline uint32_t uni_find_from(const UniSlot *__restrict__ tab, uint64_t mask, uint64_t key, uint64_t s, bool &stuck) {
    for (uint64_t step = 0; step < mask; ++step) {
        s = (s + 1) & mask;
        const uint4 v = *reinterpret_cast<const uint4 *>(tab + s);
        const uint64_t cur = ((uint64_t)v.y << 32) | v.x;
        if (cur == key) return v.z;
        if (cur == pf_count::EMPTY_KEY) return UNI_NONE;
    }
    stuck = true;
    return UNI_NONE;
}

__global__ __launch_bounds__(256) void k_uni_adj(const uint64_t *__restrict__ kmers, uint64_t n, int k, const UniSlot *__restrict__ tab, uint64_t mask,
                                                 const uint8_t *__restrict__ dead, uint8_t *__restrict__ adj, uint32_t *__restrict__ next, UniDev *d) {
    bool stuck = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (dead && dead[i]) {
            adj[i] = 0;
            *reinterpret_cast<uint2 *>(next + 2 * i) = make_uint2(UNI_NONE, UNI_NONE);
            continue;
        }
        const uint64_t x = kmers[i], rc = pf_count::rev_comp(x, k);
        uint64_t key[8], slot[8];
        uint4 first[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {   // bit j: successor j & 3 of the stored reading (j < 4) or of its reverse complement
            key[j] = pf_unitig::canon(pf_unitig::succ_of(j < 4 ? x : rc, j & 3, k), k);
            slot[j] = mix64(key[j]) & mask;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) first[j] = *reinterpret_cast<const uint4 *>(tab + slot[j]);   // eight independent loads in flight
        uint32_t bits = 0, only[2] = {UNI_NONE, UNI_NONE};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t cur = ((uint64_t)first[j].y << 32) | first[j].x;
            uint32_t at = cur == key[j] ? first[j].z : cur == pf_count::EMPTY_KEY ? UNI_NONE : uni_find_from(tab, mask, key[j], slot[j], stuck);
            if (at != UNI_NONE && dead && dead[at]) at = UNI_NONE;
            if (at == UNI_NONE) continue;
            bits |= 1u << j;
            only[j >> 2] = 2 * at + (pf_unitig::succ_of(j < 4 ? x : rc, j & 3, k) != key[j] ? 1u : 0u);   // the node that reads as the successor
        }
        adj[i] = (uint8_t)bits;
        *reinterpret_cast<uint2 *>(next + 2 * i) =
            make_uint2(__popc(bits & 0xFu) == 1 ? only[0] : UNI_NONE, __popc(bits >> 4) == 1 ? only[1] : UNI_NONE);
    }
    if (stuck) d->stuck = 1u;
}

// successors of node v / predecessors of node v from its k-mer's byte
__device__ inline int node_succs(uint8_t a, uint32_t v) { return __popc((v & 1u) ? (uint32_t)a >> 4 : (uint32_t)a & 0xFu); }
__device__ inline int node_preds(uint8_t a, uint32_t v) { return node_succs(a, v ^ 1u); }

// ---- link ----
__global__ __launch_bounds__(256) void k_uni_link(const uint64_t *__restrict__ kmers, uint64_t n, int k, const uint8_t *__restrict__ adj, uint32_t *next) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint2 w = *reinterpret_cast<const uint2 *>(next + 2 * i);   // this thread's two entries: nobody else reads or writes them here
        const uint8_t a0 = w.x != UNI_NONE ? adj[w.x >> 1] : 0, a1 = w.y != UNI_NONE ? adj[w.y >> 1] : 0;
        if (w.x != UNI_NONE && ((w.x >> 1) == i || node_preds(a0, w.x) != 1 || pf_unitig::self_complementary(kmers[i], k))) w.x = UNI_NONE;
        if (w.y != UNI_NONE && ((w.y >> 1) == i || node_preds(a1, w.y) != 1)) w.y = UNI_NONE;
        *reinterpret_cast<uint2 *>(next + 2 * i) = w;
    }
}

// ---- simplify ----
__global__ __launch_bounds__(256) void k_uni_simplify(uint64_t n_nodes, int k, const uint8_t *__restrict__ adj, const uint32_t *__restrict__ link,
                                                      int clip, int del, uint8_t *dead, UniDev *d) {
    uint64_t starts = 0, removed = 0;
    for (uint64_t v64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; v64 < n_nodes; v64 += (uint64_t)gridDim.x * 256) {
        const uint32_t v = (uint32_t)v64;
        if (link[v ^ 1u] != UNI_NONE) continue;   // it has a predecessor in its chain
        starts += 1;
        if (!clip && !del) continue;
        uint32_t u = v, m = 1;
        for (int step = 0; step < k - 1 && link[u] != UNI_NONE; ++step) { u = link[u]; ++m; }
        if (link[u] != UNI_NONE) continue;   // k k-mers or more
        if (!pf_unitig::removed(m, node_preds(adj[v >> 1], v), node_succs(adj[u >> 1], u), k, clip != 0, del != 0)) continue;
        if (v < (u ^ 1u)) removed += 1;      // the mirror chain starts at u ^ 1 and decides the same
        u = v;
        dead[u >> 1] = 1;
        for (uint32_t step = 1; step < m; ++step) { u = link[u]; dead[u >> 1] = 1; }
    }
    add_per_wave(&d->starts, starts);
    add_per_wave(&d->removed, removed);
}

// ---- rank ----
__global__ __launch_bounds__(256) void k_uni_rank_init(uint64_t n_nodes, const uint32_t *__restrict__ link, uint2 *__restrict__ a) {
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (uint64_t)gridDim.x * 256) {
        const uint32_t back = link[v ^ 1ull];   // the mirror's successor is this node's predecessor, mirrored
        a[v] = back == UNI_NONE ? make_uint2((uint32_t)v, 0u) : make_uint2(back ^ 1u, 1u);
    }
}
__global__ __launch_bounds__(256) void k_uni_jump(uint64_t n_nodes, const uint2 *__restrict__ a, uint2 *__restrict__ b, uint32_t *changed) {
    bool moved = false;
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (uint64_t)gridDim.x * 256) {
        const uint2 p = a[v];
        uint2 out = p;
        if (p.x != (uint32_t)v) {
            const uint2 q = a[p.x];
            out = make_uint2(q.x, p.y + q.y);
            moved = moved || q.x != p.x;
        }
        b[v] = out;
    }
    if (moved) *changed = 1u;
}

// ---- cycles ----
__device__ inline bool on_cycle(const uint2 *a, const uint32_t *__restrict__ link, uint64_t v) { return link[a[v].x ^ 1u] != UNI_NONE; }   // what it reached has a predecessor

__global__ __launch_bounds__(256) void k_uni_cycle_count(uint64_t n_nodes, const uint2 *__restrict__ a, const uint32_t *__restrict__ link, UniDev *d) {
    uint64_t mine = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (uint64_t)gridDim.x * 256) mine += on_cycle(a, link, v) ? 1 : 0;
    add_per_wave(&d->cycle_nodes, mine);
}
__global__ __launch_bounds__(256) void k_uni_cmin_init(uint64_t n_nodes, const uint2 *__restrict__ a, const uint32_t *__restrict__ link, uint2 *__restrict__ b) {
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (uint64_t)gridDim.x * 256)
        b[v] = make_uint2(on_cycle(a, link, v) ? link[v ^ 1ull] ^ 1u : (uint32_t)v, (uint32_t)v);
}
__global__ __launch_bounds__(256) void k_uni_jump_min(uint64_t n_nodes, const uint2 *__restrict__ a, uint2 *__restrict__ b, uint32_t *changed) {
    bool moved = false;
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (uint64_t)gridDim.x * 256) {
        const uint2 p = a[v];
        uint2 out = p;
        if (p.x != (uint32_t)v) {
            const uint2 q = a[p.x];
            out = make_uint2(q.x, q.y < p.y ? q.y : p.y);
            moved = moved || out.y != p.y;
        }
        b[v] = out;
    }
    if (moved) *changed = 1u;
}
// one thread per closed cycle (the smallest node of it): root and distance of every node of the cycle that holds its smallest k-mer as
// stored (an even smallest node); the mirror cycle gets its root only, and is never written.  rank[v ^ 1].y = k-mers - 1, where a
// chain's mirror end keeps it.
__global__ __launch_bounds__(256) void k_uni_cycle_walk(uint64_t n_nodes, const uint2 *__restrict__ cmin, const uint32_t *__restrict__ link,
                                                        const uint8_t *__restrict__ adj_first, uint2 *rank, UniDev *d) {
    for (uint64_t v64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; v64 < n_nodes; v64 += (uint64_t)gridDim.x * 256) {
        const uint32_t v = (uint32_t)v64;
        // on_cycle reads rank[v].x while other walkers store rank[u].x.  Keep this order: cmin[v].y != v is false only for the one node
        // of a cycle that walks it, and no other walker writes a node of this cycle, so rank[v] is read before anyone stores it; and a
        // store only replaces one node that has a predecessor by another, which on_cycle cannot tell apart.
        if (cmin[v].y != v || link[v ^ 1u] == UNI_NONE || !on_cycle(rank, link, v)) continue;
        const bool chosen = (v & 1u) == 0;
        bool old = true;
        uint32_t u = v;
        uint64_t steps = 0;
        do {
            rank[u].x = v;
            if (chosen) {
                rank[u].y = (uint32_t)steps;
                const uint8_t a = adj_first[u >> 1];
                old = old && __popc((uint32_t)a & 0xFu) == 1 && __popc((uint32_t)a >> 4) == 1;
            }
            u = link[u];
            ++steps;
        } while (u != v && u != UNI_NONE && steps < n_nodes);
        if (u != v) { d->stuck = 1u; continue; }
        if (chosen) {
            rank[v ^ 1u].y = (uint32_t)(steps - 1);
            atomicAdd(&d->cycles, 1ull);
            if (old) atomicAdd(&d->old_cycles, 1ull);
        }
    }
}

// ---- emit ----
// flag[v] = 1: v starts a reading that is written -- of a chain and its mirror the one whose first k-mer as read is smaller (a single
// self-complementary k-mer: the stored reading), of a closed cycle and its mirror the one that starts at an even node
__global__ __launch_bounds__(256) void k_uni_starts(uint64_t n_nodes, const uint64_t *__restrict__ kmers, int k, const uint2 *__restrict__ rank,
                                                    const uint32_t *__restrict__ link, const uint8_t *__restrict__ dead, uint8_t *__restrict__ flag) {
    for (uint64_t v64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; v64 < n_nodes; v64 += (uint64_t)gridDim.x * 256) {
        const uint32_t v = (uint32_t)v64;
        bool start = false;
        if (rank[v].x == v && !(dead && dead[v >> 1])) {
            if (link[v ^ 1u] != UNI_NONE) start = (v & 1u) == 0;   // the smallest node of a closed cycle
            else {
                const uint32_t other = rank[v ^ 1u].x;             // where the mirror chain starts
                const uint64_t mine = node_read(kmers, v, k), theirs = node_read(kmers, other, k);
                start = mine < theirs || (mine == theirs && v <= other);
            }
        }
        flag[v] = start ? 1 : 0;
    }
}
__global__ __launch_bounds__(256) void k_uni_keys(const uint32_t *__restrict__ ids, uint64_t n_lines, const uint64_t *__restrict__ kmers, int k, uint64_t *__restrict__ keys) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) keys[j] = node_read(kmers, ids[j], k);
}
__global__ __launch_bounds__(256) void k_uni_lines(const uint32_t *__restrict__ sorted, uint64_t n_lines, int k, const uint2 *__restrict__ rank,
                                                   uint32_t *__restrict__ line_of, uint32_t *__restrict__ len, uint32_t *__restrict__ m_of, UniDev *d) {
    uint64_t longest = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) {
        const uint32_t r = sorted[j];
        const uint64_t m = (uint64_t)rank[r ^ 1u].y + 1;   // the mirror of the start is the mirror chain's last node
        line_of[r] = (uint32_t)j;
        len[j] = (uint32_t)pf_unitig::line_bytes(j + 1, m, k);
        if (m_of) m_of[j] = (uint32_t)m;   // (a coloured build: the lines' k-mer counts are scanned into graph order)
        longest = m + (uint64_t)k - 1 > longest ? m + (uint64_t)k - 1 : longest;
    }
    longest = wave_max_u64(longest);
    if (lane_id() == 0 && longest) atomicMax(&d->longest, (unsigned long long)longest);
}
__global__ __launch_bounds__(256) void k_uni_emit(uint64_t n_nodes, const uint64_t *__restrict__ kmers, int k, const uint2 *__restrict__ rank,
                                                  const uint8_t *__restrict__ dead, const uint32_t *__restrict__ line_of, const uint64_t *__restrict__ off,
                                                  const uint32_t *__restrict__ len, uint64_t header_bytes, char *__restrict__ text,
                                                  const uint8_t *__restrict__ da, const uint64_t *__restrict__ km_off, uint32_t *__restrict__ flat_of) {
    for (uint64_t v64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; v64 < n_nodes; v64 += (uint64_t)gridDim.x * 256) {
        const uint32_t v = (uint32_t)v64;
        if (dead && dead[v >> 1]) continue;
        const uint2 p = rank[v];
        const uint32_t j = line_of[p.x];
        if (j == UNI_NONE) continue;   // the reading that is not written
        const uint64_t x = node_read(kmers, v, k);
        char *line = text + header_bytes + off[j];
        const uint32_t digits = pf_unitig::id_digits((uint64_t)j + 1);
        char *seq = line + 2 + digits + 1;
        seq[(uint64_t)(k - 1) + p.y] = pf_unitig::base_char(x);
        if (flat_of) flat_of[v >> 1] = (uint32_t)(km_off[j] + p.y);   // a coloured build: the k-mer's place in graph order
        if (p.x != v) continue;
        line[0] = 'S';
        line[1] = '\t';
        uint64_t id = (uint64_t)j + 1;
        for (uint32_t c = digits; c-- > 0; id /= 10) line[2 + c] = (char)('0' + id % 10);
        line[2 + digits] = '\t';
        for (int b = 0; b < k - 1; ++b) seq[b] = pf_unitig::base_char(x >> (2 * (k - 1 - b)));
        line[len[j] - 1] = '\n';
        if (da) {   // a coloured build: "\tDA:Z:<round>" before the end of the line
            uint32_t tag = da[j];
            char *end = line + len[j] - 1;
            for (uint32_t c = pf_unitig::id_digits(tag); c-- > 0; tag /= 10) *--end = (char)('0' + tag % 10);
            end -= pf_color::DA_PREFIX_BYTES;
            for (uint32_t c = 0; c < pf_color::DA_PREFIX_BYTES; ++c) end[c] = pf_color::DA_PREFIX[c];
        }
    }
}

// ---- placement of the lines' colour sets (pf_color_rule.hpp): one ask and one grant kernel a round ----
// owner[s] = the line that holds slot s, written by grants only; claim[s] = the smallest line that asked for the free slot s this
// round.  A claimed slot is granted in the same round, so a free slot's claim is NONE when a round begins.
__global__ __launch_bounds__(256) void k_uni_place_ask(const uint64_t *__restrict__ heads, uint64_t n_lines, int k, uint32_t round,
                                                       const uint32_t *__restrict__ slot, const uint32_t *__restrict__ owner, uint32_t *claim) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) {
        if (slot[j] != UNI_NONE) continue;
        const uint32_t at = pf_color::asked_slot(heads[j], k, round, n_lines);
        if (owner[at] == UNI_NONE) atomicMin(&claim[at], (uint32_t)j);
    }
}
__global__ __launch_bounds__(256) void k_uni_place_grant(const uint64_t *__restrict__ heads, uint64_t n_lines, int k, uint32_t round, uint32_t *slot,
                                                         uint32_t *owner, const uint32_t *__restrict__ claim, uint8_t *__restrict__ da) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) {
        if (slot[j] != UNI_NONE) continue;
        const uint32_t at = pf_color::asked_slot(heads[j], k, round, n_lines);
        if (claim[at] != (uint32_t)j) continue;   // (a slot taken in an earlier round keeps the claim of its placed line)
        owner[at] = (uint32_t)j;
        slot[j] = at;
        da[j] = (uint8_t)round;
    }
}
__global__ __launch_bounds__(256) void k_uni_place_left(const uint32_t *__restrict__ slot, uint64_t n_lines, uint32_t *__restrict__ left) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) left[j] = slot[j] == UNI_NONE ? 1u : 0u;
}
// the lines left over take the overflow slots in their order; every line's length grows by its tag
__global__ __launch_bounds__(256) void k_uni_place_end(uint64_t n_lines, const uint32_t *__restrict__ left, const uint32_t *__restrict__ rank, uint32_t *slot,
                                                       const uint8_t *__restrict__ da, uint32_t *len) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_lines; j += (uint64_t)gridDim.x * 256) {
        if (left[j]) slot[j] = (uint32_t)(n_lines + rank[j]);
        len[j] += pf_color::da_bytes(da[j]);
    }
}

// ---- host side ----
static UnitigState *unitig_state(pf_ctx *ctx) { return static_cast<UnitigState *>(ctx->unitig); }

void unitig_destroy(pf_ctx *ctx) {
    UnitigState *S = unitig_state(ctx);
    if (!S) return;
    color_destroy(S);
    (void)hipFree(S->text);
    (void)hipFree(S->kmers_own);
    (void)hipFree(S->flat_of);
    (void)hipFree(S->heads);
    (void)hipFree(S->m_of);
    (void)hipFree(S->km_off);
    (void)hipFree(S->slot);
    delete S;
    ctx->unitig = nullptr;
}

struct UniEvents {   // the stage times of pf_unitig_stats
    hipEvent_t e[PF_UNITIG_STAGES + 1] = {};
    ~UniEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t make() { for (hipEvent_t &x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; } return hipSuccess; }
};

// every buffer of a build is taken through here: one that does not fit is the refusal by name with the k-mer count reached
template <class T>
static int uni_alloc(pf_ctx *ctx, DevTmp<T> &buf, uint64_t bytes, uint64_t n) {
    const hipError_t e = buf.alloc((size_t)bytes);
    if (e == hipSuccess) return PF_OK;
    (void)hipGetLastError();
    buf.p = nullptr;
    if (e != hipErrorOutOfMemory) {
        pf::CtxErr{ctx} = std::string("pf_unitig_build: hipMalloc: ") + hipGetErrorString(e);
        return PF_ERR_HIP;
    }
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    pf::CtxErr{ctx} = "pf_unitig_build: " + pf_unitig::no_room_text(bytes, free_b, n);
    return PF_ERR_OVERFLOW;
}
#define UNI_ALLOC(buf, bytes)                                       \
    do {                                                            \
        const int rc_ = uni_alloc(ctx, buf, (uint64_t)(bytes), n);  \
        if (rc_ != PF_OK) return rc_;                               \
    } while (0)

static int uni_fits(pf_ctx *ctx, uint64_t need, uint64_t n) {
    size_t free_b = 0, total_b = 0;
    PF_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need <= free_b) return PF_OK;
    pf::CtxErr{ctx} = "pf_unitig_build: " + pf_unitig::no_room_text(need, free_b, n);
    return PF_ERR_OVERFLOW;
}

}  // namespace pf

using namespace pf;

// n_seeds = 0: the plain build.  Otherwise the coloured one: the lines' colour sets are placed before the text is sized, every S line
// ends in its DA tag, and what K-COLOR needs stays in the context beside the text.
static int unitig_build_impl(pf_ctx *ctx, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated, uint32_t n_seeds,
                             pf_unitig_stats *stats, uint64_t *overflow_out) {
    if (!ctx) return PF_ERR_ARG;
    const bool colored = n_seeds != 0;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (ctx->unitig) return refuse("pf_unitig_build: a built graph is held already (pf_unitig_release comes first)");
    if (!pf_count::k_ok(k)) return refuse("pf_unitig_build: k = " + std::to_string(k) + ": " + pf_count::cut_text(pf_count::CUT_K));
    if (g == PF_UNITIG_G_DEFAULT) g = (uint32_t)pf_unitig::default_g((int)k);
    if (!pf_unitig::g_ok(g, (int)k)) return refuse("pf_unitig_build: g = " + std::to_string(g) + ": " + pf_unitig::g_text((int)k));
    if (n >= pf_unitig::MAX_KMERS) return refuse(std::string("pf_unitig_build: ") + pf_unitig::TOO_MANY_TEXT);
    if (n && !kmers) return refuse("pf_unitig_build: kmers is needed");
    if ((uintptr_t)kmers & 7) return refuse("pf_unitig_build: kmers is not aligned");
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_UNITIG);
    UniEvents ev;
    PF_HIP(ev.make());
    int stage = 0;
    auto mark = [&]() { return hipEventRecord(ev.e[stage++], ctx->stream); };
    const int K = (int)k;
    const std::string header = pf_unitig::header_line(K, (int)g);
    const uint64_t n_nodes = 2 * n;
    pf_unitig_stats st = {};
    st.distinct = n;
    UniDev h = {};
    DevTmp<uint64_t> staged, keys0, keys1, off, km_off;
    DevTmp<UniSlot> tab;
    DevTmp<uint8_t> adj0, adj1, dead, flag, scratch, sort_tmp, da;
    DevTmp<uint32_t> link, line_of, ids, sorted, len, m_of, slot, owner, claim, left, left_rank, flat_of;
    uint64_t overflow = 0, n_live = 0;
    DevTmp<uint2> ra, rb, rc;
    DevTmp<UniDev> dev;
    UNI_ALLOC(dev, sizeof(UniDev));
    PF_HIP(hipMemsetAsync(dev.p, 0, sizeof(UniDev), ctx->stream));
    auto counters = [&]() {
        hipError_t e = hipMemcpyAsync(&h, dev.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
        return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
    };
    PF_HIP(mark());
    uint64_t n_lines = 0;
    const uint8_t *d_dead = nullptr;
    uint2 *rank = nullptr;
    if (n) {
        uint64_t slots = 64;
        while (slots < 2 * n) slots <<= 1;
        // held throughout: two presence bytes, dead, link (and the k-mers, when they came from the host).  Beside them the larger of
        // the table, and the two rank buffers with the start flags, the selected starts and the scan's scratch of emit.  The third
        // buffer of cycles, the buffers per line (once the lines are counted) and the text are asked for when they are known.
        const uint64_t held = n * (1 + 1 + 1 + 8) + (is_device_ptr(kmers) ? 0 : n * 8);
        const uint64_t emit = n_nodes * 16 + n_nodes * (1 + 4) + scan_scratch_bytes(n_nodes);
        { const int rc_ = uni_fits(ctx, held + std::max<uint64_t>(slots * sizeof(UniSlot), emit), n); if (rc_) return rc_; }
        if (!is_device_ptr(kmers)) {
            UNI_ALLOC(staged, n * 8);
            PF_HIP(hipMemcpyAsync(staged.p, kmers, n * 8, hipMemcpyDefault, ctx->stream));
            kmers = staged.p;
        }
        const int g_k = ctx_grid(ctx, n, 256, 8), g_n = ctx_grid(ctx, n_nodes, 256, 8);
        // ---- index ----
        k_uni_check<<<g_k, 256, 0, ctx->stream>>>(kmers, n, K, dev.p);
        PF_HIP(counters());
        if (h.bad_input) return refuse("pf_unitig_build: kmers are not sorted distinct canonical k-mers of length k (what pf_count_finish gives)");
        UNI_ALLOC(tab, slots * sizeof(UniSlot));
        k_uni_clear<<<ctx_grid(ctx, slots, 256, 8), 256, 0, ctx->stream>>>(tab.p, slots);
        k_uni_index<<<g_k, 256, 0, ctx->stream>>>(kmers, n, tab.p, slots - 1, dev.p);
        PF_HIP(mark());
        // ---- adjacency, link ----
        UNI_ALLOC(adj0, n);
        UNI_ALLOC(link, n_nodes * 4);
        k_uni_adj<<<g_k, 256, 0, ctx->stream>>>(kmers, n, K, tab.p, slots - 1, nullptr, adj0.p, link.p, dev.p);
        k_uni_link<<<g_k, 256, 0, ctx->stream>>>(kmers, n, K, adj0.p, link.p);
        PF_HIP(mark());
        // ---- simplify ----
        UNI_ALLOC(dead, n);
        PF_HIP(hipMemsetAsync(dead.p, 0, n, ctx->stream));
        k_uni_simplify<<<g_n, 256, 0, ctx->stream>>>(n_nodes, K, adj0.p, link.p, clip_tips ? 1 : 0, del_isolated ? 1 : 0, dead.p, dev.p);
        PF_HIP(counters());
        if (h.stuck) { pf::CtxErr{ctx} = "K-UNITIG: a probe went round the whole index table"; return PF_ERR_HIP; }
        const uint64_t chains_first = h.starts / 2;
        st.removed = h.removed;
        if (h.removed) {
            UNI_ALLOC(adj1, n);
            d_dead = dead.p;
            k_uni_adj<<<g_k, 256, 0, ctx->stream>>>(kmers, n, K, tab.p, slots - 1, d_dead, adj1.p, link.p, dev.p);
            k_uni_link<<<g_k, 256, 0, ctx->stream>>>(kmers, n, K, adj1.p, link.p);
        }
        PF_HIP(mark());
        PF_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(tab.p);
        tab.p = nullptr;
        // ---- rank ----
        UNI_ALLOC(ra, n_nodes * 8);
        UNI_ALLOC(rb, n_nodes * 8);
        k_uni_rank_init<<<g_n, 256, 0, ctx->stream>>>(n_nodes, link.p, ra.p);
        int cap = 1;
        while ((1ull << cap) < n_nodes) ++cap;
        cap = std::min(cap + 1, UNI_MAX_ROUNDS);   // ceil(log2(2 n)) + 1
        uint2 *cur = ra.p, *nxt = rb.p;
        for (int round = 0; round < cap; ++round) {
            k_uni_jump<<<g_n, 256, 0, ctx->stream>>>(n_nodes, cur, nxt, dev.p->changed + round);
            std::swap(cur, nxt);
            uint32_t changed = 0;
            PF_HIP(hipMemcpyAsync(&changed, dev.p->changed + round, 4, hipMemcpyDeviceToHost, ctx->stream));
            PF_HIP(hipStreamSynchronize(ctx->stream));
            st.rounds += 1;
            if (!changed) break;
        }
        rank = cur;
        uint2 *spare = nxt;
        PF_HIP(mark());
        // ---- cycles ----
        k_uni_cycle_count<<<g_n, 256, 0, ctx->stream>>>(n_nodes, rank, link.p, dev.p);
        PF_HIP(counters());
        if (h.cycle_nodes) {
            { const int rc_ = uni_fits(ctx, n_nodes * 8, n); if (rc_) return rc_; }
            UNI_ALLOC(rc, n_nodes * 8);
            k_uni_cmin_init<<<g_n, 256, 0, ctx->stream>>>(n_nodes, rank, link.p, spare);
            uint2 *c_cur = spare, *c_nxt = rc.p;
            for (int round = 0; round < cap; ++round) {
                uint32_t *word = dev.p->changed + UNI_MAX_ROUNDS + round;
                k_uni_jump_min<<<g_n, 256, 0, ctx->stream>>>(n_nodes, c_cur, c_nxt, word);
                std::swap(c_cur, c_nxt);
                uint32_t changed = 0;
                PF_HIP(hipMemcpyAsync(&changed, word, 4, hipMemcpyDeviceToHost, ctx->stream));
                PF_HIP(hipStreamSynchronize(ctx->stream));
                st.cycle_rounds += 1;
                if (!changed) break;
            }
            k_uni_cycle_walk<<<g_n, 256, 0, ctx->stream>>>(n_nodes, c_cur, link.p, adj0.p, rank, dev.p);
            PF_HIP(counters());
            if (h.stuck) { pf::CtxErr{ctx} = "K-UNITIG: a closed cycle did not come back to its start"; return PF_ERR_HIP; }
            PF_HIP(hipStreamSynchronize(ctx->stream));
            (void)hipFree(rc.p);
            rc.p = nullptr;
        }
        st.cycles = h.cycles;
        // unitigs before simplifying: every chain has two starts; a closed cycle of the end was there before unless a removal closed it
        st.unitigs = chains_first + (h.removed ? h.old_cycles : h.cycles);
        PF_HIP(mark());
        // ---- emit: the starts that are written, sorted by their first k-mer ----
        UNI_ALLOC(flag, n_nodes);
        UNI_ALLOC(ids, n_nodes * 4);
        UNI_ALLOC(scratch, scan_scratch_bytes(n_nodes));
        k_uni_starts<<<g_n, 256, 0, ctx->stream>>>(n_nodes, kmers, K, rank, link.p, d_dead, flag.p);
        uint64_t *d_count = reinterpret_cast<uint64_t *>(dev.p->changed);   // (the rounds are over: their words are reused, 8-byte aligned)
        static_assert(offsetof(UniDev, changed) % 8 == 0, "the count of lines lies in the changed words");
        PF_HIP(select_flagged_u8(flag.p, ids.p, nullptr, d_count, n_nodes, scratch.p, ctx->stream));
        PF_HIP(hipMemcpyAsync(&n_lines, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        for (int s = 0; s < 5; ++s) PF_HIP(mark());
    }
    st.unitigs_out = n_lines;
    uint64_t body = 0;
    if (n_lines) {
        const int g_l = ctx_grid(ctx, n_lines, 256, 8), g_n = ctx_grid(ctx, n_nodes, 256, 8);
        uint32_t *line_at = reinterpret_cast<uint32_t *>(rank == ra.p ? rb.p : ra.p);   // (the other rank buffer is free: 2 n words of it)
        size_t need = 0;   // (a size query: no buffer is read)
        PF_HIP(rocprim::radix_sort_pairs(nullptr, need, keys0.p, keys1.p, ids.p, sorted.p, (size_t)n_lines, 0, 2 * k, ctx->stream));
        { const int rc_ = uni_fits(ctx, n_lines * (8 + 8 + 4 + 4 + 8) + need, n); if (rc_) return rc_; }
        UNI_ALLOC(keys0, n_lines * 8);
        UNI_ALLOC(keys1, n_lines * 8);
        UNI_ALLOC(sorted, n_lines * 4);
        UNI_ALLOC(len, n_lines * 4);
        UNI_ALLOC(off, n_lines * 8);
        k_uni_keys<<<g_l, 256, 0, ctx->stream>>>(ids.p, n_lines, kmers, K, keys0.p);
        UNI_ALLOC(sort_tmp, need);
        PF_HIP(rocprim::radix_sort_pairs(sort_tmp.p, need, keys0.p, keys1.p, ids.p, sorted.p, (size_t)n_lines, 0, 2 * k, ctx->stream));
        PF_HIP(hipMemsetAsync(line_at, 0xFF, n_nodes * 4, ctx->stream));
        if (colored) {
            { const int rc_ = uni_fits(ctx, n_lines * (4 * 6 + 1 + 8) + n * 4, n); if (rc_) return rc_; }
            UNI_ALLOC(m_of, n_lines * 4);
        }
        k_uni_lines<<<g_l, 256, 0, ctx->stream>>>(sorted.p, n_lines, K, rank, line_at, len.p, m_of.p, dev.p);
        if (colored) {   // the DA digits are part of a line's length: place before the text is sized (keys1: the lines' heads, sorted)
            UNI_ALLOC(slot, n_lines * 4);
            UNI_ALLOC(owner, n_lines * 4);
            UNI_ALLOC(claim, n_lines * 4);
            UNI_ALLOC(left, n_lines * 4);
            UNI_ALLOC(left_rank, n_lines * 4);
            UNI_ALLOC(da, n_lines);
            UNI_ALLOC(km_off, n_lines * 8);
            UNI_ALLOC(flat_of, n * 4);
            PF_HIP(hipMemsetAsync(slot.p, 0xFF, n_lines * 4, ctx->stream));
            PF_HIP(hipMemsetAsync(owner.p, 0xFF, n_lines * 4, ctx->stream));
            PF_HIP(hipMemsetAsync(claim.p, 0xFF, n_lines * 4, ctx->stream));
            PF_HIP(hipMemsetAsync(da.p, 0, n_lines, ctx->stream));
            PF_HIP(hipMemsetAsync(flat_of.p, 0xFF, n * 4, ctx->stream));
            for (uint32_t round = 1; round <= n_seeds; ++round) {
                k_uni_place_ask<<<g_l, 256, 0, ctx->stream>>>(keys1.p, n_lines, K, round, slot.p, owner.p, claim.p);
                k_uni_place_grant<<<g_l, 256, 0, ctx->stream>>>(keys1.p, n_lines, K, round, slot.p, owner.p, claim.p, da.p);
            }
            k_uni_place_left<<<g_l, 256, 0, ctx->stream>>>(slot.p, n_lines, left.p);
            PF_HIP(scan_exclusive_u32(left.p, left_rank.p, n_lines, scratch.p, ctx->stream));
            uint32_t last_left = 0, last_rank = 0;
            PF_HIP(hipMemcpyAsync(&last_left, left.p + (n_lines - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
            PF_HIP(hipMemcpyAsync(&last_rank, left_rank.p + (n_lines - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
            k_uni_place_end<<<g_l, 256, 0, ctx->stream>>>(n_lines, left.p, left_rank.p, slot.p, da.p, len.p);
            PF_HIP(scan_exclusive_u32_u64(m_of.p, km_off.p, n_lines, scratch.p, ctx->stream));
            uint64_t last_km = 0;
            uint32_t last_m = 0;
            PF_HIP(hipMemcpyAsync(&last_km, km_off.p + (n_lines - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
            PF_HIP(hipMemcpyAsync(&last_m, m_of.p + (n_lines - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
            PF_HIP(hipStreamSynchronize(ctx->stream));
            overflow = (uint64_t)last_left + last_rank;
            n_live = last_km + last_m;
        }
        PF_HIP(scan_exclusive_u32_u64(len.p, off.p, n_lines, scratch.p, ctx->stream));
        uint64_t last_off = 0;
        uint32_t last_len = 0;
        PF_HIP(hipMemcpyAsync(&last_off, off.p + (n_lines - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipMemcpyAsync(&last_len, len.p + (n_lines - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(counters());
        body = last_off + last_len;
        st.longest = h.longest;
        { const int rc_ = uni_fits(ctx, header.size() + body, n); if (rc_) return rc_; }
        DevTmp<char> text;
        UNI_ALLOC(text, header.size() + body);
        UnitigState *S = new UnitigState;
        S->text = text.p;
        text.p = nullptr;   // held by the context from here
        S->bytes = header.size() + body;
        ctx->unitig = S;
        k_uni_emit<<<g_n, 256, 0, ctx->stream>>>(n_nodes, kmers, K, rank, d_dead, line_at, off.p, len.p, header.size(), S->text, da.p, km_off.p, flat_of.p);
    } else {
        DevTmp<char> text;
        UNI_ALLOC(text, header.size());
        UnitigState *S = new UnitigState;
        S->text = text.p;
        text.p = nullptr;
        S->bytes = header.size();
        ctx->unitig = S;
    }
    hipError_t e = hipMemcpyAsync(unitig_state(ctx)->text, header.data(), header.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = mark();
    if (e == hipSuccess) e = counters();
    if (e != hipSuccess || h.stuck) {
        unitig_destroy(ctx);
        pf::CtxErr{ctx} = e != hipSuccess ? std::string("pf_unitig_build: ") + hipGetErrorString(e) : std::string("K-UNITIG: a probe went round the whole index table");
        return PF_ERR_HIP;
    }
    st.bytes = header.size() + body;
    for (int s = 0; s < PF_UNITIG_STAGES; ++s) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[s], ev.e[s + 1]) == hipSuccess) st.stage_ms[s] = ms;
    }
    ctx_units(ctx, PF_K_UNITIG, n);
    if (colored) {   // what K-COLOR reads stays with the text
        UnitigState *S = unitig_state(ctx);
        S->colored = true;
        S->k = K;
        S->kmers = kmers;
        S->kmers_own = staged.p;
        S->n = n;
        S->n_live = n_live;
        S->n_lines = n_lines;
        S->longest_m = st.longest ? st.longest - k + 1 : 0;
        S->overflow = overflow;
        S->flat_of = flat_of.p;
        S->heads = keys1.p;
        S->m_of = m_of.p;
        S->km_off = km_off.p;
        S->slot = slot.p;
        staged.p = nullptr;
        flat_of.p = nullptr;
        keys1.p = nullptr;
        m_of.p = nullptr;
        km_off.p = nullptr;
        slot.p = nullptr;
    }
    if (stats) *stats = st;
    if (overflow_out) *overflow_out = overflow;
    return PF_OK;
}

extern "C" int pf_unitig_build(pf_ctx *ctx, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated,
                               pf_unitig_stats *stats) {
    return unitig_build_impl(ctx, kmers, n, k, g, clip_tips, del_isolated, 0, stats, nullptr);
}

extern "C" int pf_unitig_build_colored(pf_ctx *ctx, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated,
                                       uint32_t n_seeds, pf_unitig_stats *stats, uint64_t *overflow) {
    if (!ctx) return PF_ERR_ARG;
    if (!pf_color::seeds_ok(n_seeds)) { pf::CtxErr{ctx} = "pf_unitig_build_colored: n_seeds = " + std::to_string(n_seeds) + ": " + pf_color::seeds_text(); return PF_ERR_ARG; }
    return unitig_build_impl(ctx, kmers, n, k, g, clip_tips, del_isolated, n_seeds, stats, overflow);
}

extern "C" int pf_unitig_fetch(pf_ctx *ctx, uint64_t first_byte, uint64_t len, char *host) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    UnitigState *S = unitig_state(ctx);
    if (!S) return refuse("pf_unitig_fetch: no built graph is held (pf_unitig_build comes first)");
    if (first_byte > S->bytes || len > S->bytes - first_byte) return refuse("pf_unitig_fetch: the range lies outside the text of " + std::to_string(S->bytes) + " bytes");
    if (len && !host) return refuse("pf_unitig_fetch: host is needed");
    if (!len) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(host, S->text + first_byte, len, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_unitig_text(pf_ctx *ctx, const char **text_dev, uint64_t *n_bytes) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (!text_dev || !n_bytes) return refuse("pf_unitig_text: text_dev and n_bytes are needed");
    *text_dev = nullptr;
    *n_bytes = 0;
    UnitigState *S = unitig_state(ctx);
    if (!S) return refuse("pf_unitig_text: no built graph is held (pf_unitig_build comes first)");
    *text_dev = S->text;
    *n_bytes = S->bytes;
    return PF_OK;
}

extern "C" int pf_unitig_release(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    unitig_destroy(ctx);
    return PF_OK;
}
