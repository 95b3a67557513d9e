// K-CLIP: adapter read-through clipped on the device, in front of the steps of K-TRIM and K-TRIMCOUNT (`--adapters`).  The rule is
// pf_clip_rule.hpp; this file is its device form and the state of an open clip (pf_clip_begin .. pf_clip_end).
//
//   adapters   packed once per clip on the device: two bit planes of the 2-bit base code (128 bits each, bit j = adapter position j),
//              length and side.  A block copies them into 2.3 KB of LDS when it starts.
//   read       a ROW of 16 lanes per read, four reads a wavefront, as K-TRIM.  A row stages 256 bytes of the sequence line and 128
//              bytes of halo behind them (an adapter of 128 bases laid at the row step's last offset) with aligned 16-byte loads,
//              and every lane turns its 16 bytes into 16 bits of three planes: code low, code high, "is ACGTacgt".  They lie in the
//              row's LDS behind 128 bits of padding, so that an offset in front of the read is a plain bit position as well.
//   offsets    the lanes of a row take the offsets of an adapter strided.  Per offset: 128 bits of each plane from the offset's
//              bit position (five LDS words and a funnel shift a plane), the mismatch bitmap
//              ((code ^ adapter) | not valid) & overlap in two 64-bit registers, and the seed test as a 16-bit window sliding
//              over it with a running count (one add a position; an overlap with at most `seed` mismatches passes at once, and one
//              without a whole aligned block of 8 positions that holds at most `seed` of them is rejected at once: byte-wise counts).
//   score      only for an offset whose seed held (rare beside true read-through): one serial pass over the overlap, the quality
//              byte fetched from global memory at mismatches only.
//   result     a row-wide min of the passing offsets gives o*; lane 0 writes clip_end[r].
// Why not the 2-bit-codes-plus-XOR-of-packed-words shape: with one bit a plane the mismatch bitmap has one bit a position at
// once (no fold of bit pairs), and the same extraction serves all three planes.
// Budget: LDS 64 * 32 + 64 * 4 (adapters) + 16 rows * 3 planes * 16 words * 4 = 5376 bytes a block of 256 lanes; no array is indexed
// by a run-time value in registers (the bitmaps slide in 64-bit pairs), so nothing goes to scratch.  The counters are kept per lane
// and summed per wavefront when the kernel ends: four integer atomics a wavefront at most.  Writes are plain vector stores.
//
// K-PALIN: palindrome mode for the two reads of a pair (`--adapter-pairs`; the rule: "PALINDROME MODE" in pf_clip_rule.hpp), launched
// behind K-CLIP by clip_launch when the open clip holds prefix pairs and the call has two files.
//   strings    a row of 16 lanes per pair of reads.  S1 = P1.R1 and X2 = the reverse complement of S2 = P2.R2 (RC(R2) first, then
//              RC(P2)) as three bit planes each (code low, code high, valid), bit i = position i, 40 words a plane: 36 hold 128 + 1024
//              positions, four more let 128 bits be fetched from any of them.  A lane fills the words rl, rl + 16, rl + 32 of all six
//              planes from the bytes in global memory (the reads are at most 1024 bases here; longer pairs are no candidates).
//   candidates position i of S1 lies against position i + (n2 - p - I) of X2, so a candidate I is a plain shift of one bit string
//              against the other: clip_bits128 / clip_range128 and K-CLIP's byte-count reject serve, in pieces of 128 bits that
//              overlap by 15 so that every window of 16 lies whole in one.  The lanes take 16 consecutive I a round, upwards; the
//              round in which some I passes is the last one of the prefix pair, and the next prefix pair only looks below it.
//   score      only where the seed held: serial over pieces of 128, the quality bytes fetched from global memory at mismatches only.
//   result     lane 0 combines I* with the simple clip ends K-CLIP left in clip_end[f][r] and writes both files' final ends.
// Budget: LDS 16 rows * 6 planes * 40 words * 4 = 15360 bytes a block; no run-time-indexed register arrays.  With prefix pairs open
// K-CLIP leaves reads_clipped / reads_dropped / bases_clipped to K-PALIN, which counts the final ends.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/ploidyfrost_hip.h"
#include "pf_clip_dev.hpp"
#include "pf_clip_rule.hpp"
#include "pf_ctx.hpp"
#include "pf_reads_dev.hpp"
#include "pf_trim_dev.hpp"

static_assert(sizeof(pf_clip_stats) == sizeof(pf_clip::Stats), "the rule header restates the ABI's record");
static_assert(sizeof(pf_clip_pair_stats) == sizeof(pf_clip::PairStats), "the rule header restates the ABI's record");

namespace pf {

constexpr int CLIP_PAD_WORDS = 4;                                        // 128 bits in front of a row step: offsets down to -(128 - 16)
constexpr int CLIP_HALO_UNITS = 8;                                       // 128 bytes behind it
constexpr int CLIP_UNITS = TRIM_ROW + CLIP_HALO_UNITS;
constexpr int CLIP_PLANE_WORDS = CLIP_PAD_WORDS + CLIP_UNITS / 2;        // 16
constexpr int32_t CLIP_NO_OFFSET = 0x7FFFFFFF;
static_assert(16 * CLIP_HALO_UNITS >= (int)pf_clip::MAX_LEN && 32 * CLIP_PAD_WORDS >= (int)pf_clip::MAX_LEN, "halo and padding hold a whole adapter");
static_assert(pf_clip::MAX_LEN == 128 && pf_clip::WINDOW == 16, "the bitmaps are two 64-bit words, the seed window 16 bits");

struct ClipAdapter {   // bit j & 31 of word j >> 5 of a plane = that bit of pf_mask::base_code of adapter position j
    uint32_t lo[4], hi[4];
};
struct ClipState {
    uint32_t n_adapters = 0, seed = 0, score = 0;
    ClipAdapter *d_ad = nullptr;             // n_adapters
    uint32_t *d_meta = nullptr;              // length | side << 8
    unsigned long long *d_counts = nullptr;  // pf_clip_stats as it lies
    const uint32_t *last[2] = {nullptr, nullptr};   // the clip ends of the last launch, in the caller's workspace until its next call
    uint64_t last_n = 0;
    // K-PALIN: the prefix pairs of a clip opened with pf_clip_begin_pairs (n_pairs == 0: none)
    uint32_t n_pairs = 0, pair_score = 0, pair_min = 0, keep_both = 0;
    char *d_prefix = nullptr;                     // pair q: P1 at 256 q, P2 at 256 q + 128, upper case
    uint32_t *d_plen = nullptr;                   // p of pair q
    unsigned long long *d_pair_counts = nullptr;  // pf_clip_pair_stats as it lies
};
static inline ClipState *clip_state(pf_ctx *ctx) { return static_cast<ClipState *>(ctx->clip); }

struct ClipArgs {
    const char *text;
    uint64_t n_bytes;
    const uint32_t *lines;
    uint64_t n_rec;
    const ClipAdapter *ad;
    const uint32_t *meta;
    uint32_t n_adapters, file_side, seed, score, phred;
    uint32_t *clip_end;
    unsigned long long *counts;
    uint32_t count_ends;   // 0: K-PALIN follows and counts the final ends (candidates_scored stays here)
};

// 128 bits of a plane from bit position `at` (0 <= at, at + 128 <= 32 * CLIP_PLANE_WORDS)
__device__ inline void clip_bits128(const uint32_t *plane, int at, uint64_t &b0, uint64_t &b1) {
    const int w = at >> 5, sh = at & 31;
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (uint32_t)(((((uint64_t)plane[w + i + 1]) << 32) | plane[w + i]) >> sh);
    b0 = ((uint64_t)o[1] << 32) | o[0];
    b1 = ((uint64_t)o[3] << 32) | o[2];
}
// bits [a, z) of 128, 0 <= a < z <= 128
__device__ inline void clip_range128(int a, int z, uint64_t &m0, uint64_t &m1) {
    const uint64_t below_z0 = z >= 64 ? ~0ull : (1ull << z) - 1, below_z1 = z >= 128 ? ~0ull : z > 64 ? (1ull << (z - 64)) - 1 : 0ull;
    const uint64_t below_a0 = a >= 64 ? ~0ull : (1ull << a) - 1, below_a1 = a > 64 ? (1ull << (a - 64)) - 1 : 0ull;
    m0 = below_z0 & ~below_a0;
    m1 = below_z1 & ~below_a1;
}
__device__ inline void clip_shr128(uint64_t &b0, uint64_t &b1, int s) {   // 0 <= s < 128
    if (s >= 64) { b0 = b1 >> (s - 64); b1 = 0; }
    else if (s) { b0 = (b0 >> s) | (b1 << (64 - s)); b1 >>= s; }
}

// number of set bits in every byte of x
__device__ inline uint64_t clip_byte_counts(uint64_t x) {
    x = x - ((x >> 1) & 0x5555555555555555ull);
    x = (x & 0x3333333333333333ull) + ((x >> 2) & 0x3333333333333333ull);
    return (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0Full;
}
// does some byte of c (every byte below 128) hold less than n, 1 <= n <= 128?
__device__ inline bool clip_some_byte_below(uint64_t c, uint32_t n) {
    return ((c - 0x0101010101010101ull * n) & ~c & 0x8080808080808080ull) != 0;
}
// The reject in front of the window scan.  (s0, s1): the mismatch bitmap of an overlap of L >= 16 positions from bit 0.  Every window
// of 16 positions holds a whole block of 8 that starts at a multiple of 8 (the block at the first multiple of 8 in the window ends
// at most 15 positions behind the window's start), so a window with at most `seed` mismatches needs such a block, whole inside the
// overlap, with at most `seed` of them.  The positions behind the last whole block are counted as mismatches here.
__device__ inline bool clip_some_block_may_hold_a_seed(uint64_t s0, uint64_t s1, int L, uint32_t seed) {
    const int nb = L >> 3;   // whole blocks: 2 .. 16
    if (nb < 8) { s0 |= ~0ull << (8 * nb); s1 = ~0ull; }
    else if (nb < 16) s1 |= ~0ull << (8 * (nb - 8));
    return clip_some_byte_below(clip_byte_counts(s0), seed + 1) || clip_some_byte_below(clip_byte_counts(s1), seed + 1);
}

__global__ __launch_bounds__(TRIM_BLOCK) void k_clip(const ClipArgs a) {
    __shared__ ClipAdapter s_ad[pf_clip::MAX_ADAPTERS];
    __shared__ uint32_t s_meta[pf_clip::MAX_ADAPTERS];
    __shared__ uint32_t s_plane[TRIM_ROWS][3][CLIP_PLANE_WORDS];
    const int rl = (int)threadIdx.x & (TRIM_ROW - 1), row = (int)threadIdx.x / TRIM_ROW;
    for (uint32_t i = threadIdx.x; i < a.n_adapters * 8u; i += TRIM_BLOCK) reinterpret_cast<uint32_t *>(s_ad)[i] = reinterpret_cast<const uint32_t *>(a.ad)[i];
    for (uint32_t i = threadIdx.x; i < a.n_adapters; i += TRIM_BLOCK) s_meta[i] = a.meta[i];
    if (rl < CLIP_PAD_WORDS)
        for (int pl = 0; pl < 3; ++pl) s_plane[row][pl][rl] = 0;   // the padding: never inside an overlap
    __syncthreads();
    uint16_t *half[3];
    for (int pl = 0; pl < 3; ++pl) half[pl] = reinterpret_cast<uint16_t *>(s_plane[row][pl]) + 2 * CLIP_PAD_WORDS;
    uint64_t clipped = 0, dropped = 0, bases = 0, scored = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_ROWS + row; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_ROWS) {
        const uint32_t sb = a.lines[8 * r + 2], n = a.lines[8 * r + 3] - sb, qb = a.lines[8 * r + 6];
        const uint64_t unit0 = sb >> 4;
        const int mis = (int)(sb & 15u);   // position p of the read is byte mis + p from unit0
        int32_t best = CLIP_NO_OFFSET;
        const int32_t o_last = pf_clip::last_offset(n);
        const int n_seg = n >= pf_clip::min_overlap() ? ((mis + o_last) >> 8) + 1 : 0;   // row steps that hold an offset
        for (int ch = 0; ch < n_seg; ++ch) {
            row_sync();   // the last row step has been read
            for (int u = rl; u < CLIP_UNITS; u += TRIM_ROW) {
                const uint4 v = mask_load_unit(a.text, a.n_bytes, unit0 + (uint64_t)ch * TRIM_ROW + (uint64_t)u);
                uint32_t lo = 0, hi = 0, ok = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint8_t c = (uint8_t)unit_byte(v, k);
                    const uint32_t code = pf_mask::base_code(c);
                    lo |= (code & 1u) << k;
                    hi |= (code >> 1) << k;
                    ok |= (uint32_t)pf_mask::is_base(c) << k;
                }
                half[0][u] = (uint16_t)lo;
                half[1][u] = (uint16_t)hi;
                half[2][u] = (uint16_t)ok;
            }
            row_sync();
            // offsets of this row step: o + mis in [256 ch, 256 ch + 256); the first one also takes the offsets in front of the read
            const int32_t seg_lo = ch * TRIM_STEP_BYTES - mis, seg_hi = seg_lo + TRIM_STEP_BYTES - 1;
            for (uint32_t ai = 0; ai < a.n_adapters; ++ai) {
                const uint32_t meta = s_meta[ai], m = meta & 0xFFu;
                if (!pf_clip::applies(meta >> 8, a.file_side)) continue;
                const int32_t first = ch == 0 ? pf_clip::first_offset(m) : seg_lo;
                const int32_t last = o_last < seg_hi ? o_last : seg_hi;
                const uint64_t alo0 = ((uint64_t)s_ad[ai].lo[1] << 32) | s_ad[ai].lo[0], alo1 = ((uint64_t)s_ad[ai].lo[3] << 32) | s_ad[ai].lo[2];
                const uint64_t ahi0 = ((uint64_t)s_ad[ai].hi[1] << 32) | s_ad[ai].hi[0], ahi1 = ((uint64_t)s_ad[ai].hi[3] << 32) | s_ad[ai].hi[2];
                for (int32_t o = first + rl; o <= last; o += TRIM_ROW) {
                    const int at = 32 * CLIP_PAD_WORDS + (o - seg_lo);   // >= 128 - 112 - 15; + 128 <= 512
                    uint64_t l0, l1, h0, h1, v0, v1, in0, in1;
                    clip_bits128(s_plane[row][0], at, l0, l1);
                    clip_bits128(s_plane[row][1], at, h0, h1);
                    clip_bits128(s_plane[row][2], at, v0, v1);
                    const int j_lo = o < 0 ? -o : 0, j_hi = (int32_t)n - o < (int32_t)m ? (int32_t)n - o : (int32_t)m;   // the overlap in adapter positions
                    clip_range128(j_lo, j_hi, in0, in1);
                    uint64_t m0 = ((l0 ^ alo0) | (h0 ^ ahi0) | ~v0) & in0, m1 = ((l1 ^ alo1) | (h1 ^ ahi1) | ~v1) & in1;
                    // ---- seed: a window of 16 positions inside the overlap with at most `seed` mismatches ----
                    bool seed_ok = (uint32_t)(__popcll(m0) + __popcll(m1)) <= a.seed;
                    if (!seed_ok) {
                        uint64_t s0 = m0, s1 = m1;
                        clip_shr128(s0, s1, j_lo);
                        if (!clip_some_block_may_hold_a_seed(s0, s1, j_hi - j_lo, a.seed)) continue;   // (most overlaps of unrelated bases end here)
                        uint32_t cnt = (uint32_t)__popc((uint32_t)s0 & 0xFFFFu);
                        for (int j = j_lo;; ++j) {
                            if (cnt <= a.seed) { seed_ok = true; break; }
                            if (j + (int)pf_clip::WINDOW >= j_hi) break;
                            cnt += (uint32_t)((s0 >> 16) & 1ull) - (uint32_t)(s0 & 1ull);
                            s0 = (s0 >> 1) | (s1 << 63);
                            s1 >>= 1;
                        }
                    }
                    if (!seed_ok) continue;
                    // ---- score: the best contiguous sub-range of the overlap ----
                    scored += 1;
                    clip_shr128(m0, m1, j_lo);
                    clip_shr128(v0, v1, j_lo);
                    int32_t run = 0, top = 0;
                    for (int j = j_lo; j < j_hi; ++j) {
                        int32_t w = 0;
                        if (v0 & 1ull) w = (m0 & 1ull) ? pf_clip::mismatch_cost((uint8_t)a.text[(uint64_t)qb + (uint64_t)(o + j)], a.phred) : pf_clip::MATCH;
                        run = run + w > 0 ? run + w : 0;
                        top = run > top ? run : top;
                        m0 = (m0 >> 1) | (m1 << 63);
                        m1 >>= 1;
                        v0 = (v0 >> 1) | (v1 << 63);
                        v1 >>= 1;
                    }
                    if (pf_clip::score_passes(top, a.score) && o < best) best = o;
                }
            }
        }
        // the smallest passing offset of the row (biased: the order of signed numbers)
        const uint32_t least = row_min_u32((uint32_t)best ^ 0x80000000u) ^ 0x80000000u;
        if (rl == 0) {
            const bool found = (int32_t)least != CLIP_NO_OFFSET;
            const uint32_t e = pf_clip::clip_end(found, (int32_t)least, n);
            a.clip_end[r] = e;
            clipped += found && e != 0;
            dropped += found && e == 0;
            bases += n - e;
        }
    }
    clipped = wave_sum_u64(clipped);
    dropped = wave_sum_u64(dropped);
    bases = wave_sum_u64(bases);
    scored = wave_sum_u64(scored);
    if (lane_id() == 0) {
        const uint32_t f = a.file_side == 2 ? 1 : 0;   // pf_clip_stats: four pairs [file]
        if (clipped && a.count_ends) atomicAdd(&a.counts[0 + f], (unsigned long long)clipped);
        if (dropped && a.count_ends) atomicAdd(&a.counts[2 + f], (unsigned long long)dropped);
        if (bases && a.count_ends) atomicAdd(&a.counts[4 + f], (unsigned long long)bases);
        if (scored) atomicAdd(&a.counts[6 + f], (unsigned long long)scored);
    }
}

// ---- K-PALIN ----
constexpr int PALIN_WORDS = 40;                  // words of a plane: 36 hold 128 + 1024 positions, four more behind them
constexpr int PALIN_PIECE = 128;                 // positions of a piece
constexpr int PALIN_SEED_STEP = PALIN_PIECE - (int)pf_clip::WINDOW + 1;   // from piece to piece in the seed test: no window is split
constexpr uint32_t PALIN_NONE = 0xFFFFFFFFu;
static_assert(32 * (PALIN_WORDS - 4) >= (int)(pf_clip::MAX_LEN + pf_clip::MAX_PAIR_READ), "a plane holds a prefix and a read");

struct PalinArgs {
    const char *text[2];
    const uint32_t *lines[2];
    uint64_t n_rec;
    const char *prefix;
    const uint32_t *plen;
    uint32_t n_pairs, seed, pair_score, pair_min, keep_both, phred, have_simple;
    uint32_t *clip_end[2];
    unsigned long long *counts;        // pf_clip_stats
    unsigned long long *pair_counts;   // pf_clip_pair_stats
};

// L positions (1 .. 128) of S1 from position at1 against X2 from position at2: the positions that are no match (m) and the valid ones (v)
__device__ inline void palin_piece(const uint32_t (*pl)[PALIN_WORDS], int at1, int at2, int L, uint64_t &m0, uint64_t &m1, uint64_t &v0, uint64_t &v1) {
    uint64_t al0, al1, ah0, ah1, av0, av1, bl0, bl1, bh0, bh1, bv0, bv1, in0, in1;
    clip_bits128(pl[0], at1, al0, al1);
    clip_bits128(pl[1], at1, ah0, ah1);
    clip_bits128(pl[2], at1, av0, av1);
    clip_bits128(pl[3], at2, bl0, bl1);
    clip_bits128(pl[4], at2, bh0, bh1);
    clip_bits128(pl[5], at2, bv0, bv1);
    clip_range128(0, L, in0, in1);
    v0 = av0 & bv0 & in0;
    v1 = av1 & bv1 & in1;
    m0 = ((al0 ^ bl0) | (ah0 ^ bh0) | ~v0) & in0;
    m1 = ((al1 ^ bl1) | (ah1 ^ bh1) | ~v1) & in1;
}
// (s0, s1): the mismatch bitmap of L >= 16 positions from bit 0: does some window of 16 hold at most `seed`?
__device__ inline bool clip_some_window_holds(uint64_t s0, uint64_t s1, int L, uint32_t seed) {
    uint32_t cnt = (uint32_t)__popc((uint32_t)s0 & 0xFFFFu);
    for (int j = 0;; ++j) {
        if (cnt <= seed) return true;
        if (j + (int)pf_clip::WINDOW >= L) return false;
        cnt += (uint32_t)((s0 >> 16) & 1ull) - (uint32_t)(s0 & 1ull);
        s0 = (s0 >> 1) | (s1 << 63);
        s1 >>= 1;
    }
}

__global__ __launch_bounds__(TRIM_BLOCK) void k_palin(const PalinArgs a) {
    __shared__ uint32_t s_pl[TRIM_ROWS][6][PALIN_WORDS];
    const int rl = (int)threadIdx.x & (TRIM_ROW - 1), row = (int)threadIdx.x / TRIM_ROW;
    uint32_t (*pl)[PALIN_WORDS] = s_pl[row];
    uint64_t clipped0 = 0, clipped1 = 0, dropped0 = 0, dropped1 = 0, bases0 = 0, bases1 = 0;
    uint64_t p_clipped = 0, p_dropped = 0, p_long = 0, p_scored = 0, p_bases0 = 0, p_bases1 = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * TRIM_ROWS + row; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_ROWS) {
        const uint32_t sb1 = a.lines[0][8 * r + 2], n1 = a.lines[0][8 * r + 3] - sb1, qb1 = a.lines[0][8 * r + 6];
        const uint32_t sb2 = a.lines[1][8 * r + 2], n2 = a.lines[1][8 * r + 3] - sb2, qb2 = a.lines[1][8 * r + 6];
        const bool too_long = pf_clip::pair_too_long(n1, n2);
        uint32_t limit = too_long ? 0u : pf_clip::pair_candidates(n1, n2, a.pair_min);   // candidates lie below it
        bool found = false;
        for (uint32_t q = 0; q < a.n_pairs && limit > 0; ++q) {
            const uint32_t p = a.plen[q];
            const char *P1 = a.prefix + 256u * q, *P2 = P1 + 128;
            row_sync();   // the last strings have been read
            for (int w = rl; w < PALIN_WORDS; w += TRIM_ROW) {
                uint32_t lo = 0, hi = 0, ok = 0;
                if (32u * (uint32_t)w < p + n1) {
#pragma unroll 8
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t i = 32u * (uint32_t)w + b;
                        const uint8_t c = i < p ? (uint8_t)P1[i] : i - p < n1 ? (uint8_t)a.text[0][(uint64_t)sb1 + (i - p)] : (uint8_t)0;
                        const uint32_t code = pf_mask::base_code(c);
                        lo |= (code & 1u) << b;
                        hi |= (code >> 1) << b;
                        ok |= (uint32_t)pf_mask::is_base(c) << b;
                    }
                }
                pl[0][w] = lo;
                pl[1][w] = hi;
                pl[2][w] = ok;
                lo = hi = ok = 0;
                if (32u * (uint32_t)w < p + n2) {
#pragma unroll 8
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32u * (uint32_t)w + b;   // position k of X2: RC(R2), then RC(P2)
                        const uint8_t c = k < n2 ? (uint8_t)a.text[1][(uint64_t)sb2 + (n2 - 1 - k)] : k - n2 < p ? (uint8_t)P2[p - 1 - (k - n2)] : (uint8_t)0;
                        const uint32_t code = pf_mask::base_code(c) ^ 3u;   // the complement
                        lo |= (code & 1u) << b;
                        hi |= (code >> 1) << b;
                        ok |= (uint32_t)pf_mask::is_base(c) << b;
                    }
                }
                pl[3][w] = lo;
                pl[4][w] = hi;
                pl[5][w] = ok;
            }
            row_sync();
            for (uint32_t I0 = 0; I0 < limit; I0 += TRIM_ROW) {
                const uint32_t I = I0 + (uint32_t)rl;
                bool seed_ok = false, pass = false;
                uint32_t lo = 0, hi = 0;
                if (I < limit && pf_clip::pair_range(p, n1, n2, I, lo, hi)) {
                    const int d = (int)n2 - (int)p - (int)I;   // position i of S1 lies against position i + d of X2; lo + d >= 0
                    for (uint32_t i0 = lo; i0 + pf_clip::WINDOW <= hi && !seed_ok; i0 += PALIN_SEED_STEP) {
                        const int L = (int)(hi - i0) < PALIN_PIECE ? (int)(hi - i0) : PALIN_PIECE;
                        uint64_t m0, m1, v0, v1;
                        palin_piece(pl, (int)i0, (int)i0 + d, L, m0, m1, v0, v1);
                        seed_ok = (uint32_t)(__popcll(m0) + __popcll(m1)) <= a.seed;
                        if (!seed_ok && clip_some_block_may_hold_a_seed(m0, m1, L, a.seed)) seed_ok = clip_some_window_holds(m0, m1, L, a.seed);
                    }
                    if (seed_ok) {
                        const uint32_t T = 2 * p + I;
                        int32_t run = 0, top = 0;
                        for (uint32_t i0 = lo; i0 < hi; i0 += PALIN_PIECE) {
                            const int L = (int)(hi - i0) < PALIN_PIECE ? (int)(hi - i0) : PALIN_PIECE;
                            uint64_t m0, m1, v0, v1;
                            palin_piece(pl, (int)i0, (int)i0 + d, L, m0, m1, v0, v1);
                            for (int j = 0; j < L; ++j) {
                                int32_t w = 0;
                                if (v0 & 1ull) {
                                    w = pf_clip::MATCH;
                                    if (m0 & 1ull) {
                                        const uint32_t i = i0 + (uint32_t)j, jj = T - 1 - i;   // (i < p and jj < p never meet)
                                        const int q2 = jj >= p ? (int)(uint8_t)a.text[1][(uint64_t)qb2 + (jj - p)] - (int)a.phred : 0;
                                        const int qq = i >= p ? pf_clip::pair_mismatch_quality((int)(uint8_t)a.text[0][(uint64_t)qb1 + (i - p)] - (int)a.phred, jj >= p, q2) : q2;
                                        w = -pf_clip::PENALTY * (qq > 0 ? qq : 0);
                                    }
                                }
                                run = run + w > 0 ? run + w : 0;
                                top = run > top ? run : top;
                                m0 = (m0 >> 1) | (m1 << 63);
                                m1 >>= 1;
                                v0 = (v0 >> 1) | (v1 << 63);
                                v1 >>= 1;
                            }
                        }
                        pass = pf_clip::score_passes(top, a.pair_score);
                    }
                }
                const uint32_t least = row_min_u32(pass ? I : PALIN_NONE);
                if (least != PALIN_NONE) {   // the smallest passing I of this prefix pair: the candidates beyond it were not examined
                    p_scored += seed_ok && I <= least;
                    limit = least;
                    found = true;
                    break;
                }
                p_scored += seed_ok;
            }
        }
        if (rl == 0) {
            const uint32_t n[2] = {n1, n2};
            uint32_t took[2], e[2];
            for (int f = 0; f < 2; ++f) {
                const uint32_t simple = a.have_simple ? a.clip_end[f][r] : n[f];
                e[f] = pf_clip::pair_end(found, limit, simple, f, a.keep_both != 0);
                a.clip_end[f][r] = e[f];
                took[f] = simple - e[f];
            }
            clipped0 += e[0] != n1 && e[0] != 0;
            dropped0 += e[0] != n1 && e[0] == 0;
            bases0 += n1 - e[0];
            clipped1 += e[1] != n2 && e[1] != 0;
            dropped1 += e[1] != n2 && e[1] == 0;
            bases1 += n2 - e[1];
            p_clipped += found && limit != 0;
            p_dropped += found && limit == 0;
            p_long += too_long;
            p_bases0 += took[0];
            p_bases1 += took[1];
        }
    }
    clipped0 = wave_sum_u64(clipped0);
    clipped1 = wave_sum_u64(clipped1);
    dropped0 = wave_sum_u64(dropped0);
    dropped1 = wave_sum_u64(dropped1);
    bases0 = wave_sum_u64(bases0);
    bases1 = wave_sum_u64(bases1);
    p_clipped = wave_sum_u64(p_clipped);
    p_dropped = wave_sum_u64(p_dropped);
    p_long = wave_sum_u64(p_long);
    p_scored = wave_sum_u64(p_scored);
    p_bases0 = wave_sum_u64(p_bases0);
    p_bases1 = wave_sum_u64(p_bases1);
    if (lane_id() == 0) {
        if (clipped0) atomicAdd(&a.counts[0], (unsigned long long)clipped0);
        if (clipped1) atomicAdd(&a.counts[1], (unsigned long long)clipped1);
        if (dropped0) atomicAdd(&a.counts[2], (unsigned long long)dropped0);
        if (dropped1) atomicAdd(&a.counts[3], (unsigned long long)dropped1);
        if (bases0) atomicAdd(&a.counts[4], (unsigned long long)bases0);
        if (bases1) atomicAdd(&a.counts[5], (unsigned long long)bases1);
        if (p_clipped) atomicAdd(&a.pair_counts[0], (unsigned long long)p_clipped);
        if (p_dropped) atomicAdd(&a.pair_counts[1], (unsigned long long)p_dropped);
        if (p_long) atomicAdd(&a.pair_counts[2], (unsigned long long)p_long);
        if (p_scored) atomicAdd(&a.pair_counts[3], (unsigned long long)p_scored);
        if (p_bases0) atomicAdd(&a.pair_counts[4], (unsigned long long)p_bases0);
        if (p_bases1) atomicAdd(&a.pair_counts[5], (unsigned long long)p_bases1);
    }
}

// ---- host side ----
int clip_launch(pf_ctx *ctx, int n_files, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec, uint32_t phred,
                uint32_t *const *clip_end) {
    ClipState *S = clip_state(ctx);
    if (!S) { pf::CtxErr{ctx} = "K-CLIP: no clip is open"; return PF_ERR_ARG; }
    clip_forget(ctx);
    if (n_rec == 0) return PF_OK;
    S->last[0] = clip_end[0];
    S->last[1] = n_files == 2 ? clip_end[1] : nullptr;
    S->last_n = n_rec;
    const bool palin = n_files == 2 && S->n_pairs != 0;               // K-PALIN follows and writes the final ends
    const bool simple = S->n_adapters != 0 || !palin;                 // (a single-ended call with no simple adapter: every end is n)
    size_t at = (size_t)-1;
    if (simple) (void)ctx_begin_at(ctx, PF_K_CLIP, ctx->stream, &at);
    for (int f = 0; f < n_files && simple; ++f) {
        ClipArgs a = {};
        a.text = text[f];
        a.n_bytes = n_bytes[f];
        a.lines = lines[f];
        a.n_rec = n_rec;
        a.ad = S->d_ad;
        a.meta = S->d_meta;
        a.n_adapters = S->n_adapters;
        a.file_side = (uint32_t)f + 1;
        a.seed = S->seed;
        a.score = S->score;
        a.phred = phred;
        a.clip_end = clip_end[f];
        a.counts = S->d_counts;
        a.count_ends = palin ? 0u : 1u;
        k_clip<<<ctx_grid(ctx, n_rec * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(a);
    }
    if (simple) ctx_end_at(ctx, at, ctx->stream);
    if (palin) {
        PalinArgs a = {};
        for (int f = 0; f < 2; ++f) {
            a.text[f] = text[f];
            a.lines[f] = lines[f];
            a.clip_end[f] = clip_end[f];
        }
        a.n_rec = n_rec;
        a.prefix = S->d_prefix;
        a.plen = S->d_plen;
        a.n_pairs = S->n_pairs;
        a.seed = S->seed;
        a.pair_score = S->pair_score;
        a.pair_min = S->pair_min;
        a.keep_both = S->keep_both;
        a.phred = phred;
        a.have_simple = simple ? 1u : 0u;
        a.counts = S->d_counts;
        a.pair_counts = S->d_pair_counts;
        size_t pat = (size_t)-1;
        (void)ctx_begin_at(ctx, PF_K_PALIN, ctx->stream, &pat);
        k_palin<<<ctx_grid(ctx, n_rec * TRIM_ROW, TRIM_BLOCK, 8), TRIM_BLOCK, 0, ctx->stream>>>(a);
        ctx_end_at(ctx, pat, ctx->stream);
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-CLIP launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    if (simple) ctx_units(ctx, PF_K_CLIP, n_rec * (uint64_t)n_files);
    if (palin) ctx_units(ctx, PF_K_PALIN, n_rec);
    return PF_OK;
}

void clip_forget(pf_ctx *ctx) {
    ClipState *S = clip_state(ctx);
    if (!S) return;
    S->last[0] = S->last[1] = nullptr;
    S->last_n = 0;
}

void clip_destroy(pf_ctx *ctx) {
    ClipState *S = clip_state(ctx);
    if (!S) return;
    if (S->d_ad) (void)hipFree(S->d_ad);
    if (S->d_meta) (void)hipFree(S->d_meta);
    if (S->d_counts) (void)hipFree(S->d_counts);
    if (S->d_prefix) (void)hipFree(S->d_prefix);
    if (S->d_plen) (void)hipFree(S->d_plen);
    if (S->d_pair_counts) (void)hipFree(S->d_pair_counts);
    delete S;
    ctx->clip = nullptr;
}

}  // namespace pf

using namespace pf;

// pf_clip_begin (prefix_off == nullptr, n_pairs == 0) and pf_clip_begin_pairs
static int clip_begin(pf_ctx *ctx, const char *who, bool pairs, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                      const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs, uint32_t seed, uint32_t score, uint32_t pair_score,
                      uint32_t pair_min, int keep_both) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = std::string(who) + ": " + m; return (int)PF_ERR_ARG; };
    if (ctx->clip) return refuse("a clip is open already");
    uint32_t bad = 0;
    bool of_pair = false;   // the refusal names a prefix pair, not an adapter
    const int c = pairs ? pf_clip::pair_set_clause(bases, adapter_off, side, n_adapters, prefix_bases, prefix_off, n_pairs, seed, score, pair_score, pair_min, &bad, &of_pair)
                        : pf_clip::set_clause(bases, adapter_off, side, n_adapters, seed, score, &bad);
    if (of_pair && (c == pf_clip::REFUSE_PAIR_LENGTHS || c == pf_clip::REFUSE_LENGTH || c == pf_clip::REFUSE_BYTE)) return refuse("prefix pair " + std::to_string(bad) + ": " + pf_clip::refusal_text(c));
    if (c == pf_clip::REFUSE_LENGTH || c == pf_clip::REFUSE_BYTE || c == pf_clip::REFUSE_SIDE)
        return refuse("adapter " + std::to_string(bad) + ": " + pf_clip::refusal_text(c));
    if (c) return refuse(pf_clip::refusal_text(c));
    std::vector<ClipAdapter> ad(n_adapters, ClipAdapter{});
    std::vector<uint32_t> meta(n_adapters);
    for (uint32_t a = 0; a < n_adapters; ++a) {
        const uint32_t m = adapter_off[a + 1] - adapter_off[a];
        meta[a] = m | ((uint32_t)side[a] << 8);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t code = pf_mask::base_code((uint8_t)bases[adapter_off[a] + j]);
            ad[a].lo[j >> 5] |= (code & 1u) << (j & 31);
            ad[a].hi[j >> 5] |= (code >> 1) << (j & 31);
        }
    }
    std::vector<char> prefix((size_t)n_pairs * 256, 'N');
    std::vector<uint32_t> plen(n_pairs);
    for (uint32_t q = 0; q < n_pairs; ++q) {
        plen[q] = prefix_off[2 * q + 1] - prefix_off[2 * q];
        for (uint32_t h = 0; h < 2; ++h)
            for (uint32_t j = 0; j < plen[q]; ++j) prefix[256 * q + 128 * h + j] = (char)((uint8_t)prefix_bases[prefix_off[2 * q + h] + j] & 0xDFu);
    }
    PF_HIP(hipSetDevice(ctx->device));
    ClipState *S = new ClipState;
    ctx->clip = S;
    S->n_adapters = n_adapters;
    S->seed = seed;
    S->score = score;
    S->n_pairs = n_pairs;
    S->pair_score = pair_score;
    S->pair_min = pair_min;
    S->keep_both = keep_both ? 1u : 0u;
    struct Undo { pf_ctx *c; bool armed; ~Undo() { if (armed) clip_destroy(c); } } undo{ctx, true};
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_ad), (ad.size() + 1) * sizeof(ClipAdapter)));   // (+ 1: a clip of prefix pairs alone holds none)
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_meta), (meta.size() + 1) * 4));
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_counts), sizeof(pf_clip_stats)));
    if (n_adapters) {
        PF_HIP(hipMemcpyAsync(S->d_ad, ad.data(), ad.size() * sizeof(ClipAdapter), hipMemcpyHostToDevice, ctx->stream));
        PF_HIP(hipMemcpyAsync(S->d_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    PF_HIP(hipMemsetAsync(S->d_counts, 0, sizeof(pf_clip_stats), ctx->stream));
    if (n_pairs) {
        PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_prefix), prefix.size()));
        PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_plen), plen.size() * 4));
        PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_pair_counts), sizeof(pf_clip_pair_stats)));
        PF_HIP(hipMemcpyAsync(S->d_prefix, prefix.data(), prefix.size(), hipMemcpyHostToDevice, ctx->stream));
        PF_HIP(hipMemcpyAsync(S->d_plen, plen.data(), plen.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        PF_HIP(hipMemsetAsync(S->d_pair_counts, 0, sizeof(pf_clip_pair_stats), ctx->stream));
    }
    PF_HIP(hipStreamSynchronize(ctx->stream));   // (the host vectors go away)
    undo.armed = false;
    return PF_OK;
}

extern "C" int pf_clip_begin(pf_ctx *ctx, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t seed,
                             uint32_t score) {
    return clip_begin(ctx, "pf_clip_begin", false, bases, adapter_off, side, n_adapters, nullptr, nullptr, 0, seed, score, 0, 0, 0);
}

extern "C" int pf_clip_begin_pairs(pf_ctx *ctx, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                                   const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs, uint32_t seed, uint32_t score,
                                   uint32_t pair_score, uint32_t pair_min, int keep_both) {
    return clip_begin(ctx, "pf_clip_begin_pairs", true, bases, adapter_off, side, n_adapters, prefix_bases, prefix_off, n_pairs, seed, score, pair_score,
                      pair_min, keep_both);
}

extern "C" int pf_clip_pair_stats_get(pf_ctx *ctx, pf_clip_pair_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_clip_pair_stats_get: " + m; return (int)PF_ERR_ARG; };
    if (!ctx->clip) return refuse("no clip is open");
    if (!clip_state(ctx)->n_pairs) return refuse("the open clip holds no prefix pairs");
    if (!stats) return refuse("stats is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(stats, clip_state(ctx)->d_pair_counts, sizeof(pf_clip_pair_stats), hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_clip_stats_get(pf_ctx *ctx, pf_clip_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_clip_stats_get: " + m; return (int)PF_ERR_ARG; };
    if (!ctx->clip) return refuse("no clip is open");
    if (!stats) return refuse("stats is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(stats, clip_state(ctx)->d_counts, sizeof(pf_clip_stats), hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_clip_last_ends(pf_ctx *ctx, int file, uint32_t *clip_end, uint64_t n_records) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_clip_last_ends: " + m; return (int)PF_ERR_ARG; };
    ClipState *S = clip_state(ctx);
    if (!S) return refuse("no clip is open");
    if (file < 0 || file > 1) return refuse("file is 0 or 1");
    if (!n_records) return PF_OK;   // (also behind a call that took no whole record: it clipped none)
    if (!S->last[file]) return refuse("the last call clipped no such file");
    if (n_records > S->last_n) return refuse("the last call clipped " + std::to_string(S->last_n) + " records, not " + std::to_string(n_records));
    if (!clip_end) return refuse("clip_end is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(clip_end, S->last[file], (size_t)n_records * 4, hipMemcpyDefault, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_clip_end(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    if (!ctx->clip) { pf::CtxErr{ctx} = "pf_clip_end: no clip is open"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    clip_destroy(ctx);
    return PF_OK;
}
