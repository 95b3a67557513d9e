// The rule of `ploidyfrost run`'s second pass (K-MASKCOUNT) in one place, for the kernel (pf_maskcount.hip), the host restatement
// and the stand-alone test (tests/cpp/test_run_rule.cpp): which windows of the reads are still counted after K-MASK has painted
// its Ns -- without the paint.  `mask` followed by `build` counts every window of the masked text whose k bytes are all in
// ACGTacgt (pf_count_rule.hpp); this header says which windows of the UNMASKED text those are.
//
//   bad(q)     K-MASK's: q is a window start whose counter lies outside [low, up] (pf_mask::window_bad).  A position that is no
//              window start is never bad.
//   valid(p)   K-COUNT's: the k bytes from p are all in ACGTacgt.
//   masked(j)  pf_mask::byte_masked: a sequence byte j becomes N when some q in [j - k + 1, j] is bad.
//   survives   window p of the masked text counts when none of its bytes p .. p + k - 1 was a non-base before and none became N:
//                  survives(p) = start(p) and valid(p) and no q in [p - k + 1, p + k - 1] with bad(q)
//              (the union of [j - k + 1, j] over j = p .. p + k - 1).
//
// The test never needs the read's boundaries.  Bad bits are set at window starts only, and the window starts of two different
// reads are at least k apart: the last start of a read that ends at `end` is end - k, the first start of any later read is at or
// beyond `end` (reads do not overlap; they may touch).  So for a start p of read A no start q of another read lies in
// [p - k + 1, p + k - 1]: a later read's q >= end_A >= p + k, an earlier read's q <= end_B - k <= begin_A - k <= p - k.  Every
// set bit of the bad bitmap inside the range belongs to p's own read, whose bad windows do mask p's bytes; and the paint itself
// reaches no further (a byte j of A under a q of B would need q >= j - k + 1 > end_B - k).  For k <= 31 the range is at most 61
// consecutive bits of the bitmap: a funnel over at most three 64-bit words (the word of p and its two neighbours).
//
// valid(p) is not implied by the bits.  With low = 0 a window that holds an N has counter 0, is not bad and masks nothing -- and
// still counts nothing: the predicate asks for valid(p) itself.
//
// The key counted is the canonical form (pf_count::window_key, both strands): `build` always counts both strands.
#pragma once
#include <stdint.h>

#include "pf_count_rule.hpp"
#include "pf_mask_rule.hpp"

namespace pf_run {

// The bad bits around window start p, from the word of the bad bitmap that holds p (cur), the one before it (prev, 0 in front of
// the text) and the one after it (next, 0 behind it); b = p & 63.
//   behind: bit 63 = bad(p), bit 63 - t = bad(p - t)     (pf_mask::byte_masked's operand for byte p)
//   ahead:  bit t = bad(p + t)
PF_MASK_HD inline uint64_t bad_behind(uint64_t prev, uint64_t cur, int b) { return (cur << (63 - b)) | (b < 63 ? prev >> (b + 1) : 0ull); }
PF_MASK_HD inline uint64_t bad_ahead(uint64_t cur, uint64_t next, int b) { return (cur >> b) | (b ? next << (64 - b) : 0ull); }
// no q in [p - k + 1, p + k - 1] with bad(q)
PF_MASK_HD inline bool clear_of_bad(uint64_t prev, uint64_t cur, uint64_t next, int b, int k) {
    return !pf_mask::byte_masked(bad_behind(prev, cur, b), k) && (bad_ahead(cur, next, b) & ((1ull << k) - 1)) == 0;
}
PF_MASK_HD inline bool survives(bool start, bool valid, uint64_t prev, uint64_t cur, uint64_t next, int b, int k) {
    return start && valid && clear_of_bad(prev, cur, next, b, k);
}

// ---- the host's plain restatement (no device): what the kernel is held to ----
struct Stats {
    uint64_t reads = 0, bases = 0, kmers = 0, kmers_invalid = 0, kmers_bad = 0, kmers_kept = 0;
};

// counters[p]: the counter of the window that starts at byte p of the text (read at window starts only; 0 for a window that
// holds a non-base, as CKMCFile::GetCountersForRead gives it).  Every surviving window's canonical k-mer is counted into `table`.
// Reads are ascending and do not overlap (they may touch).
inline void count_masked_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, int k, const uint32_t *counters,
                              uint32_t low, uint32_t up, pf_count::Table &table, Stats &st) {
    const uint64_t all = (1ull << (2 * k)) - 1;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t o = off[r], n = len[r];
        st.reads += 1;
        st.bases += n;
        if (n < (uint64_t)k) continue;
        const uint64_t n_win = n - (uint64_t)k + 1;
        for (uint64_t i = 0; i < n_win; ++i) {
            st.kmers += 1;
            st.kmers_bad += pf_mask::window_bad(counters[o + i], low, up);
            uint64_t fw = 0;
            bool valid = true;
            for (int j = 0; j < k; ++j) {
                const uint8_t c = (uint8_t)text[o + i + (uint64_t)j];
                valid = valid && pf_mask::is_base(c);
                fw = ((fw << 2) | pf_mask::base_code(c)) & all;
            }
            st.kmers_invalid += !valid;
            bool clear = true;   // the read's own windows i - k + 1 .. i + k - 1: no other read's lie in the range
            const uint64_t q0 = i >= (uint64_t)(k - 1) ? i - (uint64_t)(k - 1) : 0, q1 = i + (uint64_t)k < n_win ? i + (uint64_t)k : n_win;
            for (uint64_t q = q0; q < q1; ++q) clear = clear && !pf_mask::window_bad(counters[o + q], low, up);
            if (valid && clear) {
                table[pf_count::window_key(fw, k, true)] += 1;
                st.kmers_kept += 1;
            }
        }
    }
}

}  // namespace pf_run
