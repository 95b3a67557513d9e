// The rule of `ploidyfrost count` (K-COUNT) in one place, for the kernels (pf_count.hip), the host layer (host/pf_count_host.cpp)
// and the stand-alone test (tests/cpp/test_count_rule.cpp): which windows of a read count, what their key is, what the cut-offs
// keep, and how the kept records lie in a KMC1 database.  It restates what step `2.kmc_db` of the reference's workflow asks of
// `kmc -ci<ci> -cs<cs> -cx<cx> -k<k> [-b]`; byte classes, line roles and the FASTQ format clauses are pf_mask_rule.hpp's.
//
//   windows   a read s[0..n) has one window per i in 0 .. n - k; it counts when all k bytes are in ACGTacgt (lower case read as
//             upper case) -- the windows K-MASK looks up.  3 <= k <= 31: ~0 is never a key.
//   key       min(fw, rc), first base most significant, 2-bit codes A0 C1 G2 T3; with -b (both_strands = false) the window as it
//             reads.  A k-mer equal to its own reverse complement counts once per occurrence.
//   counters  the number of counted windows of a key over all inputs, an exact uint32; a counter that would pass 2^32 - 1 ends the
//             run by name (OVERFLOW_TEXT), it never wraps.
//   cut-offs  a k-mer is written when ci <= c <= cx, with the value min(c, cs); counter_bytes = the fewest of 1..4 bytes that hold
//             min(cx, cs); the header's min_count = ci, max_count = cx, both_strands = !-b.
//   layout    KMC1 (version word 0; k >= 5): records sorted by k-mer, p = lut_prefix_len(k), a LUT of 4^p entries plus the sentinel word,
//             seven header words, the offset word, markers; (k - p) / 4 suffix bytes most significant first, counter bytes least
//             significant first.
//
// PARITY UNPINNED: `kmc` is not part of the build, and it writes the signature-binned 0x200 layout where this writes KMC1 (which
// kmc_api and this build's loader both read).
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "pf_mask_rule.hpp"

namespace pf_count {

constexpr int MIN_K = 3, MAX_K = pf_mask::MAX_K;
constexpr uint64_t EMPTY_KEY = ~0ull;               // no key of k <= 31 has its two top bits set
constexpr uint64_t COUNTER_MAX = 0xFFFFFFFFull;
constexpr uint64_t DEFAULT_CI = 2, DEFAULT_CX = 1000000000ull, DEFAULT_CS = 255;
constexpr const char *OVERFLOW_TEXT = "a k-mer occurs more than 4294967295 times";

// ---- keys ----
// reverse complement of a k-mer of 2-bit codes (first base most significant)
PF_MASK_HD inline uint64_t rev_comp(uint64_t x, int k) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * k);
}
PF_MASK_HD inline uint64_t window_key(uint64_t fw, int k, bool both_strands) {
    if (!both_strands) return fw;
    const uint64_t rc = rev_comp(fw, k);
    return rc < fw ? rc : fw;
}

// ---- cut-offs ----
enum CutClause { CUT_OK = 0, CUT_CI_ZERO, CUT_CI_ABOVE_CX, CUT_CS_ZERO, CUT_TOO_LARGE, CUT_K, CUT_K_LAYOUT };
inline int cut_clause(uint64_t ci, uint64_t cx, uint64_t cs) {
    if (ci > COUNTER_MAX || cx > COUNTER_MAX || cs > COUNTER_MAX) return CUT_TOO_LARGE;
    if (ci < 1) return CUT_CI_ZERO;
    if (ci > cx) return CUT_CI_ABOVE_CX;
    if (cs < 1) return CUT_CS_ZERO;
    return CUT_OK;
}
inline const char *cut_text(int c) {
    switch (c) {
        case CUT_CI_ZERO: return "-ci is below 1 (a k-mer that never occurs cannot be written)";
        case CUT_CI_ABOVE_CX: return "-ci is above -cx (no count lies in [ci, cx])";
        case CUT_CS_ZERO: return "-cs is below 1";
        case CUT_TOO_LARGE: return "-ci, -cx and -cs go up to 4294967295 (counters are 32 bits)";
        case CUT_K: return "-k goes from 3 to 31 (a k-mer is one 64-bit word)";
        case CUT_K_LAYOUT: return "a KMC1 database needs -k of at least 5 (a prefix of p >= 1 bases in front of whole suffix bytes)";
        default: return "no refusal";
    }
}
inline bool k_ok(int64_t k) { return k >= MIN_K && k <= MAX_K; }
PF_MASK_HD inline bool kept(uint32_t c, uint32_t ci, uint32_t cx) { return c >= ci && c <= cx; }
PF_MASK_HD inline uint32_t stored(uint32_t c, uint32_t cs) { return c < cs ? c : cs; }
inline uint32_t counter_bytes(uint64_t cx, uint64_t cs) {
    const uint64_t top = cx < cs ? cx : cs;
    return top < (1ull << 8) ? 1 : top < (1ull << 16) ? 2 : top < (1ull << 24) ? 3 : 4;
}

// ---- layout ----
// a prefix length p with (k - p) % 4 == 0, the first of 5 6 7 4 that fits (3 2 1 for the shortest k); 0 = none: k = 3 and k = 4 can be
// counted, not written
inline int lut_prefix_len(int k) {
    const int order[8] = {5, 6, 7, 4, 3, 2, 1, 8};
    for (int p : order)
        if (p < k && (k - p) % 4 == 0) return p;
    return 0;
}
PF_MASK_HD inline uint32_t suffix_bytes(int k, int p) { return (uint32_t)(k - p) / 4; }
// one record: suffix most significant byte first, counter least significant byte first
PF_MASK_HD inline void encode_record(uint64_t kmer, uint32_t count, int k, int p, uint32_t counter_bytes, uint8_t *out) {
    const uint32_t sb = suffix_bytes(k, p);
    const uint64_t suf = kmer & ((1ull << (2 * (k - p))) - 1);
    for (uint32_t b = 0; b < sb; ++b) out[b] = (uint8_t)(suf >> (8 * (sb - 1 - b)));
    for (uint32_t b = 0; b < counter_bytes; ++b) out[sb + b] = (uint8_t)((uint64_t)count >> (8 * b));
}
// the smallest key of LUT entry e (entry 4^p: beyond every key)
PF_MASK_HD inline uint64_t lut_first_key(uint64_t e, int k, int p) { return e << (2 * (k - p)); }

inline void put_u64(std::vector<uint8_t> &v, uint64_t x) { for (int b = 0; b < 8; ++b) v.push_back((uint8_t)(x >> (8 * b))); }
inline void put_u32(std::vector<uint8_t> &v, uint32_t x) { for (int b = 0; b < 4; ++b) v.push_back((uint8_t)(x >> (8 * b))); }
// <prefix>.kmc_pre from the LUT (4^p entries; the sentinel word is written here)
inline std::vector<uint8_t> kmc1_pre_bytes(const uint64_t *lut, uint64_t n_lut, uint64_t total, int k, int p, uint32_t counter_bytes, uint64_t ci,
                                           uint64_t cx, bool both_strands) {
    std::vector<uint8_t> v;
    v.reserve(4 + (size_t)(n_lut + 1 + 7) * 8 + 8);
    v.insert(v.end(), {'K', 'M', 'C', 'P'});
    for (uint64_t e = 0; e < n_lut; ++e) put_u64(v, lut[e]);
    put_u64(v, total);
    put_u64(v, (uint64_t)k);                                  // kmer_length | mode << 32
    put_u64(v, (uint64_t)counter_bytes | ((uint64_t)p << 32));
    put_u64(v, ci | ((cx & 0xFFFFFFFFull) << 32));
    put_u64(v, total);
    put_u64(v, both_strands ? 0 : 1);
    put_u64(v, 0);
    put_u64(v, 0);                                            // its last four bytes: version 0 (KMC1)
    put_u32(v, 7 * 8);
    v.insert(v.end(), {'K', 'M', 'C', 'P'});
    return v;
}

// ---- the host's plain restatement (no device): what the kernels are held to ----
struct Stats {
    uint64_t reads = 0, bases = 0, kmers = 0, kmers_bad = 0;          // while counting
    uint64_t unique = 0, below_min = 0, above_max = 0, written = 0;   // after finish
};
typedef std::map<uint64_t, uint64_t> Table;   // sorted; 64-bit sums, so that the overflow is seen and not made

// counts read i = text[off[i], off[i] + len[i]) into the table
inline void count_reads_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, int k, bool both_strands, Table &table,
                             Stats &st) {
    const uint64_t all = (1ull << (2 * k)) - 1;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const char *s = text + off[r];
        const uint64_t n = len[r];
        st.reads += 1;
        st.bases += n;
        uint64_t fw = 0, run = 0;   // run: bases in a row ending here
        for (uint64_t j = 0; j < n; ++j) {
            const uint8_t b = (uint8_t)s[j];
            if (pf_mask::is_base(b)) { fw = ((fw << 2) | pf_mask::base_code(b)) & all; ++run; }
            else run = 0;
            if (j + 1 < (uint64_t)k) continue;
            st.kmers += 1;
            if (run >= (uint64_t)k) table[window_key(fw, k, both_strands)] += 1;
            else st.kmers_bad += 1;
        }
    }
}
// the cut-offs over the table: false when a counter passed 2^32 - 1 (OVERFLOW_TEXT)
inline bool finish_host(const Table &table, uint32_t ci, uint32_t cx, uint32_t cs, std::vector<uint64_t> &kmers, std::vector<uint32_t> &counts,
                        Stats &st) {
    kmers.clear();
    counts.clear();
    st.unique = table.size();
    st.below_min = st.above_max = 0;
    for (const auto &kv : table) {
        if (kv.second > COUNTER_MAX) return false;
        const uint32_t c = (uint32_t)kv.second;
        if (c < ci) { st.below_min += 1; continue; }
        if (c > cx) { st.above_max += 1; continue; }
        kmers.push_back(kv.first);
        counts.push_back(stored(c, cs));
    }
    st.written = kmers.size();
    return true;
}
// the two files' bytes from sorted distinct k-mers
inline void encode_kmc1_host(const uint64_t *kmers, const uint32_t *counts, uint64_t n, int k, int p, uint32_t counter_bytes, uint64_t ci, uint64_t cx,
                             bool both_strands, std::vector<uint8_t> &pre, std::vector<uint8_t> &suf) {
    const uint64_t n_lut = 1ull << (2 * p);
    std::vector<uint64_t> lut((size_t)n_lut);
    uint64_t at = 0;
    for (uint64_t e = 0; e < n_lut; ++e) {   // lower bound of the entry's first key
        while (at < n && kmers[at] < lut_first_key(e, k, p)) ++at;
        lut[(size_t)e] = at;
    }
    pre = kmc1_pre_bytes(lut.data(), n_lut, n, k, p, counter_bytes, ci, cx, both_strands);
    const uint32_t rb = suffix_bytes(k, p) + counter_bytes;
    suf.assign(8 + (size_t)n * rb, 0);
    memcpy(suf.data(), "KMCS", 4);
    for (uint64_t i = 0; i < n; ++i) encode_record(kmers[i], counts[i], k, p, counter_bytes, suf.data() + 4 + (size_t)i * rb);
    memcpy(suf.data() + 4 + (size_t)n * rb, "KMCS", 4);
}

}  // namespace pf_count
