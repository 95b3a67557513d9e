// The rule of `ploidyfrost smudge` and of `run --smudge` (K-HETPAIR) in one place, for the kernels (pf_hetpair.hip), the host layer
// (host/pf_hetpair_host.cpp) and the stand-alone test (tests/cpp/test_hetpair_rule.cpp): which k-mers pair up, the table of their two
// coverages, the summary, the text of the report, and a plain host restatement.  Integers only.
//
// Keys are pf_count_rule.hpp's: canonical min(fw, rc), first base most significant, A0 C1 G2 T3, 3 <= k <= 31, distinct.
//   set         S = the keys whose counter c has lo <= c <= hi (1 <= lo <= hi, W = hi - lo + 1 <= MAX_W).
//   neighbours  of x: the 3k values canon(x with the base at position p replaced by b), p in 0 .. k - 1, b another base.  A neighbour
//               can be x itself (ACAGT: the middle base to T gives ACTGT, whose canonical form is ACAGT), and two substitutions can
//               give the same key (AATT -> AAAT twice).  The relation is symmetric.
//   partner     of x: a neighbour y with y != x and y in S (is_partner).  degree(x) = the number of DISTINCT partner keys; all that
//               is ever asked is 0, 1 or more (Degree).
//   pair        (x, y), x < y, both in S, degree(x) == 1, degree(y) == 1, y the partner of x (pair_kept) -- then x is y's.
//   order       pairs follow the order of x in the key array: ascending for the arrays pf_count_finish and pf_kmc_decode give.
//   table       T[a - lo][b - lo] += 1 per pair, a = min(c_x, c_y), b = max(c_x, c_y), u64 cells, row-major, W * W of them.
//   statistics  kmers (all keys given), in_range (|S|), one_partner and many_partners (keys of S by degree), pairs.
//   summary     with a haploid coverage n >= 1 a pair with t = a + b belongs to smudge_of(a, b, n):
//                 p = clamp((2t + n) / (2n), 2, 16), m = clamp((2ap + t) / (2t), 1, p / 2)   (integer divisions: round half up)
//               labelled p - m letters A and m letters B; the proposed ploidy is the p of the label with the most pairs, ties to the
//               smaller p, then the smaller m.
// Everything is a count: the result depends on neither chunking nor lanes nor the order of atomics.
//
// THE REPORT is text, tab-separated, a function of the table, the statistics, k, lo, hi and n alone (report_text is the definition):
//   # ploidyfrost smudge 1
//   # k K lower LO upper HI n N            n 0: no haploid coverage was given
//   >>totals     kmers in_range one_partner many_partners pairs        one row
//   >>table      cov_a cov_b pairs                                     non-zero cells, ascending by cov_a, then cov_b
//   >>total      cov_a+cov_b pairs                                     non-zero sums, ascending
//   >>smudges    label p m pairs                                       with n only; non-zero, ascending by p, then m
//   >>proposed   p label pairs                                         with n only; one row, `0 none 0` when there is no pair
//
// PARITY UNPINNED: Smudgeplot is not part of the build.  Knowingly different: pairs are over canonical forms at any of the k
// positions, and a k-mer with two partners forms no pair at all.  The open points are is_partner, pair_kept and smudge_of.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "pf_count_rule.hpp"

#define PF_HETPAIR_HD PF_MASK_HD

namespace pf_hetpair {

constexpr int MIN_K = pf_count::MIN_K, MAX_K = pf_count::MAX_K;
constexpr uint32_t MAX_W = 4096;       // 4096 x 4096 u64 cells: 128 MiB
constexpr uint32_t MIN_P = 2, MAX_P = 16;
constexpr uint64_t NO_KEY = ~0ull;     // no key of k <= 31 has its two top bits set

struct Stats {
    uint64_t kmers = 0, in_range = 0, one_partner = 0, many_partners = 0, pairs = 0;
};

// ---- the rule's pieces, shared with the kernel ----
PF_HETPAIR_HD inline bool in_range(uint32_t c, uint32_t lo, uint32_t hi) { return c >= lo && c <= hi; }
PF_HETPAIR_HD inline uint32_t base_at(uint64_t x, int k, int p) { return (uint32_t)(x >> (2 * (k - 1 - p))) & 3u; }
PF_HETPAIR_HD inline uint64_t with_base(uint64_t x, int k, int p, uint32_t b) {
    const int s = 2 * (k - 1 - p);
    return (x & ~(3ull << s)) | ((uint64_t)b << s);
}
// substitution j of 0 .. 3k - 1, before it is made canonical: position j / 3, the base there advanced by 1 + j % 3
PF_HETPAIR_HD inline uint64_t substituted(uint64_t x, int k, int j) {
    const int p = j / 3;
    return with_base(x, k, p, (base_at(x, k, p) + 1u + (uint32_t)(j % 3)) & 3u);
}
PF_HETPAIR_HD inline uint64_t neighbour(uint64_t x, int k, int j) { return pf_count::window_key(substituted(x, k, j), k, true); }
// y, a neighbour of x, found with the counter c_y (present = it is a key at all)
PF_HETPAIR_HD inline bool is_partner(uint64_t x, uint64_t y, bool present, uint32_t c_y, uint32_t lo, uint32_t hi) {
    return y != x && present && in_range(c_y, lo, hi);
}
// the distinct partners of one key as far as anybody asks: none, one (and which), more
struct Degree {
    uint64_t first = NO_KEY;
    uint32_t cov = 0;     // the first partner's counter
    uint32_t many = 0;
    PF_HETPAIR_HD inline void add(uint64_t y, uint32_t c_y) {
        if (first == NO_KEY) { first = y; cov = c_y; }
        else if (first != y) many = 1;
    }
    PF_HETPAIR_HD inline void merge(const Degree &o) {
        if (o.first == NO_KEY) return;
        many |= o.many;
        add(o.first, o.cov);
    }
    PF_HETPAIR_HD inline uint32_t degree() const { return first == NO_KEY ? 0u : many ? 2u : 1u; }   // 2: two or more
};
PF_HETPAIR_HD inline bool pair_kept(uint64_t x, uint32_t degree_x, uint64_t y, uint32_t degree_y) {
    return x < y && degree_x == 1 && degree_y == 1;
}
PF_HETPAIR_HD inline uint64_t table_cell(uint32_t c_x, uint32_t c_y, uint32_t lo, uint32_t W) {
    const uint32_t a = c_x < c_y ? c_x : c_y, b = c_x < c_y ? c_y : c_x;
    return (uint64_t)(a - lo) * W + (b - lo);
}
struct Smudge {
    uint32_t p, m;
};
PF_HETPAIR_HD inline Smudge smudge_of(uint64_t a, uint64_t b, uint64_t n) {   // 1 <= a <= b, n >= 1
    const uint64_t t = a + b;
    uint64_t p = (2 * t + n) / (2 * n);
    p = p < MIN_P ? MIN_P : p > MAX_P ? MAX_P : p;
    uint64_t m = (2 * a * p + t) / (2 * t);
    m = m < 1 ? 1 : m > p / 2 ? p / 2 : m;
    return Smudge{(uint32_t)p, (uint32_t)m};
}
inline std::string smudge_label(Smudge s) { return std::string(s.p - s.m, 'A') + std::string(s.m, 'B'); }

enum ArgClause { ARG_OK = 0, ARG_LO_ZERO, ARG_LO_ABOVE_HI, ARG_TOO_WIDE, ARG_K };
inline int arg_clause(int64_t k, uint64_t lo, uint64_t hi) {
    if (k < MIN_K || k > MAX_K) return ARG_K;
    if (lo < 1) return ARG_LO_ZERO;
    if (lo > hi) return ARG_LO_ABOVE_HI;
    if (hi - lo + 1 > MAX_W) return ARG_TOO_WIDE;
    return ARG_OK;
}
inline const char *arg_text(int c) {
    switch (c) {
        case ARG_LO_ZERO: return "the lower bound is below 1 (a k-mer that never occurs has no coverage)";
        case ARG_LO_ABOVE_HI: return "the lower bound is above the upper bound";
        case ARG_TOO_WIDE: return "upper - lower + 1 is above 4096 (the table of 4096 x 4096 cells is 128 MiB)";
        case ARG_K: return "k goes from 3 to 31 (a k-mer is one 64-bit word)";
        default: return "no refusal";
    }
}

inline std::string kmer_text(uint64_t x, int k) {
    std::string s((size_t)k, 'A');
    for (int p = 0; p < k; ++p) s[(size_t)p] = "ACGT"[base_at(x, k, p)];
    return s;
}

// ---- the host's plain restatement (no device): what the kernels are held to ----
struct Pairs {
    std::vector<uint64_t> x, y;
    std::vector<uint32_t> cov_x, cov_y;
};
// table: W * W cells, zeroed here; may be null
inline void hetpairs_host(const uint64_t *kmers, const uint32_t *counts, uint64_t n, int k, uint32_t lo, uint32_t hi, uint64_t *table, Pairs &pairs,
                          Stats &st) {
    const uint32_t W = hi - lo + 1;
    st = Stats();
    pairs = Pairs();
    if (table)
        for (uint64_t i = 0; i < (uint64_t)W * W; ++i) table[i] = 0;
    std::unordered_map<uint64_t, uint32_t> count_of;
    count_of.reserve((size_t)n * 2);
    for (uint64_t i = 0; i < n; ++i) count_of.emplace(kmers[i], counts[i]);
    auto degree_of = [&](uint64_t x) {
        Degree d;
        for (int j = 0; j < 3 * k; ++j) {
            const uint64_t y = neighbour(x, k, j);
            const auto it = count_of.find(y);
            const bool present = it != count_of.end();
            if (is_partner(x, y, present, present ? it->second : 0u, lo, hi)) d.add(y, it->second);
        }
        return d;
    };
    st.kmers = n;
    for (uint64_t i = 0; i < n; ++i) {
        if (!in_range(counts[i], lo, hi)) continue;
        st.in_range += 1;
        const uint64_t x = kmers[i];
        const Degree dx = degree_of(x);
        if (dx.degree() == 1) st.one_partner += 1;
        if (dx.degree() > 1) st.many_partners += 1;
        if (dx.degree() != 1 || !(x < dx.first)) continue;
        if (!pair_kept(x, 1, dx.first, degree_of(dx.first).degree())) continue;
        st.pairs += 1;
        pairs.x.push_back(x);
        pairs.y.push_back(dx.first);
        pairs.cov_x.push_back(counts[i]);
        pairs.cov_y.push_back(dx.cov);
        if (table) table[table_cell(counts[i], dx.cov, lo, W)] += 1;
    }
}

// ---- the summary and the report ----
struct Summary {
    uint64_t pairs[MAX_P + 1][MAX_P / 2 + 1] = {};   // [p][m]
    Smudge best = {0, 0};                            // p == 0: there is no pair
    uint64_t best_pairs = 0, all_pairs = 0;
};
inline Summary summarize(const uint64_t *table, uint32_t lo, uint32_t hi, uint64_t n) {
    Summary s;
    const uint32_t W = hi - lo + 1;
    for (uint32_t i = 0; i < W; ++i)
        for (uint32_t j = i; j < W; ++j) {
            const uint64_t c = table[(uint64_t)i * W + j];
            if (!c) continue;
            const Smudge g = smudge_of((uint64_t)lo + i, (uint64_t)lo + j, n);
            s.pairs[g.p][g.m] += c;
            s.all_pairs += c;
        }
    for (uint32_t p = MIN_P; p <= MAX_P; ++p)   // ascending p, then m: a later label wins only with more pairs
        for (uint32_t m = 1; m <= p / 2; ++m)
            if (s.pairs[p][m] > s.best_pairs) { s.best_pairs = s.pairs[p][m]; s.best = Smudge{p, m}; }
    return s;
}
// the second stderr line of the command; empty without a pair
inline std::string proposed_text(const Summary &s) {
    if (!s.best.p) return "smudge: proposed ploidy 0 (none, 0 of 0 pairs)";
    return "smudge: proposed ploidy " + std::to_string(s.best.p) + " (" + smudge_label(s.best) + ", " + std::to_string(s.best_pairs) + " of " +
           std::to_string(s.all_pairs) + " pairs)";
}
inline std::string stats_text(const Stats &st) {
    return "smudge: kmers " + std::to_string(st.kmers) + " in_range " + std::to_string(st.in_range) + " one_partner " + std::to_string(st.one_partner) +
           " many_partners " + std::to_string(st.many_partners) + " pairs " + std::to_string(st.pairs);
}
inline std::string report_text(const uint64_t *table, const Stats &st, int k, uint32_t lo, uint32_t hi, uint64_t n) {
    const uint32_t W = hi - lo + 1;
    auto num = [](uint64_t v) { return std::to_string(v); };
    std::string o = "# ploidyfrost smudge 1\n";
    o += "# k " + num((uint64_t)k) + " lower " + num(lo) + " upper " + num(hi) + " n " + num(n) + "\n";
    o += ">>totals\nkmers\tin_range\tone_partner\tmany_partners\tpairs\n";
    o += num(st.kmers) + "\t" + num(st.in_range) + "\t" + num(st.one_partner) + "\t" + num(st.many_partners) + "\t" + num(st.pairs) + "\n";
    o += ">>table\ncov_a\tcov_b\tpairs\n";
    std::map<uint64_t, uint64_t> total;
    for (uint32_t i = 0; i < W; ++i)
        for (uint32_t j = i; j < W; ++j) {
            const uint64_t c = table[(uint64_t)i * W + j];
            if (!c) continue;
            o += num((uint64_t)lo + i) + "\t" + num((uint64_t)lo + j) + "\t" + num(c) + "\n";
            total[(uint64_t)lo + i + lo + j] += c;
        }
    o += ">>total\ncov_a+cov_b\tpairs\n";
    for (const auto &kv : total) o += num(kv.first) + "\t" + num(kv.second) + "\n";
    if (n) {
        const Summary s = summarize(table, lo, hi, n);
        o += ">>smudges\nlabel\tp\tm\tpairs\n";
        for (uint32_t p = MIN_P; p <= MAX_P; ++p)
            for (uint32_t m = 1; m <= p / 2; ++m)
                if (s.pairs[p][m]) o += smudge_label(Smudge{p, m}) + "\t" + num(p) + "\t" + num(m) + "\t" + num(s.pairs[p][m]) + "\n";
        o += ">>proposed\np\tlabel\tpairs\n";
        o += s.best.p ? num(s.best.p) + "\t" + smudge_label(s.best) + "\t" + num(s.best_pairs) + "\n" : std::string("0\tnone\t0\n");
    }
    return o;
}
// one line of the pairs file
inline std::string pair_line(uint64_t x, uint64_t y, uint32_t c_x, uint32_t c_y, int k) {
    return kmer_text(x, k) + "\t" + kmer_text(y, k) + "\t" + std::to_string(c_x) + "\t" + std::to_string(c_y) + "\n";
}

}  // namespace pf_hetpair
