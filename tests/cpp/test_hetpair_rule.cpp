// Stand-alone check of ploidyfrost_amd/csrc/pf_hetpair_rule.hpp: the shared header alone, plain host C++, built with
// -fsanitize=address,undefined by tests/test_hetpair_cpu.py.  Keys, counters and the table are heap blocks of exactly the size the rule
// is given (a table of W * W cells, not one more), so a read or a write one element beyond them is reported.  The restatement of the
// header against a second, deliberately naive one (a sorted map, all neighbours compared as strings of bases); the facts the rule is
// built on at k = 4 and k = 5; the four labels worked by hand; the tie-break; the report of an empty and a small table.
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "pf_hetpair_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

template <typename T>
struct Exact {   // a heap copy of exactly n elements (at least one block, so that the pointer is never null)
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Exact(const std::vector<T> &v) : p(new T[v.size() ? v.size() : 1]), n(v.size()) { for (size_t i = 0; i < n; ++i) p[i] = v[i]; }
    explicit Exact(size_t len) : p(new T[len ? len : 1]), n(len) {}
    T *get() const { return p.get(); }
};

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

// ---- the naive restatement: strings of bases ----
static std::string rc_text(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
static std::string canon_text(const std::string &s) { const std::string r = rc_text(s); return r < s ? r : s; }
static uint64_t enc(const std::string &s) {
    uint64_t x = 0;
    for (char c : s) x = x * 4 + (c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return x;
}
static std::set<std::string> partners_text(const std::string &x, const std::map<std::string, uint32_t> &count_of, uint32_t lo, uint32_t hi) {
    std::set<std::string> out;
    for (size_t p = 0; p < x.size(); ++p)
        for (char b : std::string("ACGT")) {
            if (b == x[p]) continue;
            std::string y = x;
            y[p] = b;
            y = canon_text(y);
            const auto it = count_of.find(y);
            if (y != x && it != count_of.end() && it->second >= lo && it->second <= hi) out.insert(y);
        }
    return out;
}

static void check_case(const std::map<std::string, uint32_t> &count_of, int k, uint32_t lo, uint32_t hi) {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> counts;
    for (const auto &kv : count_of) { keys.push_back(enc(kv.first)); counts.push_back(kv.second); }   // (text order is key order)
    const uint32_t W = hi - lo + 1;
    Exact<uint64_t> ek(keys), table((size_t)W * W);
    Exact<uint32_t> ec(counts);
    pf_hetpair::Pairs pairs;
    pf_hetpair::Stats st;
    pf_hetpair::hetpairs_host(ek.get(), ec.get(), keys.size(), k, lo, hi, table.get(), pairs, st);
    // the naive one
    std::vector<uint64_t> want((size_t)W * W, 0);
    uint64_t in_range = 0, one = 0, many = 0, n_pairs = 0;
    for (const auto &kv : count_of) {
        if (kv.second < lo || kv.second > hi) continue;
        ++in_range;
        const std::set<std::string> px = partners_text(kv.first, count_of, lo, hi);
        one += px.size() == 1;
        many += px.size() > 1;
        if (px.size() != 1 || !(kv.first < *px.begin())) continue;
        const std::string &y = *px.begin();
        const std::set<std::string> py = partners_text(y, count_of, lo, hi);
        if (py.size() != 1) continue;
        CHECK(*py.begin() == kv.first);
        const uint32_t cx = kv.second, cy = count_of.at(y);
        CHECK(n_pairs < pairs.x.size() && pairs.x[n_pairs] == enc(kv.first) && pairs.y[n_pairs] == enc(y) && pairs.cov_x[n_pairs] == cx && pairs.cov_y[n_pairs] == cy);
        want[(size_t)(std::min(cx, cy) - lo) * W + (std::max(cx, cy) - lo)] += 1;
        ++n_pairs;
    }
    CHECK(st.kmers == keys.size() && st.in_range == in_range && st.one_partner == one && st.many_partners == many && st.pairs == n_pairs);
    CHECK(pairs.x.size() == n_pairs && pairs.y.size() == n_pairs && pairs.cov_x.size() == n_pairs && pairs.cov_y.size() == n_pairs);
    for (size_t i = 0; i < want.size(); ++i) CHECK(table.get()[i] == want[i]);
    // without a table, and the report from exact-size blocks
    pf_hetpair::Pairs p2;
    pf_hetpair::Stats s2;
    pf_hetpair::hetpairs_host(ek.get(), ec.get(), keys.size(), k, lo, hi, nullptr, p2, s2);
    CHECK(s2.pairs == st.pairs && p2.x == pairs.x);
    const std::string rep = pf_hetpair::report_text(table.get(), st, k, lo, hi, 20);
    CHECK(rep.find(">>proposed\n") != std::string::npos);
}

static std::string random_text(size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back("ACGT"[rnd() % 4]);
    return s;
}
static void count_text(const std::string &s, int k, uint32_t depth, std::map<std::string, uint32_t> &count_of) {
    for (size_t i = 0; i + (size_t)k <= s.size(); ++i) count_of[canon_text(s.substr(i, (size_t)k))] += depth;
}

int main() {
    // ---- keys and neighbours ----
    for (int k : {3, 4, 5, 17, 31}) {
        for (int t = 0; t < 200; ++t) {
            const std::string s = random_text((size_t)k);
            const uint64_t x = enc(s);
            CHECK(pf_hetpair::kmer_text(x, k) == s);
            CHECK(pf_count::window_key(x, k, true) == enc(canon_text(s)));
            std::set<uint64_t> seen;
            for (int j = 0; j < 3 * k; ++j) {
                const uint64_t y = pf_hetpair::substituted(x, k, j);
                CHECK(y != x && seen.insert(y).second);   // 3k different substitutions, none of them x
                int diff = 0;
                const std::string ys = pf_hetpair::kmer_text(y, k);
                for (int p = 0; p < k; ++p) diff += ys[(size_t)p] != s[(size_t)p];
                CHECK(diff == 1 && ys[(size_t)(j / 3)] != s[(size_t)(j / 3)]);
                CHECK(pf_hetpair::neighbour(x, k, j) == enc(canon_text(ys)));
            }
        }
    }
    {   // 32 of the 512 canonical 5-mers are their own neighbour; 96 ordered pairs of 4-mers are neighbours twice
        int self = 0, doubled = 0;
        for (uint64_t x = 0; x < 1024; ++x) {
            if (pf_count::window_key(x, 5, true) != x) continue;
            bool s = false;
            for (int j = 0; j < 15; ++j) s |= pf_hetpair::neighbour(x, 5, j) == x;
            self += s;
        }
        for (uint64_t x = 0; x < 256; ++x) {
            if (pf_count::window_key(x, 4, true) != x) continue;
            std::map<uint64_t, int> times;
            for (int j = 0; j < 12; ++j) times[pf_hetpair::neighbour(x, 4, j)] += 1;
            for (const auto &kv : times) doubled += kv.first != x && kv.second > 1;
        }
        CHECK(self == 32 && doubled == 96);
        CHECK(pf_hetpair::neighbour(enc("ACAGT"), 5, 3 * 2 + 2) == enc("ACAGT"));   // the middle base to T
    }
    // ---- Degree ----
    {
        pf_hetpair::Degree a, b, c;
        CHECK(a.degree() == 0);
        a.add(5, 20);
        a.add(5, 20);   // the same partner twice is one partner
        CHECK(a.degree() == 1 && a.first == 5 && a.cov == 20);
        b.add(5, 20);
        a.merge(b);
        a.merge(c);
        CHECK(a.degree() == 1);
        c.add(6, 21);
        a.merge(c);
        CHECK(a.degree() == 2);
        pf_hetpair::Degree e;
        e.merge(c);
        CHECK(e.degree() == 1 && e.first == 6 && e.cov == 21);
    }
    // ---- the restatement against the naive one ----
    {   // every canonical 5-mer, counters 1 .. 12, several bounds
        std::map<std::string, uint32_t> all5;
        for (uint64_t x = 0; x < 1024; ++x)
            if (pf_count::window_key(x, 5, true) == x) all5[pf_hetpair::kmer_text(x, 5)] = 1 + rnd() % 12;
        check_case(all5, 5, 1, 12);
        check_case(all5, 5, 3, 4);
        check_case(all5, 5, 7, 7);
    }
    for (int round = 0; round < 6; ++round) {   // sparse random subsets of the 4-mers: doubled neighbours with degree 1
        std::map<std::string, uint32_t> some;
        for (uint64_t x = 0; x < 256; ++x)
            if (pf_count::window_key(x, 4, true) == x && rnd() % 8 == 0) some[pf_hetpair::kmer_text(x, 4)] = 1 + rnd() % 6;
        check_case(some, 4, 2, 5);
    }
    for (int k : {17, 18, 25, 31}) {   // two haplotypes with substitutions, a triallelic site, two substitutions close together
        const std::string a = random_text(400);
        std::string b = a, c = a;
        for (size_t p : {60u, 150u, 158u, 300u}) b[p] = b[p] == 'A' ? 'C' : 'A';
        c[300] = c[300] == 'G' ? 'T' : 'G';
        std::map<std::string, uint32_t> count_of;
        count_text(a, k, 20, count_of);
        count_text(b, k, 20, count_of);
        count_text(c, k, 19, count_of);
        check_case(count_of, k, 10, 100);
        check_case(count_of, k, 20, 39);   // the shared k-mers (59) fall out of range
        check_case(count_of, k, 19, 19);   // W = 1
    }
    {   // no keys at all
        check_case(std::map<std::string, uint32_t>(), 25, 1, 4);
    }
    // ---- the summary ----
    {
        struct { uint64_t a, b; uint32_t p, m; const char *label; } hand[] = {{20, 20, 2, 1, "AB"}, {20, 40, 3, 1, "AAB"}, {20, 60, 4, 1, "AAAB"}, {40, 40, 4, 2, "AABB"}};
        for (const auto &h : hand) {
            const pf_hetpair::Smudge s = pf_hetpair::smudge_of(h.a, h.b, 20);
            CHECK(s.p == h.p && s.m == h.m && pf_hetpair::smudge_label(s) == h.label);
        }
        for (uint64_t a = 1; a < 50; ++a)
            for (uint64_t b = a; b < 4000; b += 37) {
                const pf_hetpair::Smudge s = pf_hetpair::smudge_of(a, b, 1 + (a * b) % 40);
                CHECK(s.p >= 2 && s.p <= 16 && s.m >= 1 && s.m <= s.p / 2);
            }
        const uint32_t lo = 10, hi = 70, W = hi - lo + 1;
        Exact<uint64_t> t((size_t)W * W);
        for (size_t i = 0; i < (size_t)W * W; ++i) t.get()[i] = 0;
        pf_hetpair::Stats st;
        CHECK(pf_hetpair::summarize(t.get(), lo, hi, 20).best.p == 0);
        CHECK(pf_hetpair::report_text(t.get(), st, 21, lo, hi, 20).find(">>proposed\np\tlabel\tpairs\n0\tnone\t0\n") != std::string::npos);
        CHECK(pf_hetpair::report_text(t.get(), st, 21, lo, hi, 0).find(">>smudges") == std::string::npos);
        auto cell = [&](uint32_t a, uint32_t b) -> uint64_t & { return t.get()[(size_t)(a - lo) * W + (b - lo)]; };
        cell(20, 20) = 5; cell(20, 40) = 5; cell(40, 40) = 5;   // ties go to the smaller p
        pf_hetpair::Summary s = pf_hetpair::summarize(t.get(), lo, hi, 20);
        CHECK(s.best.p == 2 && s.best.m == 1 && s.best_pairs == 5 && s.all_pairs == 15);
        cell(20, 20) = 4; cell(20, 40) = 0; cell(20, 60) = 5;   // ... then to the smaller m
        s = pf_hetpair::summarize(t.get(), lo, hi, 20);
        CHECK(s.best.p == 4 && s.best.m == 1 && pf_hetpair::proposed_text(s) == "smudge: proposed ploidy 4 (AAAB, 5 of 14 pairs)");
        cell(70, 70) = 9;   // the last cell of the table
        const std::string rep = pf_hetpair::report_text(t.get(), st, 21, lo, hi, 20);
        CHECK(rep.find("\n70\t70\t9\n>>total\n") != std::string::npos && rep.find("\n140\t9\n>>smudges\n") != std::string::npos);
    }
    // ---- the refusals ----
    CHECK(pf_hetpair::arg_clause(25, 0, 5) == pf_hetpair::ARG_LO_ZERO && pf_hetpair::arg_clause(25, 6, 5) == pf_hetpair::ARG_LO_ABOVE_HI);
    CHECK(pf_hetpair::arg_clause(25, 1, 4096) == pf_hetpair::ARG_OK && pf_hetpair::arg_clause(25, 1, 4097) == pf_hetpair::ARG_TOO_WIDE);
    CHECK(pf_hetpair::arg_clause(2, 1, 5) == pf_hetpair::ARG_K && pf_hetpair::arg_clause(32, 1, 5) == pf_hetpair::ARG_K);
    CHECK(pf_hetpair::arg_clause(31, 0xFFFFFFFFull, 0xFFFFFFFFull) == pf_hetpair::ARG_OK);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
