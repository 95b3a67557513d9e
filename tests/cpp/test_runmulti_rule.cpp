// pf_runmulti_rule.hpp alone (no device): the pairwise rounds of K-UNION against std::set, exhaustively over small sets and at random
// over larger ones; the refusal texts.  Built with -fsanitize=address,undefined by tests/test_run_multi_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "pf_runmulti_rule.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

typedef std::vector<uint64_t> Set;

static Set want_of(const std::vector<Set> &sets) {
    std::set<uint64_t> all;
    for (const Set &s : sets) all.insert(s.begin(), s.end());
    return Set(all.begin(), all.end());
}

int main() {
    // every pair of subsets of {0 .. 4}, and with a third set {1, 3}
    for (unsigned a = 0; a < 32; ++a)
        for (unsigned b = 0; b < 32; ++b) {
            Set A, B;
            for (uint64_t i = 0; i < 5; ++i) { if (a >> i & 1) A.push_back(i); if (b >> i & 1) B.push_back(i); }
            CHECK(pf_runmulti::union_pair_host(A, B) == want_of({A, B}));
            CHECK(pf_runmulti::union_host({A, B, Set{1, 3}}) == want_of({A, B, Set{1, 3}}));
        }
    // 1 .. 9 random sets: the odd carry at 3, 5, 7, 9, four rounds at 9; keys with bit 61 set
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int n_sets = 1; n_sets <= 9; ++n_sets) {
        std::vector<Set> sets((size_t)n_sets);
        for (Set &s : sets) {
            std::set<uint64_t> keys;
            const int n = (int)(next() % 300);
            for (int i = 0; i < n; ++i) keys.insert(next() % 500 | (next() % 4 == 0 ? 1ull << 61 : 0ull));
            s.assign(keys.begin(), keys.end());
            CHECK(pf_runmulti::set_refusal(s.data(), s.size(), 0).empty());
        }
        CHECK(pf_runmulti::union_host(sets) == want_of(sets));
    }
    CHECK(pf_runmulti::union_host({}).empty());
    CHECK(pf_runmulti::union_host({Set{}, Set{}}).empty());
    const Set unsorted{4, 3, 8}, repeat{4, 4, 8};
    CHECK(pf_runmulti::set_refusal(unsorted.data(), 3, 1) == pf_runmulti::unsorted_text(1));
    CHECK(pf_runmulti::set_refusal(repeat.data(), 3, 2) == pf_runmulti::repeat_text(2));
    CHECK(pf_runmulti::UNION_TILE == 256 * pf_runmulti::UNION_ITEMS);
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
