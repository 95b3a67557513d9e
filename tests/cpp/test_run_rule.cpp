// The shared rule header of `ploidyfrost run` (csrc/pf_run_rule.hpp) on its own, with plain g++ (and the sanitizers): which windows
// survive the masking, against the composition it replaces -- pf_mask's byte rule applied to the text, then pf_count's rule on the
// masked text.  k = 3, every read length 0 .. 9, every pattern of per-window counters in {0, low, up + 1}, every placement of one N
// (and none); the same for two reads that touch without a gap; the funnel over the bad bitmap against the definition.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pf_run_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("line %d: %s\n", __LINE__, #cond);                 \
            ++fails;                                                  \
        }                                                             \
    } while (0)

constexpr int K = 3;
constexpr uint32_t LOW = 4, UP = 9;
static const uint32_t kValues[3] = {0, LOW, UP + 1};
static const char *kBases = "ACGTTGCAAC";   // (not periodic: neighbouring windows differ, some share a canonical form)

// mask every read with pf_mask::mask_read, then count the masked text with pf_count::count_reads_host
static pf_count::Table composition(const std::string &text, const std::vector<uint64_t> &off, const std::vector<uint32_t> &len,
                                   const std::vector<uint32_t> &counters, uint32_t low, uint32_t up) {
    std::string masked = text;
    for (size_t r = 0; r < off.size(); ++r)
        (void)pf_mask::mask_read(text.data() + off[r], len[r], K, counters.data() + off[r], low, up, &masked[0] + off[r]);
    pf_count::Table t;
    pf_count::Stats st;
    pf_count::count_reads_host(masked.data(), off.data(), len.data(), off.size(), K, true, t, st);
    return t;
}

static void check_case(const std::string &text, const std::vector<uint64_t> &off, const std::vector<uint32_t> &len,
                       const std::vector<uint32_t> &counters, uint32_t low, uint32_t up) {
    pf_count::Table got;
    pf_run::Stats st;
    pf_run::count_masked_host(text.data(), off.data(), len.data(), off.size(), K, counters.data(), low, up, got, st);
    const pf_count::Table want = composition(text, off, len, counters, low, up);
    CHECK(got == want);
    uint64_t kept = 0;
    for (const auto &kv : got) kept += kv.second;
    CHECK(kept == st.kmers_kept && st.kmers_kept + st.kmers_invalid <= st.kmers && st.reads == off.size());
}

// the counter of a window that holds the N is 0, as GetCountersForRead gives it; every other window takes the pattern's value
static void one_read() {
    for (uint32_t n = 0; n <= 9; ++n) {
        const uint32_t windows = n >= (uint32_t)K ? n - K + 1 : 0;
        uint64_t patterns = 1;
        for (uint32_t i = 0; i < windows; ++i) patterns *= 3;
        for (int n_at = -1; n_at < (int)n; ++n_at) {
            std::string text(kBases, n);
            if (n_at >= 0) text[(size_t)n_at] = 'N';
            for (uint64_t pat = 0; pat < patterns; ++pat) {
                std::vector<uint32_t> c(n + 1, 0);
                uint64_t x = pat;
                for (uint32_t i = 0; i < windows; ++i, x /= 3) {
                    const bool holds_n = n_at >= (int)i && n_at < (int)i + K;
                    c[i] = holds_n ? 0 : kValues[x % 3];
                }
                for (const auto &lu : {std::pair<uint32_t, uint32_t>{LOW, UP}, {0u, UP}, {0u, 0xFFFFFFFFu}, {LOW, 0xFFFFFFFFu}})
                    check_case(text, {0}, {n}, c, lu.first, lu.second);
            }
        }
    }
}

// two reads that touch without a gap: a bad window at the end of the first must not reach into the second, and the reverse
static void two_reads_touching() {
    for (uint32_t n0 = 0; n0 <= 5; ++n0)
        for (uint32_t n1 = 0; n1 <= 5; ++n1) {
            const uint32_t w0 = n0 >= (uint32_t)K ? n0 - K + 1 : 0, w1 = n1 >= (uint32_t)K ? n1 - K + 1 : 0;
            uint64_t patterns = 1;
            for (uint32_t i = 0; i < w0 + w1; ++i) patterns *= 3;
            for (int n_at = -1; n_at < (int)(n0 + n1); ++n_at) {
                std::string text(kBases, n0 + n1);
                if (n_at >= 0) text[(size_t)n_at] = 'N';
                for (uint64_t pat = 0; pat < patterns; ++pat) {
                    std::vector<uint32_t> c(n0 + n1 + 1, 77);   // (positions that are no window start are never read)
                    uint64_t x = pat;
                    for (uint32_t i = 0; i < w0 + w1; ++i, x /= 3) {
                        const uint32_t p = i < w0 ? i : n0 + (i - w0);
                        const bool holds_n = n_at >= (int)p && n_at < (int)p + K;
                        c[p] = holds_n ? 0 : kValues[x % 3];
                    }
                    check_case(text, {0, n0}, {n0, n1}, c, LOW, UP);
                    check_case(text, {0, n0}, {n0, n1}, c, 0, UP);
                }
            }
        }
}

// the funnel: clear_of_bad over three words against "no set bit in [p - k + 1, p + k - 1]", for one bad bit at every distance
static void funnel() {
    for (int k : {3, 25, 31})
        for (int p = 64; p < 128; ++p)          // p in the middle word of a three-word bitmap
            for (int q = p - 40; q <= p + 40; ++q) {
                uint64_t w[3] = {0, 0, 0};
                w[q >> 6] |= 1ull << (q & 63);
                const bool want = !(q >= p - k + 1 && q <= p + k - 1);
                CHECK(pf_run::clear_of_bad(w[0], w[1], w[2], p & 63, k) == want);
            }
    CHECK(pf_run::clear_of_bad(0, 0, 0, 0, 31) && pf_run::clear_of_bad(0, 0, 0, 63, 31));
    CHECK(!pf_run::survives(false, true, 0, 0, 0, 5, 3) && !pf_run::survives(true, false, 0, 0, 0, 5, 3) && pf_run::survives(true, true, 0, 0, 0, 5, 3));
}

int main() {
    one_read();
    two_reads_touching();
    funnel();
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
