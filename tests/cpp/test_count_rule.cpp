// The shared rule header of `ploidyfrost count` (csrc/pf_count_rule.hpp) on its own, with plain g++ (and the sanitizers): keys against
// a definition written out base by base, the counting of windows against a quadratic recount, the cut-offs and counter_bytes at their
// boundaries, and the KMC1 bytes decoded again by the layout's own words.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pf_count_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("line %d: %s\n", __LINE__, #cond);                 \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint64_t rng_state = 12345;
static uint64_t rnd() {   // splitmix64
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the definition: base by base over the text of the window
static bool key_by_definition(const std::string &w, bool both, uint64_t &key) {
    uint64_t fw = 0, rc = 0;
    const size_t k = w.size();
    for (size_t j = 0; j < k; ++j) {
        const char c = (char)(w[j] & 0xDF);
        const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
        if (code < 0) return false;
        fw |= (uint64_t)code << (2 * (k - 1 - j));
        rc |= (uint64_t)(3 - code) << (2 * j);
    }
    key = both ? (fw < rc ? fw : rc) : fw;
    return true;
}

static void keys() {
    for (int k = pf_count::MIN_K; k <= pf_count::MAX_K; ++k) {
        for (int t = 0; t < 50; ++t) {
            std::string w(k, 'A');
            for (int j = 0; j < k; ++j) w[j] = "ACGTacgt"[rnd() % 8];
            uint64_t fw = 0, want = 0;
            for (int j = 0; j < k; ++j) fw = (fw << 2) | pf_mask::base_code((uint8_t)w[j]);
            CHECK(key_by_definition(w, true, want) && pf_count::window_key(fw, k, true) == want);
            CHECK(key_by_definition(w, false, want) && pf_count::window_key(fw, k, false) == want && want == fw);
            CHECK(pf_count::rev_comp(pf_count::rev_comp(fw, k), k) == fw);
            CHECK(pf_count::window_key(fw, k, true) != pf_count::EMPTY_KEY);
        }
    }
    CHECK(pf_count::rev_comp(0b000110011011ull, 6) == 0b000110011011ull);   // ACGCGT is its own reverse complement
}

static void counting() {
    for (int round = 0; round < 40; ++round) {
        const int k = 3 + (int)(rnd() % 6);
        const bool both = round & 1;
        std::string text;
        std::vector<uint64_t> off;
        std::vector<uint32_t> len;
        const int n_reads = 1 + (int)(rnd() % 6);
        for (int r = 0; r < n_reads; ++r) {
            const uint32_t n = (uint32_t)(rnd() % 40);
            off.push_back(text.size());
            len.push_back(n);
            for (uint32_t j = 0; j < n; ++j) text.push_back("ACGTacgtACGTACGN"[rnd() % 16]);
            if (rnd() & 1) text += "\n+\n";   // bytes between the reads are nobody's
        }
        pf_count::Table table, want;
        pf_count::Stats st;
        pf_count::count_reads_host(text.data(), off.data(), len.data(), off.size(), k, both, table, st);
        uint64_t windows = 0, bad = 0, bases = 0;
        for (size_t r = 0; r < off.size(); ++r) {
            bases += len[r];
            for (uint64_t i = 0; i + k <= len[r]; ++i) {
                uint64_t key = 0;
                ++windows;
                if (key_by_definition(text.substr(off[r] + i, k), both, key)) want[key] += 1;
                else ++bad;
            }
        }
        CHECK(table == want);
        CHECK(st.reads == off.size() && st.bases == bases && st.kmers == windows && st.kmers_bad == bad);
        // cut-offs
        const uint32_t ci = 1 + (uint32_t)(rnd() % 3), cx = ci + (uint32_t)(rnd() % 3), cs = 1 + (uint32_t)(rnd() % 4);
        std::vector<uint64_t> km;
        std::vector<uint32_t> ct;
        CHECK(pf_count::finish_host(table, ci, cx, cs, km, ct, st));
        uint64_t below = 0, above = 0, at = 0;
        for (const auto &kv : want) {
            if (kv.second < ci) { ++below; continue; }
            if (kv.second > cx) { ++above; continue; }
            CHECK(at < km.size() && km[at] == kv.first && ct[at] == (kv.second < cs ? kv.second : cs));
            ++at;
        }
        CHECK(at == km.size() && st.unique == want.size() && st.below_min == below && st.above_max == above && st.written == at);
    }
    pf_count::Table big;
    big[5] = 0x100000000ull;
    pf_count::Stats st;
    std::vector<uint64_t> km;
    std::vector<uint32_t> ct;
    CHECK(!pf_count::finish_host(big, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, km, ct, st));   // never wraps silently
    big[5] = 0xFFFFFFFFull;
    CHECK(pf_count::finish_host(big, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, km, ct, st) && ct.size() == 1 && ct[0] == 0xFFFFFFFFu);
}

static void cutoffs() {
    using namespace pf_count;
    CHECK(cut_clause(2, 1000000000, 255) == CUT_OK && cut_clause(1, 1, 1) == CUT_OK && cut_clause(COUNTER_MAX, COUNTER_MAX, COUNTER_MAX) == CUT_OK);
    CHECK(cut_clause(0, 5, 5) == CUT_CI_ZERO && cut_clause(6, 5, 5) == CUT_CI_ABOVE_CX && cut_clause(1, 5, 0) == CUT_CS_ZERO);
    CHECK(cut_clause(COUNTER_MAX + 1, COUNTER_MAX + 1, 5) == CUT_TOO_LARGE && cut_clause(1, COUNTER_MAX + 1, 5) == CUT_TOO_LARGE && cut_clause(1, 5, COUNTER_MAX + 1) == CUT_TOO_LARGE);
    CHECK(!k_ok(2) && k_ok(3) && k_ok(31) && !k_ok(32));
    CHECK(counter_bytes(DEFAULT_CX, 255) == 1 && counter_bytes(DEFAULT_CX, 256) == 2 && counter_bytes(DEFAULT_CX, 65535) == 2);
    CHECK(counter_bytes(DEFAULT_CX, 65536) == 3 && counter_bytes(DEFAULT_CX, (1u << 24) - 1) == 3 && counter_bytes(DEFAULT_CX, 1u << 24) == 4);
    CHECK(counter_bytes(200, 10000) == 1 && counter_bytes(COUNTER_MAX, COUNTER_MAX) == 4);
    for (int c = CUT_CI_ZERO; c <= CUT_K_LAYOUT; ++c) CHECK(std::string(cut_text(c)) != cut_text(CUT_OK));
    for (int k = 5; k <= MAX_K; ++k) {
        const int p = lut_prefix_len(k);
        CHECK(p >= 1 && p < k && (k - p) % 4 == 0);
    }
    CHECK(lut_prefix_len(3) == 0 && lut_prefix_len(4) == 0);   // counted, not written
    CHECK(lut_prefix_len(25) == 5 && lut_prefix_len(31) == 7 && lut_prefix_len(5) == 1 && lut_prefix_len(6) == 2);
}

static uint64_t word_at(const std::vector<uint8_t> &v, size_t at, int bytes) {
    uint64_t x = 0;
    for (int b = 0; b < bytes; ++b) x |= (uint64_t)v[at + b] << (8 * b);
    return x;
}

static void layout() {
    for (int k : {5, 6, 11, 25, 31}) {
        for (uint32_t cb_cs : {255u, 256u, 70000u, 1u << 24}) {
            const int p = pf_count::lut_prefix_len(k);
            const uint32_t cb = pf_count::counter_bytes(pf_count::DEFAULT_CX, cb_cs), sb = pf_count::suffix_bytes(k, p);
            pf_count::Table t;
            for (int i = 0; i < 300; ++i) t[rnd() & ((1ull << (2 * k)) - 1)] = 1 + rnd() % cb_cs;
            std::vector<uint64_t> km;
            std::vector<uint32_t> ct;
            for (const auto &kv : t) { km.push_back(kv.first); ct.push_back((uint32_t)kv.second); }
            std::vector<uint8_t> pre, suf;
            pf_count::encode_kmc1_host(km.data(), ct.data(), km.size(), k, p, cb, 3, 77, (k & 1) != 0, pre, suf);
            const uint64_t n_lut = 1ull << (2 * p);
            CHECK(pre.size() == 4 + (n_lut + 1 + 7) * 8 + 4 + 4 && suf.size() == 8 + km.size() * (sb + cb));
            CHECK(std::string(pre.begin(), pre.begin() + 4) == "KMCP" && std::string(pre.end() - 4, pre.end()) == "KMCP");
            CHECK(std::string(suf.begin(), suf.begin() + 4) == "KMCS" && std::string(suf.end() - 4, suf.end()) == "KMCS");
            const size_t head = 4 + (size_t)(n_lut + 1) * 8;
            CHECK(word_at(pre, head - 8, 8) == km.size());   // the sentinel word
            CHECK(word_at(pre, head, 8) == (uint64_t)k && word_at(pre, head + 8, 8) == ((uint64_t)cb | ((uint64_t)p << 32)));
            CHECK(word_at(pre, head + 16, 8) == (3ull | (77ull << 32)) && word_at(pre, head + 24, 8) == km.size());
            CHECK(word_at(pre, head + 32, 8) == ((k & 1) ? 0u : 1u) && word_at(pre, pre.size() - 12, 4) == 0 && word_at(pre, pre.size() - 8, 4) == 56);
            // the records decoded again: prefix from the table, suffix most significant byte first, counter least significant first
            uint64_t e = 0;
            for (size_t i = 0; i < km.size(); ++i) {
                while (e + 1 < n_lut && word_at(pre, 4 + (size_t)(e + 1) * 8, 8) <= i) ++e;
                uint64_t sfx = 0;
                for (uint32_t b = 0; b < sb; ++b) sfx = (sfx << 8) | suf[4 + i * (sb + cb) + b];
                CHECK(((e << (2 * (k - p))) | sfx) == km[i]);
                CHECK(word_at(suf, 4 + i * (sb + cb) + sb, (int)cb) == ct[i]);
            }
            CHECK(word_at(pre, 4, 8) == 0);
        }
    }
    std::vector<uint8_t> pre, suf;   // an empty database is a database
    pf_count::encode_kmc1_host(nullptr, nullptr, 0, 25, 5, 1, 2, 9, true, pre, suf);
    CHECK(suf.size() == 8 && pre.size() == 4 + (1024 + 1 + 7) * 8 + 8);
}

int main() {
    keys();
    counting();
    cutoffs();
    layout();
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
