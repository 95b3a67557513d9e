// Stand-alone check of ploidyfrost_amd/csrc/pf_dedup_rule.hpp: the shared header alone, plain host C++, built with
// -fsanitize=address,undefined by tests/test_dedup_cpu.py.  Every read the rule keys is a heap block of exactly the size it is given
// (behind `off` bytes of padding, for every alignment 0 .. 15), so a read one byte beyond a sequence line is reported.  The key against
// a second statement that hashes the words the way the kernel's lanes do (16 lanes, each its own words, summed in another order); the
// properties of the code; the lengths and `bases` at which the word count changes; the table's sizes.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "pf_dedup_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

// a heap block of exactly off + s.size() bytes with s behind `off` bytes (at least one byte, so that the pointer is never null)
struct Exact {
    std::unique_ptr<char[]> p;
    size_t off;
    Exact(const std::string &s, size_t off_) : p(new char[off_ + s.size() ? off_ + s.size() : 1]), off(off_) {
        memset(p.get(), '#', off);
        if (!s.empty()) memcpy(p.get() + off, s.data(), s.size());
    }
    const char *get() const { return p.get() + off; }
};

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}
static std::string bases(size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back("ACGT"[rnd() & 3]);
    return s;
}

struct Key {
    uint64_t h[2];
    bool operator==(const Key &o) const { return h[0] == o.h[0] && h[1] == o.h[1]; }
    bool operator!=(const Key &o) const { return !(*this == o); }
};
static Key key_of(const std::string &r1, const std::string *r2, uint32_t B, size_t off = 0) {
    const Exact a(r1, off), b(r2 ? *r2 : std::string(), off);
    Key k;
    pf_dedup::key_of(a.get(), (uint32_t)r1.size(), b.get(), r2 ? (uint32_t)r2->size() : 0u, r2 != nullptr, B, k.h);
    return k;
}
// the key as the kernel's row takes it: lane l owns words l, l + 16, ...; the lanes are summed from the last to the first
static Key lanes_key(const std::string &r1, const std::string *r2, uint32_t B) {
    uint64_t lane_sum[16][2] = {};
    uint32_t cov[2] = {0, 0};
    for (int f = 0; f < (r2 ? 2 : 1); ++f) {
        const std::string &s = f ? *r2 : r1;
        const uint32_t L = pf_dedup::covered((uint32_t)s.size(), B);
        cov[f] = L;
        for (int lane = 15; lane >= 0; --lane)
            for (uint64_t i0 = 16ull * lane; i0 < L; i0 += 256) {
                uint64_t word = 0;
                for (uint32_t k = 0; k < 16 && i0 + k < L; ++k) word |= (uint64_t)pf_dedup::code((uint8_t)s[i0 + k]) << (3 * k);
                lane_sum[lane][0] += pf_dedup::term(word, pf_dedup::index_of(i0 >> 4, f == 1), 0);
                lane_sum[lane][1] += pf_dedup::term(word, pf_dedup::index_of(i0 >> 4, f == 1), 1);
            }
    }
    uint64_t sum[2] = {0, 0};
    for (int lane = 15; lane >= 0; --lane) { sum[0] += lane_sum[lane][0]; sum[1] += lane_sum[lane][1]; }
    Key k;
    k.h[0] = pf_dedup::close(sum[0], cov[0], cov[1], r2 != nullptr, 0);
    k.h[1] = pf_dedup::close(sum[1], cov[0], cov[1], r2 != nullptr, 1);
    return k;
}

int main() {
    using namespace pf_dedup;
    // ---- the code ----
    for (int c = 0; c < 256; ++c) {
        const uint32_t want = (c == 'A' || c == 'a') ? 0u : (c == 'C' || c == 'c') ? 1u : (c == 'G' || c == 'g') ? 2u : (c == 'T' || c == 't') ? 3u : 4u;
        CHECK(code((uint8_t)c) == want);
    }
    CHECK(bases_ok(0) && bases_ok(16) && bases_ok(4096) && !bases_ok(15) && !bases_ok(4097) && !bases_ok(1));

    // ---- lengths x bases, every alignment, against the lane statement ----
    const size_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097};
    const uint32_t Bs[] = {0, 16, 17, 100, 4096};
    std::set<std::pair<uint64_t, uint64_t>> distinct;
    size_t n_keys = 0;
    for (size_t n : lens) {
        const std::string r = bases(n), mate = bases(n ? n - 1 : 3);
        for (uint32_t B : Bs) {
            const Key k = key_of(r, nullptr, B), kp = key_of(r, &mate, B);
            CHECK(k.h[0] != 0 && k.h[1] != 0);
            CHECK(k == lanes_key(r, nullptr, B));
            CHECK(kp == lanes_key(r, &mate, B));
            CHECK(k != kp);
            for (size_t off = 0; off < 16; ++off) {
                CHECK(key_of(r, nullptr, B, off) == k);
                CHECK(key_of(r, &mate, B, off) == kp);
            }
            if (B == 0) { distinct.insert({k.h[0], k.h[1]}); ++n_keys; }
        }
        // bases against reads shorter, equal and longer: the key covers min(n, B) bases and that length
        for (uint32_t B : {16u, 4096u}) {
            const Key k = key_of(r, nullptr, B);
            if (n <= B) CHECK(k == key_of(r, nullptr, 0));
            else {
                CHECK(k == key_of(r.substr(0, B), nullptr, 0));
                std::string other = r;
                other[B] = other[B] == 'A' ? 'C' : 'A';   // beyond the bases: no part of the key
                CHECK(key_of(other, nullptr, B) == k);
                other = r;
                other[B - 1] = other[B - 1] == 'A' ? 'C' : 'A';
                CHECK(key_of(other, nullptr, B) != k);
            }
        }
    }
    CHECK(distinct.size() == n_keys);

    // ---- what distinguishes reads and what does not ----
    for (size_t n : {1, 15, 16, 17, 33, 100, 257}) {
        const std::string r = bases(n);
        std::string lower = r, last = r, n1 = r, n2 = r;
        for (char &c : lower) c = (char)(c | 0x20);
        CHECK(key_of(lower, nullptr, 0) == key_of(r, nullptr, 0));   // case
        last[n - 1] = last[n - 1] == 'A' ? 'C' : 'A';
        CHECK(key_of(last, nullptr, 0) != key_of(r, nullptr, 0));    // the last base
        n1[n / 2] = 'N';
        n2[n / 2] = '.';
        CHECK(key_of(n1, nullptr, 0) == key_of(n2, nullptr, 0));     // which non-ACGT byte
        CHECK(key_of(n1, nullptr, 0) != key_of(r, nullptr, 0));
        CHECK(key_of(r + "A", nullptr, 0) != key_of(r, nullptr, 0)); // a prefix ('A' codes as 0: the length closes the key)
        const std::string mate = bases(n + 1);
        CHECK(key_of(r, &mate, 0) != key_of(mate, &r, 0));           // (R1, R2) against (R2, R1)
        CHECK(key_of(r, &mate, 0) != key_of(r, &r, 0));              // the same R1, another R2
        const std::string empty;
        CHECK(key_of(r, &empty, 0) != key_of(r, nullptr, 0));        // a pair with an empty mate against a single read
        CHECK(key_of(r + mate, nullptr, 0) != key_of(r, &mate, 0));  // the bases of a pair laid end to end
    }
    // all 'A' reads of different lengths: every word is 0, the lengths alone tell them apart
    {
        std::set<std::pair<uint64_t, uint64_t>> seen;
        for (size_t n = 0; n <= 70; ++n) { const Key k = key_of(std::string(n, 'A'), nullptr, 0); seen.insert({k.h[0], k.h[1]}); }
        CHECK(seen.size() == 71);
    }

    // ---- the table's sizes ----
    CHECK(round_slots(0) == DEFAULT_SLOTS && round_slots(1) == 64 && round_slots(64) == 64 && round_slots(65) == 128 && round_slots(1000) == 1024);
    CHECK(needed_slots(64, 0, 32) == 64 && needed_slots(64, 0, 33) == 128 && needed_slots(64, 31, 1) == 64 && needed_slots(64, 32, 1) == 128);
    CHECK(needed_slots(1024, 0, 1) == 1024 && needed_slots(64, 1000, 5000) == 16384);
    for (uint64_t e = 0; e < 300; e += 7)
        for (uint64_t n = 1; n < 300; n += 11) {
            const uint64_t s = needed_slots(64, e, n);
            CHECK((s & (s - 1)) == 0 && 2 * (e + n) <= s && (s == 64 || 2 * (e + n) > s / 2));
        }
    CHECK(home(0x12345, 64) == 0x05 && home(~0ull, 1024) == 1023);
    CHECK(level_of(1) == 0 && level_of(9) == 8 && level_of(10) == 9 && level_of(1000000) == 9);
    CHECK(nonzero(0) == 1 && nonzero(7) == 7);

    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
