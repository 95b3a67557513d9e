// The rule of K-DEFLATE alone (pf_deflate_rule.hpp over pf_deflate_core.hpp) against the rule of K-INFLATE (pf_inflate_rule.hpp), for plain
// g++ with -fsanitize=address,undefined: every text, and every text cut at every length up to 600, is deflated into a heap buffer of
// exactly the bound's n + 31 bytes from a heap buffer of exactly n bytes, inflated by the host rule and compared, so that a read or write
// outside them stops the program.  The texts are a few made here and, with a file name, the ones in that file (u32 length, bytes;
// repeated), which the Python test writes from tests/gzo_cases.py; texts longer than a member are cut as the writer cuts them.
// Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "pf_deflate_rule.hpp"
#include "pf_inflate_rule.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #c);               \
            exit(1);                                                    \
        }                                                               \
    } while (0)

typedef std::vector<uint8_t> Bytes;

static std::unique_ptr<pf_deflate::HostWork> work(new pf_deflate::HostWork);

static void round_trip(const uint8_t *text, uint32_t n) {
    uint8_t *in = (uint8_t *)malloc(n ? n : 1), *out = (uint8_t *)malloc(n + pf_deflate::MEMBER_EXTRA), *back = (uint8_t *)malloc(65536);
    CHECK(in && out && back);
    if (n) memcpy(in, text, n);
    memset(out, 0xa5, n + pf_deflate::MEMBER_EXTRA);
    pf_deflate::Result res;
    const uint32_t size = pf_deflate::deflate_member(in, n, out, *work, &res);
    CHECK(size <= n + pf_deflate::MEMBER_EXTRA);
    CHECK(res.kind <= 2);
    uint8_t *exact = (uint8_t *)malloc(size);   // (the reader gets the member alone)
    CHECK(exact);
    memcpy(exact, out, size);
    uint32_t got = 0;
    pf_inflate::Blocks blocks;
    const int clause = pf_inflate::inflate_bgzf_member(exact, size, back, &got, &blocks);
    if (clause) printf("n = %u: %s\n", n, pf_inflate::clause_text(clause));
    CHECK(clause == 0);
    CHECK(got == n && (n == 0 || memcmp(back, in, n) == 0));
    CHECK(blocks.stored + blocks.fixed + blocks.dynamic == 1);
    CHECK((res.kind == 0 ? blocks.stored : res.kind == 1 ? blocks.fixed : blocks.dynamic) == 1);
    if (n == 0) CHECK(size == 28 && memcmp(exact, pf_deflate::EOF_MARKER, 28) == 0);
    free(in); free(out); free(back); free(exact);
}

static void every_cut(const Bytes &text) {
    for (size_t at = 0; at < text.size() || at == 0; at += pf_deflate::MEMBER_TEXT) {
        const uint32_t n = (uint32_t)std::min<size_t>(pf_deflate::MEMBER_TEXT, text.size() - at);
        round_trip(text.data() + at, n);
        for (uint32_t cut = 0; cut <= 600 && cut < n; ++cut) round_trip(text.data() + at, cut);
    }
}

// frequencies that take Huffman's construction past the limit: the lengths stay within it, fill Kraft's sum and fall with the frequency
static void code_length_limit() {
    std::unique_ptr<pf_deflate::Codes> c(new pf_deflate::Codes);
    for (uint32_t max_bits : {15u, 7u}) {
        for (uint32_t n : {19u, 30u, 286u}) {
            for (uint32_t used : {2u, 3u, 8u, 17u, 19u, 30u, 40u}) {
                if (used > n) continue;
                if (max_bits == 7 && used > 19) continue;
                uint32_t freq[288];
                uint8_t lens[288];
                uint16_t codes[288];
                memset(freq, 0, sizeof freq);
                uint32_t a = 1, b = 1;
                for (uint32_t i = 0; i < used; ++i) {   // Fibonacci's numbers, scattered over the alphabet
                    freq[(i * 7 + 3) % n] += a;   // (7 shares no factor with 19, 30 or 286: `used` different places)
                    const uint32_t s = a + b;
                    a = b;
                    b = s;
                }
                pf_deflate::build_code(*c, freq, n, max_bits, false, lens, codes, 0u, 1u, pf_deflate::NoSync{});
                uint64_t kraft = 0;
                uint32_t longest = 0;
                for (uint32_t s = 0; s < n; ++s) {
                    CHECK((lens[s] != 0) == (freq[s] != 0));
                    CHECK(lens[s] <= max_bits);
                    if (lens[s]) kraft += 1ull << (max_bits - lens[s]);
                    if (lens[s] > longest) longest = lens[s];
                    for (uint32_t t = 0; t < n; ++t)
                        if (freq[s] && freq[t] && freq[s] < freq[t]) CHECK(lens[s] >= lens[t]);
                }
                CHECK(kraft == 1ull << max_bits);
                if (used > max_bits + 1) CHECK(longest == max_bits);   // (the construction alone would have gone deeper)
            }
        }
    }
}

int main(int argc, char **argv) {
    code_length_limit();
    uint32_t seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    std::vector<Bytes> texts;
    texts.push_back(Bytes());
    texts.push_back(Bytes(700, 'I'));
    {
        Bytes t;
        for (int i = 0; i < 300; ++i) t.insert(t.end(), {'A', 'C', 'G', 'T'});
        texts.push_back(t);
    }
    {
        Bytes t(2000);
        for (auto &b : t) b = (uint8_t)rnd();
        texts.push_back(t);
    }
    {
        Bytes t;   // records: a header that repeats, bases, runs of one quality
        for (int r = 0; r < 40; ++r) {
            const std::string h = "@A00123:45:HXXXXDSXX:1:1101:" + std::to_string(rnd() % 30000) + " 1:N:0\n";
            t.insert(t.end(), h.begin(), h.end());
            for (int i = 0; i < 100; ++i) t.push_back("ACGT"[rnd() & 3]);
            t.insert(t.end(), {'\n', '+', '\n'});
            for (int i = 0; i < 100; ++i) t.push_back(rnd() % 20 ? 'F' : ':');
            t.push_back('\n');
        }
        texts.push_back(t);
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        CHECK(f);
        uint32_t len;
        while (fread(&len, 4, 1, f) == 1) {
            Bytes t(len);
            CHECK(len == 0 || fread(t.data(), 1, len, f) == len);
            texts.push_back(t);
        }
        fclose(f);
    }
    for (const Bytes &t : texts) every_cut(t);
    printf("ok\n");
    return 0;
}
