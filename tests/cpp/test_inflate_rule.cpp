// The rule of K-INFLATE alone (pf_inflate_rule.hpp over pf_inflate_core.hpp), for plain g++ with -fsanitize=address,undefined: members
// written bit by bit here (stored, fixed and dynamic blocks), every refusal by its clause, and the corrupt-member loop -- each of the
// first 200 bits of a member flipped in turn, then seeded multi-bit flips -- over heap buffers of exactly the payload's and ISIZE's
// sizes, so that a read or write outside them stops the program.  With a file name: the same loop over the members in that file
// (u32 length, bytes; repeated), which the Python test makes with zlib.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pf_inflate_rule.hpp"

using namespace pf_inflate;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #c);               \
            exit(1);                                                    \
        }                                                               \
    } while (0)

typedef std::vector<uint8_t> Bytes;

struct BitWriter {
    Bytes out;
    uint32_t acc = 0;
    int n = 0;
    void put(uint32_t v, int bits) {   // least significant bit first
        for (int i = 0; i < bits; ++i) {
            acc |= ((v >> i) & 1u) << n;
            if (++n == 8) { out.push_back((uint8_t)acc); acc = 0; n = 0; }
        }
    }
    void code(uint32_t c, int bits) { for (int i = bits - 1; i >= 0; --i) put((c >> i) & 1u, 1); }   // a Huffman code, first bit first
    Bytes bytes() const { Bytes b = out; if (n) b.push_back((uint8_t)acc); return b; }
};

struct Code { uint32_t code; int len; };
static std::vector<Code> canonical(const std::vector<int> &lengths) {
    int count[16] = {0};
    for (int l : lengths) count[l]++;
    count[0] = 0;
    uint32_t next[16] = {0}, code = 0;
    for (int b = 1; b < 16; ++b) { code = (code + (uint32_t)count[b - 1]) << 1; next[b] = code; }
    std::vector<Code> out(lengths.size(), Code{0, 0});
    for (size_t s = 0; s < lengths.size(); ++s)
        if (lengths[s]) out[s] = Code{next[lengths[s]]++, lengths[s]};
    return out;
}
static std::vector<int> fixed_lit_lengths() {
    std::vector<int> l(288, 8);
    for (int s = 144; s < 256; ++s) l[s] = 9;
    for (int s = 256; s < 280; ++s) l[s] = 7;
    return l;
}

static Bytes wrap(const Bytes &raw, uint32_t crc, uint32_t isize, const Bytes &extra_before = Bytes()) {
    const uint32_t xlen = (uint32_t)extra_before.size() + 6, bsize = 12 + xlen + (uint32_t)raw.size() + 8 - 1;
    Bytes m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, (uint8_t)xlen, (uint8_t)(xlen >> 8)};
    m.insert(m.end(), extra_before.begin(), extra_before.end());
    const uint8_t bc[6] = {'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    m.insert(m.end(), bc, bc + 6);
    m.insert(m.end(), raw.begin(), raw.end());
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(crc >> (8 * i)));
    for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(isize >> (8 * i)));
    return m;
}
static Bytes member_of(const Bytes &raw, const std::string &text) { return wrap(raw, crc32((const uint8_t *)text.data(), text.size()), (uint32_t)text.size()); }

static Bytes stored_stream(const std::string &text) {
    Bytes b = {1, (uint8_t)text.size(), (uint8_t)(text.size() >> 8), (uint8_t)~text.size(), (uint8_t)(~text.size() >> 8)};
    b.insert(b.end(), text.begin(), text.end());
    return b;
}
// literals, and a match wherever the text repeats what lies `dist` bytes back for at least three bytes (dist = 0: literals only)
static void put_symbols(BitWriter &w, const std::string &text, const std::vector<Code> &lit, const std::vector<Code> &dst, uint32_t dist) {
    for (size_t i = 0; i < text.size();) {
        size_t run = 0;
        if (dist && i >= dist)
            while (i + run < text.size() && run < 10 && text[i + run] == text[i + run - dist]) ++run;
        if (run >= 3) {   // lengths 3 .. 10 are symbols 257 .. 264 without extra bits; distances 1 .. 4 are symbols 0 .. 3
            w.code(lit[257 + run - 3].code, lit[257 + run - 3].len);
            w.code(dst[dist - 1].code, dst[dist - 1].len);
            i += run;
        } else {
            w.code(lit[(uint8_t)text[i]].code, lit[(uint8_t)text[i]].len);
            ++i;
        }
    }
    w.code(lit[256].code, lit[256].len);
}
static Bytes fixed_stream(const std::string &text, uint32_t dist) {
    BitWriter w;
    w.put(1, 1);
    w.put(1, 2);
    put_symbols(w, text, canonical(fixed_lit_lengths()), canonical(std::vector<int>(32, 5)), dist);
    return w.bytes();
}
// a dynamic block: every literal/length symbol 0 .. 264 in nine bits or eight (complete), four distances of two bits; the code-length
// code has 13 symbols of four bits and 6 of five, and every length is sent as itself
static Bytes dynamic_stream(const std::string &text, uint32_t dist) {
    std::vector<int> lit(265, 9), dst(4, 2), cl(19, 4);
    for (int s = 0; s < 247; ++s) lit[s] = 8;   // 247 / 256 + 18 / 512 = 1
    for (int s = 13; s < 19; ++s) cl[s] = 5;
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    BitWriter w;
    w.put(1, 1);
    w.put(2, 2);
    w.put(265 - 257, 5);
    w.put(4 - 1, 5);
    w.put(19 - 4, 4);
    for (int i = 0; i < 19; ++i) w.put((uint32_t)cl[order[i]], 3);
    const std::vector<Code> clc = canonical(cl);
    for (int l : lit) w.code(clc[l].code, clc[l].len);
    for (int l : dst) w.code(clc[l].code, clc[l].len);
    put_symbols(w, text, canonical(lit), canonical(dst), dist);
    return w.bytes();
}

// one member through the rule over buffers of exactly its sizes
static int run_member(const Bytes &m, std::string *text = nullptr, Blocks *blocks = nullptr) {
    uint8_t *copy = (uint8_t *)malloc(m.size() ? m.size() : 1);
    memcpy(copy, m.data(), m.size());
    Header h;
    int c = parse_member(copy, m.size(), &h);
    if (!c) {
        const uint32_t n_in = h.member_len - h.payload_off - TRAILER;
        uint8_t *payload = (uint8_t *)malloc(n_in ? n_in : 1), *out = (uint8_t *)malloc(h.isize ? h.isize : 1);
        memcpy(payload, copy + h.payload_off, n_in);
        uint32_t made = 0;
        inflate_member(payload, n_in, out, h.isize, &c, blocks, &made);
        CHECK(made <= h.isize);
        if (!c && crc32(out, h.isize) != h.crc) c = CLAUSE_CRC;
        if (!c) CHECK(crc32_sliced(out, h.isize, 64) == h.crc && crc32_sliced(out, h.isize, 7) == h.crc);
        if (!c && text) text->assign((const char *)out, h.isize);
        free(payload);
        free(out);
    }
    free(copy);
    return c;
}

static uint32_t rnd_state = 20;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

// every flip is refused by a clause or leaves the text as it was; never other bytes behind a matching CRC
static void corrupt_loop(const Bytes &m) {
    std::string text, got;
    CHECK(run_member(m, &text) == CLAUSE_NONE);
    Header h;
    CHECK(parse_member(m.data(), m.size(), &h) == CLAUSE_NONE);
    const uint32_t n_bits = 8 * (h.member_len - h.payload_off - TRAILER);
    int refused = 0;
    for (uint32_t bit = 0; bit < 200 && bit < n_bits; ++bit) {
        Bytes bad = m;
        bad[h.payload_off + bit / 8] ^= (uint8_t)(1u << (bit % 8));
        const int c = run_member(bad, &got);
        CHECK(c != CLAUSE_NONE || got == text);
        refused += c != CLAUSE_NONE;
    }
    for (int round = 0; round < 300 && n_bits; ++round) {
        Bytes bad = m;
        for (uint32_t k = 0, n = 1 + rnd() % 3; k < n; ++k) {
            const uint32_t bit = rnd() % n_bits;
            bad[h.payload_off + bit / 8] ^= (uint8_t)(1u << (bit % 8));
        }
        const int c = run_member(bad, &got);
        CHECK(c != CLAUSE_NONE || got == text);
        refused += c != CLAUSE_NONE;
    }
    CHECK(refused > 0 || n_bits < 32);
    // the trailer's fields and a payload cut short or grown by a byte
    for (int k = 0; k < 64; ++k) {
        Bytes bad = m;
        bad[m.size() - 8 + k / 8] ^= (uint8_t)(1u << (k % 8));
        CHECK(run_member(bad) != CLAUSE_NONE);
    }
}

int main(int argc, char **argv) {
    if (argc > 1) {   // members made elsewhere
        FILE *f = fopen(argv[1], "rb");
        CHECK(f != nullptr);
        uint8_t len4[4];
        int n = 0;
        while (fread(len4, 1, 4, f) == 4) {
            Bytes m((size_t)len4[0] | ((size_t)len4[1] << 8) | ((size_t)len4[2] << 16) | ((size_t)len4[3] << 24));
            CHECK(fread(m.data(), 1, m.size(), f) == m.size());
            corrupt_loop(m);
            ++n;
        }
        fclose(f);
        CHECK(n > 0);
        printf("ok\n");
        return 0;
    }
    // ---- sound members of every kind of block ----
    const std::string fq = "@r1\nACGTACGTAACCGGTTACGT\n+\nIIIIIIIIIIHHHHHHHHHH\n@r2\nTTTTTTTTTTGGGGGGGGGG\n+\n##########IIIIIIIIII\n";
    std::string text;
    Blocks b;
    CHECK(run_member(member_of(stored_stream(fq), fq), &text, &b) == CLAUSE_NONE && text == fq && b.stored == 1 && b.fixed + b.dynamic == 0);
    for (uint32_t dist = 0; dist <= 4; ++dist) {
        CHECK(run_member(member_of(fixed_stream(fq, dist), fq), &text, &b) == CLAUSE_NONE && text == fq && b.fixed == 1);
        CHECK(run_member(member_of(dynamic_stream(fq, dist), fq), &text, &b) == CLAUSE_NONE && text == fq && b.dynamic == 1);
    }
    const std::string run(3000, 'I');   // distance 1, length > distance
    CHECK(fixed_stream(run, 1).size() < 1000 && run_member(member_of(fixed_stream(run, 1), run), &text) == CLAUSE_NONE && text == run);
    CHECK(run_member(member_of(dynamic_stream(run, 1), run), &text) == CLAUSE_NONE && text == run);
    std::string acgt;
    for (int i = 0; i < 500; ++i) acgt += "ACGT";   // distance 4, length > distance
    CHECK(run_member(member_of(dynamic_stream(acgt, 4), acgt), &text) == CLAUSE_NONE && text == acgt);
    CHECK(run_member(member_of(stored_stream(""), ""), &text, &b) == CLAUSE_NONE && text.empty() && b.stored == 1);
    {   // several blocks in one member: stored (not final), then fixed
        Bytes two = stored_stream("@r\n");
        two[0] = 0;
        const Bytes rest = fixed_stream("ACGT\n", 0);
        two.insert(two.end(), rest.begin(), rest.end());
        CHECK(run_member(member_of(two, "@r\nACGT\n"), &text, &b) == CLAUSE_NONE && text == "@r\nACGT\n" && b.stored == 1 && b.fixed == 1);
    }
    // ---- the header ----
    const Bytes eof_marker = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    Header h;
    CHECK(parse_member(eof_marker.data(), eof_marker.size(), &h) == CLAUSE_NONE && h.payload_off == 18 && h.member_len == 28 && h.isize == 0 && h.crc == 0);
    CHECK(run_member(eof_marker, &text, &b) == CLAUSE_NONE && text.empty() && b.fixed == 1);
    const Bytes sub = wrap(fixed_stream(fq, 2), crc32((const uint8_t *)fq.data(), fq.size()), (uint32_t)fq.size(), Bytes{'X', 'Y', 3, 0, 'a', 'b', 'c'});
    CHECK(parse_member(sub.data(), sub.size(), &h) == CLAUSE_NONE && h.payload_off == 25 && h.member_len == sub.size() && h.isize == fq.size());
    CHECK(run_member(sub, &text) == CLAUSE_NONE && text == fq);
    {
        const Bytes good = member_of(fixed_stream(fq, 2), fq);
        Bytes m = good;
        m[1] = 0x8c;
        CHECK(run_member(m) == CLAUSE_MAGIC);
        m = good; m[2] = 7;
        CHECK(run_member(m) == CLAUSE_METHOD);
        m = good; m[3] = 0;
        CHECK(run_member(m) == CLAUSE_FLAGS);
        m = good; m[3] = 12;
        CHECK(run_member(m) == CLAUSE_FLAGS);
        m = good; m[12] = 'X';
        CHECK(run_member(m) == CLAUSE_NOT_BLOCKED);
        m = good; m[14] = 3;   // BC of three bytes is not the BC of blocked gzip (and runs past XLEN)
        CHECK(run_member(m) == CLAUSE_NOT_BLOCKED);
        m = good; m[16] = 20; m[17] = 0;
        CHECK(run_member(m) == CLAUSE_SHORT);
        m = good; m.pop_back();
        CHECK(run_member(m) == CLAUSE_PAST_END);
        m = good; m.resize(11);
        CHECK(run_member(m) == CLAUSE_PAST_END);
        m = good; m[m.size() - 2] = 1; m[m.size() - 4] = 1;   // ISIZE = 65537 + ...
        CHECK(run_member(m) == CLAUSE_ISIZE);
        int clause = -1;
        CHECK(file_clause_gz(good.data(), good.size(), good.size(), &clause) == FILE_BGZF && clause == 0);
        CHECK(file_clause_gz((const uint8_t *)fq.data(), fq.size(), fq.size(), &clause) == FILE_PLAIN);
        m = good; m[12] = 'X';
        CHECK(file_clause_gz(m.data(), m.size(), m.size(), &clause) == FILE_REFUSED && clause == CLAUSE_NOT_BLOCKED);
        CHECK(file_clause_gz(good.data(), 30, 30, &clause) == FILE_REFUSED && clause == CLAUSE_PAST_END);
        for (int c = 1; c < CLAUSE_COUNT_; ++c) CHECK(strcmp(clause_text(c), "no refusal") != 0);
        CHECK(strstr(clause_text(CLAUSE_NOT_BLOCKED), "bgzip") && strstr(clause_text(CLAUSE_NOT_BLOCKED), "decompress"));
    }
    // ---- the stream's refusals ----
    auto hand = [&](const Bytes &raw, const std::string &t) { return run_member(member_of(raw, t)); };
    CHECK(hand(Bytes{7}, "") == CLAUSE_BTYPE3);
    CHECK(hand(Bytes{1, 1, 0, 0, 0, 'A'}, "A") == CLAUSE_STORED_LEN);
    CHECK(hand(Bytes{1, 5, 0, 0xfa, 0xff, 'A', 'B'}, "ABCDE") == CLAUSE_STORED_PAST);
    CHECK(hand(Bytes{1, 5, 0}, "ABCDE") == CLAUSE_STORED_PAST);
    {
        BitWriter w;
        w.put(1, 1); w.put(2, 2); w.put(30, 5); w.put(0, 5); w.put(0, 4); w.put(0, 12);
        CHECK(hand(w.bytes(), "") == CLAUSE_TOO_MANY_CODES);
    }
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    auto dyn_head = [&](BitWriter &w, int hlit, int hdist, const std::vector<int> &cl) {
        w.put(1, 1); w.put(2, 2); w.put((uint32_t)hlit, 5); w.put((uint32_t)hdist, 5); w.put(15, 4);
        for (int i = 0; i < 19; ++i) w.put((uint32_t)cl[order[i]], 3);
    };
    {
        BitWriter w;
        dyn_head(w, 0, 0, std::vector<int>(19, 1));   // over-subscribed
        w.put(0, 16);
        CHECK(hand(w.bytes(), "") == CLAUSE_CODE_LENGTHS);
        BitWriter v;
        std::vector<int> cl(19, 0);
        cl[0] = 1;                                    // incomplete
        dyn_head(v, 0, 0, cl);
        v.put(0, 16);
        CHECK(hand(v.bytes(), "") == CLAUSE_CODE_LENGTHS);
    }
    {
        std::vector<int> cl(19, 0);
        cl[0] = cl[16] = 1;   // symbol 0 = code 0, symbol 16 = code 1
        BitWriter w;
        dyn_head(w, 0, 0, cl);
        w.put(1, 1); w.put(0, 2); w.put(0, 16);
        CHECK(hand(w.bytes(), "") == CLAUSE_REPEAT);   // nothing to repeat
        cl[16] = 0;
        cl[18] = 1;           // symbol 18 = code 1
        BitWriter v;
        dyn_head(v, 0, 0, cl);
        v.put(1, 1); v.put(127, 7); v.put(1, 1); v.put(127, 7); v.put(0, 16);
        CHECK(hand(v.bytes(), "") == CLAUSE_REPEAT);   // 276 lengths where HLIT + HDIST is 258
        BitWriter u;
        dyn_head(u, 0, 0, cl);
        u.put(1, 1); u.put(127, 7); u.put(1, 1); u.put(109, 7); u.put(0, 16);
        CHECK(hand(u.bytes(), "") == CLAUSE_NO_EOB);   // 258 zeros
    }
    {   // 'A' and end-of-block in two bits, length symbol 257 in one, no distance code: the match has no distance to decode
        std::vector<int> cl(19, 4), lit(258, 0);
        for (int s = 13; s < 19; ++s) cl[s] = 5;
        lit[65] = lit[256] = 2;
        lit[257] = 1;
        BitWriter w;
        dyn_head(w, 1, 0, cl);
        const std::vector<Code> clc = canonical(cl), lc = canonical(lit);
        for (int l : lit) w.code(clc[l].code, clc[l].len);
        w.code(clc[0].code, clc[0].len);
        w.code(lc[65].code, 2); w.code(lc[257].code, 1); w.put(0, 24);
        CHECK(hand(w.bytes(), "AAAA") == CLAUSE_BAD_CODE);
    }
    {
        const std::vector<Code> lit = canonical(fixed_lit_lengths()), dst = canonical(std::vector<int>(32, 5));
        BitWriter w;
        w.put(1, 1); w.put(1, 2); w.code(lit[286].code, 8); w.put(0, 8);
        CHECK(hand(w.bytes(), "") == CLAUSE_LITLEN_SYM);
        BitWriter v;
        v.put(1, 1); v.put(1, 2); v.code(lit[65].code, 8); v.code(lit[257].code, 7); v.code(dst[31].code, 5); v.put(0, 8);
        CHECK(hand(v.bytes(), "AAAA") == CLAUSE_DIST_SYM);
        BitWriter u;
        u.put(1, 1); u.put(1, 2); u.code(lit[65].code, 8); u.code(lit[257].code, 7); u.code(dst[1].code, 5); u.code(lit[256].code, 7);
        CHECK(hand(u.bytes(), "AAAA") == CLAUSE_DIST_BEFORE);
    }
    {
        const Bytes raw = dynamic_stream(fq, 3);
        const uint32_t crc = crc32((const uint8_t *)fq.data(), fq.size()), n = (uint32_t)fq.size();
        CHECK(run_member(wrap(raw, crc, n - 10)) == CLAUSE_OUT_BEYOND);
        CHECK(run_member(wrap(raw, crc, n + 1)) == CLAUSE_LENGTH);
        CHECK(run_member(wrap(raw, crc ^ 0x100, n)) == CLAUSE_CRC);
        Bytes longer = raw;
        longer.push_back(0);
        CHECK(run_member(wrap(longer, crc, n)) == CLAUSE_END);
        Bytes cut = raw;
        cut.pop_back();
        CHECK(run_member(wrap(cut, crc, n)) == CLAUSE_END);
    }
    // ---- the corrupt-member loop ----
    std::string big;
    for (int i = 0; i < 300; ++i) big += fq.substr((size_t)(i * 7) % 40, 60);
    corrupt_loop(member_of(dynamic_stream(big, 3), big));
    corrupt_loop(member_of(fixed_stream(big, 2), big));
    corrupt_loop(member_of(stored_stream(fq), fq));
    printf("ok\n");
    return 0;
}
