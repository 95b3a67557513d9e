// Stand-alone check of ploidyfrost_amd/csrc/pf_clip_rule.hpp: the shared header alone, plain host C++, built with
// -fsanitize=address,undefined by tests/test_clip_cpu.py.  Every buffer the rule reads is a heap block of exactly the size it is given,
// so a read one byte beyond a read, a quality line, an adapter or an adapter file is reported.  Every read of the edge list (read
// lengths x adapter lengths x edge offsets) against a second, deliberately naive statement of the rule; adapter files cut at every
// byte; the refusals; the chunk restatement on a small text.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "pf_clip_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

// a heap copy of exactly s.size() bytes (at least one block, so that the pointer is never null)
struct Exact {
    std::unique_ptr<char[]> p;
    size_t n;
    explicit Exact(const std::string &s) : p(new char[s.size() ? s.size() : 1]), n(s.size()) { if (n) memcpy(p.get(), s.data(), n); }
    const char *get() const { return p.get(); }
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

// the rule once more, as naively as it reads: every window counted from scratch, every sub-range summed from scratch
static long naive_clip(const std::string &seq, const std::string &qual, const std::string &ad, unsigned seed, unsigned T, int phred, unsigned long *scored) {
    const long n = (long)seq.size(), m = (long)ad.size();
    long best = 0;
    bool found = false;
    auto up = [](char c) { return (char)(c & 0xDF); };
    auto valid = [&](char c) { return up(c) == 'A' || up(c) == 'C' || up(c) == 'G' || up(c) == 'T'; };
    for (long o = -(m - 16); o <= n - 16; ++o) {
        const long lo = o > 0 ? o : 0, hi = n < o + m ? n : o + m;
        if (hi - lo < 16) continue;
        bool seed_ok = false;
        for (long w = lo; w + 16 <= hi; ++w) {
            unsigned mm = 0;
            for (long p = w; p < w + 16; ++p) mm += !valid(seq[(size_t)p]) || up(seq[(size_t)p]) != up(ad[(size_t)(p - o)]);
            if (mm <= seed) seed_ok = true;
        }
        if (!seed_ok) continue;
        ++*scored;
        long top = 0;
        for (long a = lo; a < hi; ++a)
            for (long z = a + 1; z <= hi; ++z) {
                long sum = 0;
                for (long p = a; p < z; ++p) {
                    const char c = seq[(size_t)p];
                    const int q = (int)(unsigned char)qual[(size_t)p] - phred;
                    sum += !valid(c) ? 0 : up(c) == up(ad[(size_t)(p - o)]) ? 60206 : -10000 * (q > 0 ? q : 0);
                }
                if (sum > top) top = sum;
            }
        if (top >= 100000L * (long)T && (!found || o < best)) { found = true; best = o; }
    }
    return !found ? n : best <= 0 ? 0 : best;
}

static void check_read(const std::string &seq, const std::string &qual, const std::string &ad, unsigned seed, unsigned T, int phred) {
    const Exact s(seq), q(qual), a(ad);
    const uint32_t off[2] = {0, (uint32_t)ad.size()};
    const uint8_t side[1] = {0};
    uint64_t scored = 0;
    unsigned long want_scored = 0;
    const uint32_t got = pf_clip::clip_read(s.get(), q.get(), (uint32_t)seq.size(), a.get(), off, side, 1, 1, seed, T, (uint32_t)phred, &scored);
    const long want = naive_clip(seq, qual, ad, seed, T, phred, &want_scored);
    CHECK((long)got == want);
    CHECK(scored == want_scored);
}

static void edge_reads() {
    const size_t read_lengths[] = {0, 1, 15, 16, 17, 100, 255, 256, 257, 1000}, adapter_lengths[] = {16, 17, 33, 64, 65, 128};
    for (size_t m : adapter_lengths) {
        const std::string ad = bases(m);
        for (size_t n : read_lengths) {
            const long offs[] = {-(long)(m - 16), -1, 0, 1, (long)n - 16, (long)n - 15};
            for (long o : offs) {
                if (o < -(long)(m - 16)) continue;
                std::string seq = bases(n), qual(n, 'I');
                for (long p = o > 0 ? o : 0; p < (long)n && p < o + (long)m; ++p) seq[(size_t)p] = ad[(size_t)(p - o)];
                if (n > 40 && (rnd() & 1)) seq[(size_t)(rnd() % n)] = 'N';
                if (rnd() & 1) for (char &c : seq) c = (char)(c | 0x20);
                for (size_t k = 0; k < n; k += 7) qual[k] = (char)(33 + rnd() % 60);
                if (n >= 1000 && m >= 64) { check_read(seq, qual, ad, 2, 10, 33); continue; }   // (the naive sums are cubic in the overlap)
                check_read(seq, qual, ad, 2, 10, 33);
                check_read(seq, qual, ad, 0, 1, 64);
                check_read(seq, qual, ad, 8, 30, 33);
            }
        }
    }
}

static void hand() {
    const std::string ad = bases(35), head(30, 'C');
    auto clip = [&](const std::string &seq, const std::string &qual, unsigned seed, unsigned T, uint32_t file_side, uint8_t ad_side) {
        const Exact s(seq), q(qual), a(ad);
        const uint32_t off[2] = {0, (uint32_t)ad.size()};
        return pf_clip::clip_read(s.get(), q.get(), (uint32_t)seq.size(), a.get(), off, &ad_side, 1, file_side, seed, T, 33);
    };
    CHECK(clip(ad.substr(0, 17), std::string(17, 'I'), 2, 10, 1, 0) == 0);     // 17 matches: 1 023 502
    CHECK(clip(ad.substr(0, 16), std::string(16, 'I'), 2, 10, 1, 0) == 16);    // 16 matches: 963 296
    CHECK(clip(head + ad, std::string(65, 'I'), 2, 10, 1, 0) == 30);
    CHECK(clip(head + ad, std::string(65, 'I'), 2, 10, 2, 1) == 65);           // a /1 adapter and file 2
    CHECK(clip(head + ad, std::string(65, 'I'), 2, 10, 2, 2) == 30);
    CHECK(clip(head + ad, std::string(65, 'I'), 2, 10, 1, 2) == 65);
    CHECK(17 * pf_clip::MATCH == 1023502 && 16 * pf_clip::MATCH == 963296);
    CHECK(pf_clip::min_overlap() == 16 && pf_clip::first_offset(128) == -112 && pf_clip::last_offset(16) == 0);
}

static void files() {
    std::string text = ">PrefixPE/1 x\nACGTACGT\n";
    const std::string a = bases(40), b = bases(16), c = bases(128);
    text += ">one/1 words\r\n" + a.substr(0, 25) + "\r\n" + a.substr(25) + "\r\n\r\n>two/2\n" + b + "\n>three\n" + c;
    {
        const Exact t(text);
        pf_clip::Adapters A;
        uint64_t bad = 9;
        CHECK(pf_clip::parse_adapters(t.get(), t.n, A, &bad) == pf_clip::REFUSE_NONE && bad == 0);
        CHECK(A.size() == 3 && A.skipped == 1 && A.bases == a + b + c);
        CHECK(A.side[0] == 1 && A.side[1] == 2 && A.side[2] == 0 && A.names[0] == "one/1" && A.names[2] == "three");
        CHECK(pf_clip::set_clause(A.bases.data(), A.off.data(), A.side.data(), A.size(), 2, 10) == pf_clip::REFUSE_NONE);
    }
    for (size_t cut = 0; cut <= text.size(); ++cut) {   // every prefix: parsed or refused, never read beyond its end
        const Exact t(text.substr(0, cut));
        pf_clip::Adapters A;
        uint64_t bad = 0;
        const int r = pf_clip::parse_adapters(t.get(), t.n, A, &bad);
        CHECK(r >= 0 && r < pf_clip::REFUSE_COUNT_);
        CHECK((r == pf_clip::REFUSE_NONE) == (A.size() > 0));
        if (r) CHECK(A.bases.empty() && A.off.size() == 1);
        if (r == pf_clip::REFUSE_LENGTH) CHECK(bad >= 1 && bad <= 4);   // (1: the Prefix entry while its name is cut short)
    }
    auto refusal = [](const std::string &s, uint64_t *bad) {
        const Exact t(s);
        pf_clip::Adapters A;
        return pf_clip::parse_adapters(t.get(), t.n, A, bad);
    };
    uint64_t bad = 0;
    CHECK(refusal("", &bad) == pf_clip::REFUSE_NOT_FASTA);
    CHECK(refusal("ACGT\n", &bad) == pf_clip::REFUSE_NOT_FASTA);
    CHECK(refusal(">a\n" + b + "\n>b\n" + b.substr(0, 8) + "N" + b.substr(8) + "\n", &bad) == pf_clip::REFUSE_BYTE && bad == 2);
    CHECK(refusal(">a\n" + b.substr(0, 15) + "\n", &bad) == pf_clip::REFUSE_LENGTH && bad == 1);
    CHECK(refusal(">a\n" + c + "A\n", &bad) == pf_clip::REFUSE_LENGTH && bad == 1);
    CHECK(refusal(">Prefix\n" + b + "\n", &bad) == pf_clip::REFUSE_NO_ADAPTER && bad == 0);
    std::string many;
    for (int i = 0; i < 65; ++i) many += ">a\n" + b + "\n";
    CHECK(refusal(many, &bad) == pf_clip::REFUSE_TOO_MANY && bad == 65);
    CHECK(pf_clip::params_clause(9, 10) == pf_clip::REFUSE_SEED && pf_clip::params_clause(8, 0) == pf_clip::REFUSE_SCORE &&
          pf_clip::params_clause(0, 1001) == pf_clip::REFUSE_SCORE && pf_clip::params_clause(0, 1000) == pf_clip::REFUSE_NONE);
    for (int r = 1; r < pf_clip::REFUSE_COUNT_; ++r) CHECK(strcmp(pf_clip::refusal_text(r), "no refusal") != 0);
}

static void chunk() {
    const std::string ad = bases(30), r0 = bases(40) + ad, r1 = bases(50), r2 = ad.substr(3) + bases(20);
    auto rec = [](const std::string &name, const std::string &seq, const char *nl) {
        return "@" + name + nl + seq + nl + "+" + nl + std::string(seq.size(), 'I') + nl;
    };
    const uint32_t off[2] = {0, 30};
    const uint8_t side[1] = {0};
    for (const char *nl : {"\n", "\r\n"}) {
        const std::string text = rec("a", r0, nl) + rec("b", r1, nl) + rec("c", r2, nl);
        for (size_t cut = 0; cut <= text.size(); ++cut) {
            const Exact t(text.substr(0, cut)), a(ad);
            std::string out;
            uint64_t used = 0, recs = 0, bad = 0;
            std::vector<uint32_t> begin, len;
            pf_trim::Stats st = {};
            pf_clip::Stats cs = {};
            const int clause = pf_clip::trim_fastq(t.get(), t.n, false, nullptr, 0, 33, a.get(), off, side, 1, 1, 2, 10, out, used, recs, bad, &begin, &len, &st, &cs);
            CHECK(clause == pf_mask::CLAUSE_NONE && used <= cut && begin.size() == recs && len.size() == recs);
            if (cut == text.size()) {
                CHECK(recs == 3 && len[0] == 40 && len[1] == 50 && len[2] == 0 && st.kept == 2 && st.dropped == 1 && st.bases == 167 && st.bases_kept == 90);
                CHECK(cs.reads_clipped[0] == 1 && cs.reads_dropped[0] == 1 && cs.bases_clipped[0] == 30 + 47 && cs.reads_clipped[1] == 0);
                CHECK(out == "@a\n" + r0.substr(0, 40) + "\n+\n" + std::string(40, 'I') + "\n@b\n" + r1 + "\n+\n" + std::string(50, 'I') + "\n");
            }
        }
    }
}

int main() {
    hand();
    edge_reads();
    files();
    chunk();
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
