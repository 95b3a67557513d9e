// Stand-alone check of palindrome mode in ploidyfrost_amd/csrc/pf_clip_rule.hpp: the shared header alone, plain host C++, built with
// -fsanitize=address,undefined by tests/test_clip_pair_cpu.py.  Every buffer the rule reads is a heap block of exactly the size it
// is given (reads, quality lines, prefix pairs, adapter files, FASTQ chunks), so a read one byte beyond any of them is reported.  Pairs
// of the edge grid (read lengths x prefix lengths x planted insert lengths) against a second, deliberately naive statement of the
// rule built on the strings S1 and S2 themselves; adapter files with prefix pairs cut at every byte; the refusals; the chunk
// restatement on a small pair of texts.
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

static uint64_t rng_state = 1442695040888963407ull;
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
static std::string revcomp(const std::string &s) {
    std::string r;
    for (size_t i = s.size(); i-- > 0;) {
        const char c = s[i];
        r.push_back(c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c == 'a' ? 't' : c == 'c' ? 'g' : c == 'g' ? 'c' : c == 't' ? 'a' : c);
    }
    return r;
}

// the rule once more, as naively as it reads: S1 and S2 built, every window counted from scratch, the best sub-range by Kadane over
// a vector of values; no early end -- the candidates beyond a passing one are left out of the count afterwards
struct Naive { bool found; long I; unsigned long scored; };
static Naive naive_pair(const std::string &r1, const std::string &q1, const std::string &r2, const std::string &q2,
                        const std::vector<std::pair<std::string, std::string>> &pairs, unsigned seed, unsigned Tp, unsigned A, int phred) {
    Naive out = {false, 0, 0};
    const long n1 = (long)r1.size(), n2 = (long)r2.size();
    if (n1 > 1024 || n2 > 1024) return out;
    long limit = (n1 < n2 ? n1 : n2) - (long)A + 1;
    auto code = [](char c) { c = (char)(c & 0xDF); return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; };
    for (const auto &pp : pairs) {
        const long p = (long)pp.first.size();
        const std::string S1 = pp.first + r1, S2 = pp.second + r2;
        for (long I = 0; I < limit; ++I) {
            const long T = 2 * p + I, lo = p + I - n2 > 0 ? p + I - n2 : 0, hi = T < p + n1 ? T : p + n1;
            if (hi - lo < 16) continue;
            std::vector<int> no_match;
            std::vector<long> value;
            for (long i = lo; i < hi; ++i) {
                const long j = T - 1 - i;
                const int a = code(S1[(size_t)i]), b = code(S2[(size_t)j]);
                const bool valid = a >= 0 && b >= 0, match = valid && a + b == 3;
                no_match.push_back(!match);
                long v = 0;
                if (match) v = 60206;
                else if (valid) {
                    int q = 1 << 20;
                    if (i >= p) q = (int)(unsigned char)q1[(size_t)(i - p)] - phred;
                    if (j >= p) { const int qq = (int)(unsigned char)q2[(size_t)(j - p)] - phred; if (qq < q) q = qq; }
                    v = -10000L * (q > 0 ? q : 0);
                }
                value.push_back(v);
            }
            bool seed_ok = false;
            for (size_t w = 0; w + 16 <= no_match.size(); ++w) {
                unsigned mm = 0;
                for (size_t x = w; x < w + 16; ++x) mm += (unsigned)no_match[x];
                if (mm <= seed) seed_ok = true;
            }
            if (!seed_ok) continue;
            ++out.scored;
            long run = 0, top = 0;
            for (long v : value) { run = run + v > 0 ? run + v : 0; if (run > top) top = run; }
            if (top >= 100000L * (long)Tp) { out.found = true; out.I = I; limit = I; break; }
        }
    }
    return out;
}

static void check_pair(const std::string &r1, const std::string &q1, const std::string &r2, const std::string &q2,
                       const std::vector<std::pair<std::string, std::string>> &pairs, unsigned seed, unsigned Tp, unsigned A, bool keep_both, int phred) {
    const Exact s1(r1), e1(q1), s2(r2), e2(q2);
    std::string pb;
    std::vector<uint32_t> poff = {0};
    for (const auto &pp : pairs) {
        pb += pp.first;
        poff.push_back((uint32_t)pb.size());
        pb += pp.second;
        poff.push_back((uint32_t)pb.size());
    }
    const Exact pbx(pb);
    pf_clip::PairSet P;
    P.prefix_bases = pbx.get();
    P.prefix_off = poff.data();
    P.n_pairs = (uint32_t)pairs.size();
    P.pair_score = Tp;
    P.pair_min = A;
    P.keep_both = keep_both;
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pbx.get(), poff.data(), P.n_pairs, seed, 10, Tp, A) == pf_clip::REFUSE_NONE);
    uint32_t end[2] = {7, 7};
    pf_clip::Stats cs = {};
    pf_clip::PairStats ps = {};
    pf_clip::clip_pair(s1.get(), e1.get(), (uint32_t)r1.size(), s2.get(), e2.get(), (uint32_t)r2.size(), nullptr, nullptr, nullptr, 0, P, seed, 10,
                       (uint32_t)phred, end, &cs, &ps);
    const Naive want = naive_pair(r1, q1, r2, q2, pairs, seed, Tp, A, phred);
    const uint32_t w1 = want.found ? (uint32_t)want.I : (uint32_t)r1.size(), w2 = want.found ? (keep_both ? (uint32_t)want.I : 0u) : (uint32_t)r2.size();
    CHECK(end[0] == w1 && end[1] == w2);
    CHECK(ps.candidates_scored == want.scored);
    CHECK(ps.pairs_clipped == (uint64_t)(want.found && want.I != 0) && ps.pairs_dropped == (uint64_t)(want.found && want.I == 0));
    CHECK(ps.pairs_too_long == (uint64_t)(r1.size() > 1024 || r2.size() > 1024));
    CHECK(ps.bases_clipped[0] == r1.size() - w1 && ps.bases_clipped[1] == r2.size() - w2);
    CHECK(cs.bases_clipped[0] == r1.size() - w1 && cs.bases_clipped[1] == r2.size() - w2);
}

static void read_through(size_t n1, size_t n2, size_t I, const std::string &P1, const std::string &P2, std::string &r1, std::string &r2) {
    const std::string ins = bases(I);
    r1 = (ins + revcomp(P2) + bases(n1)).substr(0, n1);
    r2 = (revcomp(ins) + revcomp(P1) + bases(n2)).substr(0, n2);
}

static void edge_grid() {
    const size_t read_lengths[] = {0, 1, 15, 16, 17, 100, 255, 256, 257, 1024, 1025}, prefix_lengths[] = {16, 33, 34, 64, 65, 128};
    unsigned long found = 0, untouched = 0;
    for (size_t p : prefix_lengths) {
        const std::vector<std::pair<std::string, std::string>> pairs = {{bases(p), bases(p)}};
        for (size_t k = 0; k < 11; ++k)
            for (int other = 0; other < 2; ++other) {
                const size_t n1 = read_lengths[k], n2 = other ? read_lengths[(k + 10) % 11] : n1, m = n1 < n2 ? n1 : n2;
                const size_t inserts[] = {0, 1, m >= 8 ? m - 8 : 0, m >= 7 ? m - 7 : 0};
                for (size_t I : inserts) {
                    if (I > m) continue;
                    std::string r1, r2;
                    read_through(n1, n2, I, pairs[0].first, pairs[0].second, r1, r2);
                    std::string q1(n1, 'I'), q2(n2, 'I');
                    for (size_t x = 0; x < n1; x += 7) q1[x] = (char)(33 + rnd() % 60);
                    if (n1 > 40 && (rnd() & 1)) r1[rnd() % n1] = 'N';
                    if (rnd() & 1) for (char &c : r2) c = (char)(c | 0x20);
                    if (n1 > 20 && (rnd() & 1)) r1[rnd() % n1] = "ACGT"[rnd() & 3];
                    check_pair(r1, q1, r2, q2, pairs, 2, 30, 8, (rnd() & 1) != 0, 33);
                    if (m <= 300) {
                        check_pair(r1, q1, r2, q2, pairs, 0, 1, 1, true, 64);
                        check_pair(r1, q1, r2, q2, pairs, 8, 100, 16, false, 33);
                    }
                    const Naive w = naive_pair(r1, q1, r2, q2, pairs, 2, 30, 8, 33);
                    found += w.found;
                    untouched += !w.found;
                }
            }
    }
    CHECK(found > 100 && untouched > 100);
    // two prefix pairs: the later one gives the smaller I
    const std::vector<std::pair<std::string, std::string>> two = {{bases(34), bases(34)}, {bases(40), bases(40)}};
    std::string r1, r2;
    read_through(90, 90, 30, two[1].first, two[1].second, r1, r2);
    check_pair(r1, std::string(90, 'I'), r2, std::string(90, 'I'), two, 2, 30, 8, false, 33);
    CHECK(naive_pair(r1, std::string(90, 'I'), r2, std::string(90, 'I'), two, 2, 30, 8, 33).I == 30);
}

static std::string pair_file(const std::vector<std::pair<std::string, std::string>> &pairs, const std::string &tail) {
    std::string t;
    for (size_t q = 0; q < pairs.size(); ++q)
        t += ">PrefixPE" + std::to_string(q) + "/1\n" + pairs[q].first + "\r\n>PrefixPE" + std::to_string(q) + "/2 words\n" + pairs[q].second.substr(0, 10) + "\n" +
             pairs[q].second.substr(10) + "\n";
    return t + tail;
}

static void adapter_files() {
    const std::vector<std::pair<std::string, std::string>> pairs = {{bases(34), bases(34)}, {bases(16), bases(16)}};
    const std::string whole = pair_file(pairs, ">plain\n" + bases(20) + "\n>other/2\n" + bases(30) + "\n");
    pf_clip::Adapters A;
    uint64_t bad = 0;
    {
        const Exact t(whole);
        CHECK(pf_clip::parse_adapters(t.get(), t.n, A, &bad, true) == pf_clip::REFUSE_NONE);
        CHECK(A.pairs() == 2 && A.size() == 2 && A.skipped == 0);
        CHECK(A.prefix_bases == pairs[0].first + pairs[0].second + pairs[1].first + pairs[1].second);
        CHECK(A.prefix_off.size() == 5 && A.prefix_off[1] == 34 && A.prefix_off[2] == 68 && A.prefix_off[3] == 84 && A.prefix_off[4] == 100);
        CHECK(pf_clip::parse_adapters(t.get(), t.n, A, &bad, false) == pf_clip::REFUSE_NONE && A.skipped == 4 && A.pairs() == 0 && A.size() == 2);
    }
    for (size_t cut = 0; cut <= whole.size(); ++cut) {   // every prefix of the file, in a block of exactly its size: parsed or refused, never overrun
        const Exact t(whole.substr(0, cut));
        const int c = pf_clip::parse_adapters(t.get(), t.n, A, &bad, true);
        CHECK(c >= 0 && c < pf_clip::REFUSE_COUNT_);
        if (c) CHECK(A.pairs() == 0 && A.size() == 0);
    }
    auto refusal = [&](const std::string &text, uint64_t *record) {
        const Exact t(text);
        return pf_clip::parse_adapters(t.get(), t.n, A, record, true);
    };
    const std::string b34 = bases(34), b20 = bases(20);
    CHECK(refusal(">PrefixPE/1\n" + b34 + "\n", &bad) == pf_clip::REFUSE_PAIR_PARTNER && bad == 1);
    CHECK(refusal(">a\n" + b20 + "\n>PrefixPE/2\n" + b34 + "\n>b\n" + b20 + "\n", &bad) == pf_clip::REFUSE_PAIR_PARTNER && bad == 2);
    CHECK(refusal(">PrefixPE\n" + b34 + "\n", &bad) == pf_clip::REFUSE_PAIR_PARTNER && bad == 1);
    CHECK(refusal(">PrefixPE/1\n" + b34 + "\n>PrefixPE/1\n" + b34 + "\n", &bad) == pf_clip::REFUSE_PAIR_PARTNER && bad == 2);
    CHECK(refusal(">PrefixPE/1\n" + b34 + "\n>PrefixPE/2\n" + b20 + "\n", &bad) == pf_clip::REFUSE_PAIR_LENGTHS && bad == 2);
    CHECK(refusal(">PrefixPE/1\n" + bases(15) + "\n>PrefixPE/2\n" + bases(15) + "\n", &bad) == pf_clip::REFUSE_LENGTH && bad == 1);
    CHECK(refusal(">PrefixPE/1\n" + b34 + "\n>PrefixPE/2\n" + bases(129) + "\n", &bad) == pf_clip::REFUSE_LENGTH && bad == 2);
    CHECK(refusal(">PrefixPE/1\n" + b34 + "\n>PrefixPE/2\n" + bases(33) + "N\n", &bad) == pf_clip::REFUSE_BYTE && bad == 2);
    CHECK(refusal(">a\n" + b20 + "\n", &bad) == pf_clip::REFUSE_NO_PAIR && bad == 0);
    CHECK(refusal("", &bad) == pf_clip::REFUSE_NOT_FASTA && bad == 0);
    std::vector<std::pair<std::string, std::string>> nine;
    for (int q = 0; q < 9; ++q) nine.push_back({bases(16), bases(16)});
    CHECK(refusal(pair_file(nine, ""), &bad) == pf_clip::REFUSE_TOO_MANY_PAIRS && bad == 18);
    nine.pop_back();
    CHECK(refusal(pair_file(nine, ""), &bad) == pf_clip::REFUSE_NONE && A.pairs() == 8 && A.size() == 0);
    // the set as the ABI takes it
    const uint32_t off[3] = {0, 34, 68}, uneven[3] = {0, 34, 67}, shortp[3] = {0, 15, 30};
    const std::string pb = bases(68);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 2, 10, 30, 8) == pf_clip::REFUSE_NONE);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 0, 2, 10, 30, 8) == pf_clip::REFUSE_NO_PAIR);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 9, 2, 10, 30, 8) == pf_clip::REFUSE_TOO_MANY_PAIRS);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), uneven, 1, 2, 10, 30, 8) == pf_clip::REFUSE_PAIR_LENGTHS);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), shortp, 1, 2, 10, 30, 8) == pf_clip::REFUSE_LENGTH);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 2, 10, 0, 8) == pf_clip::REFUSE_PAIR_SCORE);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 2, 10, 1001, 8) == pf_clip::REFUSE_PAIR_SCORE);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 2, 10, 30, 0) == pf_clip::REFUSE_PAIR_MIN);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 2, 10, 30, 17) == pf_clip::REFUSE_PAIR_MIN);
    CHECK(pf_clip::pair_set_clause(nullptr, nullptr, nullptr, 0, pb.data(), off, 1, 9, 10, 30, 8) == pf_clip::REFUSE_SEED);
    for (int r = 0; r < pf_clip::REFUSE_COUNT_; ++r) CHECK(strlen(pf_clip::refusal_text(r)) > 5);
}

static void chunks() {
    const std::vector<std::pair<std::string, std::string>> pairs = {{bases(34), bases(34)}};
    const std::string pb = pairs[0].first + pairs[0].second;
    const uint32_t poff[3] = {0, 34, 68};
    pf_clip::PairSet P;
    P.prefix_bases = pb.data();
    P.prefix_off = poff;
    P.n_pairs = 1;
    P.keep_both = true;
    std::string t[2];
    const size_t inserts[] = {40, 200, 0, 95};
    for (size_t r = 0; r < 4; ++r) {
        std::string r1, r2;
        read_through(100, 100, inserts[r], pairs[0].first, pairs[0].second, r1, r2);
        t[0] += "@p" + std::to_string(r) + "/1\n" + r1 + "\n+\n" + std::string(100, 'I') + "\n";
        t[1] += "@p" + std::to_string(r) + std::string(r, 'x') + "/2\n" + r2 + "\n+\n" + std::string(100, 'I') + "\n";
    }
    for (int cut2 = 0; cut2 < 2; ++cut2) {   // the whole chunks; then file 2 cut inside its last record, not final
        const std::string t2 = cut2 ? t[1].substr(0, t[1].size() - 30) : t[1];
        const Exact x1(t[0]), x2(t2);
        const char *text[2] = {x1.get(), x2.get()};
        const uint64_t n[2] = {x1.n, x2.n};
        std::string out[4];
        uint64_t used[2] = {0, 0}, recs = 0, bad = 0;
        std::vector<uint32_t> ce[2];
        std::vector<uint32_t> *pce[2] = {&ce[0], &ce[1]};
        pf_clip::PairStats ps = {};
        pf_clip::Stats cs = {};
        pf_trim::Stats st[2];
        const int c = pf_clip::trim_fastq_pair(text, n, cut2 == 0, nullptr, 0, 33, nullptr, nullptr, nullptr, 0, P, 2, 10, out, used, recs, bad, nullptr, nullptr, st,
                                               &cs, &ps, pce);
        CHECK(c == pf_mask::CLAUSE_NONE && recs == (cut2 ? 3u : 4u));
        CHECK(used[0] == (cut2 ? t[0].size() / 4 * 3 : t[0].size()));
        CHECK(ce[0].size() == recs && ce[0][0] == 40 && ce[1][0] == 40 && ce[0][1] == 100 && ce[0][2] == 0 && ce[1][2] == 0);
        if (!cut2) CHECK(ce[0][3] == 100 && ce[1][3] == 100);   // 5 adapter bases: below A = 8
        CHECK(ps.pairs_clipped == 1 && ps.pairs_dropped == 1 && st[0].both == (cut2 ? 2u : 3u) && st[0].neither == 1);
        CHECK(out[1].empty() && out[3].empty());
    }
    {   // final chunks of different record counts
        const std::string t2 = t[1].substr(0, t[1].size() / 4 * 3 + 5 - 5);
        const Exact x1(t[0]), x2(t2.substr(0, t2.find("@p3")));
        const char *text[2] = {x1.get(), x2.get()};
        const uint64_t n[2] = {x1.n, x2.n};
        std::string out[4];
        uint64_t used[2], recs = 0, bad = 0;
        CHECK(pf_clip::trim_fastq_pair(text, n, true, nullptr, 0, 33, nullptr, nullptr, nullptr, 0, P, 2, 10, out, used, recs, bad) == pf_clip::PAIR_COUNTS_DIFFER);
        CHECK(bad == 2 * 3 + 1 && recs == 0);
    }
}

int main() {
    edge_grid();
    adapter_files();
    chunks();
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
