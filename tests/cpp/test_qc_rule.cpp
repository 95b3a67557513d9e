// Stand-alone check of ploidyfrost_amd/csrc/pf_qc_rule.hpp: the shared header alone, plain host C++, built with
// -fsanitize=address,undefined by tests/test_qc_cpu.py.  Every text the rule reads is a heap block of exactly the size it is given, so
// a read one byte beyond a chunk is reported.  A text of edge and random records, final and not, cut at every length, with steps and
// with a clip open, against a second, deliberately naive count of the same tables; the hint; the report of an empty and a small table.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "pf_qc_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

// a heap copy of exactly n bytes (at least one block, so that the pointer is never null)
struct Exact {
    std::unique_ptr<char[]> p;
    size_t n;
    Exact(const std::string &s, size_t len) : p(new char[len ? len : 1]), n(len) { if (n) memcpy(p.get(), s.data(), n); }
    const char *get() const { return p.get(); }
};

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

struct Rec { std::string seq, qual; };
static std::string fastq(const std::vector<Rec> &recs, bool crlf) {
    std::string t;
    const char *nl = crlf ? "\r\n" : "\n";
    for (size_t i = 0; i < recs.size(); ++i) t += "@r" + std::to_string(i) + nl + recs[i].seq + nl + "+" + nl + recs[i].qual + nl;
    return t;
}
static Rec make(size_t n, uint32_t phred) {
    Rec r;
    for (size_t i = 0; i < n; ++i) {
        r.seq.push_back("ACGTacgtN."[rnd() % 10]);
        const uint32_t k = rnd() % 50;
        r.qual.push_back((char)(k == 0 ? phred - 1 : k == 1 ? 126 : phred + k % 42));
    }
    return r;
}

// the raw table of whole records, counted as naively as the rule reads: per word, from scratch
static std::vector<uint64_t> naive_raw(const std::vector<Rec> &recs, size_t n_recs, uint32_t phred) {
    using namespace pf_qc;
    std::vector<uint64_t> t(TABLE_WORDS, 0);
    if (!n_recs) return t;
    t[W_SEEN] = 1;
    uint64_t min_len = ~0ull, min_byte = ~0ull;
    for (size_t r = 0; r < n_recs; ++r) {
        const Rec &x = recs[r];
        const size_t L = x.seq.size();
        t[W_READS]++;
        t[W_LENGTH + (L < 1024 ? L : 1024)]++;
        if (L < min_len) min_len = L;
        if (L > t[W_MAX_LEN]) t[W_MAX_LEN] = L;
        long sum = 0, gc = 0, acgt = 0;
        for (size_t i = 0; i < L; ++i) {
            const size_t bin = i < 1023 ? i : 1023;
            const char u = (char)(x.seq[i] & 0xDF);
            const int cls = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
            const int byte = (unsigned char)x.qual[i], q = byte - (int)phred, qcl = q < 0 ? 0 : q > 93 ? 93 : q;
            t[W_POS_BASE + bin * 5 + (size_t)cls]++;
            t[W_POS_QSUM + bin] += (uint64_t)qcl;
            if (q >= 20) t[W_POS_Q20 + bin]++;
            if (q >= 30) t[W_POS_Q30 + bin]++;
            t[W_QUALITY + (size_t)qcl]++;
            if (q < 0) t[W_QUAL_LOW]++;
            if (q > 93) t[W_QUAL_HIGH]++;
            if ((uint64_t)byte < min_byte) min_byte = (uint64_t)byte;
            if ((uint64_t)byte > t[W_MAX_BYTE]) t[W_MAX_BYTE] = (uint64_t)byte;
            sum += qcl;
            acgt += cls < 4;
            gc += cls == 1 || cls == 2;
        }
        if (!L) continue;
        t[W_READ_QUALITY + (size_t)(sum / (long)L)]++;
        if (acgt) t[W_GC_PERCENT + (size_t)(100 * gc / acgt)]++; else t[W_READS_NO_ACGT]++;
    }
    t[W_MIN_LEN] = min_len;
    t[W_MIN_BYTE] = min_byte == ~0ull ? 0 : min_byte;
    return t;
}

int main() {
    using namespace pf_qc;
    CHECK(TABLE_WORDS == 9515 && CLIP_WORDS == 1025);
    CHECK(phred_hint(58, 1) == 33 && phred_hint(59, 1) == 0 && phred_hint(63, 1) == 0 && phred_hint(64, 1) == 64 && phred_hint(33, 0) == 0);
    CHECK(base_class('a') == 0 && base_class('C') == 1 && base_class('g') == 2 && base_class('T') == 3 && base_class('N') == 4 && base_class('.') == 4);
    CHECK(quality_clamped(-1) == 0 && quality_clamped(94) == 93 && pos_bin(1022) == 1022 && pos_bin(5000) == 1023 && len_bin(1023) == 1023 && len_bin(1u << 31) == 1024);

    const pf_trim::Step steps[3] = {{pf_trim::KIND_LEADING, 10, 0}, {pf_trim::KIND_SLIDINGWINDOW, 3, 20}, {pf_trim::KIND_MINLEN, 5, 0}};
    const std::string adapter = "ACGTTGCAAGGCTTAACCGGATCA";
    const uint32_t ad_off[2] = {0, (uint32_t)adapter.size()};
    const uint8_t ad_side[1] = {0};
    for (uint32_t phred : {33u, 64u})
        for (int crlf = 0; crlf < 2; ++crlf) {
            std::vector<Rec> recs;
            for (size_t n : {0u, 1u, 15u, 16u, 17u, 255u, 256u, 257u, 1022u, 1023u, 1024u, 1025u, 1500u}) recs.push_back(make(n, phred));
            Rec through = make(60, phred);   // a read that runs into the adapter at 30
            through.seq.replace(30, adapter.size(), adapter);
            for (size_t i = 0; i < through.qual.size(); ++i) through.qual[i] = (char)(phred + 35);
            recs.push_back(through);
            const std::string text = fastq(recs, crlf != 0);
            // whole text, final
            {
                Exact x(text, text.size());
                std::vector<uint64_t> raw(TABLE_WORDS, 0), kept(TABLE_WORDS, 0), clip(CLIP_WORDS, 0);
                uint64_t used = 0, n_rec = 0, bad = 0;
                ClipSet cs;
                cs.open = true;
                cs.bases = adapter.data();
                cs.off = ad_off;
                cs.side = ad_side;
                cs.n_adapters = 1;
                CHECK(qc_fastq_chunk(x.get(), x.n, true, phred, 1, true, steps, 3, cs, raw.data(), kept.data(), clip.data(), used, n_rec, bad) == 0);
                CHECK(n_rec == recs.size() && used == text.size());
                CHECK(raw == naive_raw(recs, recs.size(), phred));
                CHECK(clip[30] == 1 && kept[W_SEEN] == 1 && kept[W_READS] <= raw[W_READS] && kept[W_MAX_LEN] <= raw[W_MAX_LEN]);
                std::vector<uint64_t> all(4 * (size_t)TABLE_WORDS, 0);
                std::copy(raw.begin(), raw.end(), all.begin());
                std::copy(kept.begin(), kept.end(), all.begin() + TABLE_WORDS);
                std::vector<uint64_t> clips(2 * (size_t)CLIP_WORDS, 0);
                std::copy(clip.begin(), clip.end(), clips.begin());
                const std::string rep = report_text(all.data(), clips.data(), phred);
                CHECK(rep.compare(0, 19, "# ploidyfrost qc 1\n") == 0 && rep.find(">>clip\nside\tclip_end\treads\n1\t30\t1\n") != std::string::npos);
                CHECK(rep.find("\t1023+\t") != std::string::npos && rep.find("\t1024+\t") != std::string::npos);
                CHECK(!side_line(0, raw.data()).empty());
            }
            // cut at every length of the last two records (and a few earlier ones), not final: whole records only, nothing read beyond the cut
            const size_t tail = fastq(std::vector<Rec>(recs.begin(), recs.end() - 2), crlf != 0).size();
            for (size_t cut = 0; cut <= text.size(); cut = cut < 200 || cut >= tail ? cut + 1 : tail) {
                Exact x(text, cut);
                std::vector<uint64_t> raw(TABLE_WORDS, 0), kept(TABLE_WORDS, 0), clip(CLIP_WORDS, 0);
                uint64_t used = 0, n_rec = 0, bad = 0;
                CHECK(qc_fastq_chunk(x.get(), x.n, false, phred, 2, true, steps, 3, ClipSet{}, raw.data(), kept.data(), clip.data(), used, n_rec, bad) == 0);
                CHECK(used <= cut && n_rec <= recs.size());
                CHECK(raw == naive_raw(recs, (size_t)n_rec, phred));
            }
        }
    // an untouched table: all zero, an empty report with every section
    {
        std::vector<uint64_t> all(4 * (size_t)TABLE_WORDS, 0);
        const std::string rep = report_text(all.data(), nullptr, 33);
        CHECK(rep.find("# phred 33 hint 0\n>>totals\n") != std::string::npos && rep.find(">>gc_percent\nside\tstage\tgc_percent\treads\n>>clip\nside\tclip_end\treads\n") != std::string::npos);
        CHECK(hint_line(all.data(), 33).empty());
    }
    // phred-64 bytes under offset 33: the warning
    {
        std::vector<uint64_t> all(4 * (size_t)TABLE_WORDS, 0);
        const std::string text = "@r\nACGT\n+\nhhhe\n";
        Exact x(text, text.size());
        std::vector<uint64_t> clip(CLIP_WORDS, 0);
        uint64_t used = 0, n_rec = 0, bad = 0;
        CHECK(qc_fastq_chunk(x.get(), x.n, true, 33, 1, false, nullptr, 0, ClipSet{}, all.data(), all.data() + TABLE_WORDS, clip.data(), used, n_rec, bad) == 0);
        CHECK(hint_of(all.data()) == 64);
        CHECK(hint_line(all.data(), 33) == "qc: quality bytes run from 101 to 104: the files look like phred 64, not 33");
        CHECK(hint_line(all.data(), 64).empty());
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
