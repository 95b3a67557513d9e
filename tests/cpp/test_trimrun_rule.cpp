// Stand-alone test of csrc/pf_trimrun_rule.hpp: the hand-on rule of `ploidyfrost run STEP...` and its host restatement against an
// independent walk over the same chunk (pf_trim::trim_fastq's kept records, re-indexed), the pair's both-kept rule, the chunk contract
// of pairs with different record counts, and the hazard: a window of the trimmed-off tail is no window for pf_run::count_masked_host.
// Plain g++ with the sanitizers; no device.  Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "pf_count_rule.hpp"
#include "pf_mask_rule.hpp"
#include "pf_run_rule.hpp"
#include "pf_trim_rule.hpp"
#include "pf_trimrun_rule.hpp"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            exit(1);                                                     \
        }                                                                \
    } while (0)

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

std::vector<pf_trim::Step> steps_of(std::initializer_list<const char *> words) {
    std::vector<const char *> w(words);
    std::vector<pf_trim::Step> s;
    CHECK(pf_trim::parse_steps(w.data(), w.size(), s) == pf_trim::REFUSE_NONE);
    return s;
}

// a record with the given sequence and qualities (phred 33)
void record(std::string &out, const std::string &name, const std::string &seq, const std::vector<int> &q, bool crlf = false) {
    const char *nl = crlf ? "\r\n" : "\n";
    std::string qual;
    for (int x : q) qual.push_back((char)(x + 33));
    out += "@" + name + nl + seq + nl + "+" + nl + qual + nl;
}

std::string random_file(Rng &r, int n_records, bool crlf) {
    std::string out;
    for (int i = 0; i < n_records; ++i) {
        const uint32_t n = r.below(90);
        std::string seq;
        std::vector<int> q;
        const uint32_t shape = r.below(4), head = r.below(12), cut = n ? r.below(n) : 0;
        for (uint32_t j = 0; j < n; ++j) {
            seq.push_back("ACGTN"[r.below(40) ? r.below(4) : 4]);
            q.push_back(shape == 0 ? 36 : shape == 1 ? 2 + (int)r.below(39) : shape == 2 ? (j < cut ? 36 : 2 + (int)r.below(20)) : (j < head || j + 9 > n ? 2 : 36));
        }
        record(out, "r" + std::to_string(i) + std::string(i % 5, 'x'), seq, q, crlf);
    }
    return out;
}

// the reads of a trimmed FASTQ text, as bytes
std::vector<std::string> reads_of(const std::string &fq) {
    uint64_t used = 0, recs = 0, bad = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    CHECK(pf_mask::index_fastq(fq.data(), fq.size(), true, used, recs, bad, &off, &len) == 0);
    std::vector<std::string> out;
    for (uint64_t i = 0; i < recs; ++i) out.push_back(fq.substr(off[i], len[i]));
    return out;
}

void check_single(const std::string &text, bool final, const std::vector<pf_trim::Step> &st, uint32_t phred = 33) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint64_t used = 0, recs = 0, bad = 0;
    pf_trim::Stats ts;
    CHECK(pf_trimrun::reads_table(text.data(), text.size(), final, st.data(), (uint32_t)st.size(), phred, off, len, used, recs, bad, &ts) == 0);
    // against pf_trim::trim_fastq: the same chunk contract, the same statistics, and the sequence lines of its output
    std::string trimmed;
    uint64_t used2 = 0, recs2 = 0, bad2 = 0;
    pf_trim::Stats ts2;
    CHECK(pf_trim::trim_fastq(text.data(), text.size(), final, st.data(), (uint32_t)st.size(), phred, trimmed, used2, recs2, bad2, nullptr, nullptr, &ts2) == 0);
    CHECK(used == used2 && recs == recs2);
    CHECK(ts.reads == ts2.reads && ts.kept == ts2.kept && ts.dropped == ts2.dropped && ts.bases == ts2.bases && ts.bases_kept == ts2.bases_kept);
    const std::vector<std::string> want = reads_of(trimmed);
    CHECK(want.size() == off.size() && off.size() == len.size() && off.size() == ts.kept);
    for (size_t i = 0; i < off.size(); ++i) {
        CHECK(len[i] > 0 && off[i] + len[i] <= used);
        CHECK(text.substr(off[i], len[i]) == want[i]);
        if (i) CHECK(off[i - 1] + len[i - 1] < off[i]);   // ascending, no overlaps (a line end lies between)
    }
}

void test_single() {
    Rng r{11};
    const auto workflow = steps_of({"LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20", "MINLEN:50"});
    const auto other = steps_of({"SLIDINGWINDOW:3:20", "LEADING:10", "TRAILING:10", "MINLEN:5"});
    for (int round = 0; round < 6; ++round) {
        const std::string text = random_file(r, 120, round == 3);
        check_single(text, true, round % 2 ? other : workflow);
        check_single(text.substr(0, text.find_last_not_of("\r\n") + 1), true, other);   // a last line without its line end
        check_single(text.substr(0, text.size() * 2 / 3 + 1), false, other);        // a chunk that ends inside a record
    }
    check_single("", true, workflow);
    // phred 64
    std::string t64;
    t64 += "@a\nACGTACGT\n+\n";
    for (int x : {2, 2, 40, 40, 40, 40, 2, 40}) t64.push_back((char)(x + 64));
    t64 += "\n";
    check_single(t64, true, steps_of({"LEADING:10", "TRAILING:10"}), 64);
    // a format error is handed back with its record, and nothing is handed on
    std::string bad = random_file(r, 5, false);
    bad[bad.find("@r2")] = '#';
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint64_t used = 7, recs = 7, rec = 0;
    CHECK(pf_trimrun::reads_table(bad.data(), bad.size(), true, workflow.data(), (uint32_t)workflow.size(), 33, off, len, used, recs, rec) == pf_mask::CLAUSE_HEADER);
    CHECK(rec == 2 && used == 0 && recs == 0 && off.empty());
}

void test_by_hand() {
    // three records, k = 3.  LEADING:10 TRAILING:10: [2, 7) of AAACGTACC, dropped, [0, 4) of GGTTA
    std::string text;
    record(text, "a", "AAACGTACC", {2, 2, 30, 30, 30, 30, 30, 2, 2});
    record(text, "b", "ACGT", {2, 2, 2, 2});
    record(text, "c", "GGTTA", {30, 30, 30, 30, 2});
    const auto st = steps_of({"LEADING:10", "TRAILING:10"});
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint64_t used = 0, recs = 0, bad = 0;
    pf_trim::Stats ts;
    CHECK(pf_trimrun::reads_table(text.data(), text.size(), true, st.data(), 2, 33, off, len, used, recs, bad, &ts) == 0);
    CHECK(recs == 3 && used == text.size() && off.size() == 2 && ts.kept == 2 && ts.dropped == 1 && ts.bases == 18 && ts.bases_kept == 9);
    CHECK(text.substr(off[0], len[0]) == "ACGTA" && text.substr(off[1], len[1]) == "GGTT");
    CHECK(off[0] == 3 + 2);   // "@a\n" then b = 2
    // the hazard at k = 3: the window starts of the table get counter 9, every other position of the text counter 0.  A rule that
    // looked beyond [b, e) would find bad windows there (the trimmed-off head and tail of record a, the tail of c) and mask their
    // neighbours; the rule looks at the table's starts alone and keeps all five windows
    std::vector<uint32_t> counters(text.size(), 0);
    for (size_t i = 0; i < off.size(); ++i)
        for (uint32_t p = 0; p + 3 <= len[i]; ++p) counters[off[i] + p] = 9;
    pf_count::Table table;
    pf_run::Stats rs;
    pf_run::count_masked_host(text.data(), off.data(), len.data(), off.size(), 3, counters.data(), 1, 0xFFFFFFFFu, table, rs);
    CHECK(rs.reads == 2 && rs.bases == 9 && rs.kmers == 3 + 2 && rs.kmers_bad == 0 && rs.kmers_invalid == 0 && rs.kmers_kept == 5);
    // the untrimmed sequence lines under the same counters: the windows of the tails are bad and take their neighbours with them
    std::vector<uint64_t> loff;
    std::vector<uint32_t> llen;
    CHECK(pf_mask::index_fastq(text.data(), text.size(), true, used, recs, bad, &loff, &llen) == 0);
    pf_count::Table t2;
    pf_run::Stats r2;
    pf_run::count_masked_host(text.data(), loff.data(), llen.data(), loff.size(), 3, counters.data(), 1, 0xFFFFFFFFu, t2, r2);
    CHECK(r2.kmers_bad > 0 && r2.kmers_kept < 5);
}

void test_pair() {
    Rng r{23};
    const auto st = steps_of({"LEADING:10", "TRAILING:10", "SLIDINGWINDOW:3:20", "MINLEN:20"});
    const std::string f1 = random_file(r, 150, false), f2 = random_file(r, 150, true);
    const char *text[2] = {f1.data(), f2.data()};
    const uint64_t n[2] = {f1.size(), f2.size()};
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> len[2];
    uint64_t used[2], recs = 0, bad = 0;
    pf_trim::Stats ts[2];
    CHECK(pf_trimrun::reads_table_pair(text, n, true, st.data(), (uint32_t)st.size(), 33, off, len, used, recs, bad, ts) == 0);
    CHECK(recs == 150 && used[0] == n[0] && used[1] == n[1]);
    // each file by itself: its kept records; the pair hands on those kept in both
    std::vector<uint64_t> soff[2];
    std::vector<uint32_t> slen[2];
    pf_trim::Stats ss[2];
    for (int f = 0; f < 2; ++f) pf_trimrun::trim_records(text[f], n[f], 150, st.data(), (uint32_t)st.size(), 33, soff[f], slen[f], ss[f]);
    uint64_t both = 0, only1 = 0, only2 = 0, neither = 0, at = 0;
    for (uint64_t i = 0; i < 150; ++i) {
        const bool k1 = slen[0][i] != 0, k2 = slen[1][i] != 0;
        both += k1 && k2; only1 += k1 && !k2; only2 += !k1 && k2; neither += !k1 && !k2;
        CHECK(pf_trimrun::handed_on(k1, k2) == (k1 && k2) && pf_trimrun::handed_on(k2, k1) == (k1 && k2));
        if (k1 && k2) {
            for (int f = 0; f < 2; ++f) CHECK(off[f][at] == soff[f][i] && len[f][at] == slen[f][i]);
            ++at;
        }
    }
    CHECK(both && only1 && only2 && neither);   // all four outcomes are in the input
    CHECK(at == both && off[0].size() == both && off[1].size() == both);
    for (int f = 0; f < 2; ++f)
        CHECK(ts[f].both == both && ts[f].only1 == only1 && ts[f].only2 == only2 && ts[f].neither == neither && ts[f].kept == ss[f].kept &&
              ts[f].bases_kept == ss[f].bases_kept && ts[f].reads == 150);
    // not final, file 1 holds more whole records: the smaller count is taken from each, bytes_used = the end of that record
    std::vector<uint64_t> lb1, lb2, le;
    pf_trim::record_lines(f1.data(), f1.size(), 150, lb1, le);
    pf_trim::record_lines(f2.data(), f2.size(), 150, lb2, le);
    {
        const uint64_t m[2] = {lb1[4 * 90] + 5, lb2[4 * 40] + 2};   // 90 and 40 whole records and a bit
        CHECK(pf_trimrun::reads_table_pair(text, m, false, st.data(), (uint32_t)st.size(), 33, off, len, used, recs, bad, ts) == 0);
        CHECK(recs == 40 && used[0] == lb1[4 * 40] && used[1] == lb2[4 * 40] && ts[0].reads == 40 && ts[1].reads == 40);
        CHECK(off[0].size() == off[1].size() && off[0].size() == ts[0].both);
        for (size_t i = 0; i < off[0].size(); ++i) CHECK(off[0][i] + len[0][i] <= used[0] && off[1][i] + len[1][i] <= used[1]);
    }
    {   // final chunks with different counts: refused with 2 * record + the file that ends first
        const uint64_t m[2] = {lb1[4 * 90], lb2[4 * 40]};
        CHECK(pf_trimrun::reads_table_pair(text, m, true, st.data(), (uint32_t)st.size(), 33, off, len, used, recs, bad, ts) == pf_trimrun::CLAUSE_PAIR_COUNT);
        CHECK(bad == 2 * 40 + 1 && recs == 0 && off[0].empty() && off[1].empty());
        CHECK(std::string(pf_trimrun::clause_text(pf_trimrun::CLAUSE_PAIR_COUNT)).find("different numbers of records") != std::string::npos);
    }
    // a format error in file 2 is reported as 2 * record + 1
    std::string broken = f2;
    broken[broken.find("@r3")] = '#';
    const char *t2[2] = {f1.data(), broken.data()};
    CHECK(pf_trimrun::reads_table_pair(t2, n, true, st.data(), (uint32_t)st.size(), 33, off, len, used, recs, bad, ts) == pf_mask::CLAUSE_HEADER);
    CHECK(bad == 2 * 3 + 1);
}

}  // namespace

int main() {
    test_single();
    test_by_hand();
    test_pair();
    printf("ok\n");
    return 0;
}
