// The rule of `ploidyfrost run STEP...` (K-TRIMCOUNT) in one place, for the device form (pf_trimcount.hip), the host restatement and
// the stand-alone test (tests/cpp/test_trimrun_rule.cpp): which bytes of a chunk of raw FASTQ go on to K-COUNT and K-MASKCOUNT when
// step `1.trim` of the reference's workflow is folded into `run`.  `2.kmc_db` lists `${i}*trim*.fq.gz`, which matches trim1 and
// trim2 only: the reads of pairs of which BOTH records were kept.  The unpaired survivors (u1, u2) are never counted.
//
//   hand-on    Given a chunk (or one chunk of each file of a pair), K-TRIM's steps and phred: the reads handed on are the sequence
//              bytes [seq_begin + b, seq_begin + e) of every whole record that pf_trim::trim_read keeps with the interval [b, e).
//              For a pair, record r of a file is handed on only when record r of BOTH files is kept (handed_on below).
//   order      record order.
//   table      they form a reads table (read_off, read_len) as pf_count_reads / pf_maskcount_reads take it: ascending, no overlaps
//              (a sub-interval of a sequence line lies inside that line, and the lines of a file ascend and do not overlap).  A pair
//              has one table per file, over that file's own text.
// K-COUNT's rule (pf_count_rule.hpp) and K-MASKCOUNT's (pf_run_rule.hpp) then apply to that table unchanged.
//
// pf_run_rule.hpp's argument still holds.  It needs one thing of the table: the window starts of two different reads are at least k
// apart.  A read here is [o + b, o + e) of a sequence line [o, o + n), 0 <= b < e <= n; its last window start is o + e - k, and the
// first start of any later read is at or beyond the later line's begin, which is beyond o + n >= o + e (a line end and three more
// lines lie between).  So a later read's q >= end_A >= p + k and an earlier read's q <= end_B - k <= begin_A - k <= p - k for every
// start p of read A, exactly as there: sub-intervals of different sequence lines only move the reads further apart.
//
// THE HAZARD.  A window that starts in [e - k + 1, e) or before b of the untrimmed read is NOT A WINDOW.  It is neither counted nor
// flagged bad: its position carries no bit of the window-start bitmap, so K-MASK's flag phase never looks it up and the bad bitmap
// holds 0 there.  A low-count k-mer in the trimmed-off tail (a sequencing error at a low-quality base, the usual reason the tail was
// trimmed) must not mask its neighbours: bad bits come from the starts of the TABLE's reads only, never from the sequence line.
// The trimmed text of `trim` followed by `run` has no such window either -- the bytes are not in the file.
//
// Statistics are two sets.  Trimming: pf_trim_stats per file, exactly what pf_trim_fastq / pf_trim_fastq_pair report for the chunk
// (every whole record taken, kept or not; the pair fields).  Counting: pf_count_stats / pf_maskcount_stats exactly as pf_count_fastq /
// pf_maskcount_fastq report them on the trimmed text: `reads` and `bases` are of the reads handed on.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pf_mask_rule.hpp"
#include "pf_trim_rule.hpp"

namespace pf_trimrun {

// is the record of a file handed on?  kept: that record's own outcome; other_kept: the outcome of the same record of the other file
// of a pair (single-ended: true)
PF_TRIM_HD inline bool handed_on(bool kept, bool other_kept) { return kept && other_kept; }

// the refusal of a pair beyond pf_mask's clauses: final chunks with different whole-record counts
constexpr int CLAUSE_PAIR_COUNT = pf_mask::CLAUSE_COUNT_;
inline const char *clause_text(int c) {
    return c == CLAUSE_PAIR_COUNT ? "the final chunks hold different numbers of records" : pf_mask::clause_text(c);
}

// ---- the host's plain restatement (no device): what the kernels are held to ----
// One file of a chunk whose index has been accepted: every record r < n_records trimmed; keep[r], and its interval as (off, len) of
// the text (len 0 = dropped).  stats: what pf_trim_fastq reports (the pair fields stay 0).
inline void trim_records(const char *text, uint64_t bytes, uint64_t n_records, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred,
                         std::vector<uint64_t> &off, std::vector<uint32_t> &len, pf_trim::Stats &stats) {
    std::vector<uint64_t> lb, le;
    pf_trim::record_lines(text, bytes, n_records, lb, le);
    off.assign(n_records, 0);
    len.assign(n_records, 0);
    stats = pf_trim::Stats{};
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t nq = (uint32_t)(le[4 * r + 3] - lb[4 * r + 3]);
        uint32_t b = 0, e = 0;
        const bool kept = pf_trim::trim_read(text + lb[4 * r + 3], nq, steps, n_steps, phred, b, e);
        off[r] = lb[4 * r + 1] + b;
        len[r] = e - b;
        stats.reads += 1;
        stats.kept += kept;
        stats.dropped += !kept;
        stats.bases += nq;
        stats.bases_kept += e - b;
    }
}

// One chunk of a single-ended file: the chunk contract and the format clauses of pf_trim_fastq (pf_mask::index_fastq's clause is
// returned with bad_record, and nothing is handed on then).  read_off / read_len: the table of the reads handed on.
inline int reads_table(const char *text, uint64_t n, bool final, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred,
                       std::vector<uint64_t> &read_off, std::vector<uint32_t> &read_len, uint64_t &bytes_used, uint64_t &n_records, uint64_t &bad_record,
                       pf_trim::Stats *stats = nullptr) {
    read_off.clear();
    read_len.clear();
    if (stats) *stats = pf_trim::Stats{};
    const int clause = pf_mask::index_fastq(text, n, final, bytes_used, n_records, bad_record);
    if (clause) { bytes_used = 0; n_records = 0; return clause; }
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    pf_trim::Stats st;
    trim_records(text, bytes_used, n_records, steps, n_steps, phred, off, len, st);
    for (uint64_t r = 0; r < n_records; ++r)
        if (handed_on(len[r] != 0, true)) { read_off.push_back(off[r]); read_len.push_back(len[r]); }
    if (stats) *stats = st;
    return pf_mask::CLAUSE_NONE;
}

// One chunk of each file of a pair: pf_trim_fastq_pair's contract.  Both chunks are indexed (file 1 first: its clause wins), n = the
// smaller whole-record count is taken from each, bytes_used[f] = the end of record n - 1 of file f; final chunks with different counts
// are CLAUSE_PAIR_COUNT.  bad_record = 2 * record + file.  read_off[f] / read_len[f]: the table of file f over text f; both tables
// have the same number of entries, entry i of both being the two records of one pair.
inline int reads_table_pair(const char *const text[2], const uint64_t n[2], bool final, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred,
                            std::vector<uint64_t> read_off[2], std::vector<uint32_t> read_len[2], uint64_t bytes_used[2], uint64_t &n_records,
                            uint64_t &bad_record, pf_trim::Stats stats[2] = nullptr) {
    n_records = 0;
    bad_record = 0;
    uint64_t used[2] = {0, 0}, recs[2] = {0, 0};
    std::vector<uint64_t> seq_off[2];
    for (int f = 0; f < 2; ++f) {
        read_off[f].clear();
        read_len[f].clear();
        bytes_used[f] = 0;
        if (stats) stats[f] = pf_trim::Stats{};
    }
    for (int f = 0; f < 2; ++f) {
        uint64_t bad = 0;
        const int clause = pf_mask::index_fastq(text[f], n[f], final, used[f], recs[f], bad, &seq_off[f]);
        if (clause) { bad_record = 2 * bad + (uint64_t)f; return clause; }
    }
    const uint64_t m = std::min(recs[0], recs[1]);
    if (final && recs[0] != recs[1]) { bad_record = 2 * m + (recs[0] < recs[1] ? 0 : 1); return CLAUSE_PAIR_COUNT; }
    if (m == 0) return pf_mask::CLAUSE_NONE;   // no whole record of both files: everything is carried
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> len[2];
    pf_trim::Stats st[2];
    for (int f = 0; f < 2; ++f) {
        if (m < recs[f]) {   // the end of record m - 1: the begin of record m's header line
            std::vector<uint64_t> lb, le;
            pf_trim::record_lines(text[f], used[f], m + 1, lb, le);
            used[f] = lb[4 * m];
        }
        trim_records(text[f], used[f], m, steps, n_steps, phred, off[f], len[f], st[f]);
    }
    for (uint64_t r = 0; r < m; ++r) {
        const bool k1 = len[0][r] != 0, k2 = len[1][r] != 0;
        st[0].both += k1 && k2;
        st[0].only1 += k1 && !k2;
        st[0].only2 += !k1 && k2;
        st[0].neither += !k1 && !k2;
        for (int f = 0; f < 2; ++f)
            if (handed_on(f == 0 ? k1 : k2, f == 0 ? k2 : k1)) { read_off[f].push_back(off[f][r]); read_len[f].push_back(len[f][r]); }
    }
    st[1].both = st[0].both; st[1].only1 = st[0].only1; st[1].only2 = st[0].only2; st[1].neither = st[0].neither;
    for (int f = 0; f < 2; ++f) {
        bytes_used[f] = used[f];
        if (stats) stats[f] = st[f];
    }
    n_records = m;
    return pf_mask::CLAUSE_NONE;
}

}  // namespace pf_trimrun
