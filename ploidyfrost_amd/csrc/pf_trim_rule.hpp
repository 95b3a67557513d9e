// The rule of `ploidyfrost trim` (K-TRIM) in one place, for the kernels (pf_trim.hip), the host layer (host/pf_trim_host.cpp, host/pf_reads_stream.cpp)
// and the stand-alone test (tests/cpp/test_trim_rule.cpp): the quality of a base, the four steps LEADING, TRAILING, SLIDINGWINDOW and
// MINLEN as Trimmomatic words them (step `1.trim` of the reference's workflow: `trimmomatic PE -phred33 ... LEADING:10 TRAILING:10
// SLIDINGWINDOW:3:20 MINLEN:50`), the parser of those words, and the refusals by name.
//
// A read is a quality line of n bytes; q[i] = (int)byte - phred, signed.  The state is a half-open interval [b, e) of the read,
// [0, n) at first, or "dropped"; the steps apply in the order given and a dropped read stays dropped.
//   LEADING:t           b = the smallest i of [b, e) with q[i] >= t; none: dropped
//   TRAILING:t          e = 1 + the largest such i; none: dropped
//   SLIDINGWINDOW:w:t   m = e - b < w: dropped.  Window j (0 <= j <= m - w) is bad when q[b+j] + ... + q[b+j+w-1] < w * t (integers:
//                       a sum of exactly w * t is good).  Window 0 bad: dropped; no bad window: unchanged; else with j the first bad
//                       window e = sliding_end(b, j, w) = b + j - 1 + w, the end of the last good window.
//   MINLEN:l            e - b < l: dropped
// and a read with e == b after the last step is dropped.
//
// PARITY UNPINNED: Trimmomatic is not part of the build.  The one place its documented wording ("cutting once the average quality
// within the window falls below a threshold") leaves open is the tail of SLIDINGWINDOW: whether bases below t are stripped from the
// end of the last good window as well (later versions may).  That is sliding_end() below and nothing else.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pf_mask_rule.hpp"

#if defined(__HIPCC__)
#define PF_TRIM_HD __host__ __device__
#else
#define PF_TRIM_HD
#endif

namespace pf_trim {

constexpr uint32_t MAX_STEPS = 8;
constexpr uint32_t MAX_T = 93, MAX_W = 64;

enum Kind { KIND_LEADING = 1, KIND_TRAILING = 2, KIND_SLIDINGWINDOW = 3, KIND_MINLEN = 4 };   // PF_TRIM_LEADING .. of ploidyfrost_hip.h
struct Step {            // pf_trim_step of ploidyfrost_hip.h
    uint32_t kind;
    uint32_t a;          // t of LEADING / TRAILING, w of SLIDINGWINDOW, l of MINLEN
    uint32_t b;          // t of SLIDINGWINDOW
};
struct Stats {           // pf_trim_stats of ploidyfrost_hip.h
    uint64_t reads, kept, dropped, bases, bases_kept;
    uint64_t both, only1, only2, neither;
};

// ---- the rule's pieces, shared with the kernels ----
PF_TRIM_HD inline int quality(uint8_t byte, uint32_t phred) { return (int)byte - (int)phred; }
PF_TRIM_HD inline bool base_good(uint8_t byte, uint32_t t, uint32_t phred) { return quality(byte, phred) >= (int)t; }
// a window of w qualities with the sum `sum_q`
PF_TRIM_HD inline bool window_bad(int64_t sum_q, uint32_t w, uint32_t t) { return sum_q < (int64_t)w * (int64_t)t; }
// the same from the sum of the window's bytes: sum_q = sum_bytes - w * phred
PF_TRIM_HD inline bool window_bad_bytes(uint32_t sum_bytes, uint32_t w, uint32_t t, uint32_t phred) { return sum_bytes < w * (t + phred); }
// the end of the read when window j (j >= 1, counted from b) is the first bad one: the end of window j - 1
PF_TRIM_HD inline uint32_t sliding_end(uint32_t b, uint32_t j, uint32_t w) { return b + j - 1 + w; }
PF_TRIM_HD inline bool too_short(uint32_t b, uint32_t e, uint32_t l) { return (uint64_t)(e - b) < (uint64_t)l; }

// ---- the refusals, each with the name it is refused by ----
enum Refusal {
    REFUSE_NONE = 0,
    REFUSE_UNKNOWN,    // a word that is none of the four steps (ILLUMINACLIP, CROP, lower case, ...)
    REFUSE_FIELD,      // a field that is missing, empty, not a number, or one too many
    REFUSE_RANGE,      // a value outside 0 <= t <= 93, 1 <= w <= 64, 0 <= l <= 2^32 - 1
    REFUSE_TOO_MANY,   // more than eight steps
    REFUSE_NO_STEP,    // no step at all
    REFUSE_PHRED,      // a quality offset other than 33 or 64
    REFUSE_COUNT_
};
inline const char *refusal_text(int r) {
    switch (r) {
        case REFUSE_UNKNOWN: return "unknown step (LEADING:t, TRAILING:t, SLIDINGWINDOW:w:t and MINLEN:l are known)";
        case REFUSE_FIELD: return "a field of the step is missing or is not a number";
        case REFUSE_RANGE: return "a value of the step is out of range (0 <= t <= 93, 1 <= w <= 64, 0 <= l <= 4294967295)";
        case REFUSE_TOO_MANY: return "more than 8 steps";
        case REFUSE_NO_STEP: return "no step is given";
        case REFUSE_PHRED: return "the quality offset is 33 or 64";
        default: return "no refusal";
    }
}
inline int step_clause(const Step &s) {
    switch (s.kind) {
        case KIND_LEADING:
        case KIND_TRAILING: return s.a <= MAX_T ? REFUSE_NONE : REFUSE_RANGE;
        case KIND_SLIDINGWINDOW: return (s.a >= 1 && s.a <= MAX_W && s.b <= MAX_T) ? REFUSE_NONE : REFUSE_RANGE;
        case KIND_MINLEN: return REFUSE_NONE;
        default: return REFUSE_UNKNOWN;
    }
}
// the steps and the offset of one call; *bad_step = the first offender
inline int steps_clause(const Step *steps, uint32_t n_steps, uint32_t phred, uint32_t *bad_step = nullptr) {
    if (bad_step) *bad_step = 0;
    if (phred != 33 && phred != 64) return REFUSE_PHRED;
    if (n_steps == 0 || !steps) return REFUSE_NO_STEP;
    if (n_steps > MAX_STEPS) return REFUSE_TOO_MANY;
    for (uint32_t i = 0; i < n_steps; ++i) {
        const int c = step_clause(steps[i]);
        if (c) { if (bad_step) *bad_step = i; return c; }
    }
    return REFUSE_NONE;
}

// ---- the parser: Trimmomatic's words, exact spelling, upper case ----
// digits only; a value beyond 2^32 - 1 is a number that is out of range
inline int parse_field(const char *p, const char *end, uint64_t &v) {
    if (p >= end) return REFUSE_FIELD;
    v = 0;
    for (; p < end; ++p) {
        if (*p < '0' || *p > '9') return REFUSE_FIELD;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > 0xFFFFFFFFull) v = 0x100000000ull;   // (stays there: out of range whatever follows)
    }
    return REFUSE_NONE;
}
inline int parse_step(const char *word, Step &s) {
    s = Step{0, 0, 0};
    const char *colon = strchr(word, ':');
    const size_t name_len = colon ? (size_t)(colon - word) : strlen(word);
    auto is = [&](const char *name) { return strlen(name) == name_len && memcmp(word, name, name_len) == 0; };
    int n_fields;
    if (is("LEADING")) { s.kind = KIND_LEADING; n_fields = 1; }
    else if (is("TRAILING")) { s.kind = KIND_TRAILING; n_fields = 1; }
    else if (is("SLIDINGWINDOW")) { s.kind = KIND_SLIDINGWINDOW; n_fields = 2; }
    else if (is("MINLEN")) { s.kind = KIND_MINLEN; n_fields = 1; }
    else return REFUSE_UNKNOWN;
    if (!colon) return REFUSE_FIELD;
    uint64_t v[2] = {0, 0};
    const char *p = colon + 1;
    for (int f = 0; f < n_fields; ++f) {
        const char *q = strchr(p, ':');
        const char *end = q ? q : p + strlen(p);
        if (f + 1 < n_fields && !q) return REFUSE_FIELD;     // a field is missing
        if (f + 1 == n_fields && q) return REFUSE_FIELD;     // one too many
        const int c = parse_field(p, end, v[f]);
        if (c) return c;
        p = end + 1;
    }
    if (v[0] > 0xFFFFFFFFull || v[1] > 0xFFFFFFFFull) return REFUSE_RANGE;
    s.a = (uint32_t)v[0];
    s.b = (uint32_t)v[1];
    return step_clause(s);
}
// all words of a command line; *bad_word = the offender
inline int parse_steps(const char *const *words, size_t n_words, std::vector<Step> &steps, size_t *bad_word = nullptr) {
    steps.clear();
    if (bad_word) *bad_word = 0;
    if (n_words == 0) return REFUSE_NO_STEP;
    for (size_t i = 0; i < n_words; ++i) {
        Step s;
        const int c = parse_step(words[i], s);
        if (bad_word) *bad_word = i;
        if (c) return c;
        if (steps.size() == MAX_STEPS) return REFUSE_TOO_MANY;
        steps.push_back(s);
    }
    return REFUSE_NONE;
}

// ---- the host's plain restatement (no device): what the kernels are held to ----
// one read: true = kept, with [b, e); false = dropped (b = e = 0)
inline bool trim_read(const char *qual, uint32_t n, const Step *steps, uint32_t n_steps, uint32_t phred, uint32_t &b_out, uint32_t &e_out) {
    uint32_t b = 0, e = n;
    bool kept = true;
    for (uint32_t s = 0; s < n_steps && kept; ++s) {
        const Step &st = steps[s];
        if (st.kind == KIND_LEADING) {
            uint32_t i = b;
            while (i < e && !base_good((uint8_t)qual[i], st.a, phred)) ++i;
            if (i == e) kept = false; else b = i;
        } else if (st.kind == KIND_TRAILING) {
            uint32_t i = e;
            while (i > b && !base_good((uint8_t)qual[i - 1], st.a, phred)) --i;
            if (i == b) kept = false; else e = i;
        } else if (st.kind == KIND_SLIDINGWINDOW) {
            const uint32_t w = st.a, m = e - b;
            if (m < w) { kept = false; break; }
            int64_t sum = 0;
            for (uint32_t i = 0; i < w; ++i) sum += quality((uint8_t)qual[b + i], phred);
            for (uint32_t j = 0; j + w <= m; ++j) {
                if (j) sum += quality((uint8_t)qual[b + j + w - 1], phred) - quality((uint8_t)qual[b + j - 1], phred);
                if (window_bad(sum, w, st.b)) {
                    if (j == 0) kept = false; else e = sliding_end(b, j, w);
                    break;
                }
            }
        } else if (st.kind == KIND_MINLEN) {
            if (too_short(b, e, st.a)) kept = false;
        }
    }
    if (kept && e == b) kept = false;
    b_out = kept ? b : 0;
    e_out = kept ? e : 0;
    return kept;
}

// the four lines of the whole records of text[0, bytes_used) (pf_mask::index_fastq has accepted them): content begin and end
inline void record_lines(const char *text, uint64_t n, uint64_t n_records, std::vector<uint64_t> &lb, std::vector<uint64_t> &le) {
    lb.assign(4 * n_records, 0);
    le.assign(4 * n_records, 0);
    uint64_t pos = 0;
    for (uint64_t l = 0; l < 4 * n_records; ++l) {
        const char *nl = static_cast<const char *>(memchr(text + pos, '\n', n - pos));
        const uint64_t end = nl ? (uint64_t)(nl - text) : n;
        lb[l] = pos;
        le[l] = pf_mask::line_content_end(text, pos, end, nl != nullptr);
        pos = nl ? end + 1 : n;
    }
}
// a kept record as it is written: four lines, each followed by one '\n'
inline void append_record(std::string &out, const char *text, const uint64_t *lb, const uint64_t *le, uint32_t b, uint32_t e) {
    out.append(text + lb[0], le[0] - lb[0]).push_back('\n');
    out.append(text + lb[1] + b, e - b).push_back('\n');
    out.append(text + lb[2], le[2] - lb[2]).push_back('\n');
    out.append(text + lb[3] + b, e - b).push_back('\n');
}
// One chunk: the index of pf_mask::index_fastq (its clause is returned, with bad_record; nothing is written then), every whole record
// trimmed, the kept ones appended to `out`.  begin / len (may be null): one entry per record, len 0 = dropped.
inline int trim_fastq(const char *text, uint64_t n, bool final, const Step *steps, uint32_t n_steps, uint32_t phred, std::string &out,
                      uint64_t &bytes_used, uint64_t &n_records, uint64_t &bad_record, std::vector<uint32_t> *begin = nullptr,
                      std::vector<uint32_t> *len = nullptr, Stats *stats = nullptr) {
    if (begin) begin->clear();
    if (len) len->clear();
    if (stats) *stats = Stats{};
    const int clause = pf_mask::index_fastq(text, n, final, bytes_used, n_records, bad_record);
    if (clause) { bytes_used = 0; n_records = 0; return clause; }
    std::vector<uint64_t> lb, le;
    record_lines(text, bytes_used, n_records, lb, le);
    Stats st = {};
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t nq = (uint32_t)(le[4 * r + 3] - lb[4 * r + 3]);
        uint32_t b = 0, e = 0;
        const bool kept = trim_read(text + lb[4 * r + 3], nq, steps, n_steps, phred, b, e);
        if (kept) append_record(out, text, &lb[4 * r], &le[4 * r], b, e);
        if (begin) begin->push_back(b);
        if (len) len->push_back(e - b);
        st.reads += 1;
        st.kept += kept;
        st.dropped += !kept;
        st.bases += nq;
        st.bases_kept += e - b;
    }
    if (stats) *stats = st;
    return pf_mask::CLAUSE_NONE;
}

}  // namespace pf_trim
