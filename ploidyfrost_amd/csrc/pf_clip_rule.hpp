// The rule of adapter clipping (K-CLIP, `--adapters`) in one place, for the kernel (pf_clip.hip), the host layer (host/pf_trim_host.cpp,
// host/pf_host_c.cpp) and the stand-alone tests (tests/cpp/test_clip_rule.cpp, test_clip_pair_rule.cpp): the adapter file and its
// parser, the alignment of one adapter against one read, the two reads of a pair against each other (palindrome mode), the refusals
// by name, and the host's plain restatement.  Integers only.
//
// Adapter file: FASTA.  A record's name is its header behind '>' up to the first blank; its sequence is the joined sequence lines (a
// '\r' in front of a '\n' is no content; blank lines are none either), folded to upper case.  A name ending in "/1" applies to file 1
// of a pair and to single-ended files (side 1), one ending in "/2" to file 2 only (side 2), any other to both (side 0).  A name
// starting with "Prefix" is a palindrome-mode entry of Trimmomatic's files: without `--adapter-pairs` (below) the entry is skipped and
// counted.  Usable adapters hold 16 .. 128 bytes of ACGTacgt, at most 64 of them, at least one.
//
// Alignment: a read of n bases with q[p] = (int)byte - phred, an adapter of m bases.  Offset o aligns adapter position j with read
// position o + j, -(m - 16) <= o <= n - 16; the overlap is the read positions [max(0, o), min(n, o + m)), L of them; L < min_overlap()
// is no candidate.  SEED: the overlap holds a window of 16 consecutive positions with at most `seed` mismatches (a read byte outside
// ACGTacgt is a mismatch there).  SCORE: per overlap position 0 for a read byte outside ACGTacgt, +60206 for equal bases (case
// folded), else -10000 * max(q, 0); the score of the offset is the largest sum over the contiguous sub-ranges of the overlap, at
// least 0.  The offset passes when the seed holds and score >= 100000 * T.  o* = the smallest passing offset over all adapters of the
// file's side: none -- the read is untouched (clip end n); o* <= 0 -- dropped (clip end 0); else the read's interval starts as [0, o*).
// Clipping comes before every step of pf_trim_rule.hpp.
//
// PARITY UNPINNED, as for the rest of `trim`: Trimmomatic is not part of the build.  Where this rule knowingly differs from
// ILLUMINACLIP's simple mode: the smallest offset over all adapters instead of the first found per adapter; no overlaps below 16
// (min_overlap() below: a match is worth 0.602, so fewer than 16 positions cannot reach T >= 10, but Trimmomatic >= 0.32 also tries
// shorter overlaps at the read's end -- that function is the one open point); N is a full seed mismatch.
//
// PALINDROME MODE (K-PALIN, `--adapter-pairs`), for the two reads of a pair.  With the switch the "Prefix" entries are no longer
// skipped: `Prefix<X>/1` and `Prefix<X>/2` of the same <X> form a prefix pair (P1, P2) of one length p, 16 .. 128, at most 8 pairs,
// at least one; the other records are parsed as above and may be none.  Reads R1 (n1 bases) and R2 (n2): S1 = P1.R1, S2 = P2.R2.  A
// candidate is an insert length I, 0 <= I <= min(n1, n2) - A (A: the fewest adapter bases, 1 .. 16).  T = 2p + I; position i of S1
// is laid against position j = T - 1 - i of S2 for i in [lo, hi) = [max(0, p + I - n2), min(T, p + n1)); fewer than
// pair_min_overlap() positions are no candidate.  A position is VALID when both bytes are ACGTacgt, a MATCH when it is valid and
// the two base codes add up to 3 (complements).  SEED: 16 consecutive i in [lo, hi) with at most `seed` positions that are no match.
// SCORE: 0 for an invalid position, +60206 for a match, else -10000 * max(qm, 0), qm = the smaller quality of those of the two
// positions that are read positions (pair_mismatch_quality()); the largest sum over contiguous sub-ranges, at least 0, must reach
// 100000 * Tp.  I* = the smallest passing I over all prefix pairs: none -- the pair is untouched by this mode; else the pair end of
// file 1 is I*, that of file 2 is 0 (the reverse read is redundant) or, with keep_both, I*.  A read's clip end is the smaller of
// its simple clip end and its pair end.  A pair with a read of more than 1024 bases is no candidate (counted as pairs_too_long).
// The candidates are examined pair by pair, I upwards, below the best I found so far: candidates_scored counts those whose seed held.
// Where this knowingly differs from Trimmomatic: pair_min_overlap() = 16; the smaller quality is charged; the smallest I instead of
// Trimmomatic's fixed seed positions.  A tandem-repeat insert is its own reverse complement at shifted I: the smallest I wins.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pf_mask_rule.hpp"
#include "pf_trim_rule.hpp"

#if defined(__HIPCC__)
#define PF_CLIP_HD __host__ __device__
#else
#define PF_CLIP_HD
#endif

namespace pf_clip {

constexpr uint32_t WINDOW = 16;                    // positions of the seed window
constexpr uint32_t MIN_LEN = 16, MAX_LEN = 128;    // bases of a usable adapter
constexpr uint32_t MAX_ADAPTERS = 64;
constexpr uint32_t MAX_SEED = 8, DEFAULT_SEED = 2;
constexpr uint32_t MIN_SCORE = 1, MAX_SCORE = 1000, DEFAULT_SCORE = 10;
constexpr int32_t MATCH = 60206, PENALTY = 10000, SCORE_UNIT = 100000;
// the largest |sum| of a sub-range: 128 positions of -10000 * (255 - 33): inside int32
static_assert((int64_t)MAX_LEN * PENALTY * 255 < 0x7FFFFFFFll && (int64_t)MAX_SCORE * SCORE_UNIT < 0x7FFFFFFFll, "scores fit int32");
// palindrome mode
constexpr uint32_t MAX_PAIRS = 8;                  // prefix pairs of a file
constexpr uint32_t MAX_PAIR_READ = 1024;           // bases of a read that is a candidate
constexpr uint32_t MIN_PAIR_MIN = 1, MAX_PAIR_MIN = 16, DEFAULT_PAIR_MIN = 8;
constexpr uint32_t DEFAULT_PAIR_SCORE = 30;        // (1 .. MAX_SCORE)
// a running sum is at least 0 and at most (2 * 128 + 1024) matches, and one mismatch takes at most 10000 * 255 from it
static_assert((int64_t)(2 * MAX_LEN + MAX_PAIR_READ) * MATCH < 0x7FFFFFFFll, "pair scores fit int32");

struct PairStats {   // pf_clip_pair_stats of ploidyfrost_hip.h
    uint64_t pairs_clipped;      // pairs with I* > 0
    uint64_t pairs_dropped;      // pairs with I* == 0
    uint64_t pairs_too_long;     // pairs with a read of more than 1024 bases
    uint64_t candidates_scored;  // (prefix pair, I) examined whose seed held
    uint64_t bases_clipped[2];   // simple clip end - final clip end: what this mode took beyond simple mode, per file
};

struct Stats {   // pf_clip_stats of ploidyfrost_hip.h: [0] file 1 (and single-ended files), [1] file 2
    uint64_t reads_clipped[2];      // reads with o* > 0
    uint64_t reads_dropped[2];      // reads with o* <= 0
    uint64_t bases_clipped[2];      // n - clip end, over both kinds
    uint64_t candidates_scored[2];  // (adapter, offset) pairs whose seed held: the ones that were scored
};

// ---- the rule's pieces, shared with the kernel ----
// THE OPEN POINT: the shortest overlap that is a candidate
PF_CLIP_HD inline uint32_t min_overlap() { return WINDOW; }
PF_CLIP_HD inline bool applies(uint32_t adapter_side, uint32_t file_side) { return adapter_side == 0 || adapter_side == file_side; }
PF_CLIP_HD inline int32_t first_offset(uint32_t m) { return -(int32_t)(m - min_overlap()); }
PF_CLIP_HD inline int32_t last_offset(uint32_t n) { return (int32_t)n - (int32_t)min_overlap(); }   // (n < 16: below every first offset)
PF_CLIP_HD inline int32_t mismatch_cost(uint8_t qual_byte, uint32_t phred) {
    const int q = (int)qual_byte - (int)phred;
    return -PENALTY * (q > 0 ? q : 0);
}
PF_CLIP_HD inline bool score_passes(int32_t score, uint32_t T) { return score >= SCORE_UNIT * (int32_t)T; }
// clip end from o* (found = some offset passed)
PF_CLIP_HD inline uint32_t clip_end(bool found, int32_t o, uint32_t n) { return !found ? n : o <= 0 ? 0u : (uint32_t)o; }
// ---- palindrome mode's pieces ----
// OPEN POINT: the fewest positions laid against each other that are a candidate
PF_CLIP_HD inline uint32_t pair_min_overlap() { return WINDOW; }
// OPEN POINT: the quality a mismatch costs, of the one or two read positions it lies under (have2: the second is a read position too)
PF_CLIP_HD inline int pair_mismatch_quality(int qa, bool have2, int qb) { return have2 && qb < qa ? qb : qa; }
// OPEN POINT: which passing I is taken -- the smallest
PF_CLIP_HD inline bool pair_better(uint32_t I, uint32_t best) { return I < best; }
PF_CLIP_HD inline bool pair_too_long(uint32_t n1, uint32_t n2) { return n1 > MAX_PAIR_READ || n2 > MAX_PAIR_READ; }
// candidates are I in [0, pair_candidates(...)): none when a read holds fewer than pair_min bases
PF_CLIP_HD inline uint32_t pair_candidates(uint32_t n1, uint32_t n2, uint32_t pair_min) {
    const uint32_t n = n1 < n2 ? n1 : n2;
    return n < pair_min ? 0u : n - pair_min + 1;
}
// the positions i of S1 that candidate I lays against S2; false: fewer than pair_min_overlap()
PF_CLIP_HD inline bool pair_range(uint32_t p, uint32_t n1, uint32_t n2, uint32_t I, uint32_t &lo, uint32_t &hi) {
    const uint32_t T = 2 * p + I;
    lo = p + I > n2 ? p + I - n2 : 0u;
    hi = T < p + n1 ? T : p + n1;
    return hi > lo && hi - lo >= pair_min_overlap();
}
PF_CLIP_HD inline bool pair_complement(uint8_t a, uint8_t b) { return pf_mask::base_code(a) + pf_mask::base_code(b) == 3; }
// the final clip ends from the simple ends and I* (found = some I passed)
PF_CLIP_HD inline uint32_t pair_end(bool found, uint32_t I, uint32_t simple_end, int file, bool keep_both) {
    if (!found) return simple_end;
    const uint32_t e = file == 0 || keep_both ? I : 0u;
    return e < simple_end ? e : simple_end;
}

// ---- the refusals, each with the name it is refused by ----
enum Refusal {
    REFUSE_NONE = 0,
    REFUSE_NOT_FASTA,   // an empty file, or one whose first line does not start with '>'
    REFUSE_BYTE,        // a sequence byte outside ACGTacgt
    REFUSE_LENGTH,      // a sequence shorter than 16 or longer than 128
    REFUSE_TOO_MANY,    // more than 64 usable adapters
    REFUSE_NO_ADAPTER,  // no usable adapter at all
    REFUSE_SEED,        // seed outside 0 .. 8
    REFUSE_SCORE,       // score outside 1 .. 1000
    REFUSE_SIDE,        // a side that is not 0, 1 or 2
    // palindrome mode
    REFUSE_PAIR_PARTNER,    // a Prefix entry without its partner (no /1 or /2 of the same name, or a second one of the same)
    REFUSE_PAIR_LENGTHS,    // the two entries of a prefix pair of different lengths
    REFUSE_TOO_MANY_PAIRS,  // more than 8 prefix pairs
    REFUSE_NO_PAIR,         // no prefix pair at all
    REFUSE_PAIR_SCORE,      // pair score outside 1 .. 1000
    REFUSE_PAIR_MIN,        // fewest adapter bases outside 1 .. 16
    REFUSE_COUNT_
};
inline const char *refusal_text(int r) {
    switch (r) {
        case REFUSE_NOT_FASTA: return "the adapter file is empty or is not FASTA (its first line starts with '>')";
        case REFUSE_BYTE: return "an adapter holds a byte outside ACGTacgt";
        case REFUSE_LENGTH: return "an adapter holds 16 to 128 bases";
        case REFUSE_TOO_MANY: return "more than 64 usable adapters";
        case REFUSE_NO_ADAPTER: return "no usable adapter";
        case REFUSE_SEED: return "the adapter seed is 0 to 8 mismatches";
        case REFUSE_SCORE: return "the adapter score is 1 to 1000";
        case REFUSE_SIDE: return "the side of an adapter is 0 (both files), 1 or 2";
        case REFUSE_PAIR_PARTNER: return "a Prefix entry needs its partner: Prefix<X>/1 and Prefix<X>/2, one of each";
        case REFUSE_PAIR_LENGTHS: return "the two entries of a prefix pair hold the same number of bases";
        case REFUSE_TOO_MANY_PAIRS: return "more than 8 prefix pairs";
        case REFUSE_NO_PAIR: return "no prefix pair (Prefix<X>/1 and Prefix<X>/2) for --adapter-pairs";
        case REFUSE_PAIR_SCORE: return "the adapter pair score is 1 to 1000";
        case REFUSE_PAIR_MIN: return "the fewest adapter bases of a pair are 1 to 16";
        default: return "no refusal";
    }
}
inline int params_clause(uint32_t seed, uint32_t score) {
    if (seed > MAX_SEED) return REFUSE_SEED;
    if (score < MIN_SCORE || score > MAX_SCORE) return REFUSE_SCORE;
    return REFUSE_NONE;
}
inline int pair_params_clause(uint32_t pair_score, uint32_t pair_min) {
    if (pair_score < MIN_SCORE || pair_score > MAX_SCORE) return REFUSE_PAIR_SCORE;
    if (pair_min < MIN_PAIR_MIN || pair_min > MAX_PAIR_MIN) return REFUSE_PAIR_MIN;
    return REFUSE_NONE;
}

// the usable adapters of one file: adapter a is bases[off[a], off[a + 1]), upper case
struct Adapters {
    std::string bases;
    std::vector<uint32_t> off = {0};
    std::vector<uint8_t> side;
    std::vector<std::string> names;
    uint32_t skipped = 0;   // "Prefix" entries
    // palindrome mode: prefix pair q is P1 = prefix_bases[prefix_off[2q], prefix_off[2q + 1]), P2 = [prefix_off[2q + 1], prefix_off[2q + 2])
    std::string prefix_bases;
    std::vector<uint32_t> prefix_off = {0};
    std::vector<std::string> prefix_names;   // <X> of Prefix<X>/1
    uint32_t size() const { return (uint32_t)side.size(); }
    uint32_t pairs() const { return (uint32_t)(prefix_off.size() - 1) / 2; }
    void clear() {
        bases.clear(); off.assign(1, 0); side.clear(); names.clear(); skipped = 0;
        prefix_bases.clear(); prefix_off.assign(1, 0); prefix_names.clear();
    }
};
// a set as the ABI takes it (pf_clip_begin): *bad = the offending adapter (0-based)
inline int set_clause(const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters, uint32_t seed, uint32_t score, uint32_t *bad = nullptr) {
    if (bad) *bad = 0;
    { const int c = params_clause(seed, score); if (c) return c; }
    if (n_adapters == 0 || !bases || !off || !side) return REFUSE_NO_ADAPTER;
    if (n_adapters > MAX_ADAPTERS) return REFUSE_TOO_MANY;
    for (uint32_t a = 0; a < n_adapters; ++a) {
        if (bad) *bad = a;
        if (off[a + 1] < off[a] || off[a + 1] - off[a] < MIN_LEN || off[a + 1] - off[a] > MAX_LEN) return REFUSE_LENGTH;
        if (side[a] > 2) return REFUSE_SIDE;
        for (uint32_t i = off[a]; i < off[a + 1]; ++i)
            if (!pf_mask::is_base((uint8_t)bases[i])) return REFUSE_BYTE;
    }
    if (bad) *bad = 0;
    return REFUSE_NONE;
}
// a set with prefix pairs as the ABI takes it (pf_clip_begin_pairs): the simple adapters may be none; *bad = the offending adapter, or
// (*of_pair) the offending prefix pair (0-based)
inline int pair_set_clause(const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters, const char *prefix_bases, const uint32_t *prefix_off,
                           uint32_t n_pairs, uint32_t seed, uint32_t score, uint32_t pair_score, uint32_t pair_min, uint32_t *bad = nullptr,
                           bool *of_pair = nullptr) {
    if (bad) *bad = 0;
    if (of_pair) *of_pair = false;
    { const int c = params_clause(seed, score); if (c) return c; }
    { const int c = pair_params_clause(pair_score, pair_min); if (c) return c; }
    if (n_adapters) { const int c = set_clause(bases, off, side, n_adapters, seed, score, bad); if (c) return c; }
    if (of_pair) *of_pair = true;
    if (n_pairs == 0 || !prefix_bases || !prefix_off) return REFUSE_NO_PAIR;
    if (n_pairs > MAX_PAIRS) return REFUSE_TOO_MANY_PAIRS;
    for (uint32_t q = 0; q < n_pairs; ++q) {
        if (bad) *bad = q;
        if (prefix_off[2 * q + 1] < prefix_off[2 * q] || prefix_off[2 * q + 2] < prefix_off[2 * q + 1]) return REFUSE_LENGTH;
        const uint32_t p = prefix_off[2 * q + 1] - prefix_off[2 * q];
        if (prefix_off[2 * q + 2] - prefix_off[2 * q + 1] != p) return REFUSE_PAIR_LENGTHS;
        if (p < MIN_LEN || p > MAX_LEN) return REFUSE_LENGTH;
        for (uint32_t i = prefix_off[2 * q]; i < prefix_off[2 * q + 2]; ++i)
            if (!pf_mask::is_base((uint8_t)prefix_bases[i])) return REFUSE_BYTE;
    }
    if (bad) *bad = 0;
    return REFUSE_NONE;
}

// ---- the parser of the adapter file: *bad_record = the 1-based record of the refusal (0: the file as a whole) ----
inline uint32_t name_side(const std::string &name) {
    const size_t n = name.size();
    if (n >= 2 && name[n - 2] == '/' && name[n - 1] == '1') return 1;
    if (n >= 2 && name[n - 2] == '/' && name[n - 1] == '2') return 2;
    return 0;
}
inline bool name_is_prefix(const std::string &name) { return name.compare(0, 6, "Prefix") == 0; }
// (pairs: `--adapter-pairs` -- the Prefix entries form prefix pairs instead of being skipped)
inline int parse_adapters(const char *text, size_t n, Adapters &A, uint64_t *bad_record = nullptr, bool pairs = false) {
    A.clear();
    if (bad_record) *bad_record = 0;
    uint64_t record = 0;
    bool open = false, prefix = false;   // a record is being read; it is a skipped one
    std::string seq, name;
    int refusal = REFUSE_NONE;
    struct Half { std::string x, seq; uint32_t side; uint64_t record; };
    std::vector<Half> waiting;   // Prefix entries whose partner has not come yet
    auto close_prefix = [&]() {
        if (seq.size() < MIN_LEN || seq.size() > MAX_LEN) { refusal = REFUSE_LENGTH; return false; }
        const uint32_t sd = name_side(name);
        if (sd == 0) { refusal = REFUSE_PAIR_PARTNER; return false; }
        const std::string x = name.substr(6, name.size() - 8);
        for (const std::string &done : A.prefix_names)
            if (done == x) { refusal = REFUSE_PAIR_PARTNER; return false; }
        for (size_t w = 0; w < waiting.size(); ++w) {
            if (waiting[w].x != x) continue;
            if (waiting[w].side == sd) { refusal = REFUSE_PAIR_PARTNER; return false; }
            if (waiting[w].seq.size() != seq.size()) { refusal = REFUSE_PAIR_LENGTHS; return false; }
            if (A.pairs() == MAX_PAIRS) { refusal = REFUSE_TOO_MANY_PAIRS; return false; }
            A.prefix_bases += sd == 2 ? waiting[w].seq : seq;
            A.prefix_off.push_back((uint32_t)A.prefix_bases.size());
            A.prefix_bases += sd == 2 ? seq : waiting[w].seq;
            A.prefix_off.push_back((uint32_t)A.prefix_bases.size());
            A.prefix_names.push_back(x);
            waiting.erase(waiting.begin() + (long)w);
            return true;
        }
        waiting.push_back(Half{x, seq, sd, record});
        return true;
    };
    auto close = [&]() {   // the record that was open
        if (!open) return true;
        open = false;
        if (prefix && pairs) return close_prefix();
        if (prefix) { A.skipped += 1; return true; }
        if (seq.size() < MIN_LEN || seq.size() > MAX_LEN) { refusal = REFUSE_LENGTH; return false; }
        if (A.size() == MAX_ADAPTERS) { refusal = REFUSE_TOO_MANY; return false; }
        A.bases += seq;
        A.off.push_back((uint32_t)A.bases.size());
        A.side.push_back((uint8_t)name_side(name));
        A.names.push_back(name);
        return true;
    };
    size_t pos = 0;
    while (pos < n) {
        const char *nl = static_cast<const char *>(memchr(text + pos, '\n', n - pos));
        const size_t end = nl ? (size_t)(nl - text) : n;
        const size_t ce = (size_t)pf_mask::line_content_end(text, pos, end, nl != nullptr);
        const size_t begin = pos;
        pos = nl ? end + 1 : n;
        if (ce == begin) continue;   // a blank line
        if (text[begin] == '>') {
            if (!close()) break;
            record += 1;
            open = true;
            size_t e = begin + 1;
            while (e < ce && text[e] != ' ' && text[e] != '\t') ++e;
            name.assign(text + begin + 1, e - begin - 1);
            prefix = name_is_prefix(name);
            seq.clear();
            continue;
        }
        if (!open) { refusal = REFUSE_NOT_FASTA; break; }
        if (prefix && !pairs) continue;
        for (size_t i = begin; i < ce && !refusal; ++i) {
            const uint8_t c = (uint8_t)text[i];
            if (!pf_mask::is_base(c)) refusal = REFUSE_BYTE;
            else if (seq.size() <= MAX_LEN) seq.push_back((char)(c & 0xDFu));   // (one beyond the limit is enough to refuse it)
        }
        if (refusal) break;
    }
    if (!refusal) close();
    if (!refusal && record == 0) refusal = REFUSE_NOT_FASTA;
    if (!refusal && !waiting.empty()) { refusal = REFUSE_PAIR_PARTNER; record = waiting[0].record; }
    if (!refusal && pairs && A.pairs() == 0) refusal = REFUSE_NO_PAIR;
    if (!refusal && !pairs && A.size() == 0) refusal = REFUSE_NO_ADAPTER;
    if (refusal) {
        if (bad_record) *bad_record = (refusal == REFUSE_NOT_FASTA || refusal == REFUSE_NO_ADAPTER || refusal == REFUSE_NO_PAIR) ? 0 : record;
        A.clear();
    }
    return refusal;
}
// the refusal of a file as the command line and the host ABI word it
inline std::string file_refusal(const std::string &path, int refusal, uint64_t bad_record) {
    std::string m = "adapters " + path;
    if (bad_record) m += ": record " + std::to_string(bad_record);
    return m + ": " + refusal_text(refusal);
}

// ---- the host's plain restatement (no device): what the kernel is held to ----
// one adapter at one offset: is it a candidate whose seed holds (*seed_ok), and its score
inline int32_t offset_score(const char *seq, const char *qual, uint32_t n, const char *ad, uint32_t m, int32_t o, uint32_t seed, uint32_t phred,
                            bool *seed_ok) {
    *seed_ok = false;
    const int32_t lo = o > 0 ? o : 0, hi = (int32_t)n < o + (int32_t)m ? (int32_t)n : o + (int32_t)m;
    if (hi - lo < (int32_t)min_overlap()) return 0;
    auto mismatch = [&](int32_t p) {
        const uint8_t c = (uint8_t)seq[p];
        return !pf_mask::is_base(c) || (c & 0xDFu) != ((uint8_t)ad[p - o] & 0xDFu);
    };
    for (int32_t w = lo; w + (int32_t)WINDOW <= hi && !*seed_ok; ++w) {
        uint32_t mm = 0;
        for (int32_t p = w; p < w + (int32_t)WINDOW; ++p) mm += mismatch(p);
        if (mm <= seed) *seed_ok = true;
    }
    if (!*seed_ok) return 0;
    int32_t run = 0, best = 0;
    for (int32_t p = lo; p < hi; ++p) {
        const uint8_t c = (uint8_t)seq[p];
        const int32_t v = !pf_mask::is_base(c) ? 0 : !mismatch(p) ? MATCH : mismatch_cost((uint8_t)qual[p], phred);
        run = run + v > 0 ? run + v : 0;
        if (run > best) best = run;
    }
    return best;
}
// one read of one file (file_side 1 or 2): the clip end -- n untouched, 0 dropped; *scored (may be null) += the candidates scored
inline uint32_t clip_read(const char *seq, const char *qual, uint32_t n, const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters,
                          uint32_t file_side, uint32_t seed, uint32_t score, uint32_t phred, uint64_t *scored = nullptr) {
    bool found = false;
    int32_t best = 0;
    for (uint32_t a = 0; a < n_adapters; ++a) {
        if (!applies(side[a], file_side)) continue;
        const uint32_t m = off[a + 1] - off[a];
        for (int32_t o = first_offset(m); o <= last_offset(n); ++o) {
            bool seed_ok = false;
            const int32_t s = offset_score(seq, qual, n, bases + off[a], m, o, seed, phred, &seed_ok);
            if (!seed_ok) continue;
            if (scored) *scored += 1;
            if (score_passes(s, score) && (!found || o < best)) { found = true; best = o; }
        }
    }
    return clip_end(found, best, n);
}

// ---- palindrome mode restated ----
// one prefix pair (P1, P2 of p bases) at one insert length I: is it a candidate whose seed holds (*seed_ok), and its score
inline int32_t pair_candidate(const char *seq1, const char *qual1, uint32_t n1, const char *seq2, const char *qual2, uint32_t n2, const char *P1,
                              const char *P2, uint32_t p, uint32_t I, uint32_t seed, uint32_t phred, bool *seed_ok) {
    *seed_ok = false;
    uint32_t lo = 0, hi = 0;
    if (!pair_range(p, n1, n2, I, lo, hi)) return 0;
    const uint32_t T = 2 * p + I;
    auto byte1 = [&](uint32_t i) { return (uint8_t)(i < p ? P1[i] : seq1[i - p]); };
    auto byte2 = [&](uint32_t j) { return (uint8_t)(j < p ? P2[j] : seq2[j - p]); };
    auto valid = [&](uint32_t i) { return pf_mask::is_base(byte1(i)) && pf_mask::is_base(byte2(T - 1 - i)); };
    auto match = [&](uint32_t i) { return valid(i) && pair_complement(byte1(i), byte2(T - 1 - i)); };
    uint32_t mm = 0;   // of the window [w, w + 16)
    for (uint32_t i = lo; i < lo + WINDOW; ++i) mm += !match(i);
    for (uint32_t w = lo;; ++w) {
        if (mm <= seed) { *seed_ok = true; break; }
        if (w + WINDOW >= hi) break;
        mm += (uint32_t)!match(w + WINDOW) - (uint32_t)!match(w);
    }
    if (!*seed_ok) return 0;
    int32_t run = 0, best = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        int32_t v = 0;
        if (match(i)) v = MATCH;
        else if (valid(i)) {
            const uint32_t j = T - 1 - i;
            int q;
            if (i >= p) q = pair_mismatch_quality((int)(uint8_t)qual1[i - p] - (int)phred, j >= p, j >= p ? (int)(uint8_t)qual2[j - p] - (int)phred : 0);
            else q = (int)(uint8_t)qual2[j - p] - (int)phred;   // (under a prefix position of S1: position j is a read position)
            v = -PENALTY * (q > 0 ? q : 0);
        }
        run = run + v > 0 ? run + v : 0;
        if (run > best) best = run;
    }
    return best;
}
// the prefix pairs of a clip and its pair values, as the restatements below take them
struct PairSet {
    const char *prefix_bases = nullptr;
    const uint32_t *prefix_off = nullptr;   // 2 * n_pairs + 1
    uint32_t n_pairs = 0, pair_score = DEFAULT_PAIR_SCORE, pair_min = DEFAULT_PAIR_MIN;
    bool keep_both = false;
};
// the two reads of one pair: *found = some I passed, I* returned (else 0); *too_long: no candidate; *scored (may be null) += candidates
inline uint32_t pair_insert(const char *seq1, const char *qual1, uint32_t n1, const char *seq2, const char *qual2, uint32_t n2, const PairSet &P, uint32_t seed,
                            uint32_t phred, bool *found, bool *too_long = nullptr, uint64_t *scored = nullptr) {
    *found = false;
    if (too_long) *too_long = pair_too_long(n1, n2);
    if (pair_too_long(n1, n2)) return 0;
    uint32_t best = pair_candidates(n1, n2, P.pair_min);   // candidates lie below it
    for (uint32_t q = 0; q < P.n_pairs; ++q) {
        const uint32_t p = P.prefix_off[2 * q + 1] - P.prefix_off[2 * q];
        for (uint32_t I = 0; I < best; ++I) {
            bool seed_ok = false;
            const int32_t s = pair_candidate(seq1, qual1, n1, seq2, qual2, n2, P.prefix_bases + P.prefix_off[2 * q], P.prefix_bases + P.prefix_off[2 * q + 1], p,
                                             I, seed, phred, &seed_ok);
            if (!seed_ok) continue;
            if (scored) *scored += 1;
            if (score_passes(s, P.pair_score) && pair_better(I, best)) { *found = true; best = I; break; }
        }
    }
    return *found ? best : 0u;
}
// the two reads of one pair under simple mode and palindrome mode: end[f] = the final clip end of file f (n_adapters may be 0).
// clip, pairs (may be null) are added to.
inline void clip_pair(const char *seq1, const char *qual1, uint32_t n1, const char *seq2, const char *qual2, uint32_t n2, const char *bases,
                      const uint32_t *off, const uint8_t *side, uint32_t n_adapters, const PairSet &P, uint32_t seed, uint32_t score, uint32_t phred,
                      uint32_t end[2], Stats *clip = nullptr, PairStats *pairs = nullptr) {
    const char *seq[2] = {seq1, seq2}, *qual[2] = {qual1, qual2};
    const uint32_t n[2] = {n1, n2};
    uint32_t simple[2];
    for (int f = 0; f < 2; ++f) {
        uint64_t sc = 0;
        simple[f] = n_adapters ? clip_read(seq[f], qual[f], n[f], bases, off, side, n_adapters, (uint32_t)f + 1, seed, score, phred, &sc) : n[f];
        if (clip) clip->candidates_scored[f] += sc;
    }
    bool found = false, too_long = false;
    uint64_t sc = 0;
    const uint32_t I = pair_insert(seq1, qual1, n1, seq2, qual2, n2, P, seed, phred, &found, &too_long, &sc);
    for (int f = 0; f < 2; ++f) {
        end[f] = pair_end(found, I, simple[f], f, P.keep_both);
        if (clip) {
            clip->reads_clipped[f] += end[f] != n[f] && end[f] != 0;
            clip->reads_dropped[f] += end[f] != n[f] && end[f] == 0;
            clip->bases_clipped[f] += n[f] - end[f];
        }
        if (pairs) pairs->bases_clipped[f] += simple[f] - end[f];
    }
    if (pairs) {
        pairs->pairs_clipped += found && I != 0;
        pairs->pairs_dropped += found && I == 0;
        pairs->pairs_too_long += too_long;
        pairs->candidates_scored += sc;
    }
}

// One chunk, clipped and then trimmed: pf_trim::trim_fastq with every read's interval starting as [0, clip end).  The steps look at
// no quality beyond the interval's end, so a read clipped to e is trimmed as a read of e bases; n_steps may be 0.  `clip` (may be
// null) is added to, in place file_side - 1.
inline int trim_fastq(const char *text, uint64_t n, bool final, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred, const char *bases,
                      const uint32_t *off, const uint8_t *side, uint32_t n_adapters, uint32_t file_side, uint32_t seed, uint32_t score, std::string &out,
                      uint64_t &bytes_used, uint64_t &n_records, uint64_t &bad_record, std::vector<uint32_t> *begin = nullptr,
                      std::vector<uint32_t> *len = nullptr, pf_trim::Stats *stats = nullptr, Stats *clip = nullptr) {
    if (begin) begin->clear();
    if (len) len->clear();
    if (stats) *stats = pf_trim::Stats{};
    const int clause = pf_mask::index_fastq(text, n, final, bytes_used, n_records, bad_record);
    if (clause) { bytes_used = 0; n_records = 0; return clause; }
    std::vector<uint64_t> lb, le;
    pf_trim::record_lines(text, bytes_used, n_records, lb, le);
    pf_trim::Stats st = {};
    const uint32_t f = file_side == 2 ? 1 : 0;
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t nq = (uint32_t)(le[4 * r + 3] - lb[4 * r + 3]);
        uint64_t scored = 0;
        const uint32_t ce = clip_read(text + lb[4 * r + 1], text + lb[4 * r + 3], nq, bases, off, side, n_adapters, file_side, seed, score, phred, &scored);
        if (clip) {
            clip->candidates_scored[f] += scored;
            clip->reads_clipped[f] += ce != nq && ce != 0;
            clip->reads_dropped[f] += ce != nq && ce == 0;
            clip->bases_clipped[f] += nq - ce;
        }
        uint32_t b = 0, e = 0;
        const bool kept = pf_trim::trim_read(text + lb[4 * r + 3], ce, steps, n_steps, phred, b, e);
        if (kept) pf_trim::append_record(out, text, &lb[4 * r], &le[4 * r], b, e);
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

// One chunk of each file of a pair, clipped by both modes and then trimmed: what pf_trim_fastq_pair gives while a clip with prefix
// pairs is open.  The records taken are the whole records both chunks hold (n_records; bytes_used[f] ends behind record
// n_records - 1 of file f).  out: o1, u1, o2, u2 as pf_trim_fastq_pair.  Returns a clause of pf_mask (bad_record = 2 * record + file),
// or PAIR_COUNTS_DIFFER for final chunks of different record counts.  end[f], begin[f], len[f] (may be null): per record.
constexpr int PAIR_COUNTS_DIFFER = pf_mask::CLAUSE_COUNT_;   // (as pf_trimrun::CLAUSE_PAIR_COUNT)
inline int trim_fastq_pair(const char *const text[2], const uint64_t n[2], bool final, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred,
                           const char *bases, const uint32_t *off, const uint8_t *side, uint32_t n_adapters, const PairSet &P, uint32_t seed, uint32_t score,
                           std::string out[4], uint64_t bytes_used[2], uint64_t &n_records, uint64_t &bad_record, std::vector<uint32_t> *begin[2] = nullptr,
                           std::vector<uint32_t> *len[2] = nullptr, pf_trim::Stats stats[2] = nullptr, Stats *clip = nullptr, PairStats *pairs = nullptr,
                           std::vector<uint32_t> *end[2] = nullptr) {
    n_records = 0;
    bad_record = 0;
    std::vector<uint64_t> lb[2], le[2];
    uint64_t used[2] = {0, 0}, recs[2] = {0, 0};
    for (int f = 0; f < 2; ++f) {
        bytes_used[f] = 0;
        if (begin && begin[f]) begin[f]->clear();
        if (len && len[f]) len[f]->clear();
        if (end && end[f]) end[f]->clear();
        if (stats) stats[f] = pf_trim::Stats{};
        uint64_t bad = 0;
        const int clause = pf_mask::index_fastq(text[f], n[f], final, used[f], recs[f], bad);
        if (clause) { bad_record = 2 * bad + (uint64_t)f; return clause; }
        pf_trim::record_lines(text[f], used[f], recs[f], lb[f], le[f]);
    }
    const uint64_t nr = recs[0] < recs[1] ? recs[0] : recs[1];
    if (final && recs[0] != recs[1]) { bad_record = 2 * nr + (recs[0] < recs[1] ? 0 : 1); return PAIR_COUNTS_DIFFER; }
    pf_trim::Stats st[2] = {};
    for (uint64_t r = 0; r < nr; ++r) {
        uint32_t nq[2], ce[2], b[2] = {0, 0}, e[2] = {0, 0};
        bool kept[2];
        for (int f = 0; f < 2; ++f) nq[f] = (uint32_t)(le[f][4 * r + 3] - lb[f][4 * r + 3]);
        clip_pair(text[0] + lb[0][4 * r + 1], text[0] + lb[0][4 * r + 3], nq[0], text[1] + lb[1][4 * r + 1], text[1] + lb[1][4 * r + 3], nq[1], bases, off, side,
                  n_adapters, P, seed, score, phred, ce, clip, pairs);
        for (int f = 0; f < 2; ++f) kept[f] = pf_trim::trim_read(text[f] + lb[f][4 * r + 3], ce[f], steps, n_steps, phred, b[f], e[f]);
        for (int f = 0; f < 2; ++f) {
            if (kept[f]) pf_trim::append_record(out[2 * f + (kept[1 - f] ? 0 : 1)], text[f], &lb[f][4 * r], &le[f][4 * r], b[f], e[f]);
            if (begin && begin[f]) begin[f]->push_back(b[f]);
            if (len && len[f]) len[f]->push_back(e[f] - b[f]);
            if (end && end[f]) end[f]->push_back(ce[f]);
            st[f].reads += 1;
            st[f].kept += kept[f];
            st[f].dropped += !kept[f];
            st[f].bases += nq[f];
            st[f].bases_kept += e[f] - b[f];
            st[f].both += kept[0] && kept[1];
            st[f].only1 += kept[0] && !kept[1];
            st[f].only2 += !kept[0] && kept[1];
            st[f].neither += !kept[0] && !kept[1];
        }
    }
    for (int f = 0; f < 2; ++f) {
        bytes_used[f] = nr < recs[f] ? lb[f][4 * nr] : used[f];
        if (stats) stats[f] = st[f];
    }
    n_records = nr;
    return pf_mask::CLAUSE_NONE;
}

}  // namespace pf_clip
