// The rule of adapter clipping (K-CLIP, `--adapters`) in one place, for the kernel (pf_clip.hip), the host layer (host/pf_trim_host.cpp,
// host/pf_host_c.cpp) and the stand-alone test (tests/cpp/test_clip_rule.cpp): the adapter file and its parser, the alignment of one
// adapter against one read, the refusals by name, and the host's plain restatement.  Integers only.
//
// Adapter file: FASTA.  A record's name is its header behind '>' up to the first blank; its sequence is the joined sequence lines (a
// '\r' in front of a '\n' is no content; blank lines are none either), folded to upper case.  A name ending in "/1" applies to file 1
// of a pair and to single-ended files (side 1), one ending in "/2" to file 2 only (side 2), any other to both (side 0).  A name
// starting with "Prefix" is a palindrome-mode entry of Trimmomatic's files: palindrome mode is not built, the entry is skipped and
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
// shorter overlaps at the read's end -- that function is the one open point); N is a full seed mismatch; no palindrome mode.
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
        default: return "no refusal";
    }
}
inline int params_clause(uint32_t seed, uint32_t score) {
    if (seed > MAX_SEED) return REFUSE_SEED;
    if (score < MIN_SCORE || score > MAX_SCORE) return REFUSE_SCORE;
    return REFUSE_NONE;
}

// the usable adapters of one file: adapter a is bases[off[a], off[a + 1]), upper case
struct Adapters {
    std::string bases;
    std::vector<uint32_t> off = {0};
    std::vector<uint8_t> side;
    std::vector<std::string> names;
    uint32_t skipped = 0;   // "Prefix" entries
    uint32_t size() const { return (uint32_t)side.size(); }
    void clear() { bases.clear(); off.assign(1, 0); side.clear(); names.clear(); skipped = 0; }
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

// ---- the parser of the adapter file: *bad_record = the 1-based record of the refusal (0: the file as a whole) ----
inline uint32_t name_side(const std::string &name) {
    const size_t n = name.size();
    if (n >= 2 && name[n - 2] == '/' && name[n - 1] == '1') return 1;
    if (n >= 2 && name[n - 2] == '/' && name[n - 1] == '2') return 2;
    return 0;
}
inline bool name_is_prefix(const std::string &name) { return name.compare(0, 6, "Prefix") == 0; }
inline int parse_adapters(const char *text, size_t n, Adapters &A, uint64_t *bad_record = nullptr) {
    A.clear();
    if (bad_record) *bad_record = 0;
    uint64_t record = 0;
    bool open = false, prefix = false;   // a record is being read; it is a skipped one
    std::string seq, name;
    int refusal = REFUSE_NONE;
    auto close = [&]() {   // the record that was open
        if (!open) return true;
        open = false;
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
        if (prefix) continue;
        for (size_t i = begin; i < ce && !refusal; ++i) {
            const uint8_t c = (uint8_t)text[i];
            if (!pf_mask::is_base(c)) refusal = REFUSE_BYTE;
            else if (seq.size() <= MAX_LEN) seq.push_back((char)(c & 0xDFu));   // (one beyond the limit is enough to refuse it)
        }
        if (refusal) break;
    }
    if (!refusal) close();
    if (!refusal && record == 0) refusal = REFUSE_NOT_FASTA;
    if (!refusal && A.size() == 0) refusal = REFUSE_NO_ADAPTER;
    if (refusal) {
        if (bad_record) *bad_record = (refusal == REFUSE_NOT_FASTA || refusal == REFUSE_NO_ADAPTER) ? 0 : record;
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

}  // namespace pf_clip
