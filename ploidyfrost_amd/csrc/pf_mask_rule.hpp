// The rule of `ploidyfrost mask` (K-MASK) in one place, for the kernels (pf_mask.hip), the host layer (host/pf_mask_host.cpp, host/pf_reads_stream.cpp)
// and the stand-alone test (tests/cpp/test_mask_rule.cpp): which bytes are bases, which line of a FASTQ record is which, when a
// window is bad, and which bytes a set of bad windows masks.  It restates what `kmc_tools filter -hm <db> <reads> -ci<L> -cx<U>`
// is documented to do with the counters of CKMCFile::GetCountersForRead (KMC/kmc_api/kmc_file.cpp:904-1090): one counter per
// window of k bytes, 0 for a window that holds a byte outside ACGTacgt or a k-mer the database does not give out.
//
// PARITY UNPINNED: the tool is not part of the build.  "Every base of every k-mer outside the bounds becomes N" is how -hm is
// documented ("k-mers are masked"); the other reading -- only the bases that NO good k-mer covers -- would change byte_masked()
// below and nothing else.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define PF_MASK_HD __host__ __device__
#else
#define PF_MASK_HD
#endif

namespace pf_mask {

constexpr int MAX_K = 31;          // a k-mer is one 64-bit word of 2-bit codes (pf_upload_counts: 3 <= k <= 31)
constexpr char MASK_BYTE = 'N';

// ---- byte classes: a base is one of ACGTacgt; lower case is read as upper case, every other byte ends every window over it ----
PF_MASK_HD inline bool is_base(uint8_t b) {
    const uint8_t c = b & 0xDFu;
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}
// A0 C1 G2 T3 (defined for bases only)
PF_MASK_HD inline uint32_t base_code(uint8_t b) { return ((b >> 1) & 3u) ^ ((b >> 2) & 1u); }

// ---- line roles: by the line's index in the file, never by its first byte (a quality line may begin with '@' or '+') ----
enum LineRole { LINE_HEADER = 0, LINE_SEQUENCE = 1, LINE_PLUS = 2, LINE_QUALITY = 3 };
PF_MASK_HD inline int line_role(uint64_t line_index) { return (int)(line_index & 3u); }
// a line is text[begin, end): end is its '\n' (or the end of the text for a last line without one); a '\r' directly in front of
// the '\n' belongs to the line end, not to the line
PF_MASK_HD inline uint64_t line_content_end(const char *text, uint64_t begin, uint64_t end, bool has_newline) {
    return (has_newline && end > begin && text[end - 1] == '\r') ? end - 1 : end;
}

// ---- the refusals, each with the name it is refused by ----
enum Clause {
    CLAUSE_NONE = 0,
    CLAUSE_HEADER,       // a record whose first line does not start with '@'
    CLAUSE_PLUS,         // a record whose third line does not start with '+'
    CLAUSE_QUALITY,      // a quality line whose length differs from its sequence line's
    CLAUSE_LINE_COUNT,   // a line count that is not a multiple of four
    CLAUSE_FASTA,        // a first byte of '>'
    CLAUSE_GZIP,         // the gzip magic 1f 8b
    CLAUSE_SAME_PATH,    // an output path equal to an input path
    CLAUSE_COUNT_
};
inline const char *clause_text(int c) {
    switch (c) {
        case CLAUSE_HEADER: return "the record's first line does not start with '@'";
        case CLAUSE_PLUS: return "the record's third line does not start with '+'";
        case CLAUSE_QUALITY: return "the quality line's length differs from the sequence line's";
        case CLAUSE_LINE_COUNT: return "the line count is not a multiple of four";
        case CLAUSE_FASTA: return "the input is FASTA (first byte '>'): only FASTQ is masked";
        case CLAUSE_GZIP: return "the input is gzip-compressed (magic 1f 8b): only plain FASTQ is masked";
        case CLAUSE_SAME_PATH: return "the output path is an input path";
        default: return "no refusal";
    }
}
// the three checks of one record from its lines' extents (content: without line end); the first that fails names the refusal
PF_MASK_HD inline int record_clause(const char *text, uint64_t head_begin, uint64_t head_end, uint64_t seq_len, uint64_t plus_begin,
                                    uint64_t plus_end, uint64_t qual_len) {
    if (head_end <= head_begin || text[head_begin] != '@') return CLAUSE_HEADER;
    if (plus_end <= plus_begin || text[plus_begin] != '+') return CLAUSE_PLUS;
    if (qual_len != seq_len) return CLAUSE_QUALITY;
    return CLAUSE_NONE;
}
// what the first bytes of a file say about it
inline int file_clause(const unsigned char *first, uint64_t n) {
    if (n >= 2 && first[0] == 0x1f && first[1] == 0x8b) return CLAUSE_GZIP;
    if (n >= 1 && first[0] == '>') return CLAUSE_FASTA;
    return CLAUSE_NONE;
}

// ---- masking ----
// window i is bad when its counter lies outside [low, up]
PF_MASK_HD inline bool window_bad(uint32_t counter, uint32_t low, uint32_t up) { return counter < low || counter > up; }
// "bad set -> masked byte".  bad_ending_here: bit 63 = window j is bad, bit 63 - t = window j - t is bad (a position that is no
// window start carries 0).  Byte j becomes N when a bad window covers it: i <= j < i + k, i.e. one of windows j - k + 1 .. j.
PF_MASK_HD inline bool byte_masked(uint64_t bad_ending_here, int k) { return (bad_ending_here >> (64 - k)) != 0; }

// ---- the host's plain restatement (no device): what the kernels are held to ----
// The rule on one read with the counters given by the caller: counters[i] for window i of 0 .. n - k (not read when n < k).
// out[0..n) = seq with every byte under a bad window replaced by N; returns the bytes that changed.
// index_fastq: lines, roles and format clauses of a chunk.  Returns the clause of the smallest offending record (0 = none) with its
// 0-based number in bad_record.  final = false: the chunk may end inside a record, bytes_used = the end of the last whole record;
// final = true: the last line may lack its '\n', bytes_used = n.  read_off / read_len receive the sequence line of every whole record.
inline uint64_t mask_read(const char *seq, uint64_t n, uint32_t k, const uint32_t *counters, uint32_t low, uint32_t up, char *out) {
    uint64_t changed = 0, ending = 0;   // ending: bit 63 = window j is bad, bit 63 - t = window j - t
    const uint64_t n_windows = (k && n >= k) ? n - k + 1 : 0;
    for (uint64_t j = 0; j < n; ++j) {
        const bool bad = j < n_windows && pf_mask::window_bad(counters[j], low, up);
        ending = (ending >> 1) | ((uint64_t)bad << 63);
        const bool m = pf_mask::byte_masked(ending, (int)k);
        out[j] = m ? pf_mask::MASK_BYTE : seq[j];
        changed += m && seq[j] != pf_mask::MASK_BYTE;
    }
    return changed;
}

inline int index_fastq(const char *text, uint64_t n, bool final, uint64_t &bytes_used, uint64_t &n_records, uint64_t &bad_record,
                        std::vector<uint64_t> *read_off = nullptr, std::vector<uint32_t> *read_len = nullptr) {
    bytes_used = 0;
    n_records = 0;
    bad_record = 0;
    if (read_off) read_off->clear();
    if (read_len) read_len->clear();
    uint64_t b[4], e[4], pos = 0, line = 0;
    while (pos < n) {
        const char *nl = static_cast<const char *>(memchr(text + pos, '\n', n - pos));
        if (!nl && !final) break;   // the rest is carried
        const uint64_t end = nl ? (uint64_t)(nl - text) : n;
        const int role = pf_mask::line_role(line);
        b[role] = pos;
        e[role] = pf_mask::line_content_end(text, pos, end, nl != nullptr);
        pos = nl ? end + 1 : n;
        ++line;
        if (role == pf_mask::LINE_QUALITY) {
            const int clause = pf_mask::record_clause(text, b[0], e[0], e[1] - b[1], b[2], e[2], e[3] - b[3]);
            if (clause) { bad_record = n_records; return clause; }
            if (read_off) read_off->push_back(b[1]);
            if (read_len) read_len->push_back((uint32_t)(e[1] - b[1]));
            ++n_records;
            bytes_used = pos;
        }
    }
    if (final && line % 4) { bad_record = n_records; return pf_mask::CLAUSE_LINE_COUNT; }
    if (final) bytes_used = n;
    return pf_mask::CLAUSE_NONE;
}

}  // namespace pf_mask
