// The rule of `--fasta` (K-FASTA) in one place, for the kernels (pf_fasta.hip), the host restatement and the stand-alone test
// (tests/cpp/test_fasta_rule.cpp): what a FASTA text says, and how it becomes what the cores of K-COUNT, K-MASKCOUNT and K-COLOR take --
// a byte text and a table (read_off, read_len).
//
//   lines      end at '\n'; a '\r' directly in front of that '\n' belongs to the line end (pf_mask::line_content_end).  A last line
//              may lack its '\n' (then a '\r' at its end is content).
//   header     a line whose first byte is '>'.  It opens a record; none of its bytes is sequence.
//   sequence   every other line is a sequence line of the record opened last; an empty line is an empty sequence line.  A '>'
//              anywhere but at a line start is a sequence byte.  No byte is refused: what is not in ACGTacgt breaks the windows over
//              it, as in FASTQ (pf_count_rule.hpp).
//   record     its sequence is the contents of its sequence lines, one behind the other.  No sequence byte: a read of length 0.
//   counts     reads = headers, bases = sequence bytes.
//   compacted  the sequences of the whole records of a chunk, one directly behind the other without a separator (reads may touch:
//              pf_run_rule.hpp; the cores take window starts from the table alone).  The table is (read_off, read_len) into it, ascending.
//   chunk      whole records, bytes_used, final -- the FASTQ contract (pf_mask::index_fastq) with FASTA's meaning of "whole": in a
//              chunk that is not final a record is whole when a later header line starts inside the chunk, and bytes_used is the
//              first byte of the last line that starts with '>' (a chunk with one such line: no record, bytes_used 0 -- the caller
//              carries all of it).  In a final chunk every record is whole.  No state crosses chunks.
//   start      a chunk starts at a record start: its first byte is '>'.  Sequence in front of the first header has no record and is
//              refused (CLAUSE_NO_HEADER).
//
// The equivalence everything else follows from: Q(F) = F with every record rewritten as the four FASTQ lines "@" + header without
// its '>', the joined sequence, "+", and 'I' once per base.  What a sub-command makes of F with --fasta is what it makes of Q(F).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pf_mask_rule.hpp"

namespace pf_fasta {

constexpr char HEADER_BYTE = '>';
enum Clause { CLAUSE_NONE = 0, CLAUSE_NO_HEADER };
inline const char *clause_text(int c) {
    return c == CLAUSE_NO_HEADER ? "the text does not start with '>' (a FASTA chunk starts at a record start)" : "no refusal";
}

PF_MASK_HD inline bool is_header_line(const char *text, uint64_t n, uint64_t line_begin) { return line_begin < n && text[line_begin] == HEADER_BYTE; }
PF_MASK_HD inline uint64_t bit_span(uint64_t a, uint64_t b) {   // bits a .. b - 1 of a word, 0 <= a <= b <= 64
    if (b <= a) return 0;
    const uint64_t len = b - a;
    return (len >= 64 ? ~0ull : ((1ull << len) - 1)) << a;
}

// ---- the word form: what one 64-byte word of the text holds, from the newline bitmap of the word and the start of the line that
// holds the word's first byte.  content: bit b = byte 64 w + b is a sequence byte; heads: bit b = a header line starts at
// byte 64 w + b.  Walks the lines that meet the word: a handful of byte loads at their first and last bytes, nothing else. ----
struct WordMasks { uint64_t content, heads; };
// the line from `begin` whose content ends at content_end, as far as it lies in the word [lo, hi)
PF_MASK_HD inline WordMasks word_line(const char *text, uint64_t n, uint64_t lo, uint64_t hi, uint64_t begin, uint64_t content_end, WordMasks m) {
    const bool header = is_header_line(text, n, begin);
    const uint64_t a = begin > lo ? begin : lo, b = content_end < hi ? content_end : hi;
    if (header && begin >= lo && begin < hi) m.heads |= 1ull << (begin - lo);
    if (!header && b > a) m.content |= bit_span(a - lo, b - lo);
    return m;
}
PF_MASK_HD inline WordMasks word_content(const char *text, uint64_t n, uint64_t w, uint64_t newlines, uint64_t first_line_begin) {
    const uint64_t lo = w * 64, hi = lo + 64 < n ? lo + 64 : n;
    WordMasks m = {0, 0};
    uint64_t begin = first_line_begin;
    while (newlines) {
        const int b = __builtin_ctzll(newlines);
        newlines &= newlines - 1;
        const uint64_t end = lo + (uint64_t)b;
        m = word_line(text, n, lo, hi, begin, pf_mask::line_content_end(text, begin, end, true), m);
        begin = end + 1;
    }
    if (begin < hi) {   // the line that goes on behind the word: only a line end directly behind it reaches back into it
        const bool ends_here = hi < n && text[hi] == '\n';
        m = word_line(text, n, lo, hi, begin, ends_here ? pf_mask::line_content_end(text, begin, hi, true) : hi, m);
    }
    return m;
}
// the sequence bytes in front of byte i, from the exclusive sums of the words' content counts (pos has an entry behind the last word)
PF_MASK_HD inline uint64_t content_rank(const uint64_t *content, const uint32_t *pos, uint64_t n_words, uint64_t i) {
    const uint64_t w = i >> 6;
    if (w >= n_words) return pos[n_words];
    const uint64_t below = content[w] & (((uint64_t)1 << (i & 63)) - 1);
    return (uint64_t)pos[w] + (uint64_t)__builtin_popcountll(below);
}

// ---- the host's plain restatement (no device): what the kernels are held to ----
struct Index {
    uint64_t bytes_used = 0, n_records = 0, bases = 0;
    std::vector<char> text;            // the compacted text: `bases` bytes
    std::vector<uint64_t> read_off;    // n_records entries
    std::vector<uint32_t> read_len;
};
// Lines split at '\n', joined per record.  Returns the clause (0 = none).
inline int index_fasta(const char *text, uint64_t n, bool final, Index &ix) {
    ix = Index{};
    if (n && text[0] != HEADER_BYTE) return CLAUSE_NO_HEADER;
    uint64_t pos = 0, open_text = 0;   // open_text: the compacted bytes when the open record's header was met
    bool open = false;
    std::vector<char> out;
    auto close_record = [&](uint64_t upto) {
        ix.read_off.push_back(open_text);
        ix.read_len.push_back((uint32_t)(out.size() - open_text));
        ix.n_records += 1;
        ix.bytes_used = upto;
    };
    while (pos < n) {
        const char *nl = static_cast<const char *>(memchr(text + pos, '\n', n - pos));
        const uint64_t end = nl ? (uint64_t)(nl - text) : n;
        if (text[pos] == HEADER_BYTE) {
            if (open) close_record(pos);
            open = true;
            open_text = out.size();
        } else {
            const uint64_t ce = pf_mask::line_content_end(text, pos, end, nl != nullptr);
            out.insert(out.end(), text + pos, text + ce);
        }
        pos = nl ? end + 1 : n;
    }
    if (final) {
        if (open) close_record(n);
        ix.bytes_used = n;
    } else if (ix.n_records) out.resize((size_t)(ix.read_off.back() + ix.read_len.back()));   // the open record is carried
    else out.clear();
    ix.bases = out.size();
    ix.text = std::move(out);
    return CLAUSE_NONE;
}

// The word form on the host, stage by stage as pf_fasta.hip runs it: newline bitmaps, line starts, word_content, the exclusive sums,
// compaction by rank, the table from the header starts.  Gives what index_fasta gives (tests/cpp/test_fasta_rule.cpp).
inline int index_fasta_words(const char *text, uint64_t n, bool final, Index &ix) {
    ix = Index{};
    if (n && text[0] != HEADER_BYTE) return CLAUSE_NO_HEADER;
    if (!n) return CLAUSE_NONE;
    const uint64_t n_words = (n + 63) / 64;
    std::vector<uint64_t> nl(n_words, 0), content(n_words, 0), heads(n_words, 0), line_start(1, 0), head_at;
    std::vector<uint32_t> pre(n_words, 0), pos(n_words + 1, 0);
    for (uint64_t i = 0; i < n; ++i)
        if (text[i] == '\n') { nl[i >> 6] |= 1ull << (i & 63); line_start.push_back(i + 1); }
    for (uint64_t w = 0, lines = 0; w < n_words; ++w) {
        pre[w] = (uint32_t)lines;
        lines += (uint64_t)__builtin_popcountll(nl[w]);
    }
    for (uint64_t w = 0; w < n_words; ++w) {
        const WordMasks m = word_content(text, n, w, nl[w], line_start[pre[w]]);
        content[w] = m.content;
        heads[w] = m.heads;
        pos[w + 1] = pos[w] + (uint32_t)__builtin_popcountll(content[w]);
        for (int b = 0; b < 64; ++b)
            if ((heads[w] >> b) & 1ull) head_at.push_back(w * 64 + (uint64_t)b);
    }
    const uint64_t n_heads = head_at.size();
    const uint64_t n_rec = final ? n_heads : (n_heads ? n_heads - 1 : 0);
    ix.n_records = n_rec;
    ix.bytes_used = final ? n : (n_heads ? head_at.back() : 0);
    if (!final && !n_rec) ix.bytes_used = 0;
    ix.bases = n_rec ? content_rank(content.data(), pos.data(), n_words, final ? n : ix.bytes_used) : 0;
    ix.text.resize((size_t)ix.bases);
    for (uint64_t i = 0; i < n; ++i)
        if ((content[i >> 6] >> (i & 63)) & 1ull) {
            const uint64_t at = content_rank(content.data(), pos.data(), n_words, i);
            if (at < ix.bases) ix.text[(size_t)at] = text[i];
        }
    for (uint64_t h = 0; h < n_rec; ++h) {
        const uint64_t a = content_rank(content.data(), pos.data(), n_words, head_at[h]);
        const uint64_t b = h + 1 < n_heads ? content_rank(content.data(), pos.data(), n_words, head_at[h + 1]) : ix.bases;
        ix.read_off.push_back(a);
        ix.read_len.push_back((uint32_t)(b - a));
    }
    return CLAUSE_NONE;
}

}  // namespace pf_fasta
