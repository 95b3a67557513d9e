// The rule of `ploidyfrost qc` and of `--report` (K-QC) in one place, for the kernel (pf_qc.hip), the host layer (host/pf_qc_host.cpp)
// and the stand-alone test (tests/cpp/test_qc_rule.cpp): what a read adds to a table, the words of a table, the hint about the
// quality offset, the text of the report, and a plain host restatement.  Integers only.
//
// A TABLE belongs to a (side, stage) pair.  Side 0: single-ended calls and file 1 of a pair; side 1: file 2.  Stage RAW: every whole
// record of a chunk with the interval [0, n).  Stage KEPT: every record K-TRIM keeps, with its final interval [b, e), the clip
// included; a dropped record adds nothing.  One record with the sequence line s, the quality line u, [b, e) and L = e - b:
//   reads += 1, length[min(L, 1024)] += 1, min_len and max_len take L;
//   for p in [b, e), i = p - b, bin = min(i, 1023) (the last bin pools everything from position 1023 on):
//     pos_base[bin][class] += 1        class: Aa 0, Cc 1, Gg 2, Tt 3, anything else 4
//     q = (int)u[p] - phred, qc = clamp(q, 0, 93)
//     pos_qsum[bin] += qc, pos_q20[bin] += (q >= 20), pos_q30[bin] += (q >= 30), quality[qc] += 1
//     qual_low += (q < 0), qual_high += (q > 93), min_byte and max_byte take u[p];
//   when L > 0: read_quality[floor(sum qc / L)] += 1; with acgt the bases of class below 4 and gc those of class 1 or 2:
//     acgt > 0: gc_percent[floor(100 * gc / acgt)] += 1, else reads_no_acgt += 1.
// The totals (bases, bases_acgt, gc, q20, q30) are sums over the position rows and are not stored.  With a clip open a side has one
// more table: clip[min(clip_end, 1024)] += 1 for every record with clip_end < n -- the curve of insert sizes.
// Everything is a sum, a minimum or a maximum: the result depends on neither chunking nor lanes nor the order of atomics.
//
// THE WORDS of a table, all uint64_t (pf_qc_get; the ABI header restates TABLE_WORDS and CLIP_WORDS):
//   W_SEEN 1 when a call with at least one whole record has added to the table, W_READS, W_MIN_LEN, W_MAX_LEN, W_MIN_BYTE, W_MAX_BYTE
//   (the minima are 0 while nothing has been seen: an untouched table is all zero), W_QUAL_LOW, W_QUAL_HIGH, W_READS_NO_ACGT,
//   W_LENGTH[1025], W_QUALITY[94], W_READ_QUALITY[94], W_GC_PERCENT[101], W_POS_BASE[1024][5], W_POS_QSUM[1024], W_POS_Q20[1024],
//   W_POS_Q30[1024].
//
// THE REPORT is text, tab-separated, a function of the tables alone (report_text below is the definition; sides print as 1 and 2,
// stages as raw and kept):
//   # ploidyfrost qc 1
//   # phred P hint H
//   >>totals        side stage reads bases bases_acgt gc q20 q30 qual_low qual_high min_len max_len min_byte max_byte reads_no_acgt
//                   one row per (side, stage) that is seen
//   >>position      side stage pos reads_here A C G T other qsum q20 q30     pos 0 .. the last non-empty bin; bin 1023 is written 1023+
//                   (reads_here = A + C + G + T + other: the reads that reach the position; in the pooled bin, its bases)
//   >>length        side stage length reads              non-zero rows, ascending; 1024 is written 1024+
//   >>quality       side stage quality bases
//   >>read_quality  side stage mean_quality reads
//   >>gc_percent    side stage gc_percent reads
//   >>clip          side clip_end reads                  1024 is written 1024+
#pragma once
#include <stdint.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "pf_clip_rule.hpp"
#include "pf_mask_rule.hpp"
#include "pf_trim_rule.hpp"

#if defined(__HIPCC__)
#define PF_QC_HD __host__ __device__
#else
#define PF_QC_HD
#endif

namespace pf_qc {

constexpr uint32_t POS_BINS = 1024, LEN_BINS = 1025, Q_BINS = 94, GC_BINS = 101, CLASSES = 5;
constexpr uint32_t Q_MAX = 93;
enum Stage { STAGE_RAW = 0, STAGE_KEPT = 1, STAGES = 2 };
enum Word : uint32_t {
    W_SEEN = 0, W_READS, W_MIN_LEN, W_MAX_LEN, W_MIN_BYTE, W_MAX_BYTE, W_QUAL_LOW, W_QUAL_HIGH, W_READS_NO_ACGT,
    W_LENGTH,
    W_QUALITY = W_LENGTH + LEN_BINS,
    W_READ_QUALITY = W_QUALITY + Q_BINS,
    W_GC_PERCENT = W_READ_QUALITY + Q_BINS,
    W_POS_BASE = W_GC_PERCENT + GC_BINS,
    W_POS_QSUM = W_POS_BASE + POS_BINS * CLASSES,
    W_POS_Q20 = W_POS_QSUM + POS_BINS,
    W_POS_Q30 = W_POS_Q20 + POS_BINS,
    TABLE_WORDS = W_POS_Q30 + POS_BINS
};
constexpr uint32_t CLIP_WORDS = LEN_BINS;
static_assert(TABLE_WORDS == 9515, "the ABI header restates the number");

// ---- the rule's pieces, shared with the kernel ----
PF_QC_HD inline uint32_t base_class(uint8_t c) {
    const uint8_t u = c & 0xDFu;   // upper case
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}
PF_QC_HD inline int quality(uint8_t byte, uint32_t phred) { return (int)byte - (int)phred; }
PF_QC_HD inline uint32_t quality_clamped(int q) { return q < 0 ? 0u : q > (int)Q_MAX ? Q_MAX : (uint32_t)q; }
PF_QC_HD inline uint32_t pos_bin(uint32_t i) { return i < POS_BINS - 1 ? i : POS_BINS - 1; }
PF_QC_HD inline uint32_t len_bin(uint32_t L) { return L < LEN_BINS - 1 ? L : LEN_BINS - 1; }
PF_QC_HD inline uint32_t mean_quality_bin(uint64_t sum_qc, uint32_t L) { return (uint32_t)(sum_qc / L); }      // L > 0
PF_QC_HD inline uint32_t gc_percent_bin(uint32_t gc, uint32_t acgt) { return (uint32_t)(100ull * gc / acgt); }   // acgt > 0
PF_QC_HD inline bool is_min_word(uint32_t w) { return w == W_MIN_LEN || w == W_MIN_BYTE; }
PF_QC_HD inline bool is_max_word(uint32_t w) { return w == W_SEEN || w == W_MAX_LEN || w == W_MAX_BYTE; }

// 33: a quality byte below 59 was seen (phred 64 has none); 64: reads were seen and no byte is below 64; else 0 (undecided)
inline uint32_t phred_hint(uint64_t min_byte, uint64_t reads_with_bases) {
    if (reads_with_bases == 0) return 0;
    if (min_byte < 59) return 33;
    if (min_byte >= 64) return 64;
    return 0;
}

// ---- the host's plain restatement (no device): what the kernel is held to ----
inline void take_min(uint64_t &cell, bool first, uint64_t v) { if (first || v < cell) cell = v; }
// one record into a table: the lines s and u, the interval [b, e)
inline void add_record(uint64_t *t, const char *s, const char *u, uint32_t b, uint32_t e, uint32_t phred) {
    const uint32_t L = e - b;
    const bool no_byte_yet = t[W_MAX_LEN] == 0;   // (no record with L > 0 so far)
    take_min(t[W_MIN_LEN], t[W_READS] == 0, L);
    if (L > t[W_MAX_LEN]) t[W_MAX_LEN] = L;
    t[W_READS] += 1;
    t[W_LENGTH + len_bin(L)] += 1;
    uint64_t sum_qc = 0;
    uint32_t gc = 0, acgt = 0;
    for (uint32_t p = b; p < e; ++p) {
        const uint32_t bin = pos_bin(p - b), cls = base_class((uint8_t)s[p]);
        const uint8_t byte = (uint8_t)u[p];
        const int q = quality(byte, phred);
        const uint32_t qc = quality_clamped(q);
        t[W_POS_BASE + bin * CLASSES + cls] += 1;
        t[W_POS_QSUM + bin] += qc;
        t[W_POS_Q20 + bin] += q >= 20;
        t[W_POS_Q30 + bin] += q >= 30;
        t[W_QUALITY + qc] += 1;
        t[W_QUAL_LOW] += q < 0;
        t[W_QUAL_HIGH] += q > (int)Q_MAX;
        take_min(t[W_MIN_BYTE], no_byte_yet && p == b, byte);
        if (byte > t[W_MAX_BYTE]) t[W_MAX_BYTE] = byte;
        sum_qc += qc;
        acgt += cls < 4;
        gc += cls == 1 || cls == 2;
    }
    if (L == 0) return;
    t[W_READ_QUALITY + mean_quality_bin(sum_qc, L)] += 1;
    if (acgt) t[W_GC_PERCENT + gc_percent_bin(gc, acgt)] += 1; else t[W_READS_NO_ACGT] += 1;
}

// the simple adapters of a clip, as pf_clip::clip_read takes them (n_adapters == 0 with `open`: a clip that clips nothing)
struct ClipSet {
    bool open = false;
    const char *bases = nullptr;
    const uint32_t *off = nullptr;
    const uint8_t *side = nullptr;
    uint32_t n_adapters = 0, seed = pf_clip::DEFAULT_SEED, score = pf_clip::DEFAULT_SCORE;
};
// One chunk of one file: the index of pf_mask::index_fastq (its clause is returned with bad_record, nothing is added then), every
// whole record into `raw`; with `trimmed`, every record's interval by pf_clip::clip_read and pf_trim::trim_read, the kept ones into
// `kept`, and with a clip open the clip ends into `clip`.  file_side: 1 or 2 (which adapters apply).  The tables are added to.
inline int qc_fastq_chunk(const char *text, uint64_t n, bool final, uint32_t phred, uint32_t file_side, bool trimmed, const pf_trim::Step *steps,
                          uint32_t n_steps, const ClipSet &cs, uint64_t *raw, uint64_t *kept, uint64_t *clip, uint64_t &bytes_used, uint64_t &n_records,
                          uint64_t &bad_record) {
    const int clause = pf_mask::index_fastq(text, n, final, bytes_used, n_records, bad_record);
    if (clause) { bytes_used = 0; n_records = 0; return clause; }
    if (n_records == 0) return pf_mask::CLAUSE_NONE;
    std::vector<uint64_t> lb, le;
    pf_trim::record_lines(text, bytes_used, n_records, lb, le);
    raw[W_SEEN] = 1;
    if (trimmed) kept[W_SEEN] = 1;
    for (uint64_t r = 0; r < n_records; ++r) {
        const char *s = text + lb[4 * r + 1], *u = text + lb[4 * r + 3];
        const uint32_t nq = (uint32_t)(le[4 * r + 3] - lb[4 * r + 3]);
        add_record(raw, s, u, 0, nq, phred);
        if (!trimmed) continue;
        uint32_t ce = nq;
        if (cs.open) {
            ce = pf_clip::clip_read(s, u, nq, cs.bases, cs.off, cs.side, cs.n_adapters, file_side, cs.seed, cs.score, phred);
            if (ce < nq && clip) clip[len_bin(ce)] += 1;
        }
        uint32_t b = 0, e = 0;
        if (pf_trim::trim_read(u, ce, steps, n_steps, phred, b, e)) add_record(kept, s, u, b, e, phred);
    }
    return pf_mask::CLAUSE_NONE;
}

// ---- the totals and the report ----
struct Totals {
    uint64_t bases = 0, bases_acgt = 0, gc = 0, q20 = 0, q30 = 0;
};
inline Totals totals_of(const uint64_t *t) {
    Totals o;
    for (uint32_t bin = 0; bin < POS_BINS; ++bin) {
        const uint64_t *c = t + W_POS_BASE + bin * CLASSES;
        o.bases += c[0] + c[1] + c[2] + c[3] + c[4];
        o.bases_acgt += c[0] + c[1] + c[2] + c[3];
        o.gc += c[1] + c[2];
        o.q20 += t[W_POS_Q20 + bin];
        o.q30 += t[W_POS_Q30 + bin];
    }
    return o;
}
// tables: [side][stage][TABLE_WORDS]; the hint over the raw stage of both sides; *lo, *hi (may be null): the bytes it was taken from
inline uint32_t hint_of(const uint64_t *tables, uint64_t *lo = nullptr, uint64_t *hi = nullptr) {
    uint64_t seen = 0, mn = 0, mx = 0;
    for (uint32_t side = 0; side < 2; ++side) {
        const uint64_t *t = tables + (size_t)(side * STAGES + STAGE_RAW) * TABLE_WORDS;
        if (t[W_MAX_LEN] == 0) continue;   // (no quality byte on this side)
        take_min(mn, seen == 0, t[W_MIN_BYTE]);
        if (t[W_MAX_BYTE] > mx) mx = t[W_MAX_BYTE];
        seen += 1;
    }
    if (lo) *lo = mn;
    if (hi) *hi = mx;
    return phred_hint(mn, seen);
}
inline const char *stage_name(uint32_t stage) { return stage == STAGE_RAW ? "raw" : "kept"; }
// clip: [side][CLIP_WORDS], or null (no clip was open: the section is empty)
inline std::string report_text(const uint64_t *tables, const uint64_t *clip, uint32_t phred) {
    auto n = [](uint64_t v) { return std::to_string(v); };
    std::string o = "# ploidyfrost qc 1\n# phred " + n(phred) + " hint " + n(hint_of(tables)) + "\n";
    auto each = [&](const std::function<void(uint32_t, uint32_t, const uint64_t *, const std::string &)> &f) {
        for (uint32_t side = 0; side < 2; ++side)
            for (uint32_t stage = 0; stage < STAGES; ++stage) {
                const uint64_t *t = tables + (size_t)(side * STAGES + stage) * TABLE_WORDS;
                if (t[W_SEEN]) f(side, stage, t, n(side + 1) + "\t" + stage_name(stage) + "\t");
            }
    };
    o += ">>totals\nside\tstage\treads\tbases\tbases_acgt\tgc\tq20\tq30\tqual_low\tqual_high\tmin_len\tmax_len\tmin_byte\tmax_byte\treads_no_acgt\n";
    each([&](uint32_t, uint32_t, const uint64_t *t, const std::string &head) {
        const Totals s = totals_of(t);
        o += head + n(t[W_READS]) + "\t" + n(s.bases) + "\t" + n(s.bases_acgt) + "\t" + n(s.gc) + "\t" + n(s.q20) + "\t" + n(s.q30) + "\t" + n(t[W_QUAL_LOW]) + "\t" +
             n(t[W_QUAL_HIGH]) + "\t" + n(t[W_MIN_LEN]) + "\t" + n(t[W_MAX_LEN]) + "\t" + n(t[W_MIN_BYTE]) + "\t" + n(t[W_MAX_BYTE]) + "\t" + n(t[W_READS_NO_ACGT]) + "\n";
    });
    o += ">>position\nside\tstage\tpos\treads_here\tA\tC\tG\tT\tother\tqsum\tq20\tq30\n";
    each([&](uint32_t, uint32_t, const uint64_t *t, const std::string &head) {
        uint32_t rows = 0;
        for (uint32_t bin = 0; bin < POS_BINS; ++bin) {
            const uint64_t *c = t + W_POS_BASE + bin * CLASSES;
            if (c[0] + c[1] + c[2] + c[3] + c[4]) rows = bin + 1;
        }
        for (uint32_t bin = 0; bin < rows; ++bin) {
            const uint64_t *c = t + W_POS_BASE + bin * CLASSES;
            o += head + n(bin) + (bin == POS_BINS - 1 ? "+" : "") + "\t" + n(c[0] + c[1] + c[2] + c[3] + c[4]);
            for (uint32_t k = 0; k < CLASSES; ++k) o += "\t" + n(c[k]);
            o += "\t" + n(t[W_POS_QSUM + bin]) + "\t" + n(t[W_POS_Q20 + bin]) + "\t" + n(t[W_POS_Q30 + bin]) + "\n";
        }
    });
    auto hist = [&](const char *title, const char *columns, uint32_t word, uint32_t bins, bool pooled) {
        o += std::string(">>") + title + "\nside\tstage\t" + columns + "\n";
        each([&](uint32_t, uint32_t, const uint64_t *t, const std::string &head) {
            for (uint32_t i = 0; i < bins; ++i)
                if (t[word + i]) o += head + n(i) + (pooled && i == bins - 1 ? "+" : "") + "\t" + n(t[word + i]) + "\n";
        });
    };
    hist("length", "length\treads", W_LENGTH, LEN_BINS, true);
    hist("quality", "quality\tbases", W_QUALITY, Q_BINS, false);
    hist("read_quality", "mean_quality\treads", W_READ_QUALITY, Q_BINS, false);
    hist("gc_percent", "gc_percent\treads", W_GC_PERCENT, GC_BINS, false);
    o += ">>clip\nside\tclip_end\treads\n";
    for (uint32_t side = 0; side < 2 && clip; ++side)
        for (uint32_t i = 0; i < CLIP_WORDS; ++i)
            if (clip[(size_t)side * CLIP_WORDS + i]) o += n(side + 1) + "\t" + n(i) + (i == CLIP_WORDS - 1 ? "+" : "") + "\t" + n(clip[(size_t)side * CLIP_WORDS + i]) + "\n";
    return o;
}
// the `qc:` line of a side on stderr, from its raw table
inline std::string side_line(uint32_t side, const uint64_t *raw) {
    auto n = [](uint64_t v) { return std::to_string(v); };
    const Totals s = totals_of(raw);
    return "qc: side " + n(side + 1) + " reads " + n(raw[W_READS]) + " bases " + n(s.bases) + " q20 " + n(s.q20) + " q30 " + n(s.q30) + " gc " + n(s.gc) + " min_len " +
           n(raw[W_MIN_LEN]) + " max_len " + n(raw[W_MAX_LEN]);
}
// the warning when the hint disagrees with the offset in use ("" = none)
inline std::string hint_line(const uint64_t *tables, uint32_t phred) {
    uint64_t lo = 0, hi = 0;
    const uint32_t h = hint_of(tables, &lo, &hi);
    if (h == 0 || h == phred) return "";
    return "qc: quality bytes run from " + std::to_string(lo) + " to " + std::to_string(hi) + ": the files look like phred " + std::to_string(h) + ", not " +
           std::to_string(phred);
}

}  // namespace pf_qc
