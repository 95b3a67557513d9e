// The row filter between the calling streams and the model, as `ploidyfrost filter` (host/pf_filter.cpp, the single-sample
// branch of run_filter) followed by `model -f` / `model -g` defines it -- as functions of one row of _bicov / _tricov / _tetracov /
// _pentacov text.  One definition for both sides, in the manner of pf_model_rows.hpp: the kernels of pf_call_model.hip call them
// with a lane per row, the host layer exports them (pfh_filter_rows) so that a CPU test holds the same code to the three-command
// chain.  The host filter is the definition; its parity with R is unpinned and stays so.
// The multi form (FilterRule::multi: `ploidyfrost filter-multi`, the opt.multi branch of run_filter) reads the rows of the colored
// tables -- A coverages, colour, isStrict, VarType, VarId, VarNum, Cramer's V, VarDis -- with the same functions.
#pragma once
#include "pf_model_rows.hpp"
#include <string>

namespace pf {

// FilterOptions of pf_filter.hpp without the prefixes; the long options as the doubles the predicates compare with
struct FilterRule {
    int simple, indel, snp;
    double low, up, num, distance, size;
    double fq;   // -q: frequencies kept in (fq, 1 - fq)
    // filter-multi: rows of A + 7 fields, Cramer's V > cramer (strictly), colour == color when color >= 0, no sum clause
    int multi;
    double cramer, color;
};
constexpr int FILTER_MAX_COLORS = 1024;   // colours a collection splits by (PF_MAX_COLORS)

constexpr int FILTER_TABLES = 4;    // bi, tri, tetra, penta
constexpr int FILTER_COLUMNS = 14;  // 2 + 3 + 4 + 5 frequency columns, table by table
PF_MODEL_HD inline int filter_column_base(int table) { return table == 0 ? 0 : table == 1 ? 2 : table == 2 ? 5 : 9; }

// Would write.table print this number in scientific notation?  The width rule above r_format_double (host/pf_filter.cpp), from
// the token's own digits: nsig = significant digits without trailing zeros, kp = decimal exponent of the first one.  (A token of
// at most 15 significant digits is the 15-digit rendering of its double, so the digits R sees are the token's.)
PF_MODEL_HD inline bool filter_r_scientific(bool neg, uint64_t m, int m_digits, int e10) {
    if (m == 0) return false;
    int nsig = m_digits;
    while (m % 10 == 0) { m /= 10; --nsig; }
    const int kp = m_digits - 1 + e10;
    const int left = kp + 1, rgt = nsig - kp - 1 > 0 ? nsig - kp - 1 : 0;
    const int w_fixed = (neg ? 1 : 0) + (left <= 0 ? 1 : left) + (rgt ? rgt + 1 : 0);
    const int mF = nsig - 1;
    const int w_sci = (neg ? 1 : 0) + (mF > 0 ? 1 : 0) + mF + 4 + ((kp >= 100 || kp <= -100) ? 2 : 1);
    return w_fixed > w_sci;
}

// atoi of R's fixed rendering of x: the integer part through strtol (saturating) and its low half
PF_MODEL_HD inline int filter_cov_int(double x) {
    long long v;
    if (x >= 9223372036854775807.0) v = 0x7FFFFFFFFFFFFFFFll;
    else if (x <= -9223372036854775807.0) v = (long long)0x8000000000000000ull;
    else v = (long long)x;   // (truncates toward zero, as the digits left of the point do)
    return (int)(uint32_t)(uint64_t)v;
}

// nearbyintl((long double)x * 1e7L) for x >= 0 without a long double: the 53-bit mantissa times 10^7 exactly in 128 bits, rounded
// to 64 significant bits (the x87 product), then to an integer, both ties-to-even.  The chain's model reads
// strtod(r_format_double(r_round7(x))), which is (double)n / 1e7 of this n (tests/test_filter_rows_cpu.py holds both).
PF_MODEL_HD inline uint64_t filter_scaled_round7(double x) {
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    const int be = (int)((bits >> 52) & 0x7FF);
    const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
    const uint64_t M = be ? (frac | (1ull << 52)) : frac;
    int e = be ? be - 1075 : -1074;
    if (M == 0) return 0;
    const uint64_t C = 10000000ull;
    const uint64_t pl = (M & 0xFFFFFFFFull) * C, ph = (M >> 32) * C;   // < 2^56, < 2^45
    uint64_t lo = pl + (ph << 32);
    uint64_t hi = (ph >> 32) + (lo < pl ? 1 : 0);
    uint64_t P = lo;   // the product's 64 leading bits, value = P * 2^e
    if (hi) {
        const int s = 64 - __builtin_clzll(hi);   // 1 .. 13
        const uint64_t rem = lo & ((1ull << s) - 1), half = 1ull << (s - 1);
        P = (hi << (64 - s)) | (lo >> s);
        e += s;
        if (rem > half || (rem == half && (P & 1))) {
            if (++P == 0) { P = 1ull << 63; ++e; }
        }
    }
    if (e >= 0) return e < 64 ? P << e : ~0ull;   // (x >= 2^40: never a frequency)
    const int k = -e;
    if (k > 64) return 0;
    if (k == 64) return P > (1ull << 63) ? 1 : 0;
    uint64_t n = P >> k;
    const uint64_t rem = P & ((1ull << k) - 1), half = 1ull << (k - 1);
    if (rem > half || (rem == half && (n & 1))) ++n;
    return n;
}

// One row of a *cov stream of A = 2 .. 5 alleles: read as read_table reads it (every cell, kept or not), then run_filter's
// predicates (pf_filter.cpp:192-212) in fp64.  cov[A] = the coverages, sci = bit c set where R would print coverage c in
// scientific notation.  Returns whether the row is kept; *err = MODEL_ROW_FIELDS / _BAD_TOKEN / _RANGE names what read_table refuses.
// The multi form has the colour behind the coverages and Cramer's V in front of VarDis (A + 7 fields; Filter-multi.R:114-120 has no
// clause on the sum of the first four coverages); *colour = the row's colour cell (single-sample rows: -1).
PF_MODEL_HD inline bool filter_row(const char *s, uint32_t len, int A, const FilterRule &f, double *cov, uint32_t *sci, int *err, double *colour = nullptr) {
    *err = MODEL_ROW_OK;
    *sci = 0;
    if (colour) *colour = -1;
    const int want = A + (f.multi ? 7 : 5);
    int fields = 0;
    for (uint32_t i = 0; i < len;) {   // fields as `in >> token` cuts them: runs of anything but white space
        while (i < len && model_isspace(s[i])) ++i;
        if (i >= len) break;
        while (i < len && !model_isspace(s[i])) ++i;
        ++fields;
    }
    if (fields != want) { *err = MODEL_ROW_FIELDS; return false; }
    double tail[7];   // isStrict VarType VarId VarNum VarDis; multi: colour isStrict VarType VarId VarNum Cramer VarDis
    uint32_t i = 0;
    for (int c = 0; c < want; ++c) {
        while (i < len && model_isspace(s[i])) ++i;
        uint32_t t = i;
        while (t < len && !model_isspace(s[t])) ++t;
        bool neg;
        uint64_t m;
        int digits, e10;
        double v;
        int st = model_token_parts(s + i, t - i, &neg, &m, &digits, &e10);
        if (st == MODEL_ROW_OK) st = model_fre_token(s + i, t - i, &v);
        if (st != MODEL_ROW_OK) { *err = st; return false; }
        if (c < A) {
            cov[c] = v;
            if (filter_r_scientific(neg, m, digits, e10)) *sci |= 1u << c;
        } else tail[c - A] = v;
        i = t;
    }
    const int t0 = f.multi ? 1 : 0;
    const double strict = tail[t0], type = tail[t0 + 1], num = tail[t0 + 3], dis = tail[f.multi ? 6 : 4];
    if (f.multi && colour) *colour = tail[0];
    bool k = true;
    if (f.simple) k = k && strict == 1;
    if (f.indel) k = k && type == 0;
    if (f.snp) k = k && type > 0;
    double first4 = 0;
    for (int c = 0; c < A; ++c) {
        k = k && cov[c] > f.low && cov[c] < f.up;
        if (c < 4) first4 += cov[c];
    }
    if (!f.multi && A >= 4) k = k && first4 < f.up;   // the penta row's fifth coverage is not in the sum
    k = k && num < f.num && dis > f.distance && type < f.size;
    if (f.multi) {
        k = k && tail[5] > f.cramer;
        if (f.color >= 0) k = k && tail[0] == f.color;
    }
    return k;
}

// source cov: what `model -f` makes of the row the filter wrote -- R's rendering of each coverage through atoi, then the rest of
// model_cov_row.  The penta table is written and never read.  A kept coverage R prints in scientific notation is refused
// (MODEL_ROW_R_SCI): atoi would read its leading digit, and which rendering a tri / tetra column gets depends on the whole column.
PF_MODEL_HD inline int filter_cov_row(const char *s, uint32_t len, int A, const FilterRule &f, double q, double *out, bool *kept, int *err, double *colour = nullptr) {
    double cov[5];
    uint32_t sci;
    *kept = filter_row(s, len, A, f, cov, &sci, err, colour);
    if (!*kept || A > 4) return 0;
    if (sci) { *err = MODEL_ROW_R_SCI; return 0; }
    int ci[4];
    for (int c = 0; c < A; ++c) ci[c] = filter_cov_int(cov[c]);
    return model_cov_ints(ci, A, q, out, err);
}

// source fre: the tokens the row adds to the filter's <out>_allele_frequency.txt, as the model reads them back.  x_c = cov_c / sum
// (sum left to right), written iff fq < x_c < 1 - fq on the unrounded value; out[c] = the written token's value.  Returns the mask
// of written columns.  (The model's own test, model_fre_keep, comes behind: the file's last token counts twice whether kept or not.)
PF_MODEL_HD inline uint32_t filter_fre_row(const char *s, uint32_t len, int A, const FilterRule &f, double *out, bool *kept, int *err, double *colour = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double cov[5];
    uint32_t sci;
    *kept = filter_row(s, len, A, f, cov, &sci, err, colour);
    if (!*kept) return 0;
    double sum = 0;
    for (int c = 0; c < A; ++c) sum += cov[c];
    uint32_t mask = 0;
    for (int c = 0; c < A; ++c) {
        const double x = cov[c] / sum;
        if (x > f.fq && x < 1 - f.fq) {
            out[c] = (double)filter_scaled_round7(x) / 1e7;
            mask |= 1u << c;
        }
    }
    return mask;
}

// A collection that splits its values by colour keys each value with its row's colour: an integer 0 .. FILTER_MAX_COLORS - 1, or -1
// for a cell that is none (a kept row with such a cell is refused: MODEL_ROW_COLOR)
PF_MODEL_HD inline int filter_color_key(double colour) {
    if (!(colour >= 0 && colour < (double)FILTER_MAX_COLORS)) return -1;
    const int k = (int)colour;
    return (double)k == colour ? k : -1;
}

// ---- the words for what a filtered collection refuses, one wording for the device path and pfh_filter_rows ----
// What read_table refuses (a row without its fields, a cell that is no finite decimal number) comes before everything else, as the
// filter reads its four tables before it decides a row; what the model says of the kept rows comes last.
PF_MODEL_HD inline bool filter_err_is_late(int code) { return code == MODEL_ROW_COV_ZERO || code == MODEL_ROW_R_SCI || code == MODEL_ROW_NO_ROOM; }

inline const char *filter_stream_name(int table) {
    static const char *name[FILTER_TABLES] = {"_bicov", "_tricov", "_tetracov", "_pentacov"};
    return name[table & 3];
}
// (R's error when no table keeps a row: fre_all is still NULL)
inline const char *filter_none_kept_text() {
    return "Error in round(fre_all[fre_all > opt$frequency & fre_all < (1 - opt$frequency)],  : \n  non-numeric argument to mathematical function";
}
inline std::string filter_error_text(int code, int table, unsigned long long row /* from 1 */, bool multi = false) {
    const std::string stream = std::string("stream ") + filter_stream_name(table), r = std::to_string(row);
    switch (code) {
        case MODEL_ROW_FIELDS:
            return "Error in scan(file = file, what = what, sep = sep, quote = quote, dec = dec,  : \n  line " + r + " did not have " + std::to_string(table + (multi ? 9 : 7)) +
                   " elements (" + stream + ")";
        case MODEL_ROW_BAD_TOKEN:
            return "pf_filter: a cell in line " + r + " of " + stream +
                   " is not a finite decimal number; R reads it as NA/NaN/Inf (or not at all) and the scripts' row predicates then give NA rows -- refused (parity unpinned)";
        case MODEL_ROW_RANGE:
            return "ERROR: row " + r + " of " + stream + " holds a number outside what the device converts exactly (more than 15 digits or a decimal exponent beyond 22)";
        case MODEL_ROW_COV_ZERO:
            return "Model::readCovFile() : row " + r + " of " + stream + ", kept by the filter, sums to 0 (the reference divides by it)";
        case MODEL_ROW_R_SCI:
            return "ERROR: row " + r + " of " + stream + " is kept with a coverage that R's write.table prints in scientific notation (1e+05, 1e-04); `model -f` reads such a cell "
                   "by its leading digit -- not reproduced here: the three-command chain (ploidyfrost, filter, model -f) handles this input";
        case MODEL_ROW_COLOR:
            return "ERROR: row " + r + " of " + stream + " is kept with a colour that is no integer in 0 .. " + std::to_string(FILTER_MAX_COLORS - 1) +
                   " (the values of a run are split by the colour column)";
        default:
            return "pf_call_model_finish: row " + r + " of " + stream + " has more values than its text allows";
    }
}

}  // namespace pf
