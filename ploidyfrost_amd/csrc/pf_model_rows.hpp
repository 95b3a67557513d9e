// The model's input values as the TEXT of the result streams defines them: the row rules of GmmModel::readCovFile /
// readFreFile (host/pf_gmm_model.cpp, reference src/GmmModel.cpp:21-257), quirks included, as functions of one row.  One
// definition for both sides: the kernels of pf_call_model.hip call them with a lane per row, the host layer exports them
// (pfh_model_rows) so that a CPU test holds the very same code to the file readers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_MODEL_HD __host__ __device__
#else
#define PF_MODEL_HD
#endif

namespace pf {

enum ModelSource : int { MODEL_COV = 0, MODEL_FRE = 1 };   // `model -f` / `model -g`
enum ModelRowErr : int {
    MODEL_ROW_OK = 0,
    MODEL_ROW_COV_ZERO = 1,    // the coverages of a row sum to 0 (the reference divides by it)
    MODEL_ROW_BAD_TOKEN = 2,   // a frequency row is not one number operator>>(double) reads ("nan", "inf", two tokens, none)
    MODEL_ROW_RANGE = 3,       // a number outside what one fp64 operation converts exactly (more than 15 digits, |exponent| > 22)
    MODEL_ROW_NO_ROOM = 4,     // device only: the value array was sized for fewer values than the rows give
    // with a row filter in front (pf_filter_rows.hpp)
    MODEL_ROW_FIELDS = 5,      // a coverage row that does not have its A + 5 fields (colored tables: A + 7)
    MODEL_ROW_R_SCI = 6,       // a kept coverage R's write.table renders in scientific notation (`model -f` then reads its leading digit)
    MODEL_ROW_COLOR = 7        // split by colour: a kept row whose colour cell is no integer 0 .. 1023
};

PF_MODEL_HD inline bool model_isspace(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// atoi(row + from) on a row of len characters (glibc: (int)strtol -- white space skipped, TABS INCLUDED, so an empty field reads
// the number of the next one; the long saturates, the int is its low half)
PF_MODEL_HD inline int model_atoi(const char *s, uint32_t len, uint32_t from) {
    uint32_t i = from;
    while (i < len && model_isspace(s[i])) ++i;
    bool neg = false;
    if (i < len && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; ++i; }
    const uint64_t lim = neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull;
    uint64_t v = 0;
    bool sat = false;
    for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i) {
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (sat || v > (lim - d) / 10) { sat = true; v = lim; }
        else v = v * 10 + d;
    }
    return (int)(uint32_t)(neg ? 0 - v : v);
}

// The part of a coverage row behind atoi: its n integers -> its values (model_cov_row below; the filtered rows of pf_filter_rows.hpp)
PF_MODEL_HD inline int model_cov_ints(const int *cov, int n, double q, double *out, int *err) {
    uint32_t usum = 0;
    for (int i = 0; i < n; ++i) usum += (uint32_t)cov[i];
    const int cov_sum = (int)usum;
    if (cov_sum >= 10000) return 0;
    if (cov_sum == 0) { *err = MODEL_ROW_COV_ZERO; return 0; }
    int lead = cov[0];
    for (int i = 1; i < n && n > 2; ++i)
        if (cov[i] < cov[i - 1]) lead = cov[i];
    const int qi = (cov_sum == -1) ? (int)(0u - (uint32_t)lead) : lead / cov_sum;
    if (!((double)qi >= q && (double)qi <= 1 - q)) return 0;
    for (int i = 0; i < n; ++i) out[i] = double(cov[i]) / cov_sum;
    return n;
}

// One row of <prefix>_bicov / _tricov / _tetracov.txt (n = 2 / 3 / 4): the values it adds to the model's array, 0 or n of them.
// The first n tab-terminated fields through atoi; fewer than n tabs: skipped; sum >= 10000: skipped; sum == 0: the error; the
// frequency test divides INTEGERS; "min" of three or more alleles only compares neighbours.
PF_MODEL_HD inline int model_cov_row(const char *s, uint32_t len, int n, double q, double *out, int *err) {
    *err = MODEL_ROW_OK;
    int cov[4];
    uint32_t from = 0;
    for (int i = 0; i < n; ++i) {
        uint32_t t = from;
        while (t < len && s[t] != '\t') ++t;
        if (t >= len) return 0;
        cov[i] = model_atoi(s, len, from);
        from = t + 1;
    }
    return model_cov_ints(cov, n, q, out, err);
}

// One token of <prefix>_allele_frequency.txt as operator>>(double) / strtod converts it, for the forms "%g" prints: an
// optional '-', digits with at most one '.', an optional exponent.  The value is m / 10^e or m * 10^e with m < 10^15 < 2^53 and
// e <= 22: m and 10^e are exact in fp64, so the one division or multiplication is correctly rounded -- the same double strtod
// gives.  Anything else is named, never approximated.
// ... in two steps: the token's decimal parts (value = +-m * 10^e10, m < 10^15; m_digits = digits of m counted from its first
// non-zero one), then the one operation
PF_MODEL_HD inline int model_token_parts(const char *s, uint32_t len, bool *negative, uint64_t *mant, int *m_digits, int *exp10) {
    uint32_t i = 0;
    bool neg = false;
    if (i < len && s[i] == '-') { neg = true; ++i; }
    uint64_t m = 0;
    int digits = 0, sig = 0, frac = 0;
    bool point = false;
    for (; i < len; ++i) {
        const char c = s[i];
        if (c == '.' && !point) { point = true; continue; }
        if (c < '0' || c > '9') break;
        ++digits;
        if (m != 0 || c != '0') ++sig;
        if (sig > 15) return MODEL_ROW_RANGE;
        m = m * 10 + (uint64_t)(c - '0');
        if (point) ++frac;
    }
    if (digits == 0) return MODEL_ROW_BAD_TOKEN;
    int e = 0;
    if (i < len && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (s[i] == '-' || s[i] == '+')) { eneg = s[i] == '-'; ++i; }
        int ed = 0;
        for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i, ++ed) e = e < 10000 ? e * 10 + (s[i] - '0') : e;
        if (ed == 0) return MODEL_ROW_BAD_TOKEN;
        if (eneg) e = -e;
    }
    if (i != len) return MODEL_ROW_BAD_TOKEN;
    *negative = neg; *mant = m; *m_digits = sig; *exp10 = e - frac;
    return MODEL_ROW_OK;
}
PF_MODEL_HD inline int model_fre_token(const char *s, uint32_t len, double *val) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    bool neg;
    uint64_t m;
    int sig, e10;
    const int st = model_token_parts(s, len, &neg, &m, &sig, &e10);
    if (st != MODEL_ROW_OK) return st;
    double v;
    if (m == 0) v = 0.0;
    else if (e10 < -22 || e10 > 22) return MODEL_ROW_RANGE;
    else if (e10 < 0) v = (double)m / p10[-e10];
    else v = (double)m * p10[e10];
    *val = neg ? -v : v;
    return MODEL_ROW_OK;
}

PF_MODEL_HD inline bool model_fre_keep(double a, double q) { return a >= q && a <= 1 - q; }

// One row of the frequency stream: K-TEXT writes one token a row.  *val = the token's value whether it is kept or not (the
// reader's `a`: a file that ends in white space counts its last token a second time); returns how many values the row adds.
PF_MODEL_HD inline int model_fre_row(const char *s, uint32_t len, double q, double *val, int *err) {
    *err = model_fre_token(s, len, val);
    if (*err != MODEL_ROW_OK) return 0;
    return model_fre_keep(*val, q) ? 1 : 0;
}

}  // namespace pf
