// The multi row rule (csrc/pf_filter_rows.hpp with FilterRule::multi) over the rows of one colored table in a file:
//     test_filter_multi_rule <table 0..3> <color> <cramer> <low> <up> <file>
// prints "<kept rows> <values for fre> <first error code>" -- a stand-alone program, so that the header can run under
// -fsanitize=address,undefined on the CPU (tests/test_filter_multi_rows_cpu.py builds it that way).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "../pf_filter_rows.hpp"

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const int table = atoi(argv[1]), A = table + 2;
    pf::FilterRule f = {};
    f.multi = 1;
    f.color = atof(argv[2]);
    f.cramer = atof(argv[3]);
    f.low = atof(argv[4]);
    f.up = atof(argv[5]);
    f.num = f.size = 10000;
    f.distance = -1;
    f.fq = 0.05;
    std::ifstream in(argv[6], std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    unsigned long long kept = 0, values = 0;
    int first = pf::MODEL_ROW_OK;
    for (size_t start = 0; start < text.size();) {
        size_t end = text.find('\n', start);
        if (end == std::string::npos) end = text.size();
        // the row in a buffer of its own size: a read past its end is the sanitizer's to find
        char *row = (char *)malloc(end - start ? end - start : 1);
        text.copy(row, end - start, start);
        double v[5], colour = 0;
        bool k = false;
        int err = pf::MODEL_ROW_OK;
        const uint32_t mask = pf::filter_fre_row(row, (uint32_t)(end - start), A, f, v, &k, &err, &colour);
        double c[4];
        bool k2 = false;
        int err2 = pf::MODEL_ROW_OK;
        (void)pf::filter_cov_row(row, (uint32_t)(end - start), A, f, 0.0, c, &k2, &err2);
        free(row);
        if (k != k2) return 3;
        kept += k;
        values += (unsigned)__builtin_popcount(mask);
        if (k && pf::filter_color_key(colour) < 0 && err == pf::MODEL_ROW_OK) err = pf::MODEL_ROW_COLOR;
        if (first == pf::MODEL_ROW_OK) first = err;
        start = end + 1;
    }
    printf("%llu %llu %d\n", kept, values, first);
    return 0;
}
