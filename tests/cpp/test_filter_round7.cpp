// The scaled rounding of the filtered frequencies (csrc/pf_filter_rows.hpp, filter_scaled_round7) against what the three-command
// chain does with long doubles and text (host/pf_filter.cpp: r_round7, r_format_double; then the model's strtod):
//   n == nearbyintl((long double)x * 1e7L)   and   (double)n / 1e7 == strtod(r_format_double(r_round7(x)))
// for   fractions LO HI : every c / s with LO <= s <= HI, 0 <= c <= s
//       ties N          : the doubles within 3 ulp of (n + 0.5) / 1e7 for n < N
// Prints "ok <cases>" or the first difference.  Plain g++ with host/pf_filter.cpp; no library, no device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ploidyfrost_amd/csrc/pf_filter_rows.hpp"
#include "pf_filter.hpp"

static unsigned long long cases = 0;

static bool check(double x) {
    ++cases;
    const unsigned long long n = pf::filter_scaled_round7(x);
    const long double want = nearbyintl((long double)x * 1e7L);
    if ((long double)n != want) {
        printf("scaled rounding differs at x = %.17g: %llu, long double path %.1Lf\n", x, n, want);
        return false;
    }
    const double v = (double)n / 1e7;
    const double chain = strtod(pfh::r_format_double(pfh::r_round7(x)).c_str(), nullptr);
    if (v != chain) {
        printf("value differs at x = %.17g: %.17g, chain reads %.17g\n", x, v, chain);
        return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "fractions")) {
        const int lo = atoi(argv[2]), hi = atoi(argv[3]);
        for (int s = lo; s <= hi; ++s)
            for (int c = 0; c <= s; ++c)
                if (!check((double)c / (double)s)) return 1;
    } else if (argc == 3 && !strcmp(argv[1], "ties")) {
        const int N = atoi(argv[2]);
        for (int n = 0; n < N; ++n) {
            const double t = ((double)n + 0.5) / 1e7;
            double down = t, up = t;
            if (!check(t)) return 1;
            for (int k = 0; k < 3; ++k) {
                down = nextafter(down, 0.0);
                up = nextafter(up, 1.0);
                if (!check(down) || !check(up)) return 1;
            }
        }
    } else {
        printf("usage: %s fractions LO HI | ties N\n", argv[0]);
        return 2;
    }
    printf("ok %llu\n", cases);
    return 0;
}
