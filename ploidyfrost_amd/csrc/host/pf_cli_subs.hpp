// The entry points of the reads sub-commands (main() in pf_main.cpp dispatches to them), and what `run` / `run-multi` take from the
// calling run's command line in pf_main.cpp: its options, the --density switches, the long options and the model's set-up.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "pf_cdbg.hpp"
#include "pf_filter.hpp"
#include "ploidyfrost_hip.h"

namespace pfcli {
struct Options {
    std::string graphfile, colorfile, outprefix = "output", db, coveragefile, hist;
    size_t nb_threads = 1, complex_size = 8, ref_threads = 1, gpus = 1;
    bool verbose = false, info = false, detach_teardown = false, gpus_seen = false;
    int coverage_lower = 10, coverage_upper = 1000, k = 25;
    std::vector<std::pair<int, int>> coverage_vec;
    double match = 2, mismatch = -1, gap = -3, frequency = 0.998;
    // --model ...: the estimate in the same run
    std::string model_source, model_ploidy = "1:9";
    bool model_only = false, model_option_seen = false, filter_seen = false, multi_seen = false, each_color = false;
    bool auto_cutoffs = false, l_seen = false, u_seen = false, cfile_seen = false;   // --auto-cutoffs and what it does not go with
    std::string filter_words;   // --filter "<options of `ploidyfrost filter`>"
    std::string multi_words;    // --filter-multi "<options of `ploidyfrost filter-multi`>"
    double model_q = 0, model_m = 5.0, model_n = 2.0, model_delta = 0.01;
    int model_iter = 1000;
};

// --density [--density-points N] [--density-adjust A]: the words as given, checked before anything is read or written
struct DensityCli {
    bool on = false, points_seen = false, adjust_seen = false;
    std::string points_word, adjust_word;
    unsigned points = 512;
    double adjust = 1.0;
    // takes argv[i] (and its value) when it is one of the three switches: 0 = not one of them, else the number of words taken
    int take(int argc, char **argv, int i) {
        if (strcmp(argv[i], "--density") == 0) { on = true; return 1; }
        const bool p = strcmp(argv[i], "--density-points") == 0, a = strcmp(argv[i], "--density-adjust") == 0;
        if ((p || a) && i + 1 < argc) {
            (p ? points_seen : adjust_seen) = true;
            (p ? points_word : adjust_word) = argv[i + 1];
            return 2;
        }
        return 0;
    }
    // false: refused, one line on stderr
    bool check(const char *points_name = "--density-points", const char *adjust_name = "--density-adjust") {
        using std::cerr;
        using std::endl;
        if ((points_seen || adjust_seen) && !on) { cerr << "Error: --density-points / --density-adjust need --density" << endl; return false; }
        if (points_seen) {
            char *end = nullptr;
            const long v = strtol(points_word.c_str(), &end, 10);
            if (end == points_word.c_str() || *end != 0 || v < PF_DENSITY_MIN_POINTS || v > PF_DENSITY_MAX_POINTS) {
                cerr << "Error: " << points_name << " " << points_word << ": grid points from " << PF_DENSITY_MIN_POINTS << " to " << PF_DENSITY_MAX_POINTS << endl;
                return false;
            }
            points = (unsigned)v;
        }
        if (adjust_seen) {
            char *end = nullptr;
            const double v = strtod(adjust_word.c_str(), &end);
            if (end == adjust_word.c_str() || *end != 0 || !std::isfinite(v) || !(v > 0)) {
                cerr << "Error: " << adjust_name << " " << adjust_word << ": the bandwidth factor is a finite positive number" << endl;
                return false;
            }
            adjust = v;
        }
        return true;
    }
};

}  // namespace pfcli

// pf_main.cpp
bool take_long_options(int &argc, char **argv, int first, pfcli::Options &opt, pfcli::DensityCli &dc);
bool model_setup(const pfcli::Options &opt, pfcli::DensityCli &dc, pfh::CDBG::ModelOptions &model, pf_filter_opts &filter, pf_filter_multi_opts &multi);

// pf_cli_reads.cpp
int count_main(int argc, char **argv);
int mask_main(int argc, char **argv);
int smudge_main(int argc, char **argv);
int qc_main(int argc, char **argv);
int trim_main(int argc, char **argv);
// pf_cli_build.cpp: `build` and, coloured, `build-multi`
int build_main(int argc, char **argv, bool colored);
// pf_cli_run.cpp
int run_main(int argc, char **argv);
int run_multi_main(int argc, char **argv);
