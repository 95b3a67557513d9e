// The coverage thresholds of the path from a k-mer histogram: one rule (reference src/Main.cpp:200-277) for the rows of a histogram
// file and for the rows K-HIST (pf_count_histogram) takes from a KMC database that is already decoded on the device.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "pf_host_graph.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

// cutoffL and cutoffH of src/Main.cpp:200-277 on the second column of a histogram, in file order.
//   lower_raw = round(1.25 * (p - 1)), p = the first index >= 1 with rows[p - 1] < rows[p], or the row count when the histogram
//               never rises (the callers take max(10, lower_raw));
//   upper     = the first index p >= 2 of the prefix sums v (v[0] = 0, v[i] = rows[0] + .. + rows[i - 1]) with
//               v[p] > size_t(quantile * (v.back() - v[1]) + v[1]), or rows.size() + 1 when there is none.
// Returns 0; 1 when there are fewer than two rows (the reference's "Histogram File is badly Formatted." of cutoffH: upper is not set,
// lower_raw is).
int cutoffs_from_rows(const std::vector<uint64_t> &rows, double quantile, int &lower_raw, int &upper);

// The rows of a database: row r = the number of records whose count is min_count + r, from the header's min_count through
// top = min(max_count, 2^(8 counter_size) - 1, PF_HIST_MAX_BINS - 1), zero rows included; records outside [min_count, max_count] are
// left out, as pf_upload_counts leaves them out, and counts above top fall into the last row.  (What `kmc_tools transform <db>
// histogram` writes as far as can be read without the tool: parity with it is unpinned.)
uint64_t kmc_rows_top(const KmcRecords &db);
// ... from the counters pf_kmc_decode left on the device (K-HIST).  PF_OK, else pf_last_error(ctx)
int kmc_rows_of_counts(pf_ctx *ctx, const KmcRecords &db, const uint32_t *counts_dev, std::vector<uint64_t> &rows);
// ... from the database files: map, decode (K-KMC) and count (K-HIST) on `ctx`.  0 = ok, else worded in err
int kmc_rows(pf_ctx *ctx, const std::string &prefix, std::vector<uint64_t> &rows, uint64_t &min_count, std::string &err);
// the same on a context of its own on `device`
int kmc_histogram(const std::string &prefix, int device, std::vector<uint64_t> &rows, uint64_t &min_count, std::string &err);
// "count<TAB>number\n" per row: the histogram file
std::string histogram_text(uint64_t min_count, const std::vector<uint64_t> &rows);

}  // namespace pfh
