// What K-TRIM (pf_trim.hip) and K-TRIMCOUNT (pf_trimcount.hip) see of K-DEDUP (pf_dedup.hip): is a dedup open on the context, and the
// host functions that launch it over the indexed records of one call.  The kernels themselves live in pf_dedup.hip alone.
#pragma once
#include <stdint.h>

#include "pf_ctx.hpp"
#include "pf_trim_dev.hpp"

namespace pf {

inline bool dedup_is_open(const pf_ctx *ctx) { return ctx->dedup != nullptr; }

// Behind k_trim_intervals, in front of K-QC: the units of the call (record r of one file, or of both files of a pair) that take part
// get their key from the raw sequence line, go into the table as units next_unit + r, and every one that is not the first of its key
// has its interval emptied in every file and leaves `counts` (kept, bases_kept of its file) again.  The unit counter advances by
// n_rec.  On the context's stream, no wait; grows the table first when 2 * (entries + n_rec) would pass its slots.  One timed launch of
// PF_K_DEDUP.
int dedup_launch(pf_ctx *ctx, int n_files, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec,
                 uint32_t *const *rec_begin, uint32_t *const *rec_len, TrimCounts *counts);
// After the caller's own final wait: takes over the entries and units the launch counted (they came back with the caller's copies).
void dedup_settle(pf_ctx *ctx);

}  // namespace pf
