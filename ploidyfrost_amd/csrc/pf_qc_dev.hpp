// What K-TRIM (pf_trim.hip) and K-TRIMCOUNT (pf_trimcount.hip) see of K-QC (pf_qc.hip): is a report open on the context, and the host
// function that launches the kernel over the indexed records of one call.  The kernel itself lives in pf_qc.hip alone.
#pragma once
#include <stdint.h>

#include "pf_ctx.hpp"

namespace pf {

inline bool qc_is_open(const pf_ctx *ctx) { return ctx->qc != nullptr; }
// The n_rec whole records of each of n_files chunks on the device (text 16-byte aligned, `lines` of fastq_index) into the tables of
// the open report: file f adds to side side0 + f.  Stage raw: every record with [0, n).  rec_begin / rec_len (null: raw alone): the
// final interval of every record as k_trim_intervals left it, len 0 = dropped -- stage kept.  clip_end (null: no clip open): every
// record with clip_end < n into the side's clip table.  On the context's stream, no wait.  One timed launch of PF_K_QC per file;
// unit: records.  A report is open and n_rec > 0.
int qc_launch(pf_ctx *ctx, int n_files, int side0, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec,
              const uint32_t *const *rec_begin, const uint32_t *const *rec_len, const uint32_t *const *clip_end);

}  // namespace pf
