// What K-TRIM (pf_trim.hip) and K-TRIMCOUNT (pf_trimcount.hip) see of K-CLIP (pf_clip.hip): is a clip open on the context, and the
// host function that launches the kernel over the indexed records of one call.  The kernel itself lives in pf_clip.hip alone.
#pragma once
#include <stdint.h>

#include "pf_ctx.hpp"

namespace pf {

inline bool clip_is_open(const pf_ctx *ctx) { return ctx->clip != nullptr; }
// the clip ends of an older call are forgotten: every call of K-TRIM / K-TRIMCOUNT starts with this, so that a call that clips nothing
// (an empty chunk, no whole record, a refusal) leaves pf_clip_last_ends nothing of an older call to hand out (no clip open: nothing)
void clip_forget(pf_ctx *ctx);
// clip_end[f][r] = the clip end of record r of file f (n: untouched, 0: dropped) for the n_rec whole records of each of n_files
// chunks on the device (text 16-byte aligned, `lines` of fastq_index).  On the context's stream, no wait; the clip's counters are
// added to on the device.  One timed launch of PF_K_CLIP; unit: records.  A clip is open.  Where it holds prefix pairs
// (pf_clip_begin_pairs) and n_files == 2, K-PALIN follows in a timed launch of its own (PF_K_PALIN; unit: pairs) and clip_end[f][r]
// is the final end -- the smaller of the simple end and the pair end; with no simple adapter K-CLIP is then not launched at all.
int clip_launch(pf_ctx *ctx, int n_files, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec, uint32_t phred,
                uint32_t *const *clip_end);

}  // namespace pf
