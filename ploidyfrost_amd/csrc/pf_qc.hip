// K-QC: the read quality report of `ploidyfrost qc` and of `--report`, accumulated on the device from arrays that are there already --
// the FASTQ index (`lines`), and behind k_trim_intervals every record's final interval and, with a clip open, its clip end.  The rule,
// the words of a table and the text of the report are pf_qc_rule.hpp; this file is the device form.
//
//   k_qc       one launch a file.  A ROW of 16 lanes per read, 16 rows a block (K-TRIM's shape).  A lane owns 16 consecutive positions of
//              a row step of 256: it reads the 16 bytes of the sequence line and of the quality line from [b + i0 ..) as two aligned
//              16-byte units each and a shift (trim_load_shifted), so the two lines may start at any alignment and no LDS is staged.
//              The block keeps a PRIVATE TABLE in LDS with the word layout of the rule: TABLE_WORDS u32 (38 060 bytes; the 1024 qsum
//              slots of it are unused), the qsum row as u64 beside it (8 192 bytes) and the clip curve (4 100 bytes): 50 352 bytes, three
//              blocks a CU.  Positions are LDS integer atomics; a lane adds a run of equal qualities to quality[] once.  Per read the
//              row reduces sum qc, gc and acgt with four xor-shuffles and lane 0 adds the per-read histograms.  Minimum and maximum
//              byte live in registers until the stage ends.
//              The stages run one after the other inside the launch (raw, then kept): zero the table, accumulate over a grid-stride
//              loop of rows, then FLUSH the non-zero cells into the report's u64 tables with global atomics (add, min, max).
//   no wrap    An LDS cell other than qsum grows by at most 1 per base or per record between two flushes, and a flush follows every
//              stage of every launch.  A launch covers one chunk of fewer than 2^32 - 256 bytes, a base takes two of them (its
//              quality byte) and a record at least four: fewer than 2^31 increments (QC_MAX_INCREMENTS below).  qsum grows by up to
//              93 a base and is 64 bits wide.  The report's own tables are 64 bits.
//   the flush  costs a block one global atomic per non-zero cell: about 8 * read length + 300.  The grid is therefore capped at two
//              blocks a CU (qc_grid) however many records there are -- 512 flushes of some 1 500 cells for reads of 150 bases --
//              instead of the eight blocks a CU K-TRIM asks ctx_grid for, which would flush four times as many tables.
// Result: sums, minima and maxima only; it depends on neither the grid nor the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_qc_dev.hpp"
#include "pf_qc_rule.hpp"
#include "pf_reads_dev.hpp"
#include "pf_trim_dev.hpp"

static_assert(PF_QC_TABLE_WORDS == pf_qc::TABLE_WORDS && PF_QC_CLIP_WORDS == pf_qc::CLIP_WORDS, "the rule header restates the ABI's word counts");
static_assert((int)PF_QC_RAW == (int)pf_qc::STAGE_RAW && (int)PF_QC_KEPT == (int)pf_qc::STAGE_KEPT, "the rule header restates the ABI's stages");

namespace pf {

constexpr uint64_t QC_MAX_INCREMENTS = 0xFFFFFF00ull / 2;   // of one u32 cell in one launch: see "no wrap"
static_assert(QC_MAX_INCREMENTS < 0xFFFFFFFFull, "a u32 cell of the block's table cannot wrap inside a launch");
constexpr uint32_t QC_NONE = 0xFFFFFFFFu;
constexpr size_t QC_TABLES = 2 * pf_qc::STAGES;   // [side][stage]

struct QcState {
    uint32_t phred = 33;
    unsigned long long *d_tab = nullptr;    // QC_TABLES tables of TABLE_WORDS, then two clip tables of CLIP_WORDS
    bool seen[2][pf_qc::STAGES] = {};
    bool clip_seen = false;
};
static inline QcState *qc_state(pf_ctx *ctx) { return static_cast<QcState *>(ctx->qc); }
constexpr size_t QC_STATE_WORDS = QC_TABLES * pf_qc::TABLE_WORDS + 2 * pf_qc::CLIP_WORDS;

struct QcArgs {
    const char *text;
    uint64_t n_bytes;
    const uint32_t *lines;
    uint64_t n_rec;
    const uint32_t *rec_begin, *rec_len;   // null: stage raw alone
    const uint32_t *clip_end;              // null: no clip open
    uint32_t phred, n_stages;
    unsigned long long *table[pf_qc::STAGES];
    unsigned long long *clip;
};

__device__ inline uint32_t qc_row_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = TRIM_ROW / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, TRIM_ROW);
    return v;
}

__global__ __launch_bounds__(TRIM_BLOCK) void k_qc(const QcArgs a) {
    using namespace pf_qc;
    __shared__ uint32_t s_tab[TABLE_WORDS];
    __shared__ unsigned long long s_qsum[POS_BINS];
    __shared__ uint32_t s_clip[CLIP_WORDS];
    const int tid = (int)threadIdx.x, rl = tid & (TRIM_ROW - 1), row = tid / TRIM_ROW;
    for (uint32_t stage = 0; stage < a.n_stages; ++stage) {
        for (uint32_t w = (uint32_t)tid; w < TABLE_WORDS; w += TRIM_BLOCK) s_tab[w] = is_min_word(w) ? QC_NONE : 0u;
        for (uint32_t w = (uint32_t)tid; w < POS_BINS; w += TRIM_BLOCK) s_qsum[w] = 0ull;
        if (stage == STAGE_RAW)
            for (uint32_t w = (uint32_t)tid; w < CLIP_WORDS; w += TRIM_BLOCK) s_clip[w] = 0u;
        __syncthreads();
        uint32_t min_byte = QC_NONE, max_byte = 0;
        for (uint64_t r = (uint64_t)blockIdx.x * TRIM_ROWS + row; r < a.n_rec; r += (uint64_t)gridDim.x * TRIM_ROWS) {
            const uint32_t sb = a.lines[8 * r + 2], n = a.lines[8 * r + 3] - sb, qb = a.lines[8 * r + 6];
            uint32_t b = 0, L = n;
            bool counted = true;
            if (stage == STAGE_KEPT) {
                L = a.rec_len[r];
                b = a.rec_begin[r];
                counted = L != 0;   // a dropped record adds nothing
            }
            if (!counted) L = 0;
            if (rl == 0 && counted) {
                atomicAdd(&s_tab[W_READS], 1u);
                atomicAdd(&s_tab[W_LENGTH + len_bin(L)], 1u);
                atomicMin(&s_tab[W_MIN_LEN], L);
                atomicMax(&s_tab[W_MAX_LEN], L);
                if (stage == STAGE_RAW && a.clip_end) {
                    const uint32_t ce = a.clip_end[r];
                    if (ce < n) atomicAdd(&s_clip[len_bin(ce)], 1u);
                }
            }
            uint64_t sum_qc = 0;
            uint32_t gc = 0, acgt = 0;
            for (uint64_t i0 = 16ull * (uint32_t)rl; i0 < L; i0 += TRIM_STEP_BYTES) {
                const uint32_t cnt = L - i0 < 16 ? (uint32_t)(L - i0) : 16u;
                const uint4 vs = trim_load_shifted(a.text, a.n_bytes, (uint64_t)sb + b + i0);
                const uint4 vq = trim_load_shifted(a.text, a.n_bytes, (uint64_t)qb + b + i0);
                uint32_t run_q = QC_NONE, run = 0;   // a run of equal qualities goes to quality[] once
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if ((uint32_t)k >= cnt) continue;
                    const uint64_t i = i0 + (uint32_t)k;
                    const uint32_t bin = pos_bin(i < POS_BINS ? (uint32_t)i : POS_BINS);
                    const uint32_t cls = base_class((uint8_t)unit_byte(vs, k)), byte = unit_byte(vq, k);
                    const int q = quality((uint8_t)byte, a.phred);
                    const uint32_t qc = quality_clamped(q);
                    atomicAdd(&s_tab[W_POS_BASE + bin * CLASSES + cls], 1u);
                    atomicAdd(&s_qsum[bin], (unsigned long long)qc);
                    if (q >= 20) atomicAdd(&s_tab[W_POS_Q20 + bin], 1u);
                    if (q >= 30) atomicAdd(&s_tab[W_POS_Q30 + bin], 1u);
                    if (q < 0) atomicAdd(&s_tab[W_QUAL_LOW], 1u);
                    if (q > (int)Q_MAX) atomicAdd(&s_tab[W_QUAL_HIGH], 1u);
                    if (qc != run_q) {
                        if (run) atomicAdd(&s_tab[W_QUALITY + run_q], run);
                        run_q = qc;
                        run = 0;
                    }
                    run += 1;
                    min_byte = min(min_byte, byte);
                    max_byte = max(max_byte, byte);
                    sum_qc += qc;
                    acgt += cls < 4;
                    gc += cls == 1 || cls == 2;
                }
                if (run) atomicAdd(&s_tab[W_QUALITY + run_q], run);
            }
            // per read: the row's sums (a lane's share of sum qc may pass 2^32: its low 20 bits and the rest are summed apart)
            const uint32_t lo = qc_row_sum_u32((uint32_t)(sum_qc & 0xFFFFFu)), hi = qc_row_sum_u32((uint32_t)(sum_qc >> 20));
            gc = qc_row_sum_u32(gc);
            acgt = qc_row_sum_u32(acgt);
            if (rl == 0 && L > 0) {
                const uint64_t total = ((uint64_t)hi << 20) + lo;
                atomicAdd(&s_tab[W_READ_QUALITY + mean_quality_bin(total, L)], 1u);
                if (acgt) atomicAdd(&s_tab[W_GC_PERCENT + gc_percent_bin(gc, acgt)], 1u);
                else atomicAdd(&s_tab[W_READS_NO_ACGT], 1u);
            }
        }
        if (min_byte != QC_NONE) {
            atomicMin(&s_tab[W_MIN_BYTE], min_byte);
            atomicMax(&s_tab[W_MAX_BYTE], max_byte);
        }
        __syncthreads();
        // ---- flush: the non-zero cells into the report's table ----
        unsigned long long *T = a.table[stage];
        for (uint32_t w = (uint32_t)tid; w < TABLE_WORDS; w += TRIM_BLOCK) {
            const unsigned long long v = (w >= W_POS_QSUM && w < W_POS_Q20) ? s_qsum[w - W_POS_QSUM] : (unsigned long long)s_tab[w];
            if (is_min_word(w)) { if (v != QC_NONE) atomicMin(&T[w], v); }
            else if (is_max_word(w)) { if (v) atomicMax(&T[w], v); }
            else if (v) atomicAdd(&T[w], v);
        }
        if (stage == STAGE_RAW && a.clip_end)
            for (uint32_t w = (uint32_t)tid; w < CLIP_WORDS; w += TRIM_BLOCK)
                if (s_clip[w]) atomicAdd(&a.clip[w], (unsigned long long)s_clip[w]);
        __syncthreads();   // the table is zeroed for the next stage
    }
}

// ---- host side ----
// at most two blocks a CU: the flush of a block's table is what a block costs beyond its reads (see "the flush")
static int qc_grid(const pf_ctx *ctx, uint64_t n_rec) {
    const uint64_t want = (n_rec + TRIM_ROWS - 1) / TRIM_ROWS, cap = 2ull * (uint64_t)std::max(ctx->n_cu, 1);
    return (int)std::max<uint64_t>(1, std::min(want, cap));
}

int qc_launch(pf_ctx *ctx, int n_files, int side0, const char *const *text, const uint64_t *n_bytes, const uint32_t *const *lines, uint64_t n_rec,
              const uint32_t *const *rec_begin, const uint32_t *const *rec_len, const uint32_t *const *clip_end) {
    QcState *S = qc_state(ctx);
    if (!S) { pf::CtxErr{ctx} = "K-QC: no report is open"; return PF_ERR_ARG; }
    if (n_rec == 0) return PF_OK;
    for (int f = 0; f < n_files; ++f) {
        const int side = side0 + f;
        QcArgs a = {};
        a.text = text[f];
        a.n_bytes = n_bytes[f];
        a.lines = lines[f];
        a.n_rec = n_rec;
        a.rec_begin = rec_begin ? rec_begin[f] : nullptr;
        a.rec_len = rec_len ? rec_len[f] : nullptr;
        a.clip_end = clip_end ? clip_end[f] : nullptr;
        a.phred = S->phred;
        a.n_stages = a.rec_len ? 2u : 1u;
        for (uint32_t st = 0; st < pf_qc::STAGES; ++st) a.table[st] = S->d_tab + ((size_t)side * pf_qc::STAGES + st) * pf_qc::TABLE_WORDS;
        a.clip = S->d_tab + QC_TABLES * pf_qc::TABLE_WORDS + (size_t)side * pf_qc::CLIP_WORDS;
        size_t at = (size_t)-1;
        (void)ctx_begin_at(ctx, PF_K_QC, ctx->stream, &at);
        k_qc<<<qc_grid(ctx, n_rec), TRIM_BLOCK, 0, ctx->stream>>>(a);
        ctx_end_at(ctx, at, ctx->stream);
        for (uint32_t st = 0; st < a.n_stages; ++st) S->seen[side][st] = true;
        if (a.clip_end) S->clip_seen = true;
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-QC launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    ctx_units(ctx, PF_K_QC, n_rec * (uint64_t)n_files);
    return PF_OK;
}

void qc_destroy(pf_ctx *ctx) {
    QcState *S = qc_state(ctx);
    if (!S) return;
    if (S->d_tab) (void)hipFree(S->d_tab);
    delete S;
    ctx->qc = nullptr;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_qc_begin(pf_ctx *ctx, uint32_t phred) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_qc_begin: " + m; return (int)PF_ERR_ARG; };
    if (ctx->qc) return refuse("a report is open already");
    if (phred != 33 && phred != 64) return refuse(std::string(pf_trim::refusal_text(pf_trim::REFUSE_PHRED)) + ", not " + std::to_string(phred));
    PF_HIP(hipSetDevice(ctx->device));
    QcState *S = new QcState;
    ctx->qc = S;
    S->phred = phred;
    struct Undo { pf_ctx *c; bool armed; ~Undo() { if (armed) qc_destroy(c); } } undo{ctx, true};
    PF_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_tab), QC_STATE_WORDS * 8));
    PF_HIP(hipMemsetAsync(S->d_tab, 0, QC_STATE_WORDS * 8, ctx->stream));
    for (size_t t = 0; t < QC_TABLES; ++t) {   // the minima start at the largest value
        PF_HIP(hipMemsetAsync(S->d_tab + t * pf_qc::TABLE_WORDS + pf_qc::W_MIN_LEN, 0xFF, 8, ctx->stream));
        PF_HIP(hipMemsetAsync(S->d_tab + t * pf_qc::TABLE_WORDS + pf_qc::W_MIN_BYTE, 0xFF, 8, ctx->stream));
    }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    undo.armed = false;
    return PF_OK;
}

extern "C" int pf_qc_get(pf_ctx *ctx, int side, int stage, uint64_t *words) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_qc_get: " + m; return (int)PF_ERR_ARG; };
    QcState *S = qc_state(ctx);
    if (!S) return refuse("no report is open");
    if (side < 0 || side > 1) return refuse("side is 0 or 1");
    if (stage < 0 || stage >= (int)pf_qc::STAGES) return refuse("stage is PF_QC_RAW or PF_QC_KEPT");
    if (!words) return refuse("words is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(words, S->d_tab + ((size_t)side * pf_qc::STAGES + (size_t)stage) * pf_qc::TABLE_WORDS, (size_t)pf_qc::TABLE_WORDS * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    words[pf_qc::W_SEEN] = S->seen[side][stage] ? 1 : 0;
    if (words[pf_qc::W_READS] == 0) words[pf_qc::W_MIN_LEN] = 0;     // nothing seen: an untouched table is all zero
    if (words[pf_qc::W_MAX_LEN] == 0) words[pf_qc::W_MIN_BYTE] = 0;   // (no read with a base: no byte)
    return PF_OK;
}

extern "C" int pf_qc_clip_get(pf_ctx *ctx, int side, uint64_t *words) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_qc_clip_get: " + m; return (int)PF_ERR_ARG; };
    QcState *S = qc_state(ctx);
    if (!S) return refuse("no report is open");
    if (side < 0 || side > 1) return refuse("side is 0 or 1");
    if (!words) return refuse("words is needed");
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipMemcpyAsync(words, S->d_tab + QC_TABLES * pf_qc::TABLE_WORDS + (size_t)side * pf_qc::CLIP_WORDS, (size_t)pf_qc::CLIP_WORDS * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_qc_fastq(pf_ctx *ctx, int side, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records,
                           uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_qc_fastq: " + m; return (int)PF_ERR_ARG; };
    if (!ctx->qc) return refuse("no report is open");
    if (side < 0 || side > 1) return refuse("side is 0 or 1");
    if (!bytes_used || !n_records) return refuse("bytes_used and n_records are needed");
    *bytes_used = 0;
    *n_records = 0;
    if (bad_record) *bad_record = 0;
    if (n_bytes && !text) return refuse("text is needed");
    if (n_bytes > 0xFFFFFF00ull) return refuse("a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    if (n_bytes == 0) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    FastqIndex ix;
    ix.want_lines = true;
    { const int rc = fastq_index(ctx, "pf_qc_fastq", dt, n_bytes, final, ix, bad_record); if (rc) return rc; }
    if (ix.n_rec) {
        const int rc = qc_launch(ctx, 1, side, &dt, &n_bytes, &ix.lines, ix.n_rec, nullptr, nullptr, nullptr);
        if (rc) return rc;
        PF_HIP(hipStreamSynchronize(ctx->stream));   // (the caller's text may go away)
    }
    *bytes_used = ix.used;
    *n_records = ix.n_rec;
    return PF_OK;
}

extern "C" int pf_qc_end(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    if (!ctx->qc) { pf::CtxErr{ctx} = "pf_qc_end: no report is open"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    qc_destroy(ctx);
    return PF_OK;
}
