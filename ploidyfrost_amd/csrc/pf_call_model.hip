// K-MODEL-ROWS: the join between the calling pipeline and K-GMM.  The model's input values are defined by the TEXT of the result
// streams (pf_model_rows.hpp: GmmModel::readCovFile / readFreFile, quirks included), and K-TEXT leaves that text in HBM one piece
// at a time (a slab: pf_call_text_range(_lane)).  pf_call_model_take turns the rows of one piece into doubles, in file order,
// behind the values of the pieces before it; pf_call_model_finish lays bi | tri | tetra end to end where pf_gmm_fit reads them.
// Nothing crosses PCIe but two words per piece (none) and one small record at the end.
//
// Per piece and stream, on one stream of their own (pieces in the order they are taken, whatever streams wrote them):
//   k_model_flags   a byte per character: is it a line feed (a last row without one gets a virtual line feed)        1 B read, 1 B written
//   select          positions of the flags, ascending = where each row ends; their number = the rows (pf_scan.hip)
//   k_model_rows    a lane per row: the row rule -> how many values the row adds (0 or n); errors by smallest (stream, row)
//   scan            exclusive, over the counts: where each row's values go
//   k_model_rows    again, writing: values at count[stream] + offset[row]
//   k_model_advance count[stream] += values, rows[stream] += rows (one thread; the next piece reads them)
// Order never depends on scheduling: every value's place is a prefix sum; the only atomic is the minimum of the error key.
#include "pf_call_kernels.hpp"
#include "pf_model_rows.hpp"
#include "pf_scan.hpp"

#define PF_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            pf::CtxErr{ctx} = std::string(#call) + ": " + hipGetErrorString(e_);             \
            return PF_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

namespace pf_call {

// device-resident record of one collection
struct ModelDev {
    unsigned long long count[3], rows[3];   // values kept / rows seen so far, per stream of the source (cov: bi, tri, tetra; fre: [0])
    unsigned long long err_key;             // smallest (stream << 58 | row << 4 | ModelRowErr) met; ~0 = none
    double last;                            // fre: value of the last token read (kept or not)
    uint32_t have_last, ends_nl;            // ... there is one; the text so far ends in a line feed
};

constexpr int MODEL_BLOCK = 256;

__global__ __launch_bounds__(MODEL_BLOCK) void k_model_flags(const char *__restrict__ text, uint64_t len, uint8_t *__restrict__ flags, ModelDev *st) {
    const uint64_t i = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x;
    if (i < len) flags[i] = text[i] == '\n' ? 1 : 0;
    else if (i == len) {
        const bool nl = text[len - 1] == '\n';   // (len > 0: empty pieces are not launched)
        flags[len] = nl ? 0 : 1;
        st->ends_nl = nl ? 1u : 0u;
    }
}

struct ModelRowsArgs {
    const char *text;
    const uint32_t *ends;       // [rows] position of each row's line feed, ascending
    const uint32_t *n_rows;
    uint32_t cap;               // rows the tables have room for (+ one entry for the total)
    int arity;                  // 2 / 3 / 4 alleles a row; 0: the frequency stream
    int ord;                    // stream of the source, in file order
    double q;
    uint32_t *nvals;            // [cap + 1], count pass
    const uint64_t *voff;       // [cap + 1], write pass
    double *dst;
    uint64_t dst_cap;           // values dst has room for
    ModelDev *st;
};

template <bool EMIT>
__global__ __launch_bounds__(MODEL_BLOCK) void k_model_rows(ModelRowsArgs a) {
    const uint32_t n_rows = *a.n_rows;
    const uint64_t stride = (uint64_t)gridDim.x * MODEL_BLOCK;
    for (uint64_t r = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x; r <= a.cap; r += stride) {
        if (r >= n_rows) {
            if (!EMIT) a.nvals[r] = 0;
            continue;
        }
        const uint32_t start = r ? a.ends[r - 1] + 1 : 0, end = a.ends[r];
        double v[4];
        int err = MODEL_ROW_OK;
        const int n = a.arity ? model_cov_row(a.text + start, end - start, a.arity, a.q, v, &err)
                              : model_fre_row(a.text + start, end - start, a.q, v, &err);
        if (!EMIT) {
            a.nvals[r] = (uint32_t)n;
            if (err != MODEL_ROW_OK) atomicMin(&a.st->err_key, ((unsigned long long)a.ord << 58) | ((a.st->rows[a.ord] + r) << 4) | (unsigned long long)err);
            else if (!a.arity && r + 1 == n_rows) { a.st->last = v[0]; a.st->have_last = 1; }
        } else if (n) {
            const uint64_t at = a.st->count[a.ord] + a.voff[r];
            if (at + (uint64_t)n <= a.dst_cap) {
                for (int i = 0; i < n; ++i) a.dst[at + i] = v[i];
            } else {   // (never with K-TEXT's rows: the host sizes dst from the bytes of the text)
                atomicMin(&a.st->err_key, ((unsigned long long)a.ord << 58) | ((a.st->rows[a.ord] + r) << 4) | (unsigned long long)MODEL_ROW_NO_ROOM);
            }
        }
    }
}

__global__ void k_model_advance(ModelDev *st, int ord, const uint64_t *__restrict__ voff, uint32_t cap, const uint32_t *__restrict__ n_rows) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->count[ord] += voff[cap];
        st->rows[ord] += *n_rows;
    }
}

// readFreFile's last turn: the read that runs into the end of a file ending in white space leaves `a` as it was
__global__ void k_model_fre_last(ModelDev *st, double q, double *dst, uint64_t dst_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && st->have_last && st->ends_nl && model_fre_keep(st->last, q) && st->count[0] < dst_cap) dst[st->count[0]++] = st->last;
}

static const char *kModelStreamName[2][3] = {{"_bicov", "_tricov", "_tetracov"}, {"_allele_frequency", "", ""}};
static const int kModelStream[2][3] = {{6, 7, 8}, {PF_OUT_ALLELE_FREQUENCY, -1, -1}};

// room for `want` values in vals[ord], keeping what is there (the copy runs on the collection's stream, behind the kernels that wrote it)
static int model_grow(pf_ctx *ctx, CallState::ModelWork &M, int ord, uint64_t want) {
    DevBuf &b = M.vals[ord];
    if (want * 8 <= b.cap && b.p) return PF_OK;
    const size_t bytes = (size_t)std::max<uint64_t>(want * 8 + want * 2, 1u << 16);
    void *np = nullptr;
    PF_HIP(hipMalloc(&np, bytes));
    if (b.p) {
        PF_HIP(hipMemcpyAsync(np, b.p, b.cap, hipMemcpyDeviceToDevice, M.stream));
        PF_HIP(hipStreamSynchronize(M.stream));
        (void)hipFree(b.p);
    }
    b.p = np;
    b.cap = bytes;
    return PF_OK;
}

}  // namespace pf_call

extern "C" {

int pf_call_model_begin(pf_ctx *ctx, int source, double q) {
    if (!ctx || (source != PF_MODEL_COV && source != PF_MODEL_FRE)) return PF_ERR_ARG;
    CallState *S = state_of(ctx);
    if (!S) return PF_ERR_HIP;
    if (S->n_colors) { pf::CtxErr{ctx} = "pf_call_model_begin: the colored coverage tables have other columns (single-sample path only)"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    CallState::ModelWork &M = S->model;
    if (!M.stream) PF_HIP(hipStreamCreateWithFlags(&M.stream, hipStreamNonBlocking));
    if (!M.state.ensure(sizeof(ModelDev))) { pf::CtxErr{ctx} = "pf_call_model_begin: out of device memory"; return PF_ERR_HIP; }
    ModelDev h;
    memset(&h, 0, sizeof h);
    h.err_key = ~0ull;
    PF_HIP(hipMemcpyAsync(M.state.p, &h, sizeof h, hipMemcpyHostToDevice, M.stream));
    PF_HIP(hipStreamSynchronize(M.stream));
    M.source = source;
    M.q = q;
    for (uint64_t &b : M.bound) b = 2;   // (the doubled last token)
    M.active = true;
    ctx->gmm_loaded = false;
    ctx->gmm_n = 0;
    return PF_OK;
}

int pf_call_model_take(pf_ctx *ctx, int slab) {
    if (!ctx || !ctx->call || slab < 0 || slab >= PF_CALL_SLABS) return PF_ERR_ARG;
    CallState *S = ctx->call;
    CallState::ModelWork &M = S->model;
    if (!M.active) { pf::CtxErr{ctx} = "pf_call_model_take: no collection was begun (pf_call_model_begin)"; return PF_ERR_ARG; }
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = M.stream;
    if (S->text_ev[slab]) PF_HIP(hipStreamWaitEvent(st, S->text_ev[slab], 0));
    size_t at = 0;
    ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &at);
    ModelDev *dst = M.state.as<ModelDev>();
    for (int ord = 0; ord < 3; ++ord) {
        const int s = kModelStream[M.source][ord];
        if (s < 0) break;
        const uint64_t len = S->txt_len[slab][s];
        if (len == 0) continue;
        if (len >= 0xFFFFFFF0ull) { pf::CtxErr{ctx} = "pf_call_model_take: a stream of one piece is 4 GB or more"; return PF_ERR_ARG; }
        const char *text = S->out[slab].as<char>() + S->txt_off[slab][s];
        const uint32_t cap = (uint32_t)len + 1;   // rows: at most one per character, and the virtual one
        // K-TEXT's rows spend more than two characters a value (a digit and its tab or line feed); the write pass checks all the same
        M.bound[ord] += len / 2 + 1;
        { const int gs = model_grow(ctx, M, ord, M.bound[ord]); if (gs != PF_OK) return gs; }
        // (a table that has to grow is freed first: not under the kernels of the piece before)
        if (cap > M.flags.cap || ((size_t)cap + 1) * 8 > M.voff.cap) PF_HIP(hipStreamSynchronize(st));
        if (!M.flags.ensure(cap) || !M.ends.ensure((size_t)cap * 4) || !M.nvals.ensure(((size_t)cap + 1) * 4) || !M.voff.ensure(((size_t)cap + 1) * 8) ||
            !M.n_rows.ensure(16) || !M.scan.ensure(scan_scratch_bytes((uint64_t)cap + 1))) {
            pf::CtxErr{ctx} = "pf_call_model_take: out of device memory";
            return PF_ERR_HIP;
        }
        k_model_flags<<<(unsigned)(((uint64_t)cap + MODEL_BLOCK - 1) / MODEL_BLOCK), MODEL_BLOCK, 0, st>>>(text, len, M.flags.as<uint8_t>(), dst);
        PF_HIP(select_flagged_u8(M.flags.as<uint8_t>(), M.ends.as<uint32_t>(), M.n_rows.as<uint32_t>(), nullptr, cap, M.scan.p, st));
        ModelRowsArgs a;
        a.text = text; a.ends = M.ends.as<uint32_t>(); a.n_rows = M.n_rows.as<uint32_t>(); a.cap = cap;
        a.arity = M.source == PF_MODEL_COV ? ord + 2 : 0; a.ord = ord; a.q = M.q;
        a.nvals = M.nvals.as<uint32_t>(); a.voff = M.voff.as<uint64_t>(); a.dst = M.vals[ord].as<double>(); a.dst_cap = M.vals[ord].cap / 8; a.st = dst;
        const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)cap + MODEL_BLOCK) / MODEL_BLOCK, (uint64_t)ctx->n_cu * 8);
        k_model_rows<false><<<grid, MODEL_BLOCK, 0, st>>>(a);
        PF_HIP(scan_exclusive_u32_u64(a.nvals, M.voff.as<uint64_t>(), (uint64_t)cap + 1, M.scan.p, st));
        k_model_rows<true><<<grid, MODEL_BLOCK, 0, st>>>(a);
        k_model_advance<<<1, 64, 0, st>>>(dst, ord, a.voff, cap, a.n_rows);
        PF_HIP(hipGetLastError());
    }
    ctx_end_at(ctx, at, st);
    ctx_units(ctx, PF_K_CALL_MODEL, 1);
    // the slab may be written again once these kernels have read it: K-TEXT's write pass waits here on its own stream
    if (!M.read_ev[slab]) PF_HIP(hipEventCreateWithFlags(&M.read_ev[slab], hipEventDisableTiming));
    PF_HIP(hipEventRecord(M.read_ev[slab], st));
    return PF_OK;
}

int pf_call_model_finish(pf_ctx *ctx, uint64_t *n_values) {
    if (!ctx || !ctx->call) return PF_ERR_ARG;
    CallState *S = ctx->call;
    CallState::ModelWork &M = S->model;
    if (!M.active) { pf::CtxErr{ctx} = "pf_call_model_finish: no collection was begun (pf_call_model_begin)"; return PF_ERR_ARG; }
    M.active = false;
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = M.stream;
    ModelDev *dst = M.state.as<ModelDev>();
    if (M.source == PF_MODEL_FRE) {
        { const int gs = model_grow(ctx, M, 0, M.bound[0]); if (gs != PF_OK) return gs; }
        size_t at = 0;
        ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &at);
        k_model_fre_last<<<1, 64, 0, st>>>(dst, M.q, M.vals[0].as<double>(), M.vals[0].cap / 8);
        ctx_end_at(ctx, at, st);
    }
    ModelDev h;
    PF_HIP(hipMemcpyAsync(&h, dst, sizeof h, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    if (h.err_key != ~0ull) {
        const int ord = (int)(h.err_key >> 58), code = (int)(h.err_key & 15);
        const unsigned long long row = ((h.err_key >> 4) & ((1ull << 54) - 1)) + 1;
        const std::string where = "row " + std::to_string(row) + " of stream " + kModelStreamName[M.source][ord < 3 ? ord : 0];
        pf::CtxErr{ctx} = code == MODEL_ROW_COV_ZERO ? "Model::readCovFile() : " + where + " sums to 0 (the reference divides by it)"
                        : code == MODEL_ROW_NO_ROOM ? "pf_call_model_finish: " + where + " has more values than two characters a value allow"
                        : code == MODEL_ROW_BAD_TOKEN ? "ERROR: " + where + " holds something that is not a number"
                                                      : "ERROR: " + where + " holds a number outside what the device converts exactly (more than 15 digits or a decimal exponent beyond 22)";
        return PF_ERR_ARG;
    }
    const int n_ord = M.source == PF_MODEL_COV ? 3 : 1;
    uint64_t n = 0;
    for (int ord = 0; ord < n_ord; ++ord) {
        if (h.count[ord] > M.bound[ord]) { pf::CtxErr{ctx} = "pf_call_model_finish: more values than their text has room for"; return PF_ERR_ARG; }
        n += h.count[ord];
    }
    double *x = (double *)ctx_ws(ctx, WS_GMM_X, (size_t)n * 8);
    if (!x) { pf::CtxErr{ctx} = "pf_call_model_finish: out of device memory"; return PF_ERR_HIP; }
    uint64_t at = 0;
    for (int ord = 0; ord < n_ord; ++ord) {
        if (h.count[ord]) PF_HIP(hipMemcpyAsync(x + at, M.vals[ord].p, (size_t)h.count[ord] * 8, hipMemcpyDeviceToDevice, st));
        at += h.count[ord];
    }
    PF_HIP(hipStreamSynchronize(st));
    ctx->gmm_n = n;
    ctx->gmm_loaded = true;
    if (n_values) *n_values = n;
    return PF_OK;
}

uint64_t pf_call_fetched_bytes(const pf_ctx *ctx) { return ctx && ctx->call ? ctx->call->fetched_bytes.load(std::memory_order_relaxed) : 0; }

}  // extern "C"
