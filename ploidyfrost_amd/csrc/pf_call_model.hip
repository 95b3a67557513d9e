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
//
// With a row filter (pf_call_model_filter; the rule is pf_filter_rows.hpp) the collection reads the four coverage streams instead,
// for either source, and a run without one launches nothing of this:
//   cov   the same launches over _bicov, _tricov, _tetracov with the filtered rule inside k_model_rows; over _pentacov the count
//         pass alone (its rows are read, and kept ones count for "does any table keep a row", but `model -f` never reads them)
//   fre   per stream of A alleles: k_model_flags, select, then
//           k_filter_fre   count: a lane per row writes A flags, column-major ([A][rows + 1]: which frequencies the filter writes)
//           scan           exclusive over that one array: a column's offsets are its part less the part's first entry
//           k_filter_fre   write: value at count[column] + offset, into the column's own buffer (14 columns over the four tables)
//           k_filter_advance  the A column counts and the stream's row counter
//         and at finish: the columns end to end (device-to-device copies), the last token once more (the file ends in a line
//         feed), then the model's own test over all of them: k_model_keep_flags, select, k_model_gather.
// With the multi rule (pf_call_model_filter_multi: the colored tables, `filter-multi`'s predicates) the same launches run with
// FilterRule::multi set, for one colour or pooled.  Split by colour (each_color) the collection is the pooled one, and the write
// passes store each value's colour (uint16_t) in a key buffer beside its value buffer -- no launch more per piece, no buffer that
// grows with the number of colours.  finish lays the keys end to end as it lays the tokens; pf_call_model_color_select then takes
// one colour's tokens out in order (k_color_flags, select, k_model_gather: fre_all of the chain run with -c c, element for
// element), counts its last token twice, and runs the model's own test (k_model_keep_flags, select, k_model_gather).
// Bytes per character of a piece (counts, not measurements): without a filter 1 + 1 flags, 4 ends, 4 + 8 counts and offsets;
// fre with a filter adds 12 A for the column flags and their scan (A = 2 .. 5).
#include "pf_call_kernels.hpp"
#include "pf_model_rows.hpp"
#include "pf_scan.hpp"

namespace pf_call {

// device-resident record of one collection
struct ModelDev {
    // values kept so far, per stream of the source (cov: bi, tri, tetra; fre: [0]; fre with a filter: per column) / rows seen per stream
    unsigned long long count[FILTER_COLUMNS], rows[FILTER_TABLES];
    // smallest (late << 60 | stream << 58 | row << 4 | ModelRowErr) met; ~0 = none.  late: with a filter, what the model says of
    // the kept rows comes behind everything the filter refuses while it reads (filter_err_is_late)
    unsigned long long err_key;
    uint32_t kept_any;                      // with a filter: some row of some table was kept (every writer stores 1)
    double last;                            // fre: value of the last token read (kept or not)
    uint32_t have_last, ends_nl;            // ... there is one; the text so far ends in a line feed
    uint8_t color_kept[FILTER_MAX_COLORS];  // split by colour: some row of this colour was kept (every writer stores 1)
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

__host__ __device__ inline unsigned long long model_err_key(bool filtered, int ord, unsigned long long row, int code) {
    return ((unsigned long long)(filtered && filter_err_is_late(code) ? 1 : 0) << 60) | ((unsigned long long)ord << 58) | (row << 4) | (unsigned long long)code;
}

struct ModelRowsArgs {
    const char *text;
    const uint32_t *ends;       // [rows] position of each row's line feed, ascending
    const uint32_t *n_rows;
    uint32_t cap;               // rows the tables have room for (+ one entry for the total)
    int arity;                  // 2 / 3 / 4 alleles a row; 0: the frequency stream
    int ord;                    // stream of the source, in file order
    int filter;                 // the filtered rule (arity 2 .. 5; 5: nothing to write)
    FilterRule rule;
    double q;
    uint32_t *nvals;            // [cap + 1], count pass
    const uint64_t *voff;       // [cap + 1], write pass
    double *dst;
    uint64_t dst_cap;           // values dst has room for
    uint16_t *key;              // split by colour: [dst_cap] the colour of each value; else null
    int each;                   // split by colour
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
        bool kept = false;
        double colour = -1;
        const int n = a.filter ? filter_cov_row(a.text + start, end - start, a.arity, a.rule, a.q, v, &kept, &err, &colour)
                    : a.arity  ? model_cov_row(a.text + start, end - start, a.arity, a.q, v, &err)
                               : model_fre_row(a.text + start, end - start, a.q, v, &err);
        if (!EMIT) {
            a.nvals[r] = (uint32_t)n;
            if (kept) a.st->kept_any = 1u;
            if (kept && a.each) {
                const int ck = filter_color_key(colour);
                if (ck >= 0) a.st->color_kept[ck] = 1;
                else if (err == MODEL_ROW_OK) err = MODEL_ROW_COLOR;
            }
            if (err != MODEL_ROW_OK) atomicMin(&a.st->err_key, model_err_key(a.filter != 0, a.ord, a.st->rows[a.ord] + r, err));
            else if (!a.arity && r + 1 == n_rows) { a.st->last = v[0]; a.st->have_last = 1; }
        } else if (n) {
            const uint64_t at = a.st->count[a.ord] + a.voff[r];
            if (at + (uint64_t)n <= a.dst_cap) {
                for (int i = 0; i < n; ++i) a.dst[at + i] = v[i];
                if (a.key) {
                    const int ck = filter_color_key(colour);
                    for (int i = 0; i < n; ++i) a.key[at + i] = (uint16_t)(ck < 0 ? 0 : ck);   // (ck < 0: refused in the count pass)
                }
            } else {   // (never with K-TEXT's rows: the host sizes dst from the bytes of the text)
                atomicMin(&a.st->err_key, model_err_key(a.filter != 0, a.ord, a.st->rows[a.ord] + r, MODEL_ROW_NO_ROOM));
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

// ---- fre behind a filter: a stream of A alleles feeds A columns ----
struct FilterFreArgs {
    const char *text;
    const uint32_t *ends;
    const uint32_t *n_rows;
    uint32_t cap;               // rows the tables have room for; a column of the flag array has cap + 1 entries
    int arity, ord;
    FilterRule rule;
    uint32_t *cflag;            // [arity * (cap + 1) + 1] count pass: column c's flags at c * (cap + 1)
    const uint64_t *coff;       // the same array scanned, write pass
    double *dst[5];
    uint64_t dst_cap[5];
    uint16_t *key[5];           // split by colour: the colour of each value, beside dst[c]; else null
    int each;
    ModelDev *st;
};

template <bool EMIT>
__global__ __launch_bounds__(MODEL_BLOCK) void k_filter_fre(FilterFreArgs a) {
    const uint32_t n_rows = *a.n_rows;
    const uint64_t stride = (uint64_t)gridDim.x * MODEL_BLOCK, cap1 = (uint64_t)a.cap + 1;
    const int base = filter_column_base(a.ord);
    for (uint64_t r = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x; r <= a.cap; r += stride) {
        uint32_t mask = 0;
        int ckey = 0;
        double v[5];
        if (r < n_rows) {
            const uint32_t start = r ? a.ends[r - 1] + 1 : 0, end = a.ends[r];
            int err = MODEL_ROW_OK;
            bool kept = false;
            double colour = -1;
            mask = filter_fre_row(a.text + start, end - start, a.arity, a.rule, v, &kept, &err, &colour);
            ckey = a.each && kept ? filter_color_key(colour) : 0;
            if (!EMIT) {
                if (kept) a.st->kept_any = 1u;
                if (kept && a.each) {
                    if (ckey >= 0) a.st->color_kept[ckey] = 1;
                    else if (err == MODEL_ROW_OK) err = MODEL_ROW_COLOR;
                }
                if (err != MODEL_ROW_OK) atomicMin(&a.st->err_key, model_err_key(true, a.ord, a.st->rows[a.ord] + r, err));
            }
        }
        if (!EMIT) {
            for (int c = 0; c < a.arity; ++c) a.cflag[(uint64_t)c * cap1 + r] = (mask >> c) & 1u;
            if (r == 0) a.cflag[(uint64_t)a.arity * cap1] = 0;
        } else {
            for (int c = 0; c < a.arity; ++c) {
                if (!((mask >> c) & 1u)) continue;
                const uint64_t at = a.st->count[base + c] + (a.coff[(uint64_t)c * cap1 + r] - a.coff[(uint64_t)c * cap1]);
                if (at < a.dst_cap[c]) {
                    a.dst[c][at] = v[c];
                    if (a.key[c]) a.key[c][at] = (uint16_t)(ckey < 0 ? 0 : ckey);
                } else atomicMin(&a.st->err_key, model_err_key(true, a.ord, a.st->rows[a.ord] + r, MODEL_ROW_NO_ROOM));
            }
        }
    }
}

__global__ void k_filter_advance(ModelDev *st, int ord, int arity, const uint64_t *__restrict__ coff, uint32_t cap, const uint32_t *__restrict__ n_rows) {
    const uint64_t cap1 = (uint64_t)cap + 1;
    const int c = (int)threadIdx.x;
    if (blockIdx.x == 0 && c < arity) st->count[filter_column_base(ord) + c] += coff[(uint64_t)(c + 1) * cap1] - coff[(uint64_t)c * cap1];
    if (blockIdx.x == 0 && c == 0) st->rows[ord] += *n_rows;
}

// finish: the tokens of the filter's frequency file lie end to end, the last one twice; the model's own test over them
__global__ __launch_bounds__(MODEL_BLOCK) void k_model_keep_flags(const double *__restrict__ tok, uint64_t n, double q, uint8_t *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x;
    if (i < n) flags[i] = model_fre_keep(tok[i], q) ? 1 : 0;
}
__global__ __launch_bounds__(MODEL_BLOCK) void k_model_gather(const double *__restrict__ tok, const uint32_t *__restrict__ ids, uint64_t n, double *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x;
    if (i < n) dst[i] = tok[ids[i]];
}

// split by colour: which of the pooled tokens are of one colour
__global__ __launch_bounds__(MODEL_BLOCK) void k_color_flags(const uint16_t *__restrict__ key, uint64_t n, uint16_t colour, uint8_t *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * MODEL_BLOCK + threadIdx.x;
    if (i < n) flags[i] = key[i] == colour ? 1 : 0;
}

// readFreFile's last turn: the read that runs into the end of a file ending in white space leaves `a` as it was
__global__ void k_model_fre_last(ModelDev *st, double q, double *dst, uint64_t dst_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && st->have_last && st->ends_nl && model_fre_keep(st->last, q) && st->count[0] < dst_cap) dst[st->count[0]++] = st->last;
}

static const char *kModelStreamName[2][3] = {{"_bicov", "_tricov", "_tetracov"}, {"_allele_frequency", "", ""}};
static const int kModelStream[2][3] = {{6, 7, 8}, {PF_OUT_ALLELE_FREQUENCY, -1, -1}};
static const int kFilterStream[FILTER_TABLES] = {PF_OUT_BICOV, PF_OUT_TRICOV, PF_OUT_TETRACOV, PF_OUT_PENTACOV};

// room for `want` values in vals[ord], keeping what is there (the copy runs on the collection's stream, behind the kernels that wrote it)
static int model_grow(pf_ctx *ctx, CallState::ModelWork &M, int ord, uint64_t want) {
    DevBuf &b = M.vals[ord];
    if (want * 8 > b.cap || !b.p) {
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
    }
    // split by colour: a key of two bytes for every value the buffer has room for
    DevBuf &k = M.keys[ord];
    if (M.each && (k.cap < b.cap / 4 || !k.p)) {
        void *nk = nullptr;
        PF_HIP(hipMalloc(&nk, b.cap / 4));
        if (k.p) {
            PF_HIP(hipMemcpyAsync(nk, k.p, k.cap, hipMemcpyDeviceToDevice, M.stream));
            PF_HIP(hipStreamSynchronize(M.stream));
            (void)hipFree(k.p);
        }
        k.p = nk;
        k.cap = b.cap / 4;
    }
    return PF_OK;
}

// the launches of one stream's piece (device text), on the collection's stream
static int model_take_stream(pf_ctx *ctx, CallState::ModelWork &M, int ord, const char *text, uint64_t len) {
    if (len == 0) return PF_OK;
    if (len >= 0xFFFFFFF0ull) { pf::CtxErr{ctx} = "pf_call_model_take: a stream of one piece is 4 GB or more"; return PF_ERR_ARG; }
    hipStream_t st = M.stream;
    ModelDev *dst = M.state.as<ModelDev>();
    const uint32_t cap = (uint32_t)len + 1;   // rows: at most one per character, and the virtual one
    const bool fre_cols = M.filter && M.source == PF_MODEL_FRE;
    const int arity = M.filter || M.source == PF_MODEL_COV ? ord + 2 : 0;
    if (fre_cols) {
        // a row that is read has its A + 5 fields, a character and a tab or line feed each at the least: at most one value a column
        for (int c = 0; c < arity; ++c) {
            const int col = filter_column_base(ord) + c;
            M.bound[col] += len / (2 * (uint64_t)(arity + 5)) + 1;
            const int gs = model_grow(ctx, M, col, M.bound[col]);
            if (gs != PF_OK) return gs;
        }
    } else if (arity <= 4) {
        // K-TEXT's rows spend more than two characters a value (a digit and its tab or line feed); the write pass checks all the same
        M.bound[ord] += len / 2 + 1;
        const int gs = model_grow(ctx, M, ord, M.bound[ord]);
        if (gs != PF_OK) return gs;
    }
    const size_t col_entries = fre_cols ? (size_t)arity * ((size_t)cap + 1) + 1 : 0;
    // (a table that has to grow is freed first: not under the kernels of the piece before)
    if (cap > M.flags.cap || ((size_t)cap + 1) * 8 > M.voff.cap || col_entries * 8 > M.coff.cap || col_entries * 4 > M.cflag.cap) PF_HIP(hipStreamSynchronize(st));
    if (!M.flags.ensure(cap) || !M.ends.ensure((size_t)cap * 4) || !M.nvals.ensure(((size_t)cap + 1) * 4) || !M.voff.ensure(((size_t)cap + 1) * 8) ||
        !M.n_rows.ensure(16) || !M.scan.ensure(scan_scratch_bytes(std::max<uint64_t>((uint64_t)cap + 1, col_entries))) ||
        (fre_cols && (!M.cflag.ensure(col_entries * 4) || !M.coff.ensure(col_entries * 8)))) {
        pf::CtxErr{ctx} = "pf_call_model_take: out of device memory";
        return PF_ERR_HIP;
    }
    k_model_flags<<<(unsigned)(((uint64_t)cap + MODEL_BLOCK - 1) / MODEL_BLOCK), MODEL_BLOCK, 0, st>>>(text, len, M.flags.as<uint8_t>(), dst);
    PF_HIP(select_flagged_u8(M.flags.as<uint8_t>(), M.ends.as<uint32_t>(), M.n_rows.as<uint32_t>(), nullptr, cap, M.scan.p, st));
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)cap + MODEL_BLOCK) / MODEL_BLOCK, (uint64_t)ctx->n_cu * 8);
    if (fre_cols) {
        FilterFreArgs f;
        f.text = text; f.ends = M.ends.as<uint32_t>(); f.n_rows = M.n_rows.as<uint32_t>(); f.cap = cap; f.arity = arity; f.ord = ord; f.rule = M.rule;
        f.cflag = M.cflag.as<uint32_t>(); f.coff = M.coff.as<uint64_t>(); f.st = dst;
        for (int c = 0; c < 5; ++c) {
            DevBuf &b = M.vals[filter_column_base(ord) + (c < arity ? c : 0)];
            f.dst[c] = b.as<double>(); f.dst_cap[c] = b.cap / 8;
            f.key[c] = M.each ? M.keys[filter_column_base(ord) + (c < arity ? c : 0)].as<uint16_t>() : nullptr;
        }
        f.each = M.each ? 1 : 0;
        k_filter_fre<false><<<grid, MODEL_BLOCK, 0, st>>>(f);
        PF_HIP(scan_exclusive_u32_u64(f.cflag, M.coff.as<uint64_t>(), (uint64_t)col_entries, M.scan.p, st));
        k_filter_fre<true><<<grid, MODEL_BLOCK, 0, st>>>(f);
        k_filter_advance<<<1, 64, 0, st>>>(dst, ord, arity, f.coff, cap, f.n_rows);
        PF_HIP(hipGetLastError());
        return PF_OK;
    }
    ModelRowsArgs a;
    a.text = text; a.ends = M.ends.as<uint32_t>(); a.n_rows = M.n_rows.as<uint32_t>(); a.cap = cap;
    a.arity = arity; a.ord = ord; a.filter = M.filter ? 1 : 0; a.rule = M.rule; a.q = M.q;
    a.nvals = M.nvals.as<uint32_t>(); a.voff = M.voff.as<uint64_t>();
    a.dst = arity <= 4 ? M.vals[ord].as<double>() : nullptr; a.dst_cap = arity <= 4 ? M.vals[ord].cap / 8 : 0; a.st = dst;
    a.key = M.each && arity <= 4 ? M.keys[ord].as<uint16_t>() : nullptr; a.each = M.each ? 1 : 0;
    k_model_rows<false><<<grid, MODEL_BLOCK, 0, st>>>(a);
    PF_HIP(scan_exclusive_u32_u64(a.nvals, M.voff.as<uint64_t>(), (uint64_t)cap + 1, M.scan.p, st));
    if (arity <= 4) k_model_rows<true><<<grid, MODEL_BLOCK, 0, st>>>(a);   // (the penta rows of a filtered cov collection add no value)
    k_model_advance<<<1, 64, 0, st>>>(dst, ord, a.voff, cap, a.n_rows);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

// finish of a collection behind a filter: the refusals in the chain's order, then the array
static int model_finish_filtered(pf_ctx *ctx, CallState::ModelWork &M, const ModelDev &h, uint64_t *n_values) {
    hipStream_t st = M.stream;
    const bool late = h.err_key != ~0ull && ((h.err_key >> 60) & 1);
    if ((h.err_key != ~0ull && !late) || (late && h.kept_any)) {
        pf::CtxErr{ctx} = filter_error_text((int)(h.err_key & 15), (int)(h.err_key >> 58) & 3, ((h.err_key >> 4) & ((1ull << 54) - 1)) + 1, M.rule.multi != 0);
        return PF_ERR_ARG;
    }
    if (!h.kept_any) { pf::CtxErr{ctx} = filter_none_kept_text(); return PF_ERR_ARG; }
    const int n_col = M.source == PF_MODEL_COV ? 3 : FILTER_COLUMNS;
    uint64_t n = 0;
    for (int c = 0; c < n_col; ++c) {
        if (h.count[c] > M.bound[c]) { pf::CtxErr{ctx} = "pf_call_model_finish: more values than their text has room for"; return PF_ERR_ARG; }
        n += h.count[c];
    }
    if (M.source == PF_MODEL_COV || n == 0) {   // bi | tri | tetra as ever (no token: an empty frequency file, an empty array)
        double *x = (double *)ctx_ws(ctx, WS_GMM_X, (size_t)n * 8);
        if (!x) { pf::CtxErr{ctx} = "pf_call_model_finish: out of device memory"; return PF_ERR_HIP; }
        uint64_t at = 0;
        for (int c = 0; c < n_col; ++c) {
            if (h.count[c]) PF_HIP(hipMemcpyAsync(x + at, M.vals[c].p, (size_t)h.count[c] * 8, hipMemcpyDeviceToDevice, st));
            at += h.count[c];
        }
        PF_HIP(hipStreamSynchronize(st));
    } else {
        // the filter's frequency file, column behind column; it ends in a line feed, so readFreFile reads its last token twice; then
        // the model's own test over every token
        const uint64_t nt = n + 1;
        if (nt >= 0xFFFFFFF0ull) { pf::CtxErr{ctx} = "pf_call_model_finish: 2^32 frequencies or more"; return PF_ERR_ARG; }
        if (!M.tokens.ensure((size_t)nt * 8) || !M.flags.ensure((size_t)nt) || !M.ends.ensure((size_t)nt * 4) || !M.n_rows.ensure(16) ||
            !M.scan.ensure(scan_scratch_bytes(nt))) {
            pf::CtxErr{ctx} = "pf_call_model_finish: out of device memory";
            return PF_ERR_HIP;
        }
        size_t tat = 0;
        ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &tat);
        double *tok = M.tokens.as<double>();
        uint64_t at = 0;
        for (int c = 0; c < n_col; ++c) {
            if (h.count[c]) PF_HIP(hipMemcpyAsync(tok + at, M.vals[c].p, (size_t)h.count[c] * 8, hipMemcpyDeviceToDevice, st));
            at += h.count[c];
        }
        PF_HIP(hipMemcpyAsync(tok + n, tok + n - 1, 8, hipMemcpyDeviceToDevice, st));
        const unsigned grid = (unsigned)((nt + MODEL_BLOCK - 1) / MODEL_BLOCK);
        k_model_keep_flags<<<grid, MODEL_BLOCK, 0, st>>>(tok, nt, M.q, M.flags.as<uint8_t>());
        PF_HIP(select_flagged_u8(M.flags.as<uint8_t>(), M.ends.as<uint32_t>(), M.n_rows.as<uint32_t>(), nullptr, nt, M.scan.p, st));
        uint32_t n_keep = 0;
        PF_HIP(hipMemcpyAsync(&n_keep, M.n_rows.p, 4, hipMemcpyDeviceToHost, st));
        PF_HIP(hipStreamSynchronize(st));
        double *x = (double *)ctx_ws(ctx, WS_GMM_X, (size_t)n_keep * 8);
        if (!x) { pf::CtxErr{ctx} = "pf_call_model_finish: out of device memory"; return PF_ERR_HIP; }
        if (n_keep) k_model_gather<<<(n_keep + MODEL_BLOCK - 1) / MODEL_BLOCK, MODEL_BLOCK, 0, st>>>(tok, M.ends.as<uint32_t>(), n_keep, x);
        PF_HIP(hipGetLastError());
        ctx_end_at(ctx, tat, st);
        PF_HIP(hipStreamSynchronize(st));
        n = n_keep;
    }
    if (M.each) {
        // what pf_call_model_color_select reads: the pooled tokens (fre: before the model's test) and their keys, end to end
        uint64_t nt = 0;
        for (int c = 0; c < n_col; ++c) nt += h.count[c];
        if (nt >= 0xFFFFFFF0ull) { pf::CtxErr{ctx} = "pf_call_model_finish: 2^32 values or more"; return PF_ERR_ARG; }
        if (!M.tokens.ensure((size_t)(nt + 1) * 8) || !M.tkeys.ensure((size_t)(nt + 1) * 2)) { pf::CtxErr{ctx} = "pf_call_model_finish: out of device memory"; return PF_ERR_HIP; }
        uint64_t at = 0;
        for (int c = 0; c < n_col; ++c) {
            if (h.count[c]) {
                PF_HIP(hipMemcpyAsync(M.tokens.as<double>() + at, M.vals[c].p, (size_t)h.count[c] * 8, hipMemcpyDeviceToDevice, st));
                PF_HIP(hipMemcpyAsync(M.tkeys.as<uint16_t>() + at, M.keys[c].p, (size_t)h.count[c] * 2, hipMemcpyDeviceToDevice, st));
            }
            at += h.count[c];
        }
        PF_HIP(hipStreamSynchronize(st));
        M.pooled_n = nt;
        M.color_count = 0;
        for (int c = 0; c < FILTER_MAX_COLORS; ++c) {
            M.color_kept[c] = h.color_kept[c];
            if (h.color_kept[c]) M.color_count = (uint32_t)c + 1;
        }
        M.each_done = true;
    }
    ctx->gmm_n = n;
    ctx->gmm_loaded = true;
    if (n_values) *n_values = n;
    return PF_OK;
}

// one colour's array out of the pooled tokens of a finished collection: a stable selection by key, then what finish does behind it
static int model_color_select_steps(pf_ctx *ctx, CallState::ModelWork &M, int color, uint64_t *n_values) {
    hipStream_t st = M.stream;
    const uint64_t nt = M.pooled_n;
    uint32_t n_c = 0, n_keep = 0;
    const double *tok = M.tokens.as<double>();
    if (nt) {
        k_color_flags<<<(unsigned)((nt + MODEL_BLOCK - 1) / MODEL_BLOCK), MODEL_BLOCK, 0, st>>>(M.tkeys.as<uint16_t>(), nt, (uint16_t)color, M.flags.as<uint8_t>());
        PF_HIP(select_flagged_u8(M.flags.as<uint8_t>(), M.ends.as<uint32_t>(), M.n_rows.as<uint32_t>(), nullptr, nt, M.scan.p, st));
        PF_HIP(hipMemcpyAsync(&n_c, M.n_rows.p, 4, hipMemcpyDeviceToHost, st));
        PF_HIP(hipStreamSynchronize(st));
    }
    if (n_c > nt) { pf::CtxErr{ctx} = "pf_call_model_color_select: more values of a colour than there are values"; return PF_ERR_ARG; }
    uint64_t n = 0;
    if (M.source == PF_MODEL_COV || n_c == 0) {
        double *x = (double *)ctx_ws(ctx, WS_GMM_X, (size_t)n_c * 8);
        if (!x) { pf::CtxErr{ctx} = "pf_call_model_color_select: out of device memory"; return PF_ERR_HIP; }
        if (n_c) k_model_gather<<<(n_c + MODEL_BLOCK - 1) / MODEL_BLOCK, MODEL_BLOCK, 0, st>>>(tok, M.ends.as<uint32_t>(), n_c, x);
        n = n_c;
    } else {
        // the colour's frequency file: its tokens, the last one twice, the model's own test
        double *ct = M.ctok.as<double>();
        const uint64_t nc1 = (uint64_t)n_c + 1;
        k_model_gather<<<(n_c + MODEL_BLOCK - 1) / MODEL_BLOCK, MODEL_BLOCK, 0, st>>>(tok, M.ends.as<uint32_t>(), n_c, ct);
        PF_HIP(hipMemcpyAsync(ct + n_c, ct + n_c - 1, 8, hipMemcpyDeviceToDevice, st));
        k_model_keep_flags<<<(unsigned)((nc1 + MODEL_BLOCK - 1) / MODEL_BLOCK), MODEL_BLOCK, 0, st>>>(ct, nc1, M.q, M.flags.as<uint8_t>());
        PF_HIP(select_flagged_u8(M.flags.as<uint8_t>(), M.ends.as<uint32_t>(), M.n_rows.as<uint32_t>(), nullptr, nc1, M.scan.p, st));
        PF_HIP(hipMemcpyAsync(&n_keep, M.n_rows.p, 4, hipMemcpyDeviceToHost, st));
        PF_HIP(hipStreamSynchronize(st));
        if (n_keep > nc1) { pf::CtxErr{ctx} = "pf_call_model_color_select: more values kept than there are tokens"; return PF_ERR_ARG; }
        double *x = (double *)ctx_ws(ctx, WS_GMM_X, (size_t)n_keep * 8);
        if (!x) { pf::CtxErr{ctx} = "pf_call_model_color_select: out of device memory"; return PF_ERR_HIP; }
        if (n_keep) k_model_gather<<<(n_keep + MODEL_BLOCK - 1) / MODEL_BLOCK, MODEL_BLOCK, 0, st>>>(ct, M.ends.as<uint32_t>(), n_keep, x);
        n = n_keep;
    }
    PF_HIP(hipGetLastError());
    PF_HIP(hipStreamSynchronize(st));
    ctx->gmm_n = n;
    ctx->gmm_loaded = true;
    if (n_values) *n_values = n;
    return PF_OK;
}

// the steps inside one timing record, which is closed however they end
static int model_color_select(pf_ctx *ctx, CallState::ModelWork &M, int color, uint64_t *n_values) {
    const uint64_t nt = M.pooled_n;
    if (!M.flags.ensure((size_t)nt + 1) || !M.ends.ensure(((size_t)nt + 1) * 4) || !M.n_rows.ensure(16) || !M.scan.ensure(scan_scratch_bytes(nt + 1)) ||
        !M.ctok.ensure(((size_t)nt + 1) * 8)) {
        pf::CtxErr{ctx} = "pf_call_model_color_select: out of device memory";
        return PF_ERR_HIP;
    }
    size_t tat = 0;
    ctx_begin_at(ctx, PF_K_CALL_MODEL, M.stream, &tat);
    const int rc = model_color_select_steps(ctx, M, color, n_values);
    ctx_end_at(ctx, tat, M.stream);
    return rc;
}

}  // namespace pf_call

extern "C" {

int pf_call_model_begin(pf_ctx *ctx, int source, double q) {
    if (!ctx || (source != PF_MODEL_COV && source != PF_MODEL_FRE)) return PF_ERR_ARG;
    CallState *S = state_of(ctx);
    if (!S) return PF_ERR_HIP;
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
    M.filter = M.taken = false;
    M.each = M.each_done = false;
    M.rule = {};
    M.active = true;
    ctx->gmm_loaded = false;
    ctx->gmm_n = 0;
    return PF_OK;
}

int pf_call_model_filter(pf_ctx *ctx, const pf_filter_opts *o) {
    if (!ctx || !ctx->call) return PF_ERR_ARG;
    CallState::ModelWork &M = ctx->call->model;
    if (!M.active || M.taken) { pf::CtxErr{ctx} = "pf_call_model_filter: between pf_call_model_begin and the first piece"; return PF_ERR_ARG; }
    M.filter = o != nullptr;
    M.each = false;
    M.rule = {};
    if (!o) return PF_OK;
    if (ctx->call->n_colors) { M.filter = false; pf::CtxErr{ctx} = "pf_call_model_filter: the colored coverage tables have other columns (single-sample path only; pf_call_model_filter_multi)"; return PF_ERR_ARG; }
    if (!(o->frequency <= 0.5)) { M.filter = false; pf::CtxErr{ctx} = "pf_call_model_filter: frequency should < 0.5"; return PF_ERR_ARG; }
    M.rule.simple = o->simple != 0; M.rule.indel = o->indel != 0; M.rule.snp = o->snp != 0;
    M.rule.low = (double)o->low; M.rule.up = (double)o->up; M.rule.num = (double)o->num; M.rule.distance = (double)o->distance; M.rule.size = (double)o->size;
    M.rule.fq = o->frequency;
    return PF_OK;
}

int pf_call_model_filter_multi(pf_ctx *ctx, const pf_filter_multi_opts *o, int each_color) {
    if (!ctx || !ctx->call) return PF_ERR_ARG;
    CallState::ModelWork &M = ctx->call->model;
    if (!M.active || M.taken) { pf::CtxErr{ctx} = "pf_call_model_filter_multi: between pf_call_model_begin and the first piece"; return PF_ERR_ARG; }
    M.filter = M.each = false;
    M.rule = {};
    if (!o) {
        if (each_color) { pf::CtxErr{ctx} = "pf_call_model_filter_multi: the values are split by colour behind a filter only"; return PF_ERR_ARG; }
        return PF_OK;
    }
    if (!(o->frequency <= 0.5)) { pf::CtxErr{ctx} = "pf_call_model_filter_multi: frequency should < 0.5"; return PF_ERR_ARG; }
    if (each_color && o->color >= 0) { pf::CtxErr{ctx} = "pf_call_model_filter_multi: every colour at once goes with color = -1, not with one colour"; return PF_ERR_ARG; }
    M.rule.simple = o->simple != 0; M.rule.indel = o->indel != 0; M.rule.snp = o->snp != 0;
    M.rule.low = (double)o->low; M.rule.up = (double)o->up; M.rule.num = (double)o->num; M.rule.distance = (double)o->distance; M.rule.size = (double)o->size;
    M.rule.fq = o->frequency;
    M.rule.multi = 1;
    M.rule.cramer = o->cramer;
    M.rule.color = o->color >= 0 ? (double)o->color : -1.0;
    M.filter = true;
    M.each = each_color != 0;
    return PF_OK;
}

uint32_t pf_call_model_color_count(const pf_ctx *ctx) {
    return ctx && ctx->call && ctx->call->model.each_done ? ctx->call->model.color_count : 0;
}

int pf_call_model_color_select(pf_ctx *ctx, int color, uint64_t *n_values) {
    if (!ctx || !ctx->call) return PF_ERR_ARG;
    CallState::ModelWork &M = ctx->call->model;
    if (!M.each_done || M.active) { pf::CtxErr{ctx} = "pf_call_model_color_select: behind the pf_call_model_finish of a collection split by colour"; return PF_ERR_ARG; }
    if (color < 0 || color >= FILTER_MAX_COLORS) { pf::CtxErr{ctx} = "pf_call_model_color_select: colours are 0 .. PF_MAX_COLORS - 1"; return PF_ERR_ARG; }
    if (!M.color_kept[color]) {
        if (n_values) *n_values = PF_MODEL_NO_ROW;
        return PF_OK;
    }
    PF_HIP(hipSetDevice(ctx->device));
    return model_color_select(ctx, M, color, n_values);
}

int pf_call_model_take_text(pf_ctx *ctx, int stream_ord, const char *host_text, uint64_t len) {
    if (!ctx || !ctx->call || (len && !host_text)) return PF_ERR_ARG;
    CallState::ModelWork &M = ctx->call->model;
    if (!M.active) { pf::CtxErr{ctx} = "pf_call_model_take_text: no collection was begun (pf_call_model_begin)"; return PF_ERR_ARG; }
    const int n_ord = M.filter ? FILTER_TABLES : M.source == PF_MODEL_COV ? 3 : 1;
    if (stream_ord < 0 || stream_ord >= n_ord) { pf::CtxErr{ctx} = "pf_call_model_take_text: the collection has no such stream"; return PF_ERR_ARG; }
    M.taken = true;
    if (len == 0) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = M.stream;
    if (len > M.upload.cap) PF_HIP(hipStreamSynchronize(st));   // (freed first: not under the kernels of the piece before)
    if (!M.upload.ensure((size_t)len)) { pf::CtxErr{ctx} = "pf_call_model_take_text: out of device memory"; return PF_ERR_HIP; }
    PF_HIP(hipMemcpyAsync(M.upload.p, host_text, (size_t)len, hipMemcpyHostToDevice, st));
    size_t at = 0;
    ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &at);
    const int rc = model_take_stream(ctx, M, stream_ord, M.upload.as<char>(), len);
    if (rc != PF_OK) return rc;
    ctx_end_at(ctx, at, st);
    ctx_units(ctx, PF_K_CALL_MODEL, 1);
    return PF_OK;
}

int pf_call_model_take(pf_ctx *ctx, int slab) {
    if (!ctx || !ctx->call || slab < 0 || slab >= PF_CALL_SLABS) return PF_ERR_ARG;
    CallState *S = ctx->call;
    CallState::ModelWork &M = S->model;
    if (!M.active) { pf::CtxErr{ctx} = "pf_call_model_take: no collection was begun (pf_call_model_begin)"; return PF_ERR_ARG; }
    if ((S->n_colors != 0) != (M.filter && M.rule.multi)) {
        pf::CtxErr{ctx} = S->n_colors ? "pf_call_model_take: the colored coverage tables have other columns: the collection needs pf_call_model_filter_multi"
                                      : "pf_call_model_take: the multi filter reads the colored tables (single-sample path: pf_call_model_filter)";
        return PF_ERR_ARG;
    }
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = M.stream;
    if (S->text_ev[slab]) PF_HIP(hipStreamWaitEvent(st, S->text_ev[slab], 0));
    size_t at = 0;
    ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &at);
    const int n_ord = M.filter ? FILTER_TABLES : M.source == PF_MODEL_COV ? 3 : 1;
    int rc = PF_OK;
    for (int ord = 0; ord < n_ord && rc == PF_OK; ++ord) {
        const int s = M.filter ? kFilterStream[ord] : kModelStream[M.source][ord];
        rc = model_take_stream(ctx, M, ord, S->out[slab].as<char>() + S->txt_off[slab][s], S->txt_len[slab][s]);
    }
    if (rc != PF_OK) return rc;
    M.taken = true;
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
    if (M.source == PF_MODEL_FRE && !M.filter) {
        { const int gs = model_grow(ctx, M, 0, M.bound[0]); if (gs != PF_OK) return gs; }
        size_t at = 0;
        ctx_begin_at(ctx, PF_K_CALL_MODEL, st, &at);
        k_model_fre_last<<<1, 64, 0, st>>>(dst, M.q, M.vals[0].as<double>(), M.vals[0].cap / 8);
        ctx_end_at(ctx, at, st);
    }
    ModelDev h;
    PF_HIP(hipMemcpyAsync(&h, dst, sizeof h, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    if (M.filter) return model_finish_filtered(ctx, M, h, n_values);
    if (h.err_key != ~0ull) {
        const int ord = (int)(h.err_key >> 58) & 3, code = (int)(h.err_key & 15);
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
