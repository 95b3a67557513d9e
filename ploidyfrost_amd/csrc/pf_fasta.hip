// K-FASTA: one chunk of FASTA text on the device turned into what the cores of K-COUNT, K-MASKCOUNT and K-COLOR take -- the sequences of
// its whole records as one compacted text, and the table (read_off, read_len) into it.  The rule is pf_fasta_rule.hpp; this file is
// its device form.  In multi-line FASTA a record's sequence is not contiguous (a window of k bases runs across line ends), so the
// line ends are squeezed out once here and every core runs unchanged behind it.  One call, on the text staged once:
//
//   newlines   k_fq_newlines of pf_reads_dev.hpp (the FASTQ index's own kernel): one bit per byte in 64-byte words, the count per
//              word, an exclusive scan (pf_scan.hpp).  One host wait: the number of lines sizes the line starts.
//   lines      k_fq_line_starts of pf_reads_dev.hpp: the first byte of every line.
//   words      k_fasta_words, one thread a word: pf_fasta::word_content walks the lines that meet the word, from line_start[pre[w]] --
//              the line that holds the word's first byte says whether the word starts inside a header -- and gives the mask of
//              sequence bytes and the mask of header starts; their popcounts go to two exclusive scans: the place of every word's
//              content in the compacted text, and the number of every header.  The '\r' test at a line end is
//              pf_mask::line_content_end's; for the word's last byte it reads the byte behind the word.
//   heads      k_fasta_heads, one thread a word: the byte position of every header, in order.  k_fasta_summary, one thread: whole
//              records, bytes_used and the length of the compacted text.  Second host wait: those three numbers size what follows.
//   compact    k_fasta_compact, a tile of FASTA_TILE bytes a block: a lane loads 16 bytes, its place in the tile's output is the
//              word's place plus the popcount of the word's mask below its bytes, the bytes go to LDS; the tile's output is one
//              contiguous range of the compacted text and is written from LDS in whole dwords (the ragged first and last dword of a
//              tile byte by byte: the neighbour tile writes the rest of them).  No atomics: every place comes from the scan.
//   table      k_fasta_table, one thread a record: read_off = the sequence bytes in front of its header (pf_fasta::content_rank),
//              read_len = up to the next header's, or to the end.
//   traffic    the chunk is read by newlines and by compact, and at the first and last bytes of its lines by words (in cache lines
//              the two others have just touched); the sequence is written once; per 64 bytes of text 48 bytes of bitmaps, counts
//              and sums are written and read.
// Compacted text, table and counts stay on the device: the cores behind it (pf_count_reads, pf_maskcount_reads, pf_color_reads) take
// device pointers.  Everything one call launches for the index is timed as one launch of PF_K_FASTA; unit: bytes of the chunk.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_count_dev.hpp"
#include "pf_ctx.hpp"
#include "pf_fasta_rule.hpp"
#include "pf_reads_dev.hpp"
#include "pf_scan.hpp"

namespace pf {

constexpr int FASTA_BLOCK = 256;
constexpr int FASTA_LANE_BYTES = 16;
constexpr int FASTA_TILE = FASTA_BLOCK * FASTA_LANE_BYTES;   // bytes of the text a block compacts at a time (PF_FASTA_TILE)
constexpr int FASTA_TILE_WORDS = FASTA_TILE / 64;
static_assert(FASTA_TILE == PF_FASTA_TILE, "the tile the header names is the kernel's");
static_assert(FASTA_BLOCK == FASTA_TILE_WORDS * (64 / FASTA_LANE_BYTES), "four lanes a word, a word's lanes side by side");

struct FastaSummary {   // what the host sizes and refuses by
    unsigned long long n_heads, n_rec, used, bases;
};

// ---- words: content mask, header starts, their counts (one entry behind the last word: the scans' totals) ----
__global__ __launch_bounds__(FASTA_BLOCK) void k_fasta_words(const char *__restrict__ text, uint64_t n, uint64_t n_words, const uint64_t *__restrict__ nl,
                                                             const uint32_t *__restrict__ pre, const uint32_t *__restrict__ line_start,
                                                             uint64_t *__restrict__ content, uint64_t *__restrict__ heads, uint32_t *__restrict__ c_cnt,
                                                             uint32_t *__restrict__ h_cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * FASTA_BLOCK + threadIdx.x;
    if (w == n_words) { c_cnt[w] = 0; h_cnt[w] = 0; }
    if (w >= n_words) return;
    const pf_fasta::WordMasks m = pf_fasta::word_content(text, n, w, nl[w], (uint64_t)line_start[pre[w]]);
    content[w] = m.content;
    heads[w] = m.heads;
    c_cnt[w] = (uint32_t)__popcll(m.content);
    h_cnt[w] = (uint32_t)__popcll(m.heads);
}

// head_at[h] = the first byte of header h
__global__ __launch_bounds__(FASTA_BLOCK) void k_fasta_heads(const uint64_t *__restrict__ heads, const uint32_t *__restrict__ h_pre, uint64_t n_words,
                                                             uint32_t *__restrict__ head_at) {
    const uint64_t w = (uint64_t)blockIdx.x * FASTA_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    uint64_t m = heads[w];
    uint32_t r = h_pre[w];
    while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        head_at[r++] = (uint32_t)(w * 64 + (uint64_t)b);
    }
}

__global__ void k_fasta_summary(int final, uint64_t n, uint64_t n_words, const uint64_t *__restrict__ content, const uint32_t *__restrict__ c_pre,
                                const uint32_t *__restrict__ h_pre, const uint32_t *__restrict__ head_at, FastaSummary *out) {
    if (blockIdx.x || threadIdx.x) return;
    FastaSummary s;
    s.n_heads = h_pre[n_words];
    if (final) {
        s.n_rec = s.n_heads;
        s.used = n;
        s.bases = c_pre[n_words];
    } else {   // the record the last header opens is carried
        s.n_rec = s.n_heads ? s.n_heads - 1 : 0;
        s.used = s.n_rec ? head_at[s.n_heads - 1] : 0;
        s.bases = s.n_rec ? pf_fasta::content_rank(content, c_pre, n_words, s.used) : 0;
    }
    *out = s;
}

// ---- compact ----
// out[c_pre[w] + rank] = every sequence byte of word w, as far as it lies in front of `bases` (behind it: the carried record's)
__global__ __launch_bounds__(FASTA_BLOCK) void k_fasta_compact(const char *__restrict__ text, uint64_t n, uint64_t n_words, uint64_t n_tiles,
                                                               const uint64_t *__restrict__ content, const uint32_t *__restrict__ c_pre, uint64_t bases,
                                                               char *__restrict__ out) {
    __shared__ uint32_t s_out32[FASTA_TILE / 4 + 2];   // the tile's output, shifted so that LDS dwords are dwords of `out`
    uint8_t *s_out = reinterpret_cast<uint8_t *>(s_out32);
    const int tid = (int)threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t w0 = tile * FASTA_TILE_WORDS, w1 = w0 + FASTA_TILE_WORDS < n_words ? w0 + FASTA_TILE_WORDS : n_words;
        const uint64_t g0 = c_pre[w0];
        uint64_t g1 = c_pre[w1];
        if (g1 > bases) g1 = bases;
        if (g0 >= g1) continue;   // (the same for the whole block)
        const uint32_t shift = (uint32_t)(g0 & 3);
        __syncthreads();   // the previous tile has been written out
        const uint64_t w = w0 + (uint64_t)(tid >> 2);
        const int q = tid & 3;
        if (w < w1) {
            const uint64_t cm = content[w];
            uint32_t m16 = (uint32_t)(cm >> (16 * q)) & 0xFFFFu;
            if (m16) {
                const uint4 v = mask_load_unit(text, n, w * 4 + (uint64_t)q);
                uint32_t at = (uint32_t)((uint64_t)c_pre[w] - g0) + (uint32_t)__popcll(cm & ((1ull << (16 * q)) - 1)) + shift;   // < FASTA_TILE + 4
                while (m16) {
                    const int b = __ffs((int)m16) - 1;
                    m16 &= m16 - 1;
                    s_out[at++] = (uint8_t)unit_byte(v, b);
                }
            }
        }
        __syncthreads();
        const uint32_t total = shift + (uint32_t)(g1 - g0);   // bytes [shift, total) of s_out go to out + g0 - shift
        char *base = out + (g0 - shift);
        for (uint32_t d = (uint32_t)tid; d * 4 < total; d += FASTA_BLOCK) {
            const uint32_t lo = d * 4, hi = lo + 4;
            if (lo >= shift && hi <= total) *reinterpret_cast<uint32_t *>(base + lo) = s_out32[d];
            else
                for (uint32_t j = lo < shift ? shift : lo; j < hi && j < total; ++j) base[j] = (char)s_out[j];
        }
    }
}

// ---- table ----
__global__ __launch_bounds__(FASTA_BLOCK) void k_fasta_table(const uint64_t *__restrict__ content, const uint32_t *__restrict__ c_pre, uint64_t n_words,
                                                             const uint32_t *__restrict__ head_at, uint64_t n_heads, uint64_t n_rec, uint64_t bases,
                                                             uint64_t *__restrict__ off, uint32_t *__restrict__ len) {
    const uint64_t r = (uint64_t)blockIdx.x * FASTA_BLOCK + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t a = pf_fasta::content_rank(content, c_pre, n_words, head_at[r]);
    const uint64_t b = r + 1 < n_heads ? pf_fasta::content_rank(content, c_pre, n_words, head_at[r + 1]) : bases;
    off[r] = a;
    len[r] = (uint32_t)(b - a);
}

// ---- host side ----

struct FastaIndex {   // what K-FASTA leaves on the device
    uint64_t n_rec = 0, used = 0, bases = 0;
    const char *text = nullptr;      // the compacted text, 16-byte aligned (null when bases = 0)
    const uint64_t *off = nullptr;   // n_rec entries (null when n_rec = 0)
    const uint32_t *len = nullptr;
};

// the index of one chunk (0 < n_bytes < 2^32 - 256, text staged on the device), by `who`
static int fasta_index_core(pf_ctx *ctx, const char *who, const char *dt, uint64_t n_bytes, int final, FastaIndex &ix) {
    Timed timed(ctx, PF_K_FASTA);
    ix = FastaIndex{};
    ctx_units(ctx, PF_K_FASTA, n_bytes);
    {   // a chunk starts at a record start
        char first = 0;
        PF_HIP(hipMemcpyAsync(&first, dt, 1, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (first != pf_fasta::HEADER_BYTE) {
            pf::CtxErr{ctx} = std::string(who) + ": record 0 of the chunk: " + pf_fasta::clause_text(pf_fasta::CLAUSE_NO_HEADER);
            return PF_ERR_ARG;
        }
    }
    const uint64_t n_words = (n_bytes + 63) / 64;
    const size_t w8 = up256((size_t)n_words * 8), w4 = up256((size_t)(n_words + 1) * 4), scr_bytes = up256(scan_scratch_bytes(n_words + 1));
    char *iw = static_cast<char *>(ctx_ws(ctx, WS_FASTA_WORK, 3 * w8 + 6 * w4 + scr_bytes + 256));
    if (!iw) return PF_ERR_HIP;
    char *at = iw;
    auto take = [&](size_t bytes) { char *p = at; at += bytes; return p; };
    uint64_t *nl = reinterpret_cast<uint64_t *>(take(w8)), *content = reinterpret_cast<uint64_t *>(take(w8)), *heads = reinterpret_cast<uint64_t *>(take(w8));
    uint32_t *cnt = reinterpret_cast<uint32_t *>(take(w4)), *pre = reinterpret_cast<uint32_t *>(take(w4));
    uint32_t *c_cnt = reinterpret_cast<uint32_t *>(take(w4)), *c_pre = reinterpret_cast<uint32_t *>(take(w4));
    uint32_t *h_cnt = reinterpret_cast<uint32_t *>(take(w4)), *h_pre = reinterpret_cast<uint32_t *>(take(w4));
    void *scratch = take(scr_bytes);
    FastaSummary *ds = reinterpret_cast<FastaSummary *>(take(256));
    const unsigned word_grid = (unsigned)((n_words + MASK_BLOCK - 1) / MASK_BLOCK);
    // newlines: bitmap, count per word, prefix
    k_fq_newlines<<<word_grid, MASK_BLOCK, 0, ctx->stream>>>(dt, n_bytes, n_words, nl, cnt);
    PF_HIP(scan_exclusive_u32(cnt, pre, n_words, scratch, ctx->stream));
    uint32_t last_pre = 0, last_cnt = 0;
    PF_HIP(hipMemcpyAsync(&last_pre, pre + (n_words - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&last_cnt, cnt + (n_words - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t n_newlines = (uint64_t)last_pre + last_cnt;
    // line starts, words, places, headers
    const size_t ls_bytes = up256((size_t)(n_newlines + 2) * 4);
    char *lw = static_cast<char *>(ctx_ws(ctx, WS_FASTA_LINES, 2 * ls_bytes));
    if (!lw) return PF_ERR_HIP;
    uint32_t *line_start = reinterpret_cast<uint32_t *>(lw), *head_at = reinterpret_cast<uint32_t *>(lw + ls_bytes);   // (a header is a line)
    k_fq_line_starts<<<word_grid, MASK_BLOCK, 0, ctx->stream>>>(nl, pre, n_words, line_start);
    k_fasta_words<<<(unsigned)(n_words / FASTA_BLOCK + 1), FASTA_BLOCK, 0, ctx->stream>>>(dt, n_bytes, n_words, nl, pre, line_start, content, heads, c_cnt, h_cnt);
    PF_HIP(scan_exclusive_u32(c_cnt, c_pre, n_words + 1, scratch, ctx->stream));
    PF_HIP(scan_exclusive_u32(h_cnt, h_pre, n_words + 1, scratch, ctx->stream));
    k_fasta_heads<<<word_grid, FASTA_BLOCK, 0, ctx->stream>>>(heads, h_pre, n_words, head_at);
    k_fasta_summary<<<1, 1, 0, ctx->stream>>>(final, n_bytes, n_words, content, c_pre, h_pre, head_at, ds);
    FastaSummary s = {};
    PF_HIP(hipMemcpyAsync(&s, ds, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    ix.n_rec = s.n_rec;
    ix.used = s.used;
    ix.bases = s.bases;
    if (!s.n_rec) return PF_OK;   // no whole record: everything is carried
    // compacted text and table
    const size_t off_bytes = up256((size_t)s.n_rec * 8), len_bytes = up256((size_t)s.n_rec * 4);
    char *tw = static_cast<char *>(ctx_ws(ctx, WS_FASTA_TABLE, off_bytes + len_bytes));
    char *out = static_cast<char *>(ctx_ws(ctx, WS_FASTA_TEXT, (size_t)s.bases + 16));
    if (!tw || !out) return PF_ERR_HIP;
    uint64_t *doff = reinterpret_cast<uint64_t *>(tw);
    uint32_t *dlen = reinterpret_cast<uint32_t *>(tw + off_bytes);
    if (s.bases) {
        const uint64_t n_tiles = (n_words + FASTA_TILE_WORDS - 1) / FASTA_TILE_WORDS;
        k_fasta_compact<<<ctx_grid(ctx, n_tiles * FASTA_BLOCK, FASTA_BLOCK, 8), FASTA_BLOCK, 0, ctx->stream>>>(dt, n_bytes, n_words, n_tiles, content, c_pre, s.bases, out);
    }
    k_fasta_table<<<(unsigned)((s.n_rec + FASTA_BLOCK - 1) / FASTA_BLOCK), FASTA_BLOCK, 0, ctx->stream>>>(content, c_pre, n_words, head_at, s.n_heads, s.n_rec, s.bases, doff, dlen);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-FASTA launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    ix.text = s.bases ? out : nullptr;
    ix.off = doff;
    ix.len = dlen;
    return PF_OK;
}

// what every entry point refuses about its chunk, by `who`; then the index of a chunk that is not empty
static int fasta_chunk(pf_ctx *ctx, const char *who_c, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *bad_record, FastaIndex &ix) {
    const std::string who = who_c;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = who + ": " + m; return (int)PF_ERR_ARG; };
    ix = FastaIndex{};
    if (!bytes_used) return refuse("bytes_used is needed");
    if (n_bytes && !text) return refuse("text is needed");
    if (n_bytes > 0xFFFFFF00ull) return refuse("a chunk holds fewer than 2^32 bytes (line starts are 32 bits)");
    *bytes_used = 0;
    if (bad_record) *bad_record = 0;
    if (n_bytes == 0) return PF_OK;
    PF_HIP(hipSetDevice(ctx->device));
    const char *dt = nullptr;
    { const int rc = mask_stage_text(ctx, text, n_bytes, &dt); if (rc) return rc; }
    { const int rc = fasta_index_core(ctx, who_c, dt, n_bytes, final, ix); if (rc) return rc; }
    *bytes_used = ix.used;
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_fasta_index(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases,
                              const char **text_dev, const uint64_t **read_off_dev, const uint32_t **read_len_dev) {
    if (!ctx) return PF_ERR_ARG;
    if (n_records) *n_records = 0;
    if (n_bases) *n_bases = 0;
    if (text_dev) *text_dev = nullptr;
    if (read_off_dev) *read_off_dev = nullptr;
    if (read_len_dev) *read_len_dev = nullptr;
    FastaIndex ix;
    { const int rc = fasta_chunk(ctx, "pf_fasta_index", text, n_bytes, final, bytes_used, nullptr, ix); if (rc) return rc; }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    if (n_records) *n_records = ix.n_rec;
    if (n_bases) *n_bases = ix.bases;
    if (text_dev) *text_dev = ix.text;
    if (read_off_dev) *read_off_dev = ix.off;
    if (read_len_dev) *read_len_dev = ix.len;
    return PF_OK;
}

extern "C" int pf_fasta_index_fetch(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases,
                                    char *text_out, uint64_t text_cap, uint64_t *read_off, uint32_t *read_len, uint64_t table_cap) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (!n_records || !n_bases) return refuse("pf_fasta_index_fetch: n_records and n_bases are needed");
    const char *dt = nullptr;
    const uint64_t *doff = nullptr;
    const uint32_t *dlen = nullptr;
    { const int rc = pf_fasta_index(ctx, text, n_bytes, final, bytes_used, n_records, n_bases, &dt, &doff, &dlen); if (rc) return rc; }
    if (*n_bases > text_cap || *n_records > table_cap)
        return refuse("pf_fasta_index_fetch: the index holds " + std::to_string(*n_bases) + " bytes and " + std::to_string(*n_records) +
                      " records, the buffers " + std::to_string(text_cap) + " and " + std::to_string(table_cap));
    if (*n_bases && !text_out) return refuse("pf_fasta_index_fetch: text_out is needed");
    if (*n_records && (!read_off || !read_len)) return refuse("pf_fasta_index_fetch: read_off and read_len are needed");
    if (*n_bases) PF_HIP(hipMemcpyAsync(text_out, dt, (size_t)*n_bases, hipMemcpyDefault, ctx->stream));
    if (*n_records) {
        PF_HIP(hipMemcpyAsync(read_off, doff, (size_t)*n_records * 8, hipMemcpyDefault, ctx->stream));
        PF_HIP(hipMemcpyAsync(read_len, dlen, (size_t)*n_records * 4, hipMemcpyDefault, ctx->stream));
    }
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

extern "C" int pf_count_fasta(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_count_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    { const int rc = count_needs_begin(ctx, "pf_count_fasta"); if (rc) return rc; }
    if (stats) *stats = pf_count_stats{};
    FastaIndex ix;
    { const int rc = fasta_chunk(ctx, "pf_count_fasta", text, n_bytes, final, bytes_used, bad_record, ix); if (rc) return rc; }
    return pf_count_reads(ctx, ix.text, ix.bases, ix.off, ix.len, ix.n_rec, stats);
}

extern "C" int pf_maskcount_fasta(pf_ctx *ctx, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, uint64_t *bytes_used,
                                  pf_maskcount_stats *stats, uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    { const int rc = maskcount_needs(ctx, "pf_maskcount_fasta"); if (rc) return rc; }
    if (low > up) { pf::CtxErr{ctx} = "pf_maskcount_fasta: low " + std::to_string(low) + " is above up " + std::to_string(up); return PF_ERR_ARG; }
    if (stats) *stats = pf_maskcount_stats{};
    FastaIndex ix;
    { const int rc = fasta_chunk(ctx, "pf_maskcount_fasta", text, n_bytes, final, bytes_used, bad_record, ix); if (rc) return rc; }
    return pf_maskcount_reads(ctx, ix.text, ix.bases, ix.off, ix.len, ix.n_rec, low, up, stats);
}

extern "C" int pf_color_fasta(pf_ctx *ctx, uint32_t colour, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_color_stats *stats,
                              uint64_t *bad_record) {
    if (!ctx) return PF_ERR_ARG;
    { const int rc = pf_color_reads(ctx, colour, nullptr, 0, nullptr, nullptr, 0, stats); if (rc) return rc; }   // an open colouring and the colour, refused before the index runs
    FastaIndex ix;
    { const int rc = fasta_chunk(ctx, "pf_color_fasta", text, n_bytes, final, bytes_used, bad_record, ix); if (rc) return rc; }
    return pf_color_reads(ctx, colour, ix.text, ix.bases, ix.off, ix.len, ix.n_rec, stats);
}
