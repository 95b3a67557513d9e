// K-GUNZIP: a plain gzip member's deflate stream inflated where the FASTQ kernels read it.  One deflate stream has no table of its
// blocks and every block may reach 32 KiB back, so the stream is cut into pieces at block starts that are searched for, every piece
// is decoded twice, and what a piece refers to in front of itself is filled in afterwards (pf_gunzip_rule.hpp runs the same stages on
// the host).  Six stages on the launch stream:
//   find     k_gunzip_find, for every nominal boundary j * piece_bytes: 64 bit offsets at a time are tested by a wavefront for a non-final
//            dynamic block header (pf_gunzip::block_candidate), by ballot; the first one found before the next boundary is a piece
//            start (sixteen wavefronts share a stride, each over its own run of bits: the smallest hit is the first).
//            k_gunzip_starts puts start_bit (always a true block start) and the candidates in one ascending list.
//   count    k_gunzip_count, one wavefront per piece: pf_gunzip::decode_piece with a CountSink, up to a final block, a piece start it
//            lands on, the end of the bits or a clause.  (decode_piece drives the decoder of pf_inflate_core.hpp, the one K-INFLATE
//            runs, and reads the compressed bytes through the same window in LDS: GzIn, pf_gz_dev.hpp.)
//   chain    k_gunzip_chain, one thread: follows the links from piece 0; the pieces on the chain are live and get their places by a
//            running sum, all others are dead and what they found is ignored.  Correctness rests here: piece 0 starts at a true block
//            start and a piece stops at block boundaries of its own decode only, so a false candidate costs one wasted wavefront.
//            One host wait here: the total, the end and a clause.
//   decode   k_gunzip_decode, one wavefront per live piece: decode_piece with a RingSink.  The last 32 Ki symbols are a ring in LDS
//            (64 KiB; with the tables and the input window 70 KiB, two blocks a CU), match copies read the ring, and the symbols go
//            to a 16-bit staging array at the piece's place in coalesced runs.  A back-reference in front of the piece is a marker.
//   window   k_gunzip_window, one block: the markers in the last 32 Ki symbols of every live piece in order, from the staging array
//            in front of the piece (already resolved, by induction) or the window passed in.
//   resolve  k_gunzip_resolve: every remaining marker by the same gather, the bytes written in dwords where the destination allows;
//            k_gunzip_tail: the raw CRC register of the text in slices, and the new window.
// No lane reads outside comp[0, n_bytes) (the window refill and block_candidate test every address) and none writes outside its
// piece's staging range (decode_piece's max_syms) or out[0, total).  Vector loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_gunzip_rule.hpp"
#include "pf_gz_dev.hpp"

namespace pf {

namespace gz = pf_gunzip;

constexpr int GUN_WAVE = GZ_WAVE;
constexpr uint32_t GUN_NO_BAD = 0xffffffffu;
constexpr uint32_t GUN_FIND_SPLIT = 16;   // wavefronts that search one stride
constexpr uint32_t GUN_CRC_SLICE = 512; // bytes of text a thread of the CRC takes

struct GunzipSmall {   // what the host reads
    unsigned long long total, end_bit, clause_bit, markers;
    uint32_t n_live, final, clause, bad_live, crc_raw, n_pieces;
    uint32_t stored, fixed, dynamic, pad_;
};
struct GunzipArgs {
    const uint8_t *comp;
    uint32_t n_bytes, stride;
    uint64_t start_bit, j0;
    uint32_t n_bound;      // nominal boundaries searched; at most 1 + n_bound pieces
    uint64_t *cand;        // n_bound
    uint64_t *starts;      // 1 + n_bound
    gz::Piece *pieces;     // 1 + n_bound: the count stage's
    gz::Piece *again;      // 1 + n_bound, by live order: the decode stage's
    uint32_t *live;        // 1 + n_bound
    uint64_t *place;       // 2 + n_bound: live pieces' places, then the total
    GunzipSmall *small;
    const uint8_t *window;
    uint32_t n_window;
    uint16_t *stage;
    uint8_t *out;
    uint8_t *new_window;
    uint32_t crc_threads;
};

// (a stride is searched by GUN_FIND_SPLIT wavefronts, each over its own run of bits; the smallest hit is the first candidate)
__global__ __launch_bounds__(GUN_WAVE) void k_gunzip_find(const GunzipArgs a) {
    const uint32_t b = blockIdx.x / GUN_FIND_SPLIT, part = blockIdx.x % GUN_FIND_SPLIT;
    const uint64_t j = a.j0 + b;
    const uint64_t end = (uint64_t)a.n_bytes * 8;
    const uint64_t run = (((uint64_t)a.stride * 8 + GUN_FIND_SPLIT - 1) / GUN_FIND_SPLIT + GUN_WAVE - 1) / GUN_WAVE * GUN_WAVE;   // bits a wavefront searches
    const uint64_t stop = min((j + 1) * a.stride * 8, end);
    const uint64_t from = j * a.stride * 8 + part * run, to = min(from + run, stop);
    uint64_t found = gz::NO_BIT;
    for (uint64_t base = from; base < to; base += GUN_WAVE) {   // (the same turns for every lane)
        const uint64_t bit = base + threadIdx.x;
        const bool ok = bit < to && gz::block_candidate(GzBytes{a.comp}, (uint64_t)a.n_bytes, bit);
        const unsigned long long hit = __ballot(ok);
        if (hit) { found = base + (uint64_t)(__ffsll((long long)hit) - 1); break; }
    }
    if (threadIdx.x == 0 && found != gz::NO_BIT) atomicMin(reinterpret_cast<unsigned long long *>(&a.cand[b]), (unsigned long long)found);
}

__global__ void k_gunzip_starts(const GunzipArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t n = 0;
    a.starts[n++] = a.start_bit;
    for (uint32_t b = 0; b < a.n_bound; ++b)
        if (a.cand[b] != gz::NO_BIT) a.starts[n++] = a.cand[b];   // (ascending: each lies within its own stride)
    a.small->n_pieces = n;
}

// comp[0, n_bytes) for a piece that starts at start_bit, the window filled around its first byte
__device__ inline GzIn gunzip_in(const GunzipArgs &a, uint64_t start_bit, uint32_t lane, uint32_t *window) {
    return GzIn(a.comp, a.n_bytes, lane, window, (uint32_t)min(start_bit >> 3, (uint64_t)(a.n_bytes ? a.n_bytes - 1 : 0)));
}

__global__ __launch_bounds__(GUN_WAVE) void k_gunzip_count(const GunzipArgs a) {
    __shared__ uint32_t window[GZ_WINDOW / 4];
    __shared__ pf_inflate::Work work;
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const uint32_t n_pieces = a.small->n_pieces;
    if (p >= n_pieces) return;
    const uint64_t start = a.starts[p];
    const GzIn in = gunzip_in(a, start, lane, window);
    gz::CountSink sink;
    gz::Piece r;
    gz::decode_piece(in, a.n_bytes, start, a.starts, n_pieces, p + 1, gz::NO_BIT, ~0ull, sink, work, lane, (uint32_t)GUN_WAVE, GzSync{}, r);
    if (lane == 0) a.pieces[p] = r;
}

__global__ void k_gunzip_chain(const GunzipArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    GunzipSmall s = *a.small;
    const uint32_t n_pieces = s.n_pieces;
    uint64_t total = 0;
    uint32_t n_live = 0;
    s.stored = s.fixed = s.dynamic = 0;
    s.final = 0;
    s.clause = 0;
    for (uint32_t p = 0;;) {   // (a link is a later piece: at most n_pieces turns)
        const gz::Piece r = a.pieces[p];
        a.live[n_live] = p;
        a.place[n_live] = total;
        ++n_live;
        total += r.symbols;
        s.stored += r.stored;
        s.fixed += r.fixed;
        s.dynamic += r.dynamic;
        s.end_bit = r.end_bit;
        if (r.link == gz::LINK_CLAUSE) { s.clause = r.clause; s.clause_bit = r.end_bit; break; }
        if (r.link == gz::LINK_FINAL) { s.final = 1; break; }
        if (r.link >= n_pieces || r.link <= p) break;   // tail
        p = r.link;
    }
    a.place[n_live] = total;
    s.n_live = n_live;
    s.total = total;
    *a.small = s;
}

__global__ __launch_bounds__(GUN_WAVE) void k_gunzip_decode(const GunzipArgs a) {
    __shared__ uint16_t ring[gz::RING];
    __shared__ uint32_t window[GZ_WINDOW / 4];
    __shared__ pf_inflate::Work work;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const uint32_t p = a.live[k];
    const gz::Piece first = a.pieces[p];
    const uint64_t start = a.starts[p], place = a.place[k];
    const GzIn in = gunzip_in(a, start, lane, window);
    gz::RingSink<GzSync> sink(ring, a.stage + place, place + a.n_window, lane, (uint32_t)GUN_WAVE, GzSync{});
    gz::Piece r;
    gz::decode_piece(in, a.n_bytes, start, (const uint64_t *)nullptr, 0u, 0u, first.end_bit, first.symbols, sink, work, lane, (uint32_t)GUN_WAVE, GzSync{}, r);
    if (lane == 0) {
        a.again[k] = r;
        if (r.link != gz::LINK_LIMIT || r.symbols != first.symbols) atomicMin(&a.small->bad_live, k);
    }
}

__global__ __launch_bounds__(1024) void k_gunzip_window(const GunzipArgs a) {
    const uint32_t n_live = a.small->n_live;
    for (uint32_t k = 0; k < n_live; ++k) {
        const uint64_t place = a.place[k], n = a.place[k + 1] - place;
        for (uint64_t s = (n > gz::RING ? n - gz::RING : 0) + threadIdx.x; s < n; s += blockDim.x) {
            const uint32_t v = a.stage[place + s];
            if (v & gz::MARKER) a.stage[place + s] = (uint16_t)(gz::RESOLVED | gz::behind(a.stage, a.window, a.n_window, place, v));   // (reads in front of `place` only)
        }
        __syncthreads();   // the next piece reads what this one wrote
    }
}

__global__ __launch_bounds__(256) void k_gunzip_resolve(const GunzipArgs a) {
    const uint64_t total = a.small->total;
    const uint32_t n_live = a.small->n_live;
    const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    uint32_t markers = 0;
    if (i0 < total) {
        uint32_t lo = 0, hi = n_live;   // the last live piece whose place is <= i0 (place[0] = 0)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (a.place[mid] <= i0) lo = mid; else hi = mid;
        }
        uint32_t k = lo;
        uint32_t word = 0;
        const uint32_t n = (uint32_t)min((uint64_t)4, total - i0);
        for (uint32_t b = 0; b < n; ++b) {
            const uint64_t i = i0 + b;
            while (k + 1 < n_live && i >= a.place[k + 1]) ++k;
            const uint32_t v = a.stage[i];
            if (v & (gz::MARKER | gz::RESOLVED)) ++markers;
            word |= ((v & gz::MARKER) ? gz::behind(a.stage, a.window, a.n_window, a.place[k], v) : (v & 0xffu)) << (8 * b);
        }
        if (n == 4 && (((uintptr_t)(a.out + i0)) & 3u) == 0) {
            *reinterpret_cast<uint32_t *>(a.out + i0) = word;
        } else {
            for (uint32_t b = 0; b < n; ++b) a.out[i0 + b] = (uint8_t)(word >> (8 * b));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) markers += (uint32_t)__shfl_xor((int)markers, d, GUN_WAVE);
    if ((threadIdx.x & (GUN_WAVE - 1)) == 0 && markers) atomicAdd(&a.small->markers, (unsigned long long)markers);
}

// the raw CRC register of out[0, total) from crc_threads slices, and the new window
__global__ __launch_bounds__(256) void k_gunzip_tail(const GunzipArgs a) {
    const uint32_t total = (uint32_t)a.small->total;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.crc_threads) {
        const uint32_t begin = pf_inflate::slice_begin(total, a.crc_threads, t), end = pf_inflate::slice_end(total, a.crc_threads, t);
        if (end > begin) {
            const uint32_t raw = pf_inflate::crc_raw(GzBytes{a.out}, begin, end);
            atomicXor(&a.small->crc_raw, pf_inflate::slice_share(raw, total, a.crc_threads, t));
        }
    }
    if (t < gz::RING) {
        const uint64_t have = (uint64_t)a.n_window + total;
        const uint32_t n_new = (uint32_t)min(have, (uint64_t)gz::RING);
        if (t < n_new) {
            const long long q = (long long)total - (long long)n_new + (long long)t;
            a.new_window[t] = q >= 0 ? a.out[q] : a.window[(long long)a.n_window + q];
        }
    }
}

struct GunzipEvents {   // the stages' own times, when the caller asks for stats with timing on
    hipEvent_t e[7] = {};
    bool on = false;
    ~GunzipEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    void start(bool want) {
        on = want;
        for (int i = 0; on && i < 7; ++i) if (hipEventCreate(&e[i]) != hipSuccess) on = false;
    }
    void mark(int i, hipStream_t s) { if (on) (void)hipEventRecord(e[i], s); }
};

}  // namespace pf

using namespace pf;

extern "C" int pf_inflate_gzip(pf_ctx *ctx, const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window,
                               uint32_t piece_bytes, char *out, uint64_t out_cap, uint8_t *new_window, pf_gunzip_result *res, pf_gunzip_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_inflate_gzip: " + m; return (int)PF_ERR_ARG; };
    if (!res) return refuse("res is needed");
    *res = pf_gunzip_result{};
    res->end_bit = start_bit;
    res->n_window = n_window;
    if (stats) *stats = pf_gunzip_stats{};
    if (n_bytes > 0x7fffffffull) return refuse("a call holds fewer than 2^31 compressed bytes");
    if (start_bit > n_bytes * 8) return refuse("start_bit lies behind the bytes");
    if (n_window > gz::RING) return refuse("a window holds at most 32768 bytes");
    if ((n_bytes && !comp) || (n_window && !window)) return refuse("comp and window are needed");
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_GUNZIP);
    GunzipEvents ev;
    ev.start(stats && ctx->timing);

    // ---- stage what the caller holds on the host ----
    DevTmp<uint8_t> d_comp_, d_win_, d_out_, d_newwin_;
    const uint8_t *d_comp = comp, *d_win = window;
    if (n_bytes && !is_device_ptr(comp)) {
        PF_HIP(d_comp_.alloc((size_t)n_bytes));
        PF_HIP(hipMemcpyAsync(d_comp_.p, comp, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
        d_comp = d_comp_.p;
    }
    if (n_window && !is_device_ptr(window)) {
        PF_HIP(d_win_.alloc((size_t)n_window));
        PF_HIP(hipMemcpyAsync(d_win_.p, window, (size_t)n_window, hipMemcpyHostToDevice, ctx->stream));
        d_win = d_win_.p;
    }
    PF_HIP(d_newwin_.alloc(gz::RING));   // (window and new_window may be the same memory)

    // ---- find, count, chain ----
    const uint32_t stride = gz::piece_stride(piece_bytes);
    const uint64_t nb64 = gz::boundary_count(n_bytes, start_bit, stride);
    const uint32_t n_bound = (uint32_t)nb64, n1 = n_bound + 1;
    const size_t cand_b = up256((size_t)n1 * 8), piece_b = up256((size_t)n1 * sizeof(gz::Piece)), live_b = up256((size_t)n1 * 4),
                 place_b = up256((size_t)(n1 + 1) * 8);
    DevTmp<char> ww_;
    PF_HIP(ww_.alloc(2 * cand_b + 2 * piece_b + live_b + place_b + 256));
    char *ww = ww_.p;
    GunzipArgs a = {};
    a.comp = d_comp;
    a.n_bytes = (uint32_t)n_bytes;
    a.stride = stride;
    a.start_bit = start_bit;
    a.j0 = gz::first_boundary(start_bit, stride);
    a.n_bound = n_bound;
    a.cand = reinterpret_cast<uint64_t *>(ww);
    a.starts = reinterpret_cast<uint64_t *>(ww + cand_b);
    a.pieces = reinterpret_cast<gz::Piece *>(ww + 2 * cand_b);
    a.again = reinterpret_cast<gz::Piece *>(ww + 2 * cand_b + piece_b);
    a.live = reinterpret_cast<uint32_t *>(ww + 2 * cand_b + 2 * piece_b);
    a.place = reinterpret_cast<uint64_t *>(ww + 2 * cand_b + 2 * piece_b + live_b);
    a.small = reinterpret_cast<GunzipSmall *>(ww + 2 * cand_b + 2 * piece_b + live_b + place_b);
    a.window = d_win;
    a.n_window = n_window;
    a.new_window = d_newwin_.p;
    GunzipSmall h_small = {};
    h_small.bad_live = GUN_NO_BAD;
    PF_HIP(hipMemcpyAsync(a.small, &h_small, sizeof h_small, hipMemcpyHostToDevice, ctx->stream));
    ev.mark(0, ctx->stream);
    if (n_bound) {
        PF_HIP(hipMemsetAsync(a.cand, 0xff, (size_t)n_bound * 8, ctx->stream));   // NO_BIT
        k_gunzip_find<<<n_bound * GUN_FIND_SPLIT, GUN_WAVE, 0, ctx->stream>>>(a);
    }
    k_gunzip_starts<<<1, 1, 0, ctx->stream>>>(a);
    ev.mark(1, ctx->stream);
    k_gunzip_count<<<n1, GUN_WAVE, 0, ctx->stream>>>(a);
    ev.mark(2, ctx->stream);
    k_gunzip_chain<<<1, 1, 0, ctx->stream>>>(a);
    {
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-GUNZIP launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    PF_HIP(hipMemcpyAsync(&h_small, a.small, sizeof h_small, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));   // the one wait of a sound call before its last

    auto refuse_stream = [&](uint32_t clause, uint64_t bit) {
        res->clause = clause;
        res->clause_bit = bit;
        res->end_bit = start_bit;
        return refuse("bit " + std::to_string(bit) + ": " + gz::clause_text((int)clause));
    };
    if (h_small.clause) return refuse_stream(h_small.clause, h_small.clause_bit);
    const uint64_t total = h_small.total;
    res->out_bytes = total;
    if (total > 0xfffffff0ull) return refuse("a call inflates to fewer than 2^32 bytes");
    if (total > out_cap) {   // (said before anything is written: the caller comes back with room)
        res->out_bytes = total;
        pf::CtxErr{ctx} = "pf_inflate_gzip: the blocks inflate to " + std::to_string(total) + " bytes, out holds " + std::to_string(out_cap);
        return PF_ERR_OVERFLOW;
    }
    if (!out && total) return refuse("out is needed");
    uint32_t n_new = n_window;
    if (total) {
        // ---- decode, window, resolve ----
        uint8_t *d_out = reinterpret_cast<uint8_t *>(out);
        if (!is_device_ptr(out)) {
            PF_HIP(d_out_.alloc((size_t)total));
            d_out = d_out_.p;
        }
        DevTmp<uint16_t> d_stage_;
        PF_HIP(d_stage_.alloc((size_t)total * 2));
        a.stage = d_stage_.p;
        a.out = d_out;
        a.crc_threads = (uint32_t)std::max<uint64_t>(gz::RING, std::min<uint64_t>((total + GUN_CRC_SLICE - 1) / GUN_CRC_SLICE, 1u << 20));
        k_gunzip_decode<<<h_small.n_live, GUN_WAVE, 0, ctx->stream>>>(a);
        ev.mark(3, ctx->stream);
        k_gunzip_window<<<1, 1024, 0, ctx->stream>>>(a);
        ev.mark(4, ctx->stream);
        k_gunzip_resolve<<<(unsigned)((total + 1023) / 1024), 256, 0, ctx->stream>>>(a);
        k_gunzip_tail<<<(a.crc_threads + 255) / 256, 256, 0, ctx->stream>>>(a);
        ev.mark(5, ctx->stream);
        {
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-GUNZIP launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
        }
        PF_HIP(hipMemcpyAsync(&h_small, a.small, sizeof h_small, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (h_small.bad_live != GUN_NO_BAD) {
            gz::Piece r = {};
            PF_HIP(hipMemcpy(&r, a.again + h_small.bad_live, sizeof r, hipMemcpyDeviceToHost));
            res->out_bytes = 0;
            return refuse_stream(r.clause ? r.clause : (uint32_t)gz::CLAUSE_PIECE_LIMIT, r.end_bit);
        }
        n_new = (uint32_t)std::min<uint64_t>((uint64_t)n_window + total, gz::RING);
        if (d_out != reinterpret_cast<uint8_t *>(out)) PF_HIP(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        if (new_window && n_new) PF_HIP(hipMemcpyAsync(new_window, d_newwin_.p, n_new, hipMemcpyDefault, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    } else if (new_window && n_window && new_window != window) {
        PF_HIP(hipMemcpyAsync(new_window, d_win, n_window, hipMemcpyDefault, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    }
    res->end_bit = h_small.end_bit;
    res->final = h_small.final;
    res->n_window = n_new;
    res->crc_raw = h_small.crc_raw;
    if (stats) {
        stats->pieces_found = h_small.n_pieces;
        stats->pieces_live = h_small.n_live;
        stats->pieces_dead = h_small.n_pieces - h_small.n_live;
        stats->markers = h_small.markers;
        stats->blocks_stored = h_small.stored;
        stats->blocks_fixed = h_small.fixed;
        stats->blocks_dynamic = h_small.dynamic;
        stats->bytes_in = (h_small.end_bit + 7) / 8 - start_bit / 8;
        stats->bytes_out = total;
        if (ev.on && total) {
            for (int s = 0; s < 5; ++s) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev.e[s], ev.e[s + 1]) == hipSuccess) stats->stage_ms[s] = ms;
            }
        }
    }
    ctx_units(ctx, PF_K_GUNZIP, total);
    return PF_OK;
}
