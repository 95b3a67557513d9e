// K-DEFLATE: text deflated to blocked gzip (BGZF) where the FASTQ kernels leave it -- the text of one call cut into members of
// member_text bytes, each an independent gzip member whose bytes are a function of its text alone (pf_deflate_core.hpp states the parse,
// the coding and the container; pf_deflate_rule.hpp runs the same code on the host).  Two kernels and a scan on the launch stream:
//   deflate   k_deflate, one block of 256 threads per member, the text staged in LDS.
//             parse    256 positions a turn.  Candidates: a position's nearest earlier one with the same hash is looked for among the
//                      lanes of its wavefront (ballots over equal hashes), then in the table, which the four wavefronts read and update
//                      one behind the other, so that the table holds exactly the positions in front of the reader.  Match lengths: a
//                      thread a position, four bytes a compare, only for positions the parse can still stand on.  The greedy walk is
//                      serial: wavefront 0 holds the turn's 256 jumps in registers and steps through them with lane reads.  A taken
//                      position sets its bit in `start`, a match leaves length and distance in the three bytes of `tok` it covers
//                      first, and the symbols are counted with integer LDS atomics (the sums are order-free).
//             coding   pf_deflate::choose_block: ranks among the used symbols and canonical codes shared by the threads, Huffman's
//                      construction over at most 286 symbols and the header's run-length code on thread 0.
//             bits     2048 positions a turn, eight a thread: the bits of their tokens, a block-wide prefix sum of the bit counts, the
//                      bits OR-ed into a 16 KiB window in LDS (which takes the place of the hash table); the window's whole dwords go
//                      to the member's slot in global memory, coalesced.  Stored members are assembled dword by dword from the text.
//             crc      every thread the raw register of a slice of the text, moved on by the bytes behind it, added up by LDS atomics.
//             LDS: text 65 288, tok 65 280, start 8 160, table / window 16 384, codes and scratch 7.5 KiB: 162 752 of 163 840 bytes, one block a CU.
//   scan      the members' sizes (pf_scan.hip): sizes are not known before coding, so members are written to slots of the bound's stride
//   pack      k_deflate_pack, one block per member: the slot to its place in out, whole dwords where the destination allows.
// Compressed bytes are written with vector stores only.  No thread reads outside text[0, n_bytes) -- the staging loop tests every dword
// against the member's end -- and none writes outside its member's slot (a member is at most its text and 31 bytes: the stored form)
// or outside out[off[m], off[m + 1]).  Every loop is bounded by the member's positions, symbols or dwords.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_deflate_rule.hpp"
#include "pf_scan.hpp"

namespace pf {

namespace dfl = pf_deflate;

constexpr int DEF_BLOCK = 256;
constexpr uint32_t DEF_TEXT_DW = (dfl::MEMBER_TEXT + 8) / 4;   // the text and eight zero bytes: a compare reads up to seven behind the end
constexpr uint32_t DEF_WIN_DW = dfl::HASH_SIZE / 2;            // the window lies where the hash table was
constexpr uint32_t DEF_PER_THREAD = 8, DEF_BATCH = DEF_PER_THREAD * DEF_BLOCK;   // positions of one turn of the bit stage
static_assert(DEF_BATCH * 48 / 32 + 8 < DEF_WIN_DW, "a turn's tokens (at most 48 bits each) fit the window behind its first dword");

struct DeflateArgs {
    const uint8_t *text;
    uint64_t n_bytes;
    uint32_t member_text;
    uint8_t *slots;             // n_members slots of `stride` bytes (a multiple of four, at least member_text + 31)
    uint32_t stride;
    uint64_t *sizes;            // n_members + 1 entries, the last 0
    unsigned long long *counts; // stored, fixed, dynamic, literals, matches
};

struct BlockSync {
    __host__ __device__ void operator()() const {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
};

struct LdsText {   // the member's text, zeros behind it
    const uint32_t *t;
    __device__ uint32_t word(uint32_t i) const {
        const uint32_t k = i >> 2;
        return __builtin_amdgcn_alignbyte(t[k + 1], t[k], i & 3u);
    }
    __device__ uint32_t operator[](uint32_t i) const { return reinterpret_cast<const uint8_t *>(t)[i]; }
};

struct WinOut {   // the member's bits from dword base_dw on, in LDS
    uint32_t *win;
    uint32_t base_dw;
    __device__ void put(uint32_t bitpos, uint64_t value, uint32_t nbits) {
        if (!nbits) return;
        value &= (1ull << nbits) - 1ull;   // nbits <= 57
        const uint32_t rel = bitpos - 32u * base_dw, k = rel >> 5, sh = rel & 31u;
        const uint64_t rest = (value >> 1) >> (31u - sh);
        const uint32_t w0 = (uint32_t)(value << sh), w1 = (uint32_t)rest, w2 = (uint32_t)(rest >> 32);
        if (w0) atomicOr(&win[k], w0);
        if (w1) atomicOr(&win[k + 1], w1);
        if (w2) atomicOr(&win[k + 2], w2);
    }
};

union DeflateScratch {
    struct { uint16_t jump[DEF_BLOCK]; uint32_t taken[DEF_BLOCK / 32]; } parse;
    uint32_t wave_sum[DEF_BLOCK / 64];
};

__global__ __launch_bounds__(DEF_BLOCK) void k_deflate(const DeflateArgs a) {
    __shared__ uint32_t text32[DEF_TEXT_DW];
    __shared__ uint32_t tok32[dfl::MEMBER_TEXT / 4];
    __shared__ uint32_t start[dfl::MEMBER_TEXT / 32];
    __shared__ uint32_t table[DEF_WIN_DW];
    __shared__ dfl::Codes codes;
    __shared__ DeflateScratch scratch;
    __shared__ uint32_t s_next, s_at, s_crc;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t m = blockIdx.x;
    const uint64_t begin = m * a.member_text;
    const uint32_t n = (uint32_t)(a.n_bytes - begin < a.member_text ? a.n_bytes - begin : a.member_text);
    const uint8_t *src = a.text + begin;
    uint8_t *tokb = reinterpret_cast<uint8_t *>(tok32);
    uint16_t *head = reinterpret_cast<uint16_t *>(table);
    const LdsText T{text32};

    // ---- stage the text; clear the tables ----
    {
        const uint32_t shift = (uint32_t)((uintptr_t)src & 3u);
        for (uint32_t k = tid; k < DEF_TEXT_DW; k += DEF_BLOCK) {
            const uint32_t b0 = 4 * k;
            uint32_t v = 0;
            if (b0 < n) {
                if (shift == 0 && b0 + 4 <= n) {
                    v = *reinterpret_cast<const uint32_t *>(src + b0);
                } else if (shift != 0 && k > 0 && b0 + 8 <= n) {   // the two whole dwords about it lie within the member
                    const uint32_t *al = reinterpret_cast<const uint32_t *>(src + b0 - shift);
                    v = __builtin_amdgcn_alignbyte(al[1], al[0], shift);
                } else {
                    for (uint32_t b = 0; b < 4; ++b)
                        if (b0 + b < n) v |= (uint32_t)src[b0 + b] << (8 * b);
                }
            }
            text32[k] = v;
        }
        for (uint32_t k = tid; k < dfl::MEMBER_TEXT / 4; k += DEF_BLOCK) tok32[k] = 0;
        for (uint32_t k = tid; k < dfl::MEMBER_TEXT / 32; k += DEF_BLOCK) start[k] = 0;
        for (uint32_t k = tid; k < DEF_WIN_DW; k += DEF_BLOCK) table[k] = 0;
        for (uint32_t k = tid; k < dfl::N_LIT + 2; k += DEF_BLOCK) codes.freq_lit[k] = 0;
        for (uint32_t k = tid; k < dfl::N_DIST + 2; k += DEF_BLOCK) codes.freq_dist[k] = 0;
        if (tid == 0) { s_next = 0; s_crc = 0; }
    }
    __syncthreads();

    // ---- parse ----
    for (uint32_t base = 0; base < n; base += DEF_BLOCK) {
        const uint32_t p = base + tid;
        const uint32_t next = s_next;   // (written before the last barrier of the turn before)
        const bool valid = p + 4 <= n;
        const uint32_t h = valid ? dfl::hash4(T.word(p)) : 0xffffffffu;
        // the nearest earlier lane of the wavefront with the same hash, and whether a later one has it
        int near = -1;
        bool last = false;
        for (uint64_t todo = __ballot(valid); todo;) {   // a turn takes the lanes of one hash off
            const int l = __builtin_ctzll(todo);
            const uint32_t hl = (uint32_t)__builtin_amdgcn_readlane((int)h, l);
            const bool same = valid && h == hl;
            const uint64_t mask = __ballot(same);
            if (same) {
                const uint64_t below = mask & ((1ull << lane) - 1ull);
                near = below ? 63 - __builtin_clzll(below) : -1;
                last = ((mask >> lane) >> 1) == 0;
            }
            todo &= ~mask;
        }
        uint32_t q1 = 0;   // the candidate's position + 1
        for (uint32_t w = 0; w < DEF_BLOCK / 64; ++w) {
            if (wave == w && valid) {
                q1 = near >= 0 ? base + 64 * wave + (uint32_t)near + 1 : head[h];
                if (last) head[h] = (uint16_t)(p + 1);
            }
            __syncthreads();
        }
        if (next >= base + DEF_BLOCK) continue;   // (the same for the whole block) a match leads over the turn
        uint32_t len = 0, dist = 0;
        if (p >= next && q1 && p - (q1 - 1) <= dfl::MAX_DIST) {
            len = dfl::match_len(T, p, q1 - 1, n - p < dfl::MAX_MATCH ? n - p : dfl::MAX_MATCH);
            dist = p - (q1 - 1);
        }
        scratch.parse.jump[tid] = (uint16_t)(len >= dfl::MIN_MATCH ? len : 1);
        __syncthreads();
        if (wave == 0) {   // the greedy walk
            uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)(next - base));
            uint32_t jv[4];
            uint64_t taken[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) jv[s] = scratch.parse.jump[64 * s + lane];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                taken[s] = 0;
                while (cur < 64u * (s + 1)) {   // a turn moves on by at least one position
                    taken[s] |= 1ull << (cur & 63u);
                    cur += (uint32_t)__builtin_amdgcn_readlane((int)jv[s], (int)(cur & 63u));
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    scratch.parse.taken[2 * s] = (uint32_t)taken[s];
                    scratch.parse.taken[2 * s + 1] = (uint32_t)(taken[s] >> 32);
                }
                s_next = base + cur;
            }
        }
        __syncthreads();
        if (p < n && ((scratch.parse.taken[tid >> 5] >> (tid & 31u)) & 1u)) {
            atomicOr(&start[p >> 5], 1u << (p & 31u));
            if (len >= dfl::MIN_MATCH) {
                tokb[p] = (uint8_t)(len - 3);   // (never 0: what says literal)
                tokb[p + 1] = (uint8_t)(dist - 1);
                tokb[p + 2] = (uint8_t)((dist - 1) >> 8);
                atomicAdd(&codes.freq_lit[dfl::len_sym(len).sym], 1u);
                atomicAdd(&codes.freq_dist[dfl::dist_sym(dist).sym], 1u);
            } else {
                atomicAdd(&codes.freq_lit[T[p]], 1u);
            }
        }
        // (the turn's last barrier is the first of the next turn's table barriers: jump and taken are written again behind them)
    }
    __syncthreads();

    // ---- CRC-32: a slice a thread ----
    {
        const uint32_t raw = pf_inflate::crc_raw(T, pf_inflate::slice_begin(n, DEF_BLOCK, tid), pf_inflate::slice_end(n, DEF_BLOCK, tid));
        if (raw) atomicXor(&s_crc, pf_inflate::slice_share(raw, n, DEF_BLOCK, tid));
    }
    // ---- coding ----
    uint32_t n_lit = 0, n_match = 0;
    if (tid == 0) {
        for (uint32_t s = 0; s < 256; ++s) n_lit += codes.freq_lit[s];
        for (uint32_t s = 0; s < dfl::N_DIST; ++s) n_match += codes.freq_dist[s];
        codes.freq_lit[dfl::EOB] = 1;
    }
    dfl::choose_block(codes, n, tid, (uint32_t)DEF_BLOCK, BlockSync{});
    const uint32_t kind = codes.kind, size = dfl::member_bytes(codes), n_dw = (size + 3) / 4;
    const uint32_t crc = pf_inflate::crc_finish(s_crc, n);
    uint32_t *slot = reinterpret_cast<uint32_t *>(a.slots + m * a.stride);   // size <= n + 31 <= stride

    // ---- bits ----
    uint32_t *win = table;
    for (uint32_t k = tid; k < DEF_WIN_DW; k += DEF_BLOCK) win[k] = 0;
    __syncthreads();
    if (tid == 0) {
        WinOut o{win, 0};
        s_at = dfl::put_headers(codes, n, o);
    }
    __syncthreads();
    if (kind == dfl::KIND_STORED) {
        // header and block header (23 bytes, in the window), the text, the trailer: a dword a thread
        const uint32_t t0 = dfl::HEADER + 5, t1 = t0 + n;
        for (uint32_t k = tid; k < n_dw; k += DEF_BLOCK) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t i = 4 * k + b;
                uint32_t byte = 0;
                if (i < t0) byte = reinterpret_cast<const uint8_t *>(win)[i];
                else if (i < t1) byte = T[i - t0];
                else if (i < t1 + 4) byte = (crc >> (8 * (i - t1))) & 0xffu;
                else if (i < t1 + 8) byte = (n >> (8 * (i - t1 - 4))) & 0xffu;
                v |= byte << (8 * b);
            }
            slot[k] = v;
        }
    } else {
        if (kind == dfl::KIND_FIXED) dfl::fixed_codes(codes, tid, (uint32_t)DEF_BLOCK, BlockSync{});
        uint32_t at = s_at, base_dw = 0;
        for (uint32_t b0 = 0; b0 < n; b0 += DEF_BATCH) {
            // the window's whole dwords to the slot; its last, begun one is the next window's first
            const uint32_t cur_dw = at >> 5;
            for (uint32_t k = base_dw + tid; k < cur_dw; k += DEF_BLOCK) slot[k] = win[k - base_dw];
            const uint32_t carry = win[cur_dw - base_dw];
            __syncthreads();
            for (uint32_t k = tid; k < DEF_WIN_DW; k += DEF_BLOCK) win[k] = k == 0 ? carry : 0u;
            base_dw = cur_dw;
            // the bits of this thread's tokens
            uint64_t val[DEF_PER_THREAD];
            uint32_t nb[DEF_PER_THREAD], sum = 0;
            const uint32_t p0 = b0 + DEF_PER_THREAD * tid;
#pragma unroll
            for (uint32_t j = 0; j < DEF_PER_THREAD; ++j) {
                const uint32_t p = p0 + j;
                nb[j] = 0;
                val[j] = 0;
                if (p < n && ((start[p >> 5] >> (p & 31u)) & 1u)) {
                    const uint32_t l3 = tokb[p];
                    nb[j] = l3 ? dfl::match_bits(codes, l3 + 3, ((uint32_t)tokb[p + 1] | ((uint32_t)tokb[p + 2] << 8)) + 1, &val[j])
                               : dfl::literal_bits(codes, T[p], &val[j]);
                }
                sum += nb[j];
            }
            // block-wide exclusive prefix sum of `sum`
            uint32_t incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                if ((int)lane >= d) incl += up;
            }
            if (lane == 63) scratch.wave_sum[wave] = incl;
            __syncthreads();   // (the window is cleared as well)
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < DEF_BLOCK / 64; ++w) {
                const uint32_t s = scratch.wave_sum[w];
                if (w < wave) before += s;
                total += s;
            }
            WinOut o{win, base_dw};
            uint32_t bit = at + before + incl - sum;
#pragma unroll
            for (uint32_t j = 0; j < DEF_PER_THREAD; ++j) {
                o.put(bit, val[j], nb[j]);
                bit += nb[j];
            }
            at += total;
            __syncthreads();
        }
        if (tid == 0) {
            WinOut o{win, base_dw};
            dfl::put_end(codes, at, crc, n, o);
        }
        __syncthreads();
        for (uint32_t k = base_dw + tid; k < n_dw; k += DEF_BLOCK) slot[k] = win[k - base_dw];
    }
    if (tid == 0) {
        a.sizes[m] = size;
        atomicAdd(&a.counts[kind], 1ull);
        if (n_lit) atomicAdd(&a.counts[3], (unsigned long long)n_lit);
        if (n_match) atomicAdd(&a.counts[4], (unsigned long long)n_match);
    }
}

// slot m -> out[off[m], off[m + 1]): bytes up to the first dword boundary of the destination, dwords, bytes
__global__ __launch_bounds__(DEF_BLOCK) void k_deflate_pack(const uint8_t *__restrict__ slots, uint32_t stride, const uint64_t *__restrict__ off,
                                                            uint8_t *__restrict__ out) {
    const uint64_t m = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t size = (uint32_t)(off[m + 1] - off[m]);
    const uint8_t *src = slots + m * stride;
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
    uint8_t *dst = out + off[m];
    const uint32_t head = min(size, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
    const uint32_t n_dw = (size - head) / 4, stride_dw = stride / 4;
    if (tid < head) dst[tid] = src[tid];
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t k = tid; k < n_dw; k += DEF_BLOCK) {
        const uint32_t i = (head + 4 * k) >> 2;   // head + 4k + 4 <= size <= stride
        const uint32_t lo = src32[i], hi = i + 1 < stride_dw ? src32[i + 1] : 0u;
        dst32[k] = __builtin_amdgcn_alignbyte(hi, lo, head);
    }
    for (uint32_t i = head + 4 * n_dw + tid; i < size; i += DEF_BLOCK) dst[i] = src[i];
}

}  // namespace pf

using namespace pf;

extern "C" int pf_deflate_bgzf(pf_ctx *ctx, const char *text, uint64_t n_bytes, uint32_t member_text, uint8_t *out, uint64_t out_cap,
                               uint64_t *out_bytes, uint64_t *member_off, pf_deflate_stats *stats) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_deflate_bgzf: " + m; return (int)PF_ERR_ARG; };
    if (!out_bytes) return refuse("out_bytes is needed");
    *out_bytes = 0;
    if (stats) *stats = pf_deflate_stats{};
    if (member_text < 1 || member_text > dfl::MEMBER_TEXT)
        return refuse("member_text is " + std::to_string(member_text) + ", a member holds 1 .. " + std::to_string(dfl::MEMBER_TEXT) + " bytes of text");
    const uint64_t n_members = dfl::n_members(n_bytes, member_text), bound = dfl::bound(n_bytes, member_text);
    if (n_members > 0x7FFFFFFFull) return refuse("a call holds fewer than 2^31 members");
    if (out_cap < bound) {
        pf::CtxErr{ctx} = "pf_deflate_bgzf: out holds " + std::to_string(out_cap) + " bytes, " + std::to_string(n_members) + " members of " +
                          std::to_string(n_bytes) + " bytes of text may take " + std::to_string(bound);
        return PF_ERR_OVERFLOW;
    }
    PF_HIP(hipSetDevice(ctx->device));
    const uint64_t zero = 0;
    if (n_members == 0) {
        if (member_off) PF_HIP(hipMemcpy(member_off, &zero, 8, hipMemcpyDefault));
        return PF_OK;
    }
    if (!text || !out) return refuse("text and out are needed");
    Timed timed(ctx, PF_K_DEFLATE);

    // ---- stage what the caller holds on the host ----
    DevTmp<uint8_t> d_text_, d_out_;
    const uint8_t *d_text = reinterpret_cast<const uint8_t *>(text);
    if (!is_device_ptr(text)) {
        PF_HIP(d_text_.alloc((size_t)n_bytes));
        PF_HIP(hipMemcpyAsync(d_text_.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
        d_text = d_text_.p;
    }
    uint8_t *d_out = out;
    if (!is_device_ptr(out)) {
        PF_HIP(d_out_.alloc((size_t)bound));
        d_out = d_out_.p;
    }

    // ---- slots, sizes, places ----
    const uint32_t stride = (member_text + dfl::MEMBER_EXTRA + 3) & ~3u;
    const uint64_t n1 = n_members + 1;
    const size_t slot_bytes = up256((size_t)n_members * stride), size_bytes = up256((size_t)n1 * 8), scr_bytes = up256(scan_scratch_bytes(n1));
    DevTmp<char> ww_;
    PF_HIP(ww_.alloc(slot_bytes + 2 * size_bytes + scr_bytes + 256));
    char *ww = ww_.p;
    DeflateArgs a = {};
    a.text = d_text;
    a.n_bytes = n_bytes;
    a.member_text = member_text;
    a.slots = reinterpret_cast<uint8_t *>(ww);
    a.stride = stride;
    a.sizes = reinterpret_cast<uint64_t *>(ww + slot_bytes);
    uint64_t *d_off = reinterpret_cast<uint64_t *>(ww + slot_bytes + size_bytes);
    void *scratch = ww + slot_bytes + 2 * size_bytes;
    a.counts = reinterpret_cast<unsigned long long *>(ww + slot_bytes + 2 * size_bytes + scr_bytes);
    PF_HIP(hipMemsetAsync(a.sizes + n_members, 0, 8, ctx->stream));
    PF_HIP(hipMemsetAsync(a.counts, 0, 5 * 8, ctx->stream));
    k_deflate<<<(unsigned)n_members, DEF_BLOCK, 0, ctx->stream>>>(a);
    {
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-DEFLATE launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    PF_HIP(scan_exclusive_u64(a.sizes, d_off, n1, scratch, ctx->stream));
    k_deflate_pack<<<(unsigned)n_members, DEF_BLOCK, 0, ctx->stream>>>(a.slots, stride, d_off, d_out);
    {
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-DEFLATE pack launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    }
    uint64_t total = 0;
    unsigned long long h_counts[5] = {0, 0, 0, 0, 0};
    PF_HIP(hipMemcpyAsync(&total, d_off + n_members, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(h_counts, a.counts, sizeof h_counts, hipMemcpyDeviceToHost, ctx->stream));
    if (member_off) PF_HIP(hipMemcpyAsync(member_off, d_off, (size_t)n1 * 8, hipMemcpyDefault, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    if (total > bound) return refuse("the members take " + std::to_string(total) + " bytes, above the bound " + std::to_string(bound));   // (never)
    if (d_out != out) {   // only packed bytes leave the device
        PF_HIP(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out_bytes = total;
    if (stats) {
        stats->members = n_members;
        stats->bytes_in = n_bytes;
        stats->bytes_out = total;
        stats->blocks_stored = h_counts[0];
        stats->blocks_fixed = h_counts[1];
        stats->blocks_dynamic = h_counts[2];
        stats->literals = h_counts[3];
        stats->matches = h_counts[4];
    }
    ctx_units(ctx, PF_K_DEFLATE, n_bytes);
    return PF_OK;
}
