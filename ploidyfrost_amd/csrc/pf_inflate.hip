// K-INFLATE: blocked gzip (BGZF) inflated where the FASTQ kernels read it -- the members of one call, each an independent gzip member of
// at most 64 KiB (pf_inflate_rule.hpp), to their texts one behind the other in device memory.  Three stages on the launch stream:
//   headers   k_inflate_headers, one thread per member: the header by pf_inflate::parse_member_bytes, the payload's bounds, ISIZE and the
//             CRC; an exclusive scan of ISIZE (pf_scan.hip) gives every member's place in the output and the total.  One host wait
//             here: the total (the caller's buffer may be too small) and the smallest member refused so far.
//   inflate   k_inflate, one wavefront per member.  The decode is serial within a member, so all 64 lanes run pf_inflate::inflate_stream
//             (pf_inflate_core.hpp, the decoder the host rule and K-GUNZIP run) with the same arguments; what is not serial is shared by
//             the lanes: the look-up tables of a block's codes (build_huff), the match copies (LaneOut::copy, up to 258 bytes, distance
//             < length as a repeating pattern), stored blocks (LaneOut::stored), the refill of the input window (GzIn, pf_gz_dev.hpp,
//             which K-GUNZIP shares), the CRC and the final write.
//             The member's text is assembled in LDS (64 KiB) and written once, in whole dwords where the destination allows; with the
//             tables (4 KiB) and the input window (1 KiB) a block takes 70 KiB, two blocks a CU.  (The form that writes the text to
//             global memory as it is produced was not built: a copy would wait for the stores of the match before it -- DESIGN.md.)
//   crc       inside k_inflate: every lane takes the raw CRC register of a slice of the text in LDS, moves it on by the bytes behind
//             the slice (multiplication by x^(8n) mod P), and the shares are added up across the wavefront.  Always made.
// Compressed bytes are read with vector loads only: the window refill (a dword a lane, bytes at the member's edges) and the stored-block
// copy.  No lane reads outside [member_off[m], member_off[m + 1]) -- the refill and the header reads test every address against it --
// and none writes outside [out_off[m], out_off[m] + ISIZE): the core tests every put and copy against ISIZE before it is made, and the
// final write loops to ISIZE.  Every loop is bounded by the payload's bits and ISIZE (pf_inflate_core.hpp).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"
#include "pf_gz_dev.hpp"
#include "pf_inflate_rule.hpp"
#include "pf_scan.hpp"

namespace pf {

constexpr int INF_WAVE = GZ_WAVE;
constexpr uint32_t INF_TABLE_LEN = 100, INF_TABLE_ORDER = 101;   // member_off itself is wrong: not clauses of the rule
constexpr unsigned long long INF_NO_BAD = ~0ull;

struct InflateMember {    // what the header stage leaves for the inflate stage
    uint32_t payload_off, n_in, crc, clause;
};
struct InflateArgs {
    const uint8_t *comp;
    uint64_t n_bytes;
    const uint64_t *member_off;
    uint64_t n_members;
    InflateMember *members;
    uint64_t *isize;          // n_members + 1 entries, the last 0
    const uint64_t *out_off;  // their exclusive scan
    uint8_t *out;
    unsigned long long *bad;  // the smallest member refused
    unsigned long long *blocks;   // stored, fixed, dynamic
};

__global__ __launch_bounds__(256) void k_inflate_headers(const InflateArgs a) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m > a.n_members) return;
    if (m == a.n_members) { a.isize[m] = 0; return; }
    const uint64_t off = a.member_off[m], end = a.member_off[m + 1];
    InflateMember mem = {0, 0, 0, 0};
    uint64_t isize = 0;
    if (off > end || end > a.n_bytes) {
        mem.clause = INF_TABLE_ORDER;
    } else {
        pf_inflate::Header h;
        mem.clause = (uint32_t)pf_inflate::parse_member_bytes(GzBytes{a.comp + off}, end - off, h);   // (reads [off, end) only)
        if (!mem.clause && (uint64_t)h.member_len != end - off) mem.clause = INF_TABLE_LEN;
        if (!mem.clause) {
            mem.payload_off = h.payload_off;
            mem.n_in = h.member_len - h.payload_off - pf_inflate::TRAILER;
            mem.crc = h.crc;
            isize = h.isize;
        }
    }
    a.members[m] = mem;
    a.isize[m] = isize;
    if (mem.clause) atomicMin(a.bad, (unsigned long long)m);
}

// the member's text in LDS; the core has tested every range
struct LaneOut {
    typedef uint32_t Pos;
    static constexpr int BEYOND = pf_inflate::CLAUSE_OUT_BEYOND;
    uint8_t *o;
    uint32_t lane;
    __device__ uint32_t reach() const { return 0; }   // a member refers to nothing in front of itself
    __device__ void put(uint32_t at, uint8_t b) { if (lane == 0) o[at] = b; }
    __device__ void copy(uint32_t at, uint32_t dist, uint32_t len) {
        __syncthreads();   // the bytes in front of `at` are in place
        const uint8_t *src = o + at - dist;
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += INF_WAVE) o[at + i] = src[i];
        } else {
            for (uint32_t i = lane; i < len; i += INF_WAVE) o[at + i] = src[i % dist];   // only bytes in front of `at` are read
        }
    }
    __device__ void stored(const GzIn &in, uint32_t src, uint32_t at, uint32_t len) {   // src + len <= n_in
        for (uint32_t i = lane; i < len; i += INF_WAVE) o[at + i] = in.raw(src + i);
    }
};

__global__ __launch_bounds__(INF_WAVE) void k_inflate(const InflateArgs a) {
    __shared__ uint32_t text32[pf_inflate::MAX_ISIZE / 4];
    __shared__ uint32_t window[GZ_WINDOW / 4];
    __shared__ pf_inflate::Work work;
    const uint64_t m = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const InflateMember mem = a.members[m];
    if (mem.clause) return;   // refused by its header
    const uint32_t isize = (uint32_t)a.isize[m];
    uint8_t *text = reinterpret_cast<uint8_t *>(text32);
    const uint8_t *payload = a.comp + a.member_off[m] + mem.payload_off;
    const GzIn in(payload, mem.n_in, lane, window, 0u);
    LaneOut out{text, lane};
    pf_inflate::Blocks blocks;
    uint32_t produced = 0;
    int clause = pf_inflate::inflate_stream(in, mem.n_in, out, isize, work, lane, (uint32_t)INF_WAVE, GzSync{}, blocks, produced);
    __syncthreads();
    if (!clause) {
        const uint32_t raw = pf_inflate::crc_raw(GzBytes{text}, pf_inflate::slice_begin(isize, INF_WAVE, lane), pf_inflate::slice_end(isize, INF_WAVE, lane));
        uint32_t sum = pf_inflate::slice_share(raw, isize, INF_WAVE, lane);
        for (int d = 32; d >= 1; d >>= 1) sum ^= (uint32_t)__shfl_xor((int)sum, d, INF_WAVE);
        if (pf_inflate::crc_finish(sum, isize) != mem.crc) clause = pf_inflate::CLAUSE_CRC;
    }
    if (clause) {
        if (lane == 0) {
            a.members[m].clause = (uint32_t)clause;
            atomicMin(a.bad, (unsigned long long)m);
        }
        return;
    }
    // the text to its place: bytes up to the first dword boundary of the destination, dwords, bytes
    uint8_t *dst = a.out + a.out_off[m];
    const uint32_t head = min(isize, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
    const uint32_t n_dw = (isize - head) / 4;
    if (lane < head) dst[lane] = text[lane];
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t k = lane; k < n_dw; k += INF_WAVE) {
        const uint8_t *s = text + head + 4 * k;
        dst32[k] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    for (uint32_t i = head + 4 * n_dw + lane; i < isize; i += INF_WAVE) dst[i] = text[i];
    if (lane == 0) {
        if (blocks.stored) atomicAdd(&a.blocks[0], (unsigned long long)blocks.stored);
        if (blocks.fixed) atomicAdd(&a.blocks[1], (unsigned long long)blocks.fixed);
        if (blocks.dynamic) atomicAdd(&a.blocks[2], (unsigned long long)blocks.dynamic);
    }
}

}  // namespace pf

using namespace pf;

extern "C" int pf_inflate_bgzf(pf_ctx *ctx, const uint8_t *comp, uint64_t n_bytes, const uint64_t *member_off, uint64_t n_members, char *out,
                               uint64_t out_cap, uint64_t *out_bytes, pf_inflate_stats *stats, uint64_t *bad_member) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = "pf_inflate_bgzf: " + m; return (int)PF_ERR_ARG; };
    if (!out_bytes) return refuse("out_bytes is needed");
    *out_bytes = 0;
    if (bad_member) *bad_member = 0;
    if (stats) *stats = pf_inflate_stats{};
    if (n_members == 0) return PF_OK;
    if (!comp || !member_off) return refuse("comp and member_off are needed");
    if (n_members > 0x7FFFFFFFull) return refuse("a call holds fewer than 2^31 members");
    PF_HIP(hipSetDevice(ctx->device));
    Timed timed(ctx, PF_K_INFLATE);

    // ---- stage what the caller holds on the host ----
    DevTmp<uint8_t> d_comp_;
    DevTmp<uint64_t> d_off_;
    DevTmp<uint8_t> d_out_;
    const uint8_t *d_comp = comp;
    const uint64_t *d_off = member_off;
    if (!is_device_ptr(comp)) {
        PF_HIP(d_comp_.alloc((size_t)n_bytes));
        if (n_bytes) PF_HIP(hipMemcpyAsync(d_comp_.p, comp, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
        d_comp = d_comp_.p;
    }
    if (!is_device_ptr(member_off)) {
        PF_HIP(d_off_.alloc((size_t)(n_members + 1) * 8));
        PF_HIP(hipMemcpyAsync(d_off_.p, member_off, (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = d_off_.p;
    }

    // ---- headers, places ----
    const uint64_t n1 = n_members + 1;
    const size_t mem_bytes = up256((size_t)n_members * sizeof(InflateMember)), size_bytes = up256((size_t)n1 * 8), scr_bytes = up256(scan_scratch_bytes(n1));
    DevTmp<char> ww_;   // the members' headers, sizes and places of this call
    PF_HIP(ww_.alloc(mem_bytes + 2 * size_bytes + scr_bytes + 256));
    char *ww = ww_.p;
    InflateArgs a = {};
    a.comp = d_comp;
    a.n_bytes = n_bytes;
    a.member_off = d_off;
    a.n_members = n_members;
    a.members = reinterpret_cast<InflateMember *>(ww);
    a.isize = reinterpret_cast<uint64_t *>(ww + mem_bytes);
    uint64_t *d_out_off = reinterpret_cast<uint64_t *>(ww + mem_bytes + size_bytes);
    a.out_off = d_out_off;
    void *scratch = ww + mem_bytes + 2 * size_bytes;
    unsigned long long *d_small = reinterpret_cast<unsigned long long *>(ww + mem_bytes + 2 * size_bytes + scr_bytes);   // bad, blocks[3]
    a.bad = d_small;
    a.blocks = d_small + 1;
    const unsigned long long small0[4] = {INF_NO_BAD, 0, 0, 0};
    PF_HIP(hipMemcpyAsync(d_small, small0, sizeof small0, hipMemcpyHostToDevice, ctx->stream));
    k_inflate_headers<<<(unsigned)((n1 + 255) / 256), 256, 0, ctx->stream>>>(a);
    PF_HIP(scan_exclusive_u64(a.isize, d_out_off, n1, scratch, ctx->stream));
    unsigned long long h_small[4] = {INF_NO_BAD, 0, 0, 0};
    uint64_t total = 0, off_first = 0, off_last = 0;
    PF_HIP(hipMemcpyAsync(&total, d_out_off + n_members, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&h_small[0], d_small, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&off_first, d_off, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(&off_last, d_off + n_members, 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));   // the one wait of a sound call before its last

    auto refuse_member = [&](uint64_t m) -> int {
        InflateMember mem = {};
        PF_HIP(hipMemcpy(&mem, a.members + m, sizeof mem, hipMemcpyDeviceToHost));
        if (bad_member) *bad_member = m;
        const std::string what = mem.clause == INF_TABLE_ORDER  ? "member_off does not ascend within n_bytes"
                                 : mem.clause == INF_TABLE_LEN ? "member_off does not give the member's BSIZE + 1 bytes"
                                                               : pf_inflate::clause_text((int)mem.clause);
        return refuse("member " + std::to_string(m) + " of the call: " + what);
    };
    if (total <= out_cap) {   // (with a header refused as well: a member in front of it may be refused by its stream)
        // ---- inflate (members of no bytes as well: their streams and CRCs are checked like any other) ----
        if (!out && total) return refuse("out is needed");
        uint8_t *d_out = reinterpret_cast<uint8_t *>(out);
        if (!out || !is_device_ptr(out)) {
            PF_HIP(d_out_.alloc((size_t)total));
            d_out = d_out_.p;
        }
        a.out = d_out;
        k_inflate<<<(unsigned)n_members, INF_WAVE, 0, ctx->stream>>>(a);
        {
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-INFLATE launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
        }
        PF_HIP(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        if (h_small[0] == INF_NO_BAD && total && d_out != reinterpret_cast<uint8_t *>(out)) {
            PF_HIP(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
            PF_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    *out_bytes = total;
    if (total > out_cap) {   // (said first: the caller comes back with room, and every member is judged then)
        pf::CtxErr{ctx} = "pf_inflate_bgzf: the members inflate to " + std::to_string(total) + " bytes, out holds " + std::to_string(out_cap);
        return PF_ERR_OVERFLOW;
    }
    if (h_small[0] != INF_NO_BAD) { *out_bytes = 0; return refuse_member((uint64_t)h_small[0]); }
    if (stats) {
        stats->members = n_members;
        stats->bytes_in = off_last - off_first;
        stats->bytes_out = total;
        stats->blocks_stored = h_small[1];
        stats->blocks_fixed = h_small[2];
        stats->blocks_dynamic = h_small[3];
    }
    ctx_units(ctx, PF_K_INFLATE, total);
    return PF_OK;
}
