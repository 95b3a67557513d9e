// K-HIST: the histogram of the counters K-KMC decodes -- the k-mer histogram file `kmc_tools transform <db> histogram` writes and
// the reference's cutoffL / cutoffU / -h read (src/Main.cpp:200-277), taken from the array that is already in HBM.
//   hist[min(c, n_bins - 1)] += 1 for every counter c with lo <= c <= hi; every other bin 0.
// One kernel, k_hist, one read of 4 bytes a record:
//   load      16 bytes a lane (four counters), grid-stride over the aligned body of the array; the at most six counters in front of
//             and behind the body are read one by one by block 0;
//   combine   real databases have a dominant bin (count 1: the sequencing errors).  Before any atomic the lanes of a wavefront that
//             hold the bin of the first lane with a counter in range are counted by one ballot and that lane adds their number;
//             a lane with another bin issues its own add.  A wavefront of equal counters costs one atomic a load component
//             instead of 64 adds to one address, a wavefront of distinct counters costs one ballot more than the plain kernel;
//   low bins  HIST_LDS_BINS u32 counters in LDS per block (16 KB: eight blocks of 256 threads fill the CU's 32 wavefront slots
//             with 128 of its 160 KB, so LDS never lowers the occupancy the launch asks for); the non-zero ones are flushed with
//             one u64 atomic each when the block ends;
//   high bins bins at or above HIST_LDS_BINS (rare in any real database: -u defaults to 1000) go to the u64 bins in HBM directly;
//   32 bits   a block never counts 2^32 records into LDS: the launch is refused when the grid's shape would let it (hist_launch).
// Integer atomics only: the result is the same bits on every call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"

namespace pf {

constexpr int HIST_BLOCK = 256;
constexpr int HIST_PER_CU = 8;                 // blocks a CU holds: 32 wavefronts, 8 x 16 KB of LDS
constexpr uint32_t HIST_LDS_BINS = 4096;       // bins counted in LDS
constexpr int HIST_VEC = 4;                    // counters a lane loads at once

struct HistArgs {
    const uint32_t *counts;
    uint64_t n;          // all counters
    uint64_t head;       // counters in front of the 16-byte aligned body
    uint64_t n_vec;      // uint4 groups of the body
    uint64_t lo, hi;
    uint32_t n_bins;
    unsigned long long *hist;
};

__device__ inline void hist_bin_add(uint32_t bin, uint32_t c, unsigned int *h, unsigned long long *hist) {
    if (bin < HIST_LDS_BINS) atomicAdd(&h[bin], c);
    else atomicAdd(&hist[bin], (unsigned long long)c);
}

// one counter a lane (have: the lane holds one).  Called by every lane of the wavefront together.
__device__ inline void hist_count(uint32_t v, bool have, const HistArgs &a, unsigned int *h) {
    const bool in = have && (uint64_t)v >= a.lo && (uint64_t)v <= a.hi;
    const unsigned long long act = __ballot(in);
    if (!act) return;
    const uint32_t bin = v < a.n_bins - 1 ? v : a.n_bins - 1;
    const int leader = __ffsll(act) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, leader, 64);
    const unsigned long long same = __ballot(in && bin == b0);
    if (!in) return;
    if (bin != b0) hist_bin_add(bin, 1u, h, a.hist);
    else if ((int)(threadIdx.x & 63) == leader) hist_bin_add(b0, (uint32_t)__popcll(same), h, a.hist);
}

__global__ __launch_bounds__(HIST_BLOCK) void k_hist(const HistArgs a) {
    __shared__ unsigned int h[HIST_LDS_BINS];
    const uint32_t lds_bins = a.n_bins < HIST_LDS_BINS ? a.n_bins : HIST_LDS_BINS;
    for (uint32_t i = threadIdx.x; i < lds_bins; i += HIST_BLOCK) h[i] = 0;
    __syncthreads();
    // every thread of a block makes the same number of turns: the ballots inside hist_count see whole wavefronts
    const uint4 *body = reinterpret_cast<const uint4 *>(a.counts + a.head);
    const uint64_t stride = (uint64_t)gridDim.x * HIST_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * HIST_BLOCK; base < a.n_vec; base += stride) {
        const uint64_t j = base + threadIdx.x;
        const bool have = j < a.n_vec;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (have) v = body[j];
        hist_count(v.x, have, a, h);
        hist_count(v.y, have, a, h);
        hist_count(v.z, have, a, h);
        hist_count(v.w, have, a, h);
    }
    if (blockIdx.x == 0) {   // the counters around the body: fewer than 2 * HIST_VEC
        const uint64_t n_edge = a.n - a.n_vec * HIST_VEC;
        for (uint64_t base = 0; base < n_edge; base += HIST_BLOCK) {
            const uint64_t j = base + threadIdx.x;
            const bool have = j < n_edge;
            const uint64_t at = j < a.head ? j : j + a.n_vec * HIST_VEC;
            hist_count(have ? a.counts[at] : 0u, have, a, h);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < lds_bins; i += HIST_BLOCK)
        if (h[i]) atomicAdd(&a.hist[i], (unsigned long long)h[i]);
}

// the launch of k_hist over n counters in device memory into n_bins zeroed u64 bins in device memory
static int hist_launch(pf_ctx *ctx, const uint32_t *counts, uint64_t n, uint64_t lo, uint64_t hi, uint32_t n_bins, unsigned long long *hist) {
    HistArgs a;
    a.counts = counts;
    a.n = n;
    a.head = std::min<uint64_t>(n, ((16 - ((uintptr_t)counts & 15)) & 15) / 4);
    a.n_vec = (n - a.head) / HIST_VEC;
    a.lo = lo;
    a.hi = hi;
    a.n_bins = n_bins;
    a.hist = hist;
    const int grid = ctx_grid(ctx, a.n_vec, HIST_BLOCK, HIST_PER_CU);
    // records one block counts: its turns of HIST_BLOCK x HIST_VEC, and block 0 the edges as well.  Below 2^32, or its u32 bins in
    // LDS could wrap (with 2048 blocks: 2^43 records, far more than HBM holds)
    const uint64_t turns = (a.n_vec + (uint64_t)grid * HIST_BLOCK - 1) / ((uint64_t)grid * HIST_BLOCK);
    if (turns >= (1ull << 32) / (HIST_BLOCK * HIST_VEC) - 1) {
        pf::CtxErr{ctx} = "pf_count_histogram: " + std::to_string(n) + " records are more than a block of this device counts in 32 bits";
        return PF_ERR_ARG;
    }
    ctx_begin(ctx, PF_K_HIST);
    k_hist<<<grid, HIST_BLOCK, 0, ctx->stream>>>(a);
    const hipError_t le = hipGetLastError();
    ctx_end(ctx);
    ctx_units(ctx, PF_K_HIST, n);
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-HIST launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_count_histogram(pf_ctx *ctx, const uint32_t *counts, uint64_t n, uint64_t lo, uint64_t hi, uint32_t n_bins, uint64_t *hist) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (n_bins == 0 || n_bins > PF_HIST_MAX_BINS)
        return refuse("pf_count_histogram: " + std::to_string(n_bins) + " bins: a histogram holds 1 to " + std::to_string(PF_HIST_MAX_BINS));
    if (!hist || (n && !counts)) return refuse("pf_count_histogram: counts and hist are needed");
    if ((uintptr_t)counts & 3) return refuse("pf_count_histogram: counts is not aligned to 4 bytes");
    PF_HIP(hipSetDevice(ctx->device));
    // stage the counters and the bins on the device if the caller passed host memory
    DevTmp<uint32_t> dc_;
    DevTmp<unsigned long long> dh_;
    const uint32_t *pc = counts;
    if (n && !is_device_ptr(counts)) {
        PF_HIP(dc_.alloc((size_t)n * 4));
        PF_HIP(hipMemcpyAsync(dc_.p, counts, (size_t)n * 4, hipMemcpyDefault, ctx->stream));
        pc = dc_.p;
    }
    const bool hist_on_dev = is_device_ptr(hist);
    unsigned long long *ph = reinterpret_cast<unsigned long long *>(hist);
    if (!hist_on_dev) {
        PF_HIP(dh_.alloc((size_t)n_bins * 8));
        ph = dh_.p;
    }
    PF_HIP(hipMemsetAsync(ph, 0, (size_t)n_bins * 8, ctx->stream));
    if (n && lo <= hi) {
        const int rc = hist_launch(ctx, pc, n, lo, hi, n_bins, ph);
        if (rc) return rc;
    }
    if (!hist_on_dev) PF_HIP(hipMemcpyAsync(hist, ph, (size_t)n_bins * 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}
