// K-DENSITY: the Gaussian kernel density of the values K-GMM fits -- the curve the reference's script/Drawfreq.R draws with
// ggplot2's geom_density (stats::density with bw.nrd0, 512 points over [min, max]), as numbers.  The values stay where
// pf_gmm_fit reads them (workspace WS_GMM_X) and are not changed.  Three groups of kernels, every launch of one
// pf_gmm_density enqueued back to back with one synchronisation at the end:
//   moments   k_den_moments1 (min, max, sum, first value that is not finite) and k_den_moments2 (squared deviations from the
//             mean): grid-stride, fixed-order block reduction into per-block partials, folded in block order by one block
//             (k_den_fold1 / k_den_fold2) -- the pattern of k_gmm_pass / k_gmm_update;
//   select    the four order statistics behind the type-7 quartiles by radix select, no sort and no second array: a double maps
//             to a 64-bit key that orders like the value, k_den_hist counts one 8-bit digit a pass, most significant first, in LDS
//             (integer atomics) and flushes to HBM (integer atomics), k_den_pick finds for every wanted rank the bucket that
//             holds it and the rank within.  One pass per digit serves all four ranks: ranks whose prefixes are still equal share
//             a histogram, a rank whose prefix has split off counts into its own.  After the eighth digit the key is the value.
//             (8-bit digits: four histograms are 4 KB of LDS; a single 16-bit one would be 256 KB, more than a CU's 160 KB.)
//   sum       k_den_prepare makes bandwidth, grid and record; k_den_sum: a block takes a chunk of values (staged through LDS
//             DEN_SUM_TILE at a time and broadcast from there: the value of a step is the same for every lane), a thread owns
//             DEN_PPT grid points in registers, grid.y covers the point tiles, the block writes one partial per point;
//             k_den_fold adds each point's partials in chunk order and scales by 1 / (n bw sqrt(2 pi)).
// Everything is fp64.  Block counts and chunk lengths are functions of n (and the point count) alone and no sum goes through a
// floating-point atomic, so the result is the same bits on every call and every device.  exp() is evaluated for every pair: a
// term below fp64's range is exactly 0 by itself, nothing is skipped on a looser test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/ploidyfrost_hip.h"
#include "pf_ctx.hpp"

// the quantile, the bandwidth and the grid are stated operation by operation: no fused multiply-add takes two of them at once
#pragma clang fp contract(off)

namespace pf {

constexpr int DEN_BLOCK = 256;
constexpr int DEN_MOM_ITEMS = 2048;        // values per moments block until the grid stops growing
constexpr int DEN_MOM_MAX_BLOCKS = 1024;
constexpr int DEN_SEL_ITEMS = 4096;        // values per select block until the grid stops growing
constexpr int DEN_SEL_MAX_BLOCKS = 1024;
constexpr int DEN_DIGIT_BITS = 8;
constexpr int DEN_BINS = 1 << DEN_DIGIT_BITS;
constexpr int DEN_RANKS = 4;               // x(lo), x(lo + 1) of Q(0.25), then of Q(0.75)
constexpr int DEN_SUM_TILE = 1024;         // values in LDS at a time; a chunk is a whole number of tiles
constexpr int DEN_SUM_MAX_CHUNKS = 2048;
constexpr int DEN_PPT = 2;                 // grid points a thread of k_den_sum owns
constexpr unsigned long long DEN_NONE = ~0ull;

struct DenState {
    double min, max, sum, mean, ssd;
    unsigned long long bad;                   // index of the first value that is not finite, DEN_NONE: all are
    unsigned long long prefix[DEN_RANKS];     // the digits found so far (key >> shift of the last pass)
    unsigned long long rank[DEN_RANKS];       // rank among the keys that share the prefix
    int slot[DEN_RANKS];                      // the histogram a rank counts into: the first rank with the same prefix
    double inv_bw, scale;
    pf_density_info info;
};

// values per chunk of k_den_sum and values per block of the other two groups: functions of n alone
__host__ inline uint64_t den_sum_chunk(uint64_t n) {
    const uint64_t span = (uint64_t)DEN_SUM_TILE * DEN_SUM_MAX_CHUNKS;
    return (uint64_t)DEN_SUM_TILE * std::max<uint64_t>(1, (n + span - 1) / span);
}
__host__ inline int den_blocks(uint64_t n, int items, int max_blocks) {
    return (int)std::min<uint64_t>(std::max<uint64_t>(1, (n + (uint64_t)items - 1) / (uint64_t)items), (uint64_t)max_blocks);
}

// a 64-bit key that orders like the double: positives get their sign bit set, negatives are inverted
__device__ inline unsigned long long den_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double den_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__device__ inline double den_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ inline double den_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
    return v;
}
__device__ inline double den_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}
__device__ inline unsigned long long den_wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_down(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// ---- moments ----
// partial[block] = { min, max, sum } of the block's values; the first value that is not finite goes to the state
__global__ __launch_bounds__(DEN_BLOCK) void k_den_moments1(const double *__restrict__ x, uint64_t n, DenState *st, double *__restrict__ partial) {
    double mn = INFINITY, mx = -INFINITY, s = 0.0;
    unsigned long long bad = DEN_NONE;
    const uint64_t stride = (uint64_t)gridDim.x * DEN_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * DEN_BLOCK + threadIdx.x; j < n; j += stride) {
        const double v = x[j];
        if (!isfinite(v) && bad == DEN_NONE) bad = j;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        s += v;
    }
    __shared__ double red[DEN_BLOCK / 64][3];
    __shared__ unsigned long long red_bad[DEN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    mn = den_wave_min(mn);
    mx = den_wave_max(mx);
    s = den_wave_sum(s);
    bad = den_wave_min_u64(bad);
    if (lane == 0) { red[wv][0] = mn; red[wv][1] = mx; red[wv][2] = s; red_bad[wv] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < DEN_BLOCK / 64; ++q) {
            mn = fmin(mn, red[q][0]);
            mx = fmax(mx, red[q][1]);
            s += red[q][2];
            bad = red_bad[q] < bad ? red_bad[q] : bad;
        }
        partial[(size_t)blockIdx.x * 3 + 0] = mn;
        partial[(size_t)blockIdx.x * 3 + 1] = mx;
        partial[(size_t)blockIdx.x * 3 + 2] = s;
        if (bad != DEN_NONE) atomicMin(&st->bad, bad);
    }
}

// folds a column of the partials in block order: thread t takes blocks t, t + 256, ..., then the block's fixed tree
__device__ inline double den_fold_sum(const double *partial, int n_blocks, int stride, int col, double (*red)[3]) {
    double t = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += DEN_BLOCK) t += partial[(size_t)b * stride + col];
    t = den_wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][2] = t;
    __syncthreads();
    double r = red[0][2];
    for (int q = 1; q < DEN_BLOCK / 64; ++q) r += red[q][2];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(DEN_BLOCK) void k_den_fold1(const double *__restrict__ partial, int n_blocks, uint64_t n, DenState *st) {
    __shared__ double red[DEN_BLOCK / 64][3];
    double mn = INFINITY, mx = -INFINITY;
    for (int b = threadIdx.x; b < n_blocks; b += DEN_BLOCK) {
        mn = fmin(mn, partial[(size_t)b * 3 + 0]);
        mx = fmax(mx, partial[(size_t)b * 3 + 1]);
    }
    mn = den_wave_min(mn);
    mx = den_wave_max(mx);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = mn; red[threadIdx.x >> 6][1] = mx; }
    __syncthreads();
    for (int q = 0; q < DEN_BLOCK / 64; ++q) { mn = fmin(mn, red[q][0]); mx = fmax(mx, red[q][1]); }
    __syncthreads();
    const double s = den_fold_sum(partial, n_blocks, 3, 2, red);
    if (threadIdx.x == 0) {
        st->min = mn;
        st->max = mx;
        st->sum = s;
        st->mean = s / (double)n;
    }
}

// partial[block] = sum of (v - mean)^2 over the block's values
__global__ __launch_bounds__(DEN_BLOCK) void k_den_moments2(const double *__restrict__ x, uint64_t n, const DenState *__restrict__ st, double *__restrict__ partial) {
    const double mean = st->mean;
    double s = 0.0;
    const uint64_t stride = (uint64_t)gridDim.x * DEN_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * DEN_BLOCK + threadIdx.x; j < n; j += stride) {
        const double d = x[j] - mean;
        s += d * d;
    }
    __shared__ double red[DEN_BLOCK / 64];
    s = den_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < DEN_BLOCK / 64; ++q) s += red[q];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(DEN_BLOCK) void k_den_fold2(const double *__restrict__ partial, int n_blocks, DenState *st) {
    __shared__ double red[DEN_BLOCK / 64][3];
    const double s = den_fold_sum(partial, n_blocks, 1, 0, red);
    if (threadIdx.x == 0) st->ssd = s;
}

// ---- order statistics ----
// one digit of every key that still carries a wanted prefix: hist[slot][digit] += 1.  shift = bit position of the digit.
__global__ __launch_bounds__(DEN_BLOCK) void k_den_hist(const double *__restrict__ x, uint64_t n, const DenState *__restrict__ st, int shift,
                                                        unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[DEN_RANKS * DEN_BINS];
    for (int i = threadIdx.x; i < DEN_RANKS * DEN_BINS; i += DEN_BLOCK) h[i] = 0;
    unsigned long long prefix[DEN_RANKS];
    bool own[DEN_RANKS];
#pragma unroll
    for (int r = 0; r < DEN_RANKS; ++r) {
        prefix[r] = st->prefix[r];
        own[r] = st->slot[r] == r;
    }
    const bool first = shift == 64 - DEN_DIGIT_BITS;   // no digit found yet: every key counts, into histogram 0
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * DEN_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * DEN_BLOCK + threadIdx.x; j < n; j += stride) {
        const unsigned long long key = den_key(x[j]);
        const unsigned int digit = (unsigned int)(key >> shift) & (DEN_BINS - 1);
        if (first) {
            atomicAdd(&h[digit], 1u);
        } else {
            const unsigned long long above = key >> (shift + DEN_DIGIT_BITS);
#pragma unroll
            for (int r = 0; r < DEN_RANKS; ++r)
                if (own[r] && above == prefix[r]) atomicAdd(&h[r * DEN_BINS + digit], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DEN_RANKS * DEN_BINS; i += DEN_BLOCK)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// for every rank the bucket that holds it and the rank within; then which ranks still share a prefix; the histograms are cleared
// for the next digit
__global__ __launch_bounds__(DEN_BLOCK) void k_den_pick(unsigned long long *__restrict__ hist, DenState *st, int shift) {
    __shared__ unsigned long long new_prefix[DEN_RANKS];
    if (threadIdx.x < DEN_RANKS) {
        const int r = threadIdx.x;
        const unsigned long long *hr = hist + (size_t)st->slot[r] * DEN_BINS;
        unsigned long long rank = st->rank[r], cum = 0;
        int d = 0;
        for (; d < DEN_BINS - 1; ++d) {
            const unsigned long long c = hr[d];
            if (rank < cum + c) break;
            cum += c;
        }
        const unsigned long long before = shift == 64 - DEN_DIGIT_BITS ? 0ull : st->prefix[r] << DEN_DIGIT_BITS;
        new_prefix[r] = before | (unsigned long long)d;
        st->rank[r] = rank - cum;
    }
    __syncthreads();
    if (threadIdx.x < DEN_RANKS) {
        const int r = threadIdx.x;
        int s = r;
        for (int q = r - 1; q >= 0; --q)
            if (new_prefix[q] == new_prefix[r]) s = q;
        st->prefix[r] = new_prefix[r];
        st->slot[r] = s;
    }
    for (int i = threadIdx.x; i < DEN_RANKS * DEN_BINS; i += DEN_BLOCK) hist[i] = 0;
}

// ---- the sum ----
// bandwidth, record and grid.  g25 / g75: the type-7 weights h - floor(h) of the two quartiles; npow = n^(-1/5)
__global__ __launch_bounds__(DEN_BLOCK) void k_den_prepare(const double *__restrict__ x, uint64_t n, DenState *st, uint32_t points, double adjust,
                                                           double npow, double g25, double g75, double *__restrict__ grid) {
    __shared__ double lo_hi[2];
    if (threadIdx.x == 0) {
        pf_density_info info;
        info.n = n;
        info.min = st->min;
        info.max = st->max;
        for (int r = 0; r < DEN_RANKS; ++r) info.order[r] = den_unkey(st->prefix[r]);
        info.q1 = (1.0 - g25) * info.order[0] + g25 * info.order[1];
        info.q3 = (1.0 - g75) * info.order[2] + g75 * info.order[3];
        info.sd = sqrt(st->ssd / (double)(n - 1));
        const double iqr = info.q3 - info.q1;
        double s = fmin(info.sd, iqr / 1.34);
        if (s == 0.0) s = info.sd != 0.0 ? info.sd : (fabs(x[0]) != 0.0 ? fabs(x[0]) : 1.0);
        info.bw = adjust * 0.9 * s * npow;
        st->info = info;
        st->inv_bw = 1.0 / info.bw;
        st->scale = 1.0 / ((double)n * info.bw * sqrt(2.0 * M_PI));
        lo_hi[0] = info.min;
        lo_hi[1] = info.max;
    }
    __syncthreads();
    const double lo = lo_hi[0], hi = lo_hi[1];
    for (uint32_t j = threadIdx.x; j < points; j += DEN_BLOCK)
        grid[j] = j == points - 1 ? hi : lo + (double)j * (hi - lo) / (double)(points - 1);
}

// partial[chunk][j] = sum over the chunk's values of exp(-((x_j - v) / bw)^2 / 2), in the chunk's order
__global__ __launch_bounds__(DEN_BLOCK) void k_den_sum(const double *__restrict__ x, uint64_t n, const DenState *__restrict__ st,
                                                       const double *__restrict__ grid, uint32_t points, uint64_t chunk, double *__restrict__ partial) {
    __shared__ double tile[DEN_SUM_TILE];
    const double inv_bw = st->inv_bw;
    double xj[DEN_PPT], acc[DEN_PPT];
#pragma unroll
    for (int p = 0; p < DEN_PPT; ++p) {
        const uint32_t j = (blockIdx.y * DEN_PPT + p) * DEN_BLOCK + threadIdx.x;
        xj[p] = j < points ? grid[j] : 0.0;
        acc[p] = 0.0;
    }
    const uint64_t begin = (uint64_t)blockIdx.x * chunk, end = begin + chunk < n ? begin + chunk : n;
    for (uint64_t t = begin; t < end; t += DEN_SUM_TILE) {
        __syncthreads();
        for (int i = threadIdx.x; i < DEN_SUM_TILE; i += DEN_BLOCK) tile[i] = t + i < end ? x[t + i] : 0.0;
        __syncthreads();
        const int cnt = end - t < (uint64_t)DEN_SUM_TILE ? (int)(end - t) : DEN_SUM_TILE;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const double v = tile[i];
#pragma unroll
            for (int p = 0; p < DEN_PPT; ++p) {
                const double z = (xj[p] - v) * inv_bw;
                acc[p] += exp(-0.5 * (z * z));
            }
        }
    }
#pragma unroll
    for (int p = 0; p < DEN_PPT; ++p) {
        const uint32_t j = (blockIdx.y * DEN_PPT + p) * DEN_BLOCK + threadIdx.x;
        if (j < points) partial[(size_t)blockIdx.x * points + j] = acc[p];
    }
}

// density[j] = scale * (partial[0][j] + partial[1][j] + ...), chunk by chunk
__global__ __launch_bounds__(DEN_BLOCK) void k_den_fold(const double *__restrict__ partial, uint32_t n_chunks, uint32_t points, const DenState *__restrict__ st,
                                                        double *__restrict__ density) {
    const uint32_t j = blockIdx.x * DEN_BLOCK + threadIdx.x;
    if (j >= points) return;
    double s = 0.0;
    for (uint32_t c = 0; c < n_chunks; ++c) s += partial[(size_t)c * points + j];
    density[j] = s * st->scale;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_gmm_density(pf_ctx *ctx, uint32_t points, double adjust, double *x, double *density, pf_density_info *info) {
    if (!ctx) return PF_ERR_ARG;
    auto refuse = [&](const std::string &m) { pf::CtxErr{ctx} = m; return (int)PF_ERR_ARG; };
    if (!x || !density || !info) return refuse("pf_gmm_density: x, density and info are needed");
    if (points < PF_DENSITY_MIN_POINTS || points > PF_DENSITY_MAX_POINTS)
        return refuse("pf_gmm_density: " + std::to_string(points) + " points: the grid holds " + std::to_string(PF_DENSITY_MIN_POINTS) + " to " +
                      std::to_string(PF_DENSITY_MAX_POINTS));
    if (!(adjust > 0.0) || !std::isfinite(adjust)) return refuse("pf_gmm_density: adjust is a finite positive number");
    const uint64_t n = ctx->gmm_loaded ? ctx->gmm_n : 0;
    if (n < 2) return refuse("need at least 2 data points");
    PF_HIP(hipSetDevice(ctx->device));
    const double *dx = (const double *)ctx_ws(ctx, WS_GMM_X, (size_t)n * 8);
    const int mom_blocks = den_blocks(n, DEN_MOM_ITEMS, DEN_MOM_MAX_BLOCKS), sel_blocks = den_blocks(n, DEN_SEL_ITEMS, DEN_SEL_MAX_BLOCKS);
    const uint64_t chunk = den_sum_chunk(n);
    const uint32_t n_chunks = (uint32_t)((n + chunk - 1) / chunk);
    const uint32_t point_tiles = (points + DEN_PPT * DEN_BLOCK - 1) / (DEN_PPT * DEN_BLOCK);
    // one workspace: state | histograms | x, density | partials
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_hist = up(sizeof(DenState)), o_out = o_hist + up((size_t)DEN_RANKS * DEN_BINS * 8), o_part = o_out + up((size_t)points * 16);
    const size_t part_bytes = std::max<size_t>((size_t)mom_blocks * 3, (size_t)n_chunks * points) * 8;
    uint8_t *ws = (uint8_t *)ctx_ws(ctx, WS_DENSITY, o_part + part_bytes);
    if (!dx || !ws) return PF_ERR_HIP;
    DenState *dst = (DenState *)ws;
    unsigned long long *dhist = (unsigned long long *)(ws + o_hist);
    double *dgrid = (double *)(ws + o_out), *dden = dgrid + points, *dpart = (double *)(ws + o_part);

    // the type-7 quantile Q(p): h = (n - 1) p, lo = floor(h), g = h - lo
    DenState h{};
    h.bad = DEN_NONE;
    double g[2];
    const double p[2] = {0.25, 0.75};
    for (int q = 0; q < 2; ++q) {
        const double hq = (double)(n - 1) * p[q], lo = std::floor(hq);
        g[q] = hq - lo;
        h.rank[2 * q] = (unsigned long long)lo;
        h.rank[2 * q + 1] = (unsigned long long)lo + 1;   // (p < 1: lo + 1 <= n - 1)
    }
    PF_HIP(hipMemcpyAsync(dst, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
    PF_HIP(hipMemsetAsync(dhist, 0, (size_t)DEN_RANKS * DEN_BINS * 8, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    ctx_begin(ctx, PF_K_DENSITY);
    k_den_moments1<<<mom_blocks, DEN_BLOCK, 0, ctx->stream>>>(dx, n, dst, dpart);
    k_den_fold1<<<1, DEN_BLOCK, 0, ctx->stream>>>(dpart, mom_blocks, n, dst);
    k_den_moments2<<<mom_blocks, DEN_BLOCK, 0, ctx->stream>>>(dx, n, dst, dpart);
    k_den_fold2<<<1, DEN_BLOCK, 0, ctx->stream>>>(dpart, mom_blocks, dst);
    for (int shift = 64 - DEN_DIGIT_BITS; shift >= 0; shift -= DEN_DIGIT_BITS) {
        k_den_hist<<<sel_blocks, DEN_BLOCK, 0, ctx->stream>>>(dx, n, dst, shift, dhist);
        k_den_pick<<<1, DEN_BLOCK, 0, ctx->stream>>>(dhist, dst, shift);
    }
    k_den_prepare<<<1, DEN_BLOCK, 0, ctx->stream>>>(dx, n, dst, points, adjust, std::pow((double)n, -0.2), g[0], g[1], dgrid);
    k_den_sum<<<dim3(n_chunks, point_tiles), DEN_BLOCK, 0, ctx->stream>>>(dx, n, dst, dgrid, points, chunk, dpart);
    k_den_fold<<<(points + DEN_BLOCK - 1) / DEN_BLOCK, DEN_BLOCK, 0, ctx->stream>>>(dpart, n_chunks, points, dst, dden);
    const hipError_t le = hipGetLastError();
    ctx_end(ctx);
    ctx_units(ctx, PF_K_DENSITY, n * points);
    if (le != hipSuccess) { pf::CtxErr{ctx} = std::string("K-DENSITY launch: ") + hipGetErrorString(le); return PF_ERR_HIP; }
    PF_HIP(hipMemcpyAsync(&h, dst, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    if (h.bad != DEN_NONE) {
        double v = 0;
        PF_HIP(hipMemcpyAsync(&v, dx + h.bad, 8, hipMemcpyDeviceToHost, ctx->stream));
        PF_HIP(hipStreamSynchronize(ctx->stream));
        return refuse(std::string("pf_gmm_density: value ") + std::to_string(h.bad) + " is not finite (" + (std::isnan(v) ? "NaN" : v > 0 ? "Inf" : "-Inf") + ")");
    }
    PF_HIP(hipMemcpyAsync(x, dgrid, (size_t)points * 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipMemcpyAsync(density, dden, (size_t)points * 8, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    *info = h.info;
    return PF_OK;
}
